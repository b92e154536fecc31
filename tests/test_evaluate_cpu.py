"""evaluate() without a GPU: argument validation, the summary lines and CSV files against the reference's own output
(tests/golden/eval.npz, made by make_eval_golden.py from pose_estimator.evaluate), the argument checks of urso_pose_eval (they run
before any launch) and the batch plan of the evaluation feeder."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from ursonet_amd import evaluate as ev
from ursonet_amd.feeder import eval_batch_plan

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")


class _Cfg(object):
    def __init__(self, **kw):
        self.REGRESS_LOC, self.REGRESS_ORI, self.REGRESS_KEYPOINTS = True, True, False
        self.ORIENTATION_PARAM, self.BETA, self.ORI_BINS_PER_DIM = "quaternion", 6.0, 8
        self.__dict__.update(kw)


class _Model(object):
    def __init__(self, mode="inference", **kw):
        self.mode, self.config = mode, _Cfg(**kw)


class _Data(object):
    image_ids = [0, 1]


def test_training_model_is_refused():
    with pytest.raises(AssertionError, match="Create model in inference mode."):
        ev.evaluate(_Model("training"), _Data())


def test_multimodal_needs_soft_classification():
    for kw in ({}, {"ORIENTATION_PARAM": "euler_angles"}, {"REGRESS_KEYPOINTS": True}):
        with pytest.raises(ValueError, match="soft-classification"):
            ev.evaluate(_Model(**kw), _Data(), multimodal=True)


def test_location_classification_needs_histogram_3d_map():
    with pytest.raises(ValueError, match="histogram_3D_map"):
        ev.evaluate(_Model(REGRESS_LOC=False), _Data())


def test_utils_reexports_evaluate():
    from ursonet_amd import utils
    assert utils.evaluate is ev.evaluate


def test_fixture_maps_match_the_codecs():
    from ursonet_amd.pose import OrientationCodec, location_map
    g = np.load(GOLD)
    for n in (8, 16):
        hq = OrientationCodec(n, float(g["beta"])).H_quat
        assert hashlib.sha256(np.ascontiguousarray(hq).tobytes()).hexdigest() == str(g["ori_map_sha256_n%d" % n])
    mx, mn = g["loc_class/loc_lims"]
    H = location_map(int(g["loc_class/loc_bins"]), mx, mn)
    assert hashlib.sha256(np.ascontiguousarray(H).tobytes()).hexdigest() == str(g["loc_class/loc_map_sha256"])
    assert {"quaternion", "euler", "angle_axis", "soft_n8", "soft_n16", "loc_class", "keypoints"} <= set(g["cases"])
    for c in g["cases"]:
        assert np.all(g[c + "/margin_branch"] > float(g["tie_floor"])) and np.all(g[c + "/margin_dot"] >= 0), c


def test_summary_lines_and_csvs_reproduce_the_reference(tmp_path):
    g = np.load(GOLD)
    for c in g["cases"]:
        loc_enc = g[c + "/loc_enc_err"]
        means = [np.mean(g[c + "/loc_err"]), np.mean(g[c + "/ori_err"]), np.mean(g[c + "/esa"]),
                 np.mean(loc_enc) if not np.all(np.isnan(loc_enc)) else np.float64(np.nan)]
        lines = ev.summary_lines(means)
        for mine, ref in zip(lines, g[c + "/summary"]):
            lab_m, v_m = mine.split(":", 1)
            lab_r, v_r = str(ref).split(":", 1)
            assert lab_m == lab_r and v_m[:2] == v_r[:2] == "  ", (c, mine, ref)
            vm, vr = float(v_m), float(v_r)
            assert (np.isnan(vm) and np.isnan(vr)) or abs(vm - vr) <= 1e-12 * max(1.0, abs(vr)), (c, mine, ref)
        d = tmp_path / c
        d.mkdir()
        ev.write_csvs(str(d), g[c + "/ori_err"], g[c + "/loc_err"], g[c + "/dist"])
        for name, ref in zip(ev.CSV_FILES, g[c + "/csv"]):
            mine = (d / name).read_text()
            rl, ml = str(ref).splitlines(), mine.splitlines()
            assert ml[0] == rl[0] == ",0" and len(ml) == len(rl), (c, name)
            for a, b in zip(ml[1:], rl[1:]):
                ia, va = a.split(",")
                ib, vb = b.split(",")
                assert ia == ib and float(va) == float(vb), (c, name, a, b)


def test_csv_text_without_pandas_matches_pandas():
    pd = pytest.importorskip("pandas")
    for a in (np.array([0.1, 2.5e-7, 33.0]), np.array([1.5, 12.345678], dtype=np.float32)):
        assert ev.csv_text(a) == pd.DataFrame(a).to_csv()
    import builtins
    real = builtins.__import__

    def no_pandas(name, *args, **kw):
        if name == "pandas":
            raise ImportError(name)
        return real(name, *args, **kw)
    a = np.array([0.1, 2.5e-7, 33.0])
    builtins.__import__ = no_pandas
    try:
        text = ev.csv_text(a)
    finally:
        builtins.__import__ = real
    assert text == pd.DataFrame(a).to_csv()


def _args(**kw):
    import ursonet_amd.hip as hip
    a = hip.PoseEvalArgs()
    a.B, a.n, a.row0, a.loc_mode, a.ori_mode, a.loc_ld, a.ori_ld = 4, 4, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, 3, 4
    a.loc = a.ori = a.loc_gt = a.q_gt = a.table = 4096                  # never dereferenced: every case fails validation
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_pose_eval_argument_validation_without_gpu():
    import ursonet_amd.hip as hip
    assert "urso_pose_eval" in hip.EXPORTED_SYMBOLS
    cases = [
        (dict(loc=None), "null"), (dict(q_gt=None), "null"), (dict(table=None), "null"),
        (dict(n=5), "n <= B"), (dict(n=-1), "n <= B"), (dict(B=0, n=0), "B > 0"),
        (dict(ori_mode=7), "unknown ori_mode"), (dict(loc_mode=2), "unknown loc_mode"),
        (dict(loc_mode=hip.EVAL_LOC_CLASS, loc_bins=512, loc_map_rows=343, loc_map=4096, loc_ld=512), "loc_bins"),
        (dict(ori_mode=hip.EVAL_ORI_SOFT, enc_ori=4096, ori_map=4096, ori_bins=512, ori_map_rows=4096), "ori_bins"),
        (dict(enc_ori=4096, ori_map=4096, ori_bins=512, ori_map_rows=512), "soft classification only"),
        (dict(ori_mode=hip.EVAL_ORI_KEYPOINTS, ori_ld=3), "ori2"),
        (dict(ori_ld=3), "ori_ld"),
    ]
    for kw, msg in cases:
        a = _args(**kw)
        assert hip._lib.urso_pose_eval(ctypes.byref(a), None) == -1, kw
        assert msg in hip.last_error(), (kw, hip.last_error())
    assert hip._lib.urso_pose_eval(None, None) == -1


@pytest.mark.parametrize("N,B", [(0, 4), (3, 4), (8, 4), (10, 4), (5, 1)])
def test_eval_batch_plan(N, B):
    ids = [100 + 7 * i for i in range(N)]                              # ids need not be 0..N-1
    plan = eval_batch_plan(ids, B)
    assert len(plan) == -(-N // B)
    covered = []
    for k, (row0, n, slots) in enumerate(plan):
        assert row0 == k * B and len(slots) == B and 1 <= n <= B
        assert slots[:n] == ids[row0:row0 + n]                         # valid slots: the next images, in order
        assert slots[n:] == [ids[row0 + n - 1]] * (B - n)              # padding repeats the last valid image
        assert n == B or k == len(plan) - 1                            # only the tail is short
        covered += list(range(row0, row0 + n))
    assert covered == list(range(N))                                   # each table row written exactly once
