"""predict() / the submit command without a GPU: the submission writer against the reference's own exported text
(tests/golden/submit.npz, made by make_submit_golden.py from pose_estimator.test_and_submit), the argument checks of
urso_pose_decode (they run before any launch) and those of predict() / test_and_submit()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ursonet_amd import predict as pr
from ursonet_amd import submission as sub

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "submit.npz")
CASES = ("quaternion", "euler", "angle_axis", "soft_n8", "soft_n16")


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


def _fill(writer, g, c):
    for tag, add in (("virtual", writer.append_test), ("real", writer.append_real_test)):
        qt, rt = np.dtype(str(g[c + "/q_dtype"])).type, np.dtype(str(g[c + "/r_dtype"])).type
        for name, q, r in zip(g["%s/names_%s" % (c, tag)], g["%s/q_%s" % (c, tag)], g["%s/r_%s" % (c, tag)]):
            add(str(name), [qt(v) for v in q], [rt(v) for v in r])


def test_fixture_covers_the_cases():
    g = np.load(GOLD)
    assert tuple(g["cases"]) == CASES
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(HERE, "golden", "eval.npz"))
    for c in CASES:
        for tag in ("virtual", "real"):
            names = [str(n) for n in g["%s/names_%s" % (c, tag)]]
            assert names != sorted(names), (c, tag)                        # the writer has something to sort


@pytest.mark.parametrize("case", CASES)
def test_writer_reproduces_the_reference_bytes(tmp_path, capsys, case):
    g = np.load(GOLD)
    w = sub.SubmissionWriter()
    _fill(w, g, case)
    w.export(out_dir=str(tmp_path), suffix="debug")
    path = tmp_path / "submission_debug.csv"
    assert capsys.readouterr().out == "Submission saved to %s.\n" % path
    assert path.read_bytes() == str(g[case + "/csv"]).encode()             # sorting, group order, float32 / float64 text, line ends
    rows = path.read_text().split("\n")
    assert rows[-1] == "" and all(len(r.split(",")) == 8 for r in rows[:-1])


def test_writer_default_name_is_the_timestamp(tmp_path, capsys):
    w = sub.SubmissionWriter()
    w.append_real_test("b.jpg", [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 5.0])
    w.append_test("z.jpg", [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 5.0])
    w.append_test("a.jpg", (np.float32(0.1), 0.0, 0.0, 0.0), np.array([0.0, 0.0, 5.0], dtype=np.float32))
    w.export(out_dir=str(tmp_path))
    files = os.listdir(str(tmp_path))
    assert len(files) == 1 and re.fullmatch(r"submission_\d{8}-\d{4}\.csv", files[0]), files
    assert (tmp_path / files[0]).read_text() == "a.jpg,0.1,0.0,0.0,0.0,0.0,0.0,5.0\nz.jpg,1.0,0.0,0.0,0.0,0.0,0.0,5.0\nb.jpg,1.0,0.0,0.0,0.0,0.0,0.0,5.0\n"
    assert "Submission saved to" in capsys.readouterr().out


def test_submission_rows_reorder_and_type():
    class R(object):
        image_ids = np.array([1, 0])
        q_est = np.array([[0.1, 0.2, 0.3, 0.9], [0.0, 0.0, 0.0, 1.0]])
        loc_est = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])

    class D(object):
        image_info = [{"path": "/x/y/img0.jpg"}, {"path": "img1.jpg"}]
    rows = sub.submission_rows(R, D, _Cfg())
    assert [r[0] for r in rows] == ["img1.jpg", "img0.jpg"]
    assert rows[0][1] == [np.float32(0.9), np.float32(0.1), np.float32(0.2), np.float32(0.3)]      # [w, x, y, z]
    assert {type(v) for r in rows for v in r[1] + r[2]} == {np.float32}
    for kw in ({"ORIENTATION_PARAM": "euler_angles"}, {"ORIENTATION_PARAM": "angle_axis"}, {"REGRESS_KEYPOINTS": True}):
        rows = sub.submission_rows(R, D, _Cfg(**kw))
        assert {type(v) for r in rows for v in r[1]} == {np.float64} and {type(v) for r in rows for v in r[2]} == {np.float32}
    rows = sub.submission_rows(R, D, _Cfg(REGRESS_ORI=False, REGRESS_LOC=False))
    assert {type(v) for r in rows for v in r[1]} == {np.float32} and {type(v) for r in rows for v in r[2]} == {np.float64}


def test_training_model_is_refused():
    with pytest.raises(AssertionError, match="Create model in inference mode."):
        pr.predict(_Model("training"), _Data())
    with pytest.raises(AssertionError, match="Create model in inference mode."):
        sub.test_and_submit(_Model("training"), _Data(), _Data())


def test_multimodal_needs_soft_classification():
    for kw in ({}, {"ORIENTATION_PARAM": "euler_angles"}, {"REGRESS_KEYPOINTS": True}):
        with pytest.raises(ValueError, match=r"predict\(multimodal=True\) needs the soft-classification"):
            pr.predict(_Model(**kw), _Data(), multimodal=True)


def test_missing_bin_maps_are_refused():
    with pytest.raises(ValueError, match="histogram_3D_map"):
        pr.predict(_Model(REGRESS_LOC=False), _Data())
    with pytest.raises(ValueError, match="ori_histogram_map"):
        pr.predict(_Model(REGRESS_ORI=False), _Data())
    with pytest.raises(ValueError, match="histogram_3D_map"):
        sub.test_and_submit(_Model(REGRESS_LOC=False), _Data(), _Data())


def test_symbol_is_declared_bound_and_exported():
    import ursonet_amd.hip as hip
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ursonet_hip.h")).read()
    assert re.search(r"\bint\s+urso_pose_decode\s*\(\s*const\s+urso_pose_decode_args\s*\*", hdr)
    assert "urso_pose_decode" in hip.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T urso_pose_decode$", out, re.M)
    for name in ("LOC_EST", "Q_EST", "LOC_PEAK", "ORI_PEAK", "ORI_LAMBDA", "COLS"):                # hip.py mirrors the header's columns
        m = re.search(r"\bURSO_DEC_%s\s*=\s*(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(hip, "DEC_" + name), name
    assert hip._lib.urso_abi_version() == 9


def _args(**kw):
    import ursonet_amd.hip as hip
    a = hip.PoseDecodeArgs()
    a.B, a.n, a.row0, a.loc_mode, a.ori_mode, a.loc_ld, a.ori_ld = 4, 4, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, 3, 4
    a.loc = a.ori = a.table = 4096                                      # never dereferenced: every case fails validation
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_pose_decode_argument_validation_without_gpu():
    import ursonet_amd.hip as hip
    soft, cls, kp = hip.EVAL_ORI_SOFT, hip.EVAL_LOC_CLASS, hip.EVAL_ORI_KEYPOINTS
    cases = [
        (dict(loc=None), "null"), (dict(ori=None), "null"), (dict(table=None), "null"),
        (dict(B=0, n=0), "B > 0"), (dict(B=-1, n=0), "B > 0"), (dict(n=5), "n <= B"), (dict(n=-1), "n <= B"),
        (dict(row0=-1), "row0"),
        (dict(ori_mode=7), "unknown ori_mode"), (dict(ori_mode=-1), "unknown ori_mode"), (dict(loc_mode=2), "unknown loc_mode"),
        (dict(loc_mode=cls, loc_bins=512, loc_map_rows=343, loc_map=4096, loc_ld=512), "loc_bins"),
        (dict(loc_mode=cls, loc_bins=512, loc_map_rows=512, loc_map=None, loc_ld=512), "loc_map"),
        (dict(ori_mode=soft, ori_logits=4096, ori_bins=512, ori_map_rows=4096, ori_logits_ld=512), "ori_bins"),
        (dict(loc_ld=2), "loc_ld"), (dict(loc_mode=cls, loc_bins=512, loc_map_rows=512, loc_map=4096, loc_ld=511), "loc_ld"),
        (dict(ori_ld=3), "ori_ld"), (dict(ori_mode=hip.EVAL_ORI_EULER, ori_ld=2), "ori_ld"),
        (dict(ori_mode=soft, ori_logits=4096, ori_bins=512, ori_map_rows=512, ori_logits_ld=511), "ori_logits_ld"),
        (dict(ori_mode=kp, ori_ld=3), "ori2"),
        (dict(ori_logits=4096, ori_bins=512, ori_map_rows=512, ori_logits_ld=512), "soft classification only"),
        (dict(ori_mode=hip.EVAL_ORI_EULER, ori_ld=3, ori_scatter=4096), "soft classification only"),
    ]
    for kw, msg in cases:
        a = _args(**kw)
        assert hip._lib.urso_pose_decode(ctypes.byref(a), None) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_pose_decode:") and msg in err, (kw, err)
    assert hip._lib.urso_pose_decode(None, None) == -1
    assert hip.last_error().startswith("urso_pose_decode:") and "null" in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU)
    assert hip._lib.urso_pose_decode(ctypes.byref(_args(n=0)), None) == 0


def test_label_free_feeder_refuses_encoded_targets():
    from ursonet_amd.feeder import EvalFeeder
    with pytest.raises(AssertionError, match="labels"):
        EvalFeeder(None, None, None, enc_ori=True, labels=False)
