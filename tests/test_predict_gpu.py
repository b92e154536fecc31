"""urso_pose_decode, predict() and the submit command on the GPU: the kernel's estimates bit for bit against urso_pose_eval on the
reference-recorded raw outputs (tests/golden/eval.npz), its confidence columns against NumPy float64, edge cases, the exported
submission against the reference's own file (tests/golden/submit.npz), and predict() end to end against evaluate() and a detect loop
decoded on the host."""
import os

import numpy as np
import pytest
import torch

from util import make_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "eval.npz")
GOLD_SUBMIT = os.path.join(HERE, "golden", "submit.npz")


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def _softmax64(z):
    e = np.exp(z.astype(np.float64) - z.astype(np.float64).max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _case_inputs(g, c):
    """Device inputs of the golden case c, as test_evaluate_gpu feeds them to urso_pose_eval."""
    from ursonet_amd import hip
    from ursonet_amd.pose import OrientationCodec, location_map
    regress_loc, regress_ori, kp = (bool(x) for x in g[c + "/config"])
    param = str(g[c + "/ori_param"])
    d = {"loc": _dev(g[c + "/loc"], np.float32), "logits": None, "ori2": None, "loc_map": None, "hq": None, "scatter": None}
    ori = _dev(g[c + "/ori"], np.float32)
    n = d["n"] = ori.shape[0]
    d["loc_mode"] = hip.EVAL_LOC_REGRESS if regress_loc else hip.EVAL_LOC_CLASS
    if kp:
        d["ori_mode"], d["ori2"] = hip.EVAL_ORI_KEYPOINTS, _dev(g[c + "/ori2"], np.float32)
    elif regress_ori:
        d["ori_mode"] = {"quaternion": hip.EVAL_ORI_QUAT, "euler_angles": hip.EVAL_ORI_EULER, "angle_axis": hip.EVAL_ORI_ANGLE_AXIS}[param]
    else:
        d["ori_mode"] = hip.EVAL_ORI_SOFT
        d["hq"] = _dev(OrientationCodec(int(g[c + "/ori_bins"]), float(g["beta"])).H_quat, np.float32)
        d["logits"] = ori
        ori = torch.empty(n, 4, dtype=torch.float32, device="cuda")
        d["scatter"] = torch.empty(n, 16, dtype=torch.float32, device="cuda")
        hip.quat_wavg_decode(n, d["logits"].shape[1], d["logits"], d["hq"], ori, d["scatter"])
    if not regress_loc:
        mx, mn = g[c + "/loc_lims"]
        d["loc_map"] = _dev(location_map(int(g[c + "/loc_bins"]), mx, mn), np.float64)
    d["ori"] = ori
    return d


def _decode(d):
    from ursonet_amd import hip
    n = d["n"]
    t = torch.full((n, hip.DEC_COLS), np.nan, dtype=torch.float64, device="cuda")
    hip.pose_decode(n, n, 0, d["loc_mode"], d["ori_mode"], d["loc"], d["ori"], t, ori2=d["ori2"], loc_map=d["loc_map"], ori_logits=d["logits"],
                    ori_map_rows=0 if d["hq"] is None else d["hq"].shape[0], ori_scatter=d["scatter"])
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_estimates_are_bit_identical_to_pose_eval():
    """Every case of eval.npz, loc_class and keypoints included: LOC_EST and Q_EST of urso_pose_decode are the bits urso_pose_eval
    writes for the same inputs, so the reference bounds of test_evaluate_gpu.test_kernel_against_reference_evaluate hold for them."""
    from ursonet_amd import hip
    g = np.load(GOLD)
    assert len(g["cases"]) == 7
    for c in g["cases"]:
        d = _case_inputs(g, c)
        n = d["n"]
        te = torch.full((n, hip.EVAL_COLS), np.nan, dtype=torch.float64, device="cuda")
        hip.pose_eval(n, n, 0, d["loc_mode"], d["ori_mode"], d["loc"], d["ori"], _dev(g[c + "/loc_gt"], np.float64), _dev(g[c + "/q_gt"], np.float64),
                      te, ori2=d["ori2"], loc_map=d["loc_map"])
        torch.cuda.synchronize()
        te, td = te.cpu().numpy(), _decode(d)
        assert np.all(np.isfinite(td[:, :7])), c
        assert np.array_equal(td[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3], te[:, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3]), c
        assert np.array_equal(td[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4], te[:, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4]), c
        assert np.all(td[:, hip.DEC_ORI_LAMBDA + 1:] == 0), c


def test_confidence_columns_against_numpy_float64():
    """LOC_PEAK / ORI_PEAK = max of the fp64 softmax of the fp32 logits, ORI_LAMBDA = q^T A q / q^T q from the very q and A the
    decode produced: fp64 evaluations of fp32 inputs, relative bound 1e-9 (the bound test_evaluate_gpu uses for such columns)."""
    from ursonet_amd import hip
    g = np.load(GOLD)
    seen = set()
    for c in g["cases"]:
        d = _case_inputs(g, c)
        t = _decode(d)
        if d["loc_mode"] == hip.EVAL_LOC_CLASS:
            ref = _softmax64(g[c + "/loc"].astype(np.float32)).max(axis=1)
            print(c, "LOC_PEAK rel", _rel(t[:, hip.DEC_LOC_PEAK], ref).max())
            assert np.all(_rel(t[:, hip.DEC_LOC_PEAK], ref) <= 1e-9), c
            seen.add("loc")
        else:
            assert np.all(np.isnan(t[:, hip.DEC_LOC_PEAK])), c
        if d["ori_mode"] == hip.EVAL_ORI_SOFT:
            ref = _softmax64(g[c + "/ori"].astype(np.float32)).max(axis=1)
            print(c, "ORI_PEAK rel", _rel(t[:, hip.DEC_ORI_PEAK], ref).max())
            assert np.all(_rel(t[:, hip.DEC_ORI_PEAK], ref) <= 1e-9), c
            q, A = d["ori"].cpu().numpy().astype(np.float64), d["scatter"].cpu().numpy().astype(np.float64).reshape(-1, 4, 4)
            lam = np.einsum("bi,bij,bj->b", q, A, q) / np.einsum("bi,bi->b", q, q)
            print(c, "ORI_LAMBDA rel", _rel(t[:, hip.DEC_ORI_LAMBDA], lam).max(), t[:, hip.DEC_ORI_LAMBDA])
            assert np.all(_rel(t[:, hip.DEC_ORI_LAMBDA], lam) <= 1e-9), c
            assert np.all((t[:, hip.DEC_ORI_LAMBDA] >= 0.25 - 1e-6) & (t[:, hip.DEC_ORI_LAMBDA] <= 1 + 1e-6)), c
            seen.add("ori")
        else:
            assert np.all(np.isnan(t[:, hip.DEC_ORI_PEAK])) and np.all(np.isnan(t[:, hip.DEC_ORI_LAMBDA])), c
    assert seen == {"loc", "ori"}


def _soft_decode(z, hq):
    from ursonet_amd import hip
    B = z.shape[0]
    q = torch.empty(B, 4, dtype=torch.float32, device="cuda")
    A = torch.empty(B, 16, dtype=torch.float32, device="cuda")
    hip.quat_wavg_decode(B, z.shape[1], z, hq, q, A)
    return q, A


def test_confidence_anchors():
    """One bin 200 above the rest: ORI_PEAK == 1.0 exactly (exp(-200) vanishes beside 1 in fp64) and |ORI_LAMBDA - 1| <= 1e-5 (the bin map
    and a_d are fp32; 1e-5 is the project's bound for the soft head).  All-equal logits: ORI_PEAK == 1 / K to 1e-12 relative."""
    from ursonet_amd import hip
    from ursonet_amd.pose import OrientationCodec
    for nb in (8, 24):
        hq = _dev(OrientationCodec(nb, 6.0).H_quat, np.float32)
        K = hq.shape[0]
        z = np.full((2, K), -3.0, dtype=np.float32)
        z[0, K // 3] = 197.0
        zd = _dev(z)
        q, A = _soft_decode(zd, hq)
        t = torch.full((2, hip.DEC_COLS), np.nan, dtype=torch.float64, device="cuda")
        loc = _dev(np.zeros((2, 3), dtype=np.float32))
        hip.pose_decode(2, 2, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_SOFT, loc, q, t, ori_logits=zd, ori_map_rows=K, ori_scatter=A)
        h = t.cpu().numpy()
        print(nb, "anchors", h[:, hip.DEC_ORI_PEAK], h[:, hip.DEC_ORI_LAMBDA])
        assert h[0, hip.DEC_ORI_PEAK] == 1.0
        assert abs(h[0, hip.DEC_ORI_LAMBDA] - 1) <= 1e-5
        assert abs(h[1, hip.DEC_ORI_PEAK] * K - 1) <= 1e-12
        assert 0.25 - 1e-6 <= h[1, hip.DEC_ORI_LAMBDA] <= 1 + 1e-6


def _table(n_rows):
    from ursonet_amd import hip
    return torch.full((n_rows, hip.DEC_COLS), np.nan, dtype=torch.float64, device="cuda")


def test_edge_cases():
    from ursonet_amd import hip
    from ursonet_amd.pose import OrientationCodec, location_map
    B = 4
    q = np.array([[0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5], [0, 0, 0, 1], [0, 1, 0, 0]], dtype=np.float32)
    loc = np.array([[0, 0, 10], [1, 2, 3], [0, 0, 5], [1, 1, 1]], dtype=np.float32)
    # n = 0: nothing is written
    t = _table(B)
    hip.pose_decode(B, 0, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), t)
    torch.cuda.synchronize()
    assert np.all(np.isnan(t.cpu().numpy()))
    # n < B and row0 > 0: rows outside [row0, row0 + n) keep their NaN prefill; optional inputs absent: NaN columns
    t = _table(8)
    hip.pose_decode(B, 3, 2, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), t)
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert np.all(np.isnan(h[:2])) and np.all(np.isnan(h[5:]))
    assert np.array_equal(h[2:5, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3], loc[:3].astype(np.float64))
    assert np.array_equal(h[2:5, hip.DEC_Q_EST:hip.DEC_Q_EST + 4], q[:3].astype(np.float64))
    assert np.all(np.isnan(h[2:5, hip.DEC_LOC_PEAK:hip.DEC_ORI_LAMBDA + 1])) and np.all(h[2:5, hip.DEC_ORI_LAMBDA + 1:] == 0)
    # soft classification without ori_logits / ori_scatter: both columns NaN, each alone: only its own column
    hq = _dev(OrientationCodec(8, 6.0).H_quat, np.float32)
    K = hq.shape[0]
    rng = np.random.default_rng(5)
    z = rng.normal(size=(B, K)).astype(np.float32)
    z[2, 17] = np.nan                                                     # a NaN logit in row 2 only
    zd = _dev(z)
    qs, A = _soft_decode(zd, hq)
    tabs = {}
    for key, kw in (("none", {}), ("logits", dict(ori_logits=zd, ori_map_rows=K)), ("scatter", dict(ori_scatter=A)),
                    ("both", dict(ori_logits=zd, ori_map_rows=K, ori_scatter=A))):
        t = _table(B)
        hip.pose_decode(B, B, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_SOFT, _dev(loc), qs, t, **kw)
        tabs[key] = t.cpu().numpy()
    ok = [0, 1, 3]
    assert np.all(np.isnan(tabs["none"][:, [hip.DEC_ORI_PEAK, hip.DEC_ORI_LAMBDA]]))
    assert np.all(np.isfinite(tabs["logits"][ok, hip.DEC_ORI_PEAK])) and np.all(np.isnan(tabs["logits"][:, hip.DEC_ORI_LAMBDA]))
    assert np.all(np.isfinite(tabs["scatter"][ok, hip.DEC_ORI_LAMBDA])) and np.all(np.isnan(tabs["scatter"][:, hip.DEC_ORI_PEAK]))
    assert np.array_equal(tabs["both"][ok, hip.DEC_ORI_PEAK], tabs["logits"][ok, hip.DEC_ORI_PEAK])
    assert np.array_equal(tabs["both"][ok, hip.DEC_ORI_LAMBDA], tabs["scatter"][ok, hip.DEC_ORI_LAMBDA])
    # the NaN logit row: NaN estimates and NaN confidence, the other rows finite
    assert np.all(np.isnan(tabs["both"][2, hip.DEC_Q_EST:hip.DEC_Q_EST + 4])) and np.isnan(tabs["both"][2, hip.DEC_ORI_PEAK])
    assert np.isnan(tabs["both"][2, hip.DEC_ORI_LAMBDA]) and np.all(np.isfinite(tabs["both"][ok, :hip.DEC_LOC_PEAK]))
    # padded row strides: views of wider buffers give the same table as the packed inputs
    m = 4
    lmap = _dev(location_map(m, np.array([0.5, 0.5, 40.0]), np.array([-0.5, -0.5, 3.0])), np.float64)
    ll = rng.normal(size=(B, m ** 3)).astype(np.float32)
    ll[1, 5] = np.nan
    wide_l = torch.full((B, m ** 3 + 7), 1e30, dtype=torch.float32, device="cuda")
    wide_l[:, :m ** 3] = _dev(ll)
    wide_q = torch.full((B, 9), 1e30, dtype=torch.float32, device="cuda")
    wide_q[:, :4] = _dev(q)
    wide_z = torch.full((B, K + 5), 1e30, dtype=torch.float32, device="cuda")
    wide_z[:, :K] = zd
    t1, t2 = _table(B), _table(B)
    hip.pose_decode(B, B, 0, hip.EVAL_LOC_CLASS, hip.EVAL_ORI_SOFT, _dev(ll), _dev(q), t1, loc_map=lmap, ori_logits=zd, ori_map_rows=K)
    hip.pose_decode(B, B, 0, hip.EVAL_LOC_CLASS, hip.EVAL_ORI_SOFT, wide_l[:, :m ** 3], wide_q[:, :4], t2, loc_map=lmap,
                    ori_logits=wide_z[:, :K], ori_map_rows=K)
    h1, h2 = t1.cpu().numpy(), t2.cpu().numpy()
    assert np.array_equal(h1, h2, equal_nan=True)
    assert np.all(np.isnan(h1[1, :3])) and np.isnan(h1[1, hip.DEC_LOC_PEAK]) and np.all(np.isfinite(h1[[0, 2, 3], :hip.DEC_ORI_PEAK]))
    ref = _softmax64(ll[[0, 2, 3]])
    assert np.all(_rel(h1[[0, 2, 3], hip.DEC_LOC_PEAK], ref.max(axis=1)) <= 1e-9)
    # bad arguments: URSO_EINVAL, nothing launched (the prefill survives)
    t3 = _table(B)
    with pytest.raises(hip.UrsoHipError, match="n <= B"):
        hip.pose_decode(B, B + 1, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), t3)
    with pytest.raises(hip.UrsoHipError, match="soft classification only"):
        hip.pose_decode(B, B, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), t3, ori_scatter=A)
    torch.cuda.synchronize()
    assert np.all(np.isnan(t3.cpu().numpy()))


class _Result(object):
    """What submission_rows reads of a PredictResult."""

    def __init__(self, ids, table):
        from ursonet_amd import hip
        self.image_ids = ids
        self.loc_est, self.q_est = table[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3], table[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4]


class _Info(object):
    def __init__(self, names):
        self.image_info = [{"path": "some/dir/" + str(n)} for n in names]


class _HeadCfg(object):
    def __init__(self, regress_ori, param):
        self.REGRESS_LOC, self.REGRESS_ORI, self.REGRESS_KEYPOINTS, self.ORIENTATION_PARAM = True, regress_ori, False, param


@pytest.mark.parametrize("case", ["quaternion", "euler", "angle_axis", "soft_n8", "soft_n16"])
def test_submission_against_the_reference_file(tmp_path, case):
    """Golden raw outputs -> urso_pose_decode -> PredictResult columns -> test_and_submit's row builder -> writer, against the text the
    reference's test_and_submit exported.  quaternion: byte for byte (the kernel passes fp32 values through exactly).  The other heads:
    the same file names in the same order, locations equal as numbers, quaternions ([w, x, y, z]) within the bounds
    test_evaluate_gpu has against this reference data: 1 - |dot| <= 1e-10 (closed-form heads), 1e-5 (soft head), sign-agnostic."""
    from ursonet_amd import submission as sub
    g, gs = np.load(GOLD), np.load(GOLD_SUBMIT)
    table = _decode(_case_inputs(g, case))
    cfg = _HeadCfg(bool(g[case + "/config"][1]), str(g[case + "/ori_param"]))
    w = sub.SubmissionWriter()
    for tag, add in (("virtual", w.append_test), ("real", w.append_real_test)):
        rows = gs["%s/rows_%s" % (case, tag)]
        for row in sub.submission_rows(_Result(np.arange(len(rows)), table[rows]), _Info(gs["%s/names_%s" % (case, tag)]), cfg):
            add(*row)
    mine = open(w.export(out_dir=str(tmp_path), suffix="debug"), newline="").read()
    ref = str(gs[case + "/csv"])
    if case == "quaternion":
        assert mine == ref
        return
    ml, rl = mine.split("\n"), ref.split("\n")
    assert len(ml) == len(rl) and ml[-1] == rl[-1] == ""
    worst = 0.0
    for a, b in zip(ml[:-1], rl[:-1]):
        fa, fb = a.split(","), b.split(",")
        assert len(fa) == len(fb) == 8 and fa[0] == fb[0], (a, b)
        assert [float(v) for v in fa[5:]] == [float(v) for v in fb[5:]], (a, b)
        qa, qb = np.array([float(v) for v in fa[1:5]]), np.array([float(v) for v in fb[1:5]])
        worst = max(worst, 1 - abs(np.dot(qa, qb)) / (np.linalg.norm(qa) * np.linalg.norm(qb)))
    print(case, "max 1 - |dot|:", worst)
    assert worst <= (1e-5 if case.startswith("soft") else 1e-10), case


class _NoLabels(object):
    """A SyntheticPoses dataset whose label loaders raise: what a SPEED test split offers."""

    def __init__(self, ds):
        self._ds = ds
        self.image_info = [{"path": "images/%s/img%06d.jpg" % (ds.name, 900 - 7 * i)} for i in range(len(ds.image_info))]

    @property
    def image_ids(self):
        return self._ds.image_ids

    def load_image(self, image_id):
        return self._ds.load_image(image_id)

    def __getattr__(self, name):
        if name.startswith("load_"):
            raise AssertionError("predict() must not call dataset.%s" % name)
        if name in ("histogram_3D_map", "ori_histogram_map"):
            return getattr(self._ds, name)
        raise AttributeError(name)


def _models(tmp_path, batches, regress_ori, regress_loc, h=128, w=192):
    """Inference models with the given engine batches that share one set of weights."""
    from ursonet_amd import net
    out = []
    path = None
    for B in batches:
        cfg = make_config("resnet18", h, w, batch=B, regress_ori=regress_ori, regress_loc=regress_loc, ori_bins=8, loc_bins=4, dtype="float32")
        cfg.NAME = "syn"
        if path is None:
            tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
            path = str(tmp_path / ("weights_%d_%d_0001.npz" % (regress_ori, regress_loc)))
            tr.save_weights(path)
            del tr
        inf = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
        inf.load_weights(path, path, by_name=True)
        out.append((cfg, inf))
    return out


def _detect_loop(model, ds, cfg, gmm=None):
    """The reference-style loop, as test_evaluate_gpu runs it: detect on the same batches (tail padded with the last frame), every image
    decoded on the host -> (loc, q); with gmm = (hq, var), also urso_quat_gmm_fit on the engine's own logits of each batch."""
    from oracle import pose_math as P
    from ursonet_amd import hip, pose
    from ursonet_amd.feeder import eval_batch_plan
    eng = model._engine
    loc_all, q_all, modes = [], [], ([], [], [])
    for row0, n, slots in eval_batch_plan(ds.image_ids, eng.B):
        res = model.detect([ds.load_image(i) for i in slots])[:n]
        for r in res:
            loc = r["loc"] if cfg.REGRESS_LOC else P.decode_location_classified(r["loc"].astype(np.float64), ds.histogram_3D_map)
            q = r["ori"] if cfg.REGRESS_ORI else pose.decode_orientations(r["ori"][None], ds.ori_histogram_map)[0]
            loc_all.append(np.asarray(loc, np.float64).ravel()); q_all.append(np.asarray(q).astype(np.float64))
        if gmm is not None:
            hq, var = gmm
            z = eng.outputs()[1][:n].contiguous()
            mean = torch.empty(n, 3, 4, dtype=torch.float32, device="cuda")
            gv, gp, gsc = (torch.empty(n, 3, dtype=torch.float32, device="cuda") for _ in range(3))
            nm = torch.empty(n, dtype=torch.int32, device="cuda")
            hip.quat_gmm_fit(n, z.shape[1], z, False, hq, var, 5, 4, mean, gv, gp, gsc, nm)
            for lst, t in zip(modes, (mean, gp, nm)):
                lst.append(t.cpu().numpy())
    return np.asarray(loc_all), np.asarray(q_all), [np.concatenate(m) for m in modes] if gmm is not None else None


@pytest.mark.parametrize("regress_ori,regress_loc", [(True, True), (False, True), (True, False), (False, False)])
def test_predict_end_to_end(tmp_path, regress_ori, regress_loc):
    """ResNet-18, engine batch 3, 7 images (two full batches and a tail of one)."""
    from ursonet_amd import evaluate as ev, predict as pr
    from ursonet_amd.dataset import SyntheticPoses
    (cfg, model), = _models(tmp_path, [3], regress_ori, regress_loc)
    ds = SyntheticPoses(7, 128, 192, cfg, seed=3)
    ds._image_ids = np.array([3, 1, 4, 0, 6, 2, 5])                        # prediction follows image_ids order, not 0..N-1
    # (a) a dataset without labels
    r = pr.predict(model, _NoLabels(ds))
    assert list(r.image_ids) == list(ds.image_ids) and r.loc_est.shape == (7, 3) and r.q_est.shape == (7, 4)
    assert np.all(np.isfinite(r.loc_est)) and np.all(np.isfinite(r.q_est))
    assert (r.loc_peak is None) == regress_loc and (r.ori_peak is None) == regress_ori and (r.ori_lambda is None) == regress_ori
    assert r.modes is None and r.mode_priors is None and r.n_modes is None
    if not regress_loc:
        assert np.all((r.loc_peak >= 1.0 / 64) & (r.loc_peak <= 1))
    if not regress_ori:
        assert np.all((r.ori_peak >= 1.0 / 512) & (r.ori_peak <= 1)) and np.all((r.ori_lambda >= 0.25 - 1e-6) & (r.ori_lambda <= 1 + 1e-6))
    # (b) the labelled twin: evaluate()'s estimates, bit for bit
    e = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0)
    r2 = pr.predict(model, ds)
    for k in ("loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda"):
        a, b = getattr(r, k), getattr(r2, k)
        assert (a is None and b is None) or np.array_equal(a, b), k
    assert np.array_equal(r.loc_est, e.loc_est) and np.array_equal(r.q_est, e.q_est)
    # (c) the detect loop decoded on the host, with test_evaluate_matches_detect_loop's tolerances
    gmm = None
    if not regress_ori:
        gmm = (_dev(ds.ori_histogram_map, np.float32), (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12)
    loc_ref, q_ref, modes_ref = _detect_loop(model, ds, cfg, gmm)
    if regress_loc:
        assert np.array_equal(r.loc_est, loc_ref)
    else:
        assert np.all(_rel(r.loc_est, loc_ref) <= 1e-9)
    assert np.array_equal(r.q_est, q_ref)
    # (e) multimodal: the fit of the same engine's logits at the same batch composition
    if not regress_ori:
        rm = pr.predict(model, _NoLabels(ds), multimodal=True)
        assert np.array_equal(rm.q_est, r.q_est) and np.array_equal(rm.ori_lambda, r.ori_lambda)       # q_est stays the soft-argmax estimate
        assert rm.modes.shape == (7, 3, 4) and rm.mode_priors.shape == (7, 3) and rm.n_modes.shape == (7,)
        assert np.array_equal(rm.modes, modes_ref[0], equal_nan=True) and np.array_equal(rm.mode_priors, modes_ref[1], equal_nan=True)
        assert np.array_equal(rm.n_modes, modes_ref[2]) and np.all(rm.n_modes >= 1)
    else:
        with pytest.raises(ValueError, match="soft-classification"):
            pr.predict(model, _NoLabels(ds), multimodal=True)
    # (d) DEVICE_RESIZE on native-size uint8 frames (130 x 200 -> 128 x 192): the same result as the host-resize path
    big = SyntheticPoses(7, 130, 200, cfg, seed=4)
    if not regress_ori:
        big.ori_histogram_map = ds.ori_histogram_map
    if not regress_loc:
        big.histogram_3D_map = ds.histogram_3D_map
    res = {}
    try:
        for on in (False, True):
            cfg.DEVICE_RESIZE = on
            res[on] = pr.predict(model, _NoLabels(big))
    finally:
        cfg.DEVICE_RESIZE = False
    for k in ("loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda"):
        a, b = getattr(res[False], k), getattr(res[True], k)
        assert (a is None and b is None) or (np.array_equal(a, b) and np.all(np.isfinite(a))), k


def test_device_resize_leg_runs_the_resize_kernel(tmp_path, monkeypatch):
    from ursonet_amd import hip, predict as pr
    from ursonet_amd.dataset import SyntheticPoses
    launches, real = [], hip.resize_images_u8

    def counted(*a, **kw):
        launches.append(a[0])
        return real(*a, **kw)
    monkeypatch.setattr(hip, "resize_images_u8", counted)
    (cfg, model), = _models(tmp_path, [3], True, True)
    big = SyntheticPoses(7, 130, 200, cfg, seed=4)
    try:
        pr.predict(model, _NoLabels(big))
        assert launches == []
        cfg.DEVICE_RESIZE = True
        pr.predict(model, _NoLabels(big))
    finally:
        cfg.DEVICE_RESIZE = False
    assert len(launches) == 3                                             # 7 images at batch 3: one launch per batch


def test_predict_b1_matches_detect_at_batch_1(tmp_path):
    """Engine batch 1: predict() against detect() one image at a time, decoded on the host (test_evaluate_b1_matches_its_detect_loop's
    comparison and tolerances)."""
    from ursonet_amd import predict as pr
    from ursonet_amd.dataset import SyntheticPoses
    (cfg, model), = _models(tmp_path, [1], False, True)
    ds = SyntheticPoses(3, 128, 192, cfg, seed=4)
    r = pr.predict(model, _NoLabels(ds))
    loc_ref, q_ref, _ = _detect_loop(model, ds, cfg)
    assert np.array_equal(r.loc_est, loc_ref) and np.array_equal(r.q_est, q_ref)


def test_test_and_submit_end_to_end(tmp_path, capsys):
    from ursonet_amd import submission as sub
    from ursonet_amd.dataset import SyntheticPoses
    (cfg, model), = _models(tmp_path, [3], True, True)
    virt, real = _NoLabels(SyntheticPoses(5, 128, 192, cfg, seed=6)), _NoLabels(SyntheticPoses(4, 128, 192, cfg, seed=7))
    real.image_info = [{"path": "real/" + d["path"].split("/")[-1].replace(".jpg", "real.jpg")} for d in real.image_info]
    rv, rr = sub.test_and_submit(model, virt, real, out_dir=str(tmp_path), suffix="unit")
    out = capsys.readouterr().out.splitlines()
    path = tmp_path / "submission_unit.csv"
    assert out[-2:] == ["Submission saved to %s." % path, "Submission exported."]
    text = path.read_text()
    assert text.endswith("\n") and "\r" not in text
    rows = [l.split(",") for l in text.split("\n")[:-1]]
    assert len(rows) == 9 and all(len(r) == 8 for r in rows)
    names = [r[0] for r in rows]
    assert names[:5] == sorted(names[:5]) and names[5:] == sorted(names[5:])
    assert all(not n.endswith("real.jpg") for n in names[:5]) and all(n.endswith("real.jpg") for n in names[5:])
    for res, data in ((rv, virt), (rr, real)):
        for i, image_id in enumerate(res.image_ids):
            row = rows[names.index(data.image_info[image_id]["path"].split("/")[-1])]
            q = res.q_est[i]
            assert [np.float32(v) for v in row[1:5]] == [np.float32(q[3]), np.float32(q[0]), np.float32(q[1]), np.float32(q[2])]
            assert [np.float32(v) for v in row[5:]] == [np.float32(v) for v in res.loc_est[i]]


class _PreparedLabelled(object):
    """A labelled dataset whose images are the host-prepared video frames (tests/test_video_gpu.py's _Prepared, with the labels kept):
    what evaluate(), predict() and detect_dataset() must see to run on the pixels track() prepares on the device."""

    def __init__(self, ds, frames, prep):
        self._ds, self._frames, self._prep = ds, frames, prep

    def load_image(self, image_id):
        return self._prep.host(self._frames[image_id])

    def __getattr__(self, name):
        return getattr(self._ds, name)


def test_four_commands_share_one_pass(tmp_path):
    """evaluate(), predict(), detect_dataset() and track() over the same 5 images: ResNet-18 at 128 x 192, engine batch 2 (the tail batch
    is padded), soft-classification orientation, regressed location, float32.  The frames are test_video_gpu's: 60 x 90, prepared (pad 8,
    crop (0, 0, 1, 3)) to 76 x 102 on the host for the three dataset commands and on the device by track().  The estimates are the same
    bits in all four, the confidences in predict and track, the errors in evaluate and detect."""
    from ursonet_amd import detect, evaluate as ev, predict as pr, video
    from ursonet_amd.dataset import SyntheticPoses
    (cfg, model), = _models(tmp_path, [2], False, True)
    ds = SyntheticPoses(5, 60, 90, cfg, seed=21)
    frames = [ds.load_image(i) for i in ds.image_ids]
    prep = video.VideoPrep(pad=8, crop=(0, 0, 1, 3))
    data = _PreparedLabelled(ds, frames, prep)
    e = ev.evaluate(model, data, out_dir=str(tmp_path), verbose=0)
    p = pr.predict(model, data)
    d = detect.detect_dataset(model, data, 0, image_ids=list(ds.image_ids), render=False, verbose=0)
    t = video.track(model, frames, data, prep=prep)
    assert e.loc_est.shape == (5, 3) and e.q_est.shape == (5, 4) and np.all(np.isfinite(e.loc_est)) and np.all(np.isfinite(e.q_est))
    for other in (p, d, t):
        assert np.array_equal(other.loc_est, e.loc_est) and np.array_equal(other.q_est, e.q_est)
    assert np.all(np.isfinite(p.ori_peak)) and np.all(np.isfinite(p.ori_lambda))
    assert np.array_equal(t.ori_peak, p.ori_peak) and np.array_equal(t.ori_lambda, p.ori_lambda)
    assert np.all(np.isfinite(e.loc_err)) and np.all(np.isfinite(e.ori_err))
    assert np.array_equal(d.loc_err, e.loc_err) and np.array_equal(d.ori_err, e.ori_err)
