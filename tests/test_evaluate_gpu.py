"""urso_pose_eval and evaluate() on the GPU: the kernel against the reference's own evaluate (tests/golden/eval.npz, recorded raw
outputs fed directly), edge cases, and evaluate() end to end against a detect loop scored on the host."""
import os

import numpy as np
import pytest
import torch

from util import make_config

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _run_case(g, c):
    """urso_pose_eval on the golden case c -> (table [n, COLS] numpy, q_soft or None)."""
    from ursonet_amd import hip
    from ursonet_amd.pose import OrientationCodec, location_map
    regress_loc, regress_ori, kp = (bool(x) for x in g[c + "/config"])
    param = str(g[c + "/ori_param"])
    loc, ori = _dev(g[c + "/loc"], np.float32), _dev(g[c + "/ori"], np.float32)
    n = loc.shape[0]
    loc_mode = hip.EVAL_LOC_REGRESS if regress_loc else hip.EVAL_LOC_CLASS
    ori2 = loc_map = hq = enc_loc = enc_ori = q_soft = None
    if kp:
        ori_mode, ori2 = hip.EVAL_ORI_KEYPOINTS, _dev(g[c + "/ori2"], np.float32)
    elif regress_ori:
        ori_mode = {"quaternion": hip.EVAL_ORI_QUAT, "euler_angles": hip.EVAL_ORI_EULER, "angle_axis": hip.EVAL_ORI_ANGLE_AXIS}[param]
    else:
        ori_mode = hip.EVAL_ORI_SOFT
        hq = _dev(OrientationCodec(int(g[c + "/ori_bins"]), float(g["beta"])).H_quat, np.float32)
        q_soft = torch.empty(n, 4, dtype=torch.float32, device="cuda")
        hip.quat_wavg_decode(n, ori.shape[1], ori, hq, q_soft)
        enc_ori = _dev(g[c + "/enc_ori"], np.float32)
    if not regress_loc:
        mx, mn = g[c + "/loc_lims"]
        loc_map = _dev(location_map(int(g[c + "/loc_bins"]), mx, mn), np.float64)
        enc_loc = _dev(g[c + "/enc_loc"], np.float32)
    table = torch.full((n, hip.EVAL_COLS), np.nan, dtype=torch.float64, device="cuda")
    hip.pose_eval(n, n, 0, loc_mode, ori_mode, loc, q_soft if q_soft is not None else ori, _dev(g[c + "/loc_gt"], np.float64),
                  _dev(g[c + "/q_gt"], np.float64), table, ori2=ori2, loc_map=loc_map, ori_map=hq, enc_loc=enc_loc, enc_ori=enc_ori)
    torch.cuda.synchronize()
    return table.cpu().numpy(), (None if q_soft is None else q_soft.cpu().numpy())


def _angle(a, b):
    """Rotation angle [rad] between the directions of quaternions a and b (rows), accurate near 0."""
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    s = np.where(np.sum(a * b, axis=1) < 0, -1.0, 1.0)[:, None]
    return 4 * np.arcsin(np.minimum(1, np.linalg.norm(a - s * b, axis=1) / 2))


def _norm_term(q, q_gt):
    """First-order change of 2 acos|q . q_gt| [rad] when q is scaled to unit length."""
    n = np.linalg.norm(q, axis=1)
    d = np.minimum(np.abs(np.sum(q * q_gt, axis=1)) / n, 1 - 1e-12)
    return 2 * np.abs(n - 1) * d / np.sqrt(1 - d * d)


def _fp32_term(q, q_gt):
    """Rounding of the reference's own angle where its q_est is float32 (quat_weighted_avg): the 4-term dot product in fp32 is off
    by up to 4 ulp(1), which 2 acos turns into 8 eps32 / sqrt(1 - d^2) [rad]."""
    d = np.minimum(np.abs(np.sum(q * q_gt, axis=1)) / np.linalg.norm(q, axis=1), 1 - 1e-12)
    return 8 * np.finfo(np.float32).eps / np.sqrt(1 - d * d)


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def test_kernel_against_reference_evaluate():
    from ursonet_amd import hip
    g = np.load(GOLD)
    report = {}
    for c in g["cases"]:
        t, q_soft = _run_case(g, c)
        regress_loc, regress_ori, kp = (bool(x) for x in g[c + "/config"])
        q = t[:, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4]
        qr = g[c + "/q_ref"].astype(np.float64)                                          # fp32 for the soft head: norms and dots in float64
        dq = 1 - np.abs(np.sum(q * qr, axis=1)) / (np.linalg.norm(q, axis=1) * np.linalg.norm(qr, axis=1))   # q_out is unit only to fp32
        if regress_ori or kp:
            assert np.all(dq <= 1e-10), (c, dq)
            tol = 1e-9
        else:
            assert np.array_equal(q, q_soft.astype(np.float64)), c                        # bit-equal to urso_quat_wavg_decode
            assert np.all(dq <= 1e-9), (c, dq)        # margin over the golden's and the kernel's fp32 rounding: tests/test_poseref_cpu.py
            # triangle inequality: |err(q) - err(q_ref)| <= angle(q, q_ref), plus the first-order effect of |q| != 1 (the decode's
            # quaternion is unit to fp32) on 2 acos|q . q_gt|
            bound = np.degrees(_angle(q, qr) + _norm_term(q, g[c + "/q_gt"]) + _fp32_term(q, g[c + "/q_gt"])) + 1e-6
            assert np.all(np.abs(t[:, hip.EVAL_ORI_ERR] - g[c + "/ori_err"]) <= bound), c
            qe = g[c + "/q_enc_ref"]
            assert np.all(np.abs(t[:, hip.EVAL_ORI_ENC_ERR] - g[c + "/ori_enc_err"]) <= 2 * 180 / np.pi * np.sqrt(2 * 1e-5) + 1e-6), c
            assert np.all(np.isfinite(qe))
            tol = None
        le = t[:, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3]
        if regress_loc:
            assert np.array_equal(le, g[c + "/loc"].astype(np.float64)), c
        else:
            report[c + " loc_est"] = float(_rel(le, g[c + "/loc_ref"]).max())
            assert np.all(_rel(le, g[c + "/loc_ref"]) <= 1e-5), c
            lenc = t[:, hip.EVAL_LOC_ENC_ERR]
            assert np.all(_rel(lenc, g[c + "/loc_enc_err"]) <= 1e-9), (c, lenc, g[c + "/loc_enc_err"])
            report[c + " loc_enc_err"] = float(_rel(lenc, g[c + "/loc_enc_err"]).max())
        assert np.array_equal(t[:, hip.EVAL_DIST], g[c + "/dist"]), c
        ltol = 1e-9 if regress_loc else 1e-5
        assert np.all(_rel(t[:, hip.EVAL_LOC_ERR], g[c + "/loc_err"]) <= ltol), c
        if tol is not None:
            assert np.all(_rel(t[:, hip.EVAL_ORI_ERR], g[c + "/ori_err"]) <= tol) or np.all(np.abs(t[:, hip.EVAL_ORI_ERR] - g[c + "/ori_err"]) <= 1e-9), c
            assert np.all(_rel(t[:, hip.EVAL_ESA], g[c + "/esa"]) <= ltol), c
        else:
            bound_r = _angle(q, qr) + _norm_term(q, g[c + "/q_gt"]) + _fp32_term(q, g[c + "/q_gt"]) + 1e-6
            assert np.all(np.abs(t[:, hip.EVAL_ESA] - g[c + "/esa"]) <= bound_r + ltol * np.abs(g[c + "/esa"])), c
        # the case's printed means, from the kernel's rows
        for k, col in ((0, hip.EVAL_LOC_ERR), (1, hip.EVAL_ORI_ERR), (2, hip.EVAL_ESA)):
            ref = float(str(g[c + "/summary"][k]).split(":", 1)[1])
            per = np.abs(t[:, col] - np.asarray(g[c + "/" + ("loc_err", "ori_err", "esa")[k]]))
            assert abs(np.mean(t[:, col]) - ref) <= per.max() * 1.001 + 1e-12 * abs(ref), (c, k)
    print("max relative deviation (classification location):", report)


def _table(n_rows):
    from ursonet_amd import hip
    return torch.full((n_rows, hip.EVAL_COLS), -7.0, dtype=torch.float64, device="cuda")


def test_edge_cases():
    from ursonet_amd import hip
    B = 4
    q = np.array([[0, 0, 0, 1], [0.5, 0.5, 0.5, 0.5], [0, 0, 0, 1], [0, 1, 0, 0]], dtype=np.float32)
    loc = np.array([[0, 0, 10], [1, 2, 3], [0, 0, 5], [1, 1, 1]], dtype=np.float32)
    q[2, 1] = np.nan                                                      # a non-finite output in row 2 only
    t = _table(8)
    hip.pose_eval(B, 3, 2, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), _dev(loc, np.float64), _dev(q[[0, 1, 0, 3]], np.float64), t)
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert np.all(h[:2] == -7.0) and np.all(h[5:] == -7.0)               # rows outside [row0, row0 + n) untouched
    assert h[2, hip.EVAL_ORI_ERR] == 0 and h[2, hip.EVAL_LOC_ERR] == 0 and h[2, hip.EVAL_ESA] == 0   # identical quaternions: 0, not NaN
    assert h[3, hip.EVAL_ORI_ERR] == 0 and np.isfinite(h[3]).sum() >= 11
    assert np.isnan(h[4, hip.EVAL_ORI_ERR]) and np.isnan(h[4, hip.EVAL_ESA]) and h[4, hip.EVAL_LOC_ERR] == 0
    assert h[4, hip.EVAL_DIST] == 5
    # theta = 0 angle-axis: the identity quaternion
    aa = np.zeros((B, 3), dtype=np.float32)
    aa[1] = [3e-7, 0, 0]
    t2 = _table(B)
    hip.pose_eval(B, B, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_ANGLE_AXIS, _dev(loc), _dev(aa), _dev(loc, np.float64),
                  _dev(np.tile([0, 0, 0, 1.0], (B, 1))), t2)
    h2 = t2.cpu().numpy()
    assert np.array_equal(h2[0, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4], [0, 0, 0, 1.0]) and h2[0, hip.EVAL_ORI_ERR] == 0
    assert np.array_equal(h2[1, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4], [0, 0, 0, np.cos(np.float64(np.float32(3e-7)) / 2)])   # theta < 1e-6: axis 0
    # bad arguments: URSO_EINVAL, nothing launched (the sentinel survives)
    t3 = _table(B)
    with pytest.raises(hip.UrsoHipError, match="n <= B"):
        hip.pose_eval(B, B + 1, 0, hip.EVAL_LOC_REGRESS, hip.EVAL_ORI_QUAT, _dev(loc), _dev(q), _dev(loc, np.float64), _dev(q, np.float64), t3)
    with pytest.raises(hip.UrsoHipError, match="unknown ori_mode"):
        hip.pose_eval(B, B, 0, hip.EVAL_LOC_REGRESS, 9, _dev(loc), _dev(q), _dev(loc, np.float64), _dev(q, np.float64), t3)
    torch.cuda.synchronize()
    assert np.all(t3.cpu().numpy() == -7.0)


def _models(tmp_path, backbone, B, regress_ori, regress_loc):
    """A training-mode model writes weights; an inference model with engine batch B loads them."""
    from ursonet_amd import net
    cfg = make_config(backbone, 128, 192, batch=B, regress_ori=regress_ori, regress_loc=regress_loc, ori_bins=8, loc_bins=4,
                      dtype="bfloat16" if backbone == "resnet50" else "float32")
    cfg.NAME = "syn"
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    path = str(tmp_path / ("weights_%s_%d_%d_0001.npz" % (backbone, regress_ori, regress_loc)))
    tr.save_weights(path)
    del tr
    inf = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    inf.load_weights(path, path, by_name=True)
    return cfg, inf


def _detect_loop(model, ds, cfg):
    """The reference-style loop: detect on the same batches (tail padded with the last frame), decoded and scored on the host with
    the oracle's formulas -> (loc_est, q_est, loc_err, ori_err, esa) per image; soft classification also returns the logits."""
    from oracle import pose_math as P
    from ursonet_amd import pose
    from ursonet_amd.feeder import eval_batch_plan
    B = model._engine.B
    out = {k: [] for k in ("loc", "q", "le", "oe", "esa", "logits")}
    for row0, n, slots in eval_batch_plan(ds.image_ids, B):
        res = model.detect([ds.load_image(i) for i in slots])[:n]
        for r, i in zip(res, slots[:n]):
            loc_gt, q_gt = np.asarray(ds.load_location(i), np.float64), np.asarray(ds.load_quaternion(i), np.float64)
            loc = r["loc"] if cfg.REGRESS_LOC else P.decode_location_classified(r["loc"].astype(np.float64), ds.histogram_3D_map)
            if cfg.REGRESS_ORI:
                q = r["ori"].astype(np.float64)
            else:
                q = pose.decode_orientations(r["ori"][None], ds.ori_histogram_map)[0].astype(np.float64)
                out["logits"].append(r["ori"])
            d = min(1.0, abs(float(np.dot(q, q_gt))))
            le = np.linalg.norm(np.asarray(loc, np.float64) - loc_gt)
            out["loc"].append(np.asarray(loc, np.float64)); out["q"].append(q); out["le"].append(le)
            out["oe"].append(2 * np.arccos(d) * 180 / np.pi); out["esa"].append(le / np.linalg.norm(loc_gt) + 2 * np.arccos(d))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("backbone,regress_ori,regress_loc", [("resnet18", True, True), ("resnet18", False, True),
                                                              ("resnet18", False, False), ("resnet50", False, True)])
def test_evaluate_matches_detect_loop(tmp_path, backbone, regress_ori, regress_loc):
    from ursonet_amd import evaluate as ev
    from ursonet_amd.dataset import SyntheticPoses
    cfg, model = _models(tmp_path, backbone, 4, regress_ori, regress_loc)
    ds = SyntheticPoses(10, 128, 192, cfg, seed=3)
    ds._image_ids = np.array([3, 1, 4, 0, 9, 2, 6, 5, 8, 7])            # evaluation follows image_ids order, not 0..N-1
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir(); d2.mkdir()
    r = ev.evaluate(model, ds, out_dir=str(d1), verbose=0)
    r2 = ev.evaluate(model, ds, out_dir=str(d2), verbose=0)
    for k in ("loc_est", "q_est", "loc_err", "ori_err", "esa", "dist"):
        assert np.array_equal(getattr(r, k), getattr(r2, k)), k                  # two runs are bit-identical
    for name in ev.CSV_FILES:
        assert (d1 / name).read_text() == (d2 / name).read_text()
    assert list(r.image_ids) == list(ds.image_ids)
    ref = _detect_loop(model, ds, cfg)
    if regress_loc:
        assert np.array_equal(r.loc_est, ref["loc"])                            # bit for bit with detect
        assert np.all(_rel(r.loc_err, ref["le"]) <= 1e-9)
    else:
        assert np.all(_rel(r.loc_est, ref["loc"]) <= 1e-9)
        assert r.loc_encoded_err is not None and np.all(np.isfinite(r.loc_encoded_err))
    assert np.array_equal(r.q_est, ref["q"])                                    # q_out / the same decode, bit for bit
    assert np.allclose(r.ori_err, ref["oe"], rtol=1e-9, atol=1e-9)
    assert np.allclose(r.esa, ref["esa"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(r.dist, [np.float64(ds.load_location(i)[2]) for i in ds.image_ids])
    lines = (d1 / "ori_err.csv").read_text().splitlines()
    assert lines[0] == ",0" and len(lines) == 11


def test_evaluate_b1_matches_its_detect_loop(tmp_path):
    from ursonet_amd import evaluate as ev
    from ursonet_amd.dataset import SyntheticPoses
    cfg, model = _models(tmp_path, "resnet18", 1, False, True)
    ds = SyntheticPoses(3, 128, 192, cfg, seed=4)
    r = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0)
    ref = _detect_loop(model, ds, cfg)
    assert np.array_equal(r.loc_est, ref["loc"]) and np.array_equal(r.q_est, ref["q"])
    assert np.allclose(r.ori_err, ref["oe"], rtol=1e-9, atol=1e-9)


def test_evaluate_multimodal_matches_host_selection(tmp_path, capsys):
    from ursonet_amd import evaluate as ev, pose
    from ursonet_amd.dataset import SyntheticPoses
    cfg, model = _models(tmp_path, "resnet18", 4, False, True)
    ds = SyntheticPoses(10, 128, 192, cfg, seed=5)
    r = ev.evaluate(model, ds, multimodal=True, out_dir=str(tmp_path), verbose=1)
    out = capsys.readouterr().out.splitlines()
    assert [l.split(":")[0] for l in out[-4:]] == [s.rstrip(": ") for s in ev.SUMMARY]
    assert out[-1] == "Mean encoded location error:  nan"
    ref = _detect_loop(model, ds, cfg)
    logits = np.stack(ref["logits"])
    var = (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12
    mean, _, _, _, nm = pose.fit_orientation_modes(logits, ds.ori_histogram_map, var, 5, 4)
    q_gt = np.stack([ds.load_quaternion(i) for i in ds.image_ids]).astype(np.float64)
    err = pose.mode_errors(mean, nm, q_gt)
    pick = np.where((nm == 1) | (err[:, 0] < err[:, 1]), 0, 1)
    assert np.array_equal(r.mode, pick)
    q_sel = mean[np.arange(len(pick)), pick].astype(np.float64)
    assert np.array_equal(r.q_est, q_sel)
    assert np.allclose(r.ori_err, err[np.arange(len(pick)), pick], rtol=1e-9, atol=1e-9)
    assert np.allclose(r.ori_err_soft, ref["oe"], rtol=1e-9, atol=1e-9)
