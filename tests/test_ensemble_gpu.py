"""Ensemble inference on the GPU: urso_ens_add / urso_ens_settle against their float64 statement (ursonet_amd.ensemble.add64 / settle64;
cases and bounds: tests/ensref.py), their determinism, and predict / evaluate / test_and_submit with members=... end to end on the
small model and dataset of tests/test_predict_gpu.py."""
import numpy as np
import pytest
import torch

import ensref as R
import poseref as P
from ursonet_amd import ensemble as E
from util import make_config

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32).copy()


class _Case(object):
    """The device buffers of one kernel case, NaN wherever the kernels must neither read nor write: the logits sit one float behind a
    16-byte boundary (misalign) in rows ld apart; acc / stat / table have rows in front of row0 and behind row0 + n."""

    def __init__(self, K, B, n, row0, ld, misalign=1):
        rows = row0 + B + 1
        self.K, self.B, self.n, self.row0, self.ld, self.rows, self.mis = K, B, n, row0, ld, rows, misalign
        self.store = torch.full((B * ld + 8,), NAN, dtype=torch.float32, device="cuda")
        self.logits = self.store[misalign:misalign + B * ld].view(B, ld)[:, :K]
        assert self.logits.data_ptr() % 16 == 4 * (misalign % 4)
        self.acc = torch.full((rows, K), NAN, dtype=torch.float64, device="cuda")
        self.stat = torch.full((rows, 4), NAN, dtype=torch.float64, device="cuda")
        self.table = torch.full((rows, 8), NAN, dtype=torch.float64, device="cuda")
        self.logp = torch.full((B, K), NAN, dtype=torch.float32, device="cuda")

    def run(self, z):
        """z [M, n, K]: M adds and one settle -> (acc, stat, logp, table) of the valid rows, after checking every untouched element."""
        from ursonet_amd import hip
        M = len(z)
        for j in range(M):
            self.logits[:self.n] = _dev(z[j])
            hip.ens_add(self.B, self.n, self.row0, self.logits, self.acc, self.stat, j == 0)
        hip.ens_settle(self.n, self.row0, M, self.acc, self.stat, self.logp, self.table)
        torch.cuda.synchronize()
        keep = np.ones(self.rows, dtype=bool)
        keep[self.row0:self.row0 + self.n] = False
        for t in (self.acc, self.stat, self.table):
            assert np.all(np.isnan(t.cpu().numpy()[keep])), "a row outside [row0, row0 + n) was written"
        assert np.all(np.isnan(self.logp.cpu().numpy()[self.n:])), "a logp row past n was written"
        pad = self.store.cpu().numpy().copy()
        pad[self.mis:self.mis + self.B * self.ld].reshape(self.B, self.ld)[:self.n, :self.K] = NAN
        assert np.all(np.isnan(pad)), "the padding of the logits was written"
        sl = slice(self.row0, self.row0 + self.n)
        return self.acc[sl], self.stat[sl], self.logp[:self.n], self.table[sl]


def _check(tag, got, ref, K, M, counts):
    """One case against the reference; prints each figure before it asserts.  counts: [elements of logp that differ, elements]."""
    acc, stat, logp, table = (t.cpu().numpy() for t in got)
    racc, rstat, rlogp, rtable = ref
    tol = R.tol(K, M)
    nanrow = np.isnan(rtable[:, E.H_MEAN])
    assert np.array_equal(np.isnan(acc), np.isnan(racc)) and np.array_equal(np.isnan(table), np.isnan(rtable)), tag
    assert np.array_equal(np.isnan(logp), np.isnan(rlogp)) and np.array_equal(stat[:, 1:], rstat[:, 1:]), tag
    assert np.all(table[:, E.N_MEMBERS] == M) and np.all(table[:, 6:] == 0), tag
    ok = ~nanrow
    if not ok.any():
        return
    a, ra, t, rt = acc[ok], racc[ok], table[ok], rtable[ok]
    fig = dict(acc=float((np.abs(a - ra) / np.where(ra > 0, ra, 1.0)).max() / tol))
    assert np.array_equal(a == 0, ra == 0), tag
    for name, col in (("H_MEAN", E.H_MEAN), ("H_MEMBERS", E.H_MEMBERS), ("PEAK", E.PEAK)):
        den = np.where(rt[:, col] != 0, np.abs(rt[:, col]), 1.0)
        fig[name] = float((np.abs(t[:, col] - rt[:, col]) / den).max() / tol)
    hsum = rt[:, E.H_MEAN] + rt[:, E.H_MEMBERS]
    fig["MI"] = float((np.abs(t[:, E.MI] - rt[:, E.MI]) / np.where(hsum > 0, tol * hsum, 1.0)).max())
    fig["H_MEMBERS(stat)"] = float((np.abs(stat[ok, 0] - rstat[ok, 0]) / np.where(rstat[ok, 0] != 0, np.abs(rstat[ok, 0]), 1.0)).max() / tol)
    l, rl = logp[ok], rlogp[ok]
    diff = l != rl
    counts[0] += int(diff.sum())
    counts[1] += l.size
    with np.errstate(over="ignore"):                                         # (the spacing of FLT_MAX; those elements are compared exactly below)
        fig["logp_ulp"] = float((np.abs(l.astype(np.float64) - rl.astype(np.float64)) / np.spacing(np.abs(rl)).astype(np.float64)).max())
    print(tag, "observed / bound:", {k: "%.3g" % v for k, v in fig.items()}, "logp elements that differ:", int(diff.sum()), "of", l.size)
    assert np.all(t[:, E.MI] >= 0), tag
    assert np.array_equal(l == -E.FLT_MAX, ra == 0) and np.all(np.isfinite(l)), tag
    if K > 1:
        top = np.sort(ra, axis=1)[:, -2:]
        clear = top[:, 1] - top[:, 0] > tol * top[:, 1]
        assert np.array_equal(t[clear, E.ARGMAX], rt[clear, E.ARGMAX]), tag
    else:
        assert np.all(t[:, E.ARGMAX] == 0), tag
    assert fig["logp_ulp"] <= 1, (tag, fig)
    for k in ("acc", "H_MEAN", "H_MEMBERS", "H_MEMBERS(stat)", "PEAK", "MI"):
        assert fig[k] <= 1, (tag, k, fig)


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("K", R.KS + (R.BIG_K,))
def test_kernels_against_the_float64_statement(K, scale):
    """Both kernels on normal logits of the given scale, M = 1, 2, 5 members (K = 32768: B = 2, M = 2), B = 3, n = 2, row0 = 5, ld = K + 3,
    a logits base one float off the 16-byte boundary, every buffer NaN before the first add; scale 1 has a -inf bin (a zero bin of the
    average), scale 30 a NaN logit.  Bounds of tests/ensref.py, per member added: acc, H_MEAN, H_MEMBERS, PEAK relative within
    (K + 16) 2^-52, MI within that times (H_MEAN + H_MEMBERS), ARGMAX equal where the reference's top two are further apart, logp within
    one fp32 ulp everywhere."""
    B, n, row0, ld = R.shape_of(K)
    for M in (R.MS if K != R.BIG_K else (2,)):
        z = R.member_logits(K, M, scale)
        _check("K=%d M=%d scale=%g" % (K, M, scale), _Case(K, B, n, row0, ld).run(z), R.reference(z), K, M, [0, 0])


def test_logp_differs_from_the_reference_in_at_most_the_cap():
    """Over all cases together, logp may differ at all from fl32(log(pbar_ref)) in at most 0.1 % of the elements: a cap, not a tolerance
    (the expected share is about 1e-5; tests/test_ensemble_cpu.py shows that the reference moved by the whole bound stays under it)."""
    differ = total = 0
    for K, M, scale in R.all_cases():
        B, n, row0, ld = R.shape_of(K)
        z = R.member_logits(K, M, scale)
        logp, rlogp = _Case(K, B, n, row0, ld).run(z)[2].cpu().numpy(), R.reference(z)[2]
        fin = np.isfinite(rlogp)
        assert np.array_equal(np.isnan(logp), np.isnan(rlogp))
        differ, total = differ + int((logp != rlogp)[fin].sum()), total + int(fin.sum())
    print("%d of %d logp elements differ from the reference (cap %g)" % (differ, total, R.CAP))
    assert differ <= R.CAP * total


@pytest.mark.parametrize("K", [63, 257, 4096])
def test_outputs_are_a_function_of_the_row_alone(K):
    """Two launches give equal bits; the row at (B, n, row0) = (3, 2, 5) in padded, misaligned rows and the same row alone at
    (1, 1, 0), packed and aligned, give equal bits in acc, stat, logp and the table -- the NaN row included."""
    M = 5
    z = R.member_logits(K, M, 30.0)
    first = [_bits(t) for t in _Case(K, 3, 2, 5, K + 3).run(z)]
    again = [_bits(t) for t in _Case(K, 3, 2, 5, K + 3).run(z)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    for r in (0, 1):
        for mis in (0, 2):
            alone = [_bits(t) for t in _Case(K, 1, 1, 0, K, misalign=mis).run(z[:, r:r + 1])]
            for a, b in zip(first, alone):
                assert np.array_equal(a[r], b[0]), (r, mis)


# ------------------------------------------------------------------ end to end
_CACHE = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("ensemble")


def _setup(workdir, regress_ori, regress_loc):
    """(cfg, model, dataset, [A, B, C]): an inference ResNet-18 at 128 x 192, engine batch 3, 7 images (two batches and a tail of one),
    and three member files written with save_weights: the model's weights and two copies with every kernel moved by 3 % of its spread."""
    key = (regress_ori, regress_loc)
    if key in _CACHE:
        return _CACHE[key]
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config("resnet18", 128, 192, batch=3, regress_ori=regress_ori, regress_loc=regress_loc, ori_bins=8, loc_bins=4, dtype="float32")
    cfg.NAME = "syn"
    d = workdir / ("m%d%d" % key)
    d.mkdir()
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(d))
    paths = [str(d / ("weights_%s_0001.npz" % c)) for c in "abc"]
    tr.save_weights(paths[0])
    del tr
    model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(d))
    model.load_weights(paths[0], paths[0], by_name=True)
    eng = model._engine
    base = eng.get_weights()
    rng = np.random.default_rng(11)
    for p in paths[1:]:
        moved = {ln: {wn: (a + 0.03 * a.std() * rng.normal(size=a.shape).astype(np.float32) if wn == "kernel" else a) for wn, a in ws.items()}
                 for ln, ws in base.items()}
        eng.set_weights(moved, strict=True)
        model.save_weights(p)
    eng.set_weights(base, strict=True)
    ds = SyntheticPoses(7, 128, 192, cfg, seed=3)
    ds._image_ids = np.array([3, 1, 4, 0, 6, 2, 5])
    _CACHE[key] = (cfg, model, ds, paths)
    return _CACHE[key]


def _weight_bits(model):
    eng = model._engine
    return eng.flat_w.detach().cpu().numpy().view(np.int32).copy(), eng.flat_stats.detach().cpu().numpy().view(np.int32).copy()


def _same(a, b, keys):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), k


PKEYS = ("image_ids", "loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda", "loc_spread", "ori_spread", "view_lambda", "n_views")
MKEYS = ("n_members", "member_loc_spread", "member_ori_spread", "member_lambda", "ori_entropy", "ori_member_entropy", "ori_mi", "loc_entropy",
         "loc_member_entropy", "loc_mi")


def _under(model, path, fn):
    """fn() with the weights of a member file in the model, which has its own back afterwards."""
    from ursonet_amd.net import read_weights_file
    eng = model._engine
    saved = eng.get_weights()
    try:
        eng.set_weights(read_weights_file(path), strict=True)
        return fn()
    finally:
        eng.set_weights(saved, strict=True)


def test_members_none_is_the_code_of_before(workdir, capsys):
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds, paths = _setup(workdir, False, True)
    p0 = pr.predict(model, ds)
    (workdir / "e0").mkdir(); (workdir / "e1").mkdir()
    e0 = ev.evaluate(model, ds, out_dir=str(workdir / "e0"))
    out0 = capsys.readouterr().out
    pr.predict(model, ds, members=paths)                                     # an ensemble call in between leaves nothing behind
    p1 = pr.predict(model, ds, members=None, max_gb=1e-9)
    e1 = ev.evaluate(model, ds, out_dir=str(workdir / "e1"), members=None)
    out1 = capsys.readouterr().out
    _same(p0, p1, PKEYS)
    _same(e0, e1, ("loc_est", "q_est", "loc_err", "ori_err", "esa", "dist", "loc_encoded_err", "ori_encoded_err"))
    assert out0 == out1 and len(out0.splitlines()) == 4
    for name in ev.CSV_FILES:
        assert (workdir / "e0" / name).read_bytes() == (workdir / "e1" / name).read_bytes()
    for r in (p0, p1, e0, e1):
        assert all(getattr(r, k) is None for k in MKEYS)


def test_regression_heads_pass_through_and_fuse(workdir):
    """One member: the bits of plain predict() under that member's weights (V == 1 passes through).  Three members: a NumPy fusion of
    three plain predict() calls, by test_views_gpu's comparison for fuse_ref."""
    from test_views_gpu import GAP, _close, fuse_ref
    from ursonet_amd import predict as pr
    cfg, model, ds, paths = _setup(workdir, True, True)
    before = _weight_bits(model)
    plain = [_under(model, p, lambda: pr.predict(model, ds)) for p in paths]
    assert not np.array_equal(plain[0].q_est, plain[1].q_est) and not np.array_equal(plain[1].loc_est, plain[2].loc_est)
    for j in (0, 1):
        one = pr.predict(model, ds, members=[paths[j]])
        assert np.array_equal(one.loc_est, plain[j].loc_est) and np.array_equal(one.q_est, plain[j].q_est)
        assert one.n_members == 1 and np.all(one.member_loc_spread == 0) and np.all(one.member_ori_spread == 0)
        assert one.ori_mi is None and one.loc_mi is None and one.ori_peak is None and one.n_views is None
    three = pr.predict(model, ds, members=paths)
    assert three.n_members == 3 and list(three.image_ids) == list(ds.image_ids)
    per = np.stack([np.concatenate([r.loc_est, r.q_est], axis=1) for r in plain])          # [3, N, 7]
    eye, qi = np.stack([np.eye(3)] * 3), np.stack([np.array([0.0, 0, 0, 1])] * 3)
    left_out = 0
    for i in range(per.shape[1]):
        ref = fuse_ref(per[:, i], eye, qi)
        assert np.abs(three.loc_est[i] - ref["loc"]).max() <= 1e-12 * np.linalg.norm(ref["loc"]), i
        assert _close(three.member_loc_spread[i], ref["loc_spread"]) and _close(three.member_lambda[i], ref["lam"]), i
        if ref["gap"] < GAP:
            left_out += 1
            continue
        assert 1 - abs(np.dot(three.q_est[i], ref["q"])) <= 1e-12, i
        assert _close(three.member_ori_spread[i], ref["ori_spread"]), (i, three.member_ori_spread[i], ref["ori_spread"])
    assert left_out <= 1 and np.all(three.member_ori_spread > 0)
    after = _weight_bits(model)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def _member_logits(model, ds, paths):
    """Per member, the engine's own outputs over the dataset at predict()'s batch composition: (loc [M, N, n_loc], ori [M, N, n_ori])."""
    from ursonet_amd.feeder import eval_batch_plan
    eng = model._engine

    def walk():
        locs, oris = [], []
        for _row0, n, slots in eval_batch_plan(ds.image_ids, eng.B):
            model.detect([ds.load_image(i) for i in slots])
            loc, ori = eng.outputs()
            locs.append(loc[:n].cpu().numpy().copy()); oris.append(ori[:n].cpu().numpy().copy())
        return np.concatenate(locs), np.concatenate(oris)
    got = [_under(model, p, walk) for p in paths]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def test_classification_heads_average_the_pmfs(workdir):
    """Soft orientation head and classified location: the per-member logits of the engine, averaged by add64 / settle64 and decoded by
    the float64 references of tests/poseref.py under their eigen-gap gate (no row may need excluding: the reference alone passes),
    against predict(members=...); the entropies within the kernel bounds; MI of three identical members at the bound, of distinct ones
    strictly above it."""
    from ursonet_amd import predict as pr
    cfg, model, ds, paths = _setup(workdir, False, False)
    loc_z, ori_z = _member_logits(model, ds, paths)
    Ko, Kl, M = ori_z.shape[2], loc_z.shape[2], 3
    r = pr.predict(model, ds, members=paths)
    assert r.n_members == 3 and r.loc_est.shape == (7, 3) and r.q_est.shape == (7, 4)
    _acc, _stat, logp_o, tab_o = R.reference(ori_z)
    _acc, _stat, logp_l, tab_l = R.reference(loc_z)
    # orientation: the decode of the averaged PMF
    hq = np.ascontiguousarray(ds.ori_histogram_map, dtype=np.float32)
    A, Mm = P.scatter(logp_o, hq)
    ratio, excl = P.gate_decode(r.q_est, Ko, A, Mm)
    print("q_est observed / bound", ratio, "excluded", int(excl.sum()), "gap", P.top_vector(A)[1])
    assert not excl.any() and ratio <= 1
    # location: softmax(logp) @ map, and the peak, as test_predict_gpu bounds them (1e-9 relative)
    loc_ref, peak_ref = P.loc_softmax(logp_l, np.asarray(ds.histogram_3D_map, dtype=np.float64))
    assert np.all(np.abs(r.loc_est - loc_ref) <= 1e-9 * np.abs(loc_ref)) and np.all(np.abs(r.loc_peak - peak_ref) <= 1e-9 * peak_ref)
    assert np.all(np.abs(r.ori_peak - P.peak(logp_o)) <= 1e-9 * P.peak(logp_o))
    assert np.all((r.ori_lambda >= 0.25 - 1e-6) & (r.ori_lambda <= 1 + 1e-6))
    # the entropies within the kernel bounds
    for name, tab, K in (("ori", tab_o, Ko), ("loc", tab_l, Kl)):
        tol = R.tol(K, M)
        h, hm, mi = (getattr(r, "%s_%s" % (name, k)) for k in ("entropy", "member_entropy", "mi"))
        fig = (np.abs(h - tab[:, E.H_MEAN]).max() / (tol * tab[:, E.H_MEAN].min()), np.abs(hm - tab[:, E.H_MEMBERS]).max() / (tol * tab[:, E.H_MEMBERS].min()),
               (np.abs(mi - tab[:, E.MI]) / (tol * (tab[:, E.H_MEAN] + tab[:, E.H_MEMBERS]))).max())
        print(name, "entropy, member entropy, MI observed / bound:", fig, "MI", mi)
        assert np.all(np.abs(h - tab[:, E.H_MEAN]) <= tol * tab[:, E.H_MEAN]) and np.all(np.abs(hm - tab[:, E.H_MEMBERS]) <= tol * tab[:, E.H_MEMBERS])
        assert np.all(np.abs(mi - tab[:, E.MI]) <= tol * (tab[:, E.H_MEAN] + tab[:, E.H_MEMBERS]))
        assert np.all(mi > tol * (h + hm)), name                              # distinct members: strictly above the bound
    same = pr.predict(model, ds, members=[paths[1]] * 3)
    for name, K in (("ori", Ko), ("loc", Kl)):
        h, hm, mi = (getattr(same, "%s_%s" % (name, k)) for k in ("entropy", "member_entropy", "mi"))
        assert np.all(mi >= 0) and np.all(mi <= R.tol(K, M) * (h + hm)), (name, mi)
    # identical poses: no spread beyond the fusion's own rounding (test_views_gpu's absolute bound for the spreads, 1e-9)
    assert np.all(same.member_ori_spread <= 1e-9) and np.all(same.member_loc_spread <= 1e-9)
    # multimodal: the modes are fitted on the averaged PMF, q_est stays the soft-argmax estimate
    mm = pr.predict(model, ds, members=paths, multimodal=True)
    assert np.array_equal(mm.q_est, r.q_est) and mm.modes.shape == (7, 3, 4) and np.all(mm.n_modes >= 1)
    from ursonet_amd import pose
    ref_modes = pose.fit_orientation_modes(logp_o, ds.ori_histogram_map, (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12, 5, 4)
    assert np.array_equal(mm.n_modes, ref_modes[4])


@pytest.mark.parametrize("regress_ori,regress_loc", [(True, True), (False, True), (False, False)])
def test_evaluate_has_predicts_estimate_and_its_own_errors(workdir, capsys, regress_ori, regress_loc):
    from test_views_gpu import _close, _errors
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds, paths = _setup(workdir, regress_ori, regress_loc)
    out_dir = workdir / ("ev%d%d" % (regress_ori, regress_loc))
    out_dir.mkdir()
    p = pr.predict(model, ds, members=paths)
    capsys.readouterr()
    e = ev.evaluate(model, ds, out_dir=str(out_dir), members=paths)
    lines = capsys.readouterr().out.splitlines()
    assert np.array_equal(e.loc_est, p.loc_est) and np.array_equal(e.q_est, p.q_est)
    _same(e, p, MKEYS)
    loc_gt = np.stack([np.asarray(ds.load_location(i), dtype=np.float64) for i in ds.image_ids])
    q_gt = np.stack([np.asarray(ds.load_quaternion(i), dtype=np.float64) for i in ds.image_ids])
    for i in range(7):
        want = _errors(e.loc_est[i], e.q_est[i], loc_gt[i], q_gt[i])
        for got, w in zip((e.loc_err[i], e.ori_err[i], e.esa[i], e.dist[i]), want):
            assert _close(got, w), (i, got, w)
    assert (e.loc_encoded_err is None) == regress_loc and (e.ori_encoded_err is None) == regress_ori
    plain = ev.evaluate(model, ds, out_dir=str(out_dir), verbose=0)
    if not regress_loc:
        assert np.array_equal(e.loc_encoded_err, plain.loc_encoded_err)       # the encoded errors do not depend on the estimate
    if not regress_ori:
        assert np.array_equal(e.ori_encoded_err, plain.ori_encoded_err)
    assert len(lines) == 5 and lines[:4] == ev.summary_lines(e.means()) and lines[4] == ev.ensemble_line(e)
    assert lines[4].startswith("Ensemble of 3 members: mean ") and ("orientation MI" in lines[4]) == (not regress_ori)
    for name in ev.CSV_FILES:
        assert (out_dir / name).exists()
    if not regress_ori:
        # multimodal: the modes predict() fits on the averaged PMF, picked by test_evaluate_gpu's rule; ORI_ERR_SOFT is the plain ensemble's
        from ursonet_amd import pose
        em = ev.evaluate(model, ds, out_dir=str(out_dir), verbose=0, members=paths, multimodal=True)
        pm = pr.predict(model, ds, members=paths, multimodal=True)
        err = pose.mode_errors(pm.modes, pm.n_modes, q_gt)
        pick = np.where((pm.n_modes == 1) | (err[:, 0] < err[:, 1]), 0, 1)
        assert np.array_equal(em.mode, pick) and np.array_equal(em.q_est, pm.modes[np.arange(7), pick].astype(np.float64))
        assert np.array_equal(em.ori_err_soft, e.ori_err) and np.array_equal(em.loc_est, e.loc_est)
        assert np.allclose(em.ori_err, err[np.arange(7), pick], rtol=1e-9, atol=1e-9)


def test_weights_come_back_after_the_call_and_after_an_exception(workdir):
    from ursonet_amd import evaluate as ev, predict as pr
    from ursonet_amd.net import read_weights_file, write_weights_file
    cfg, model, ds, paths = _setup(workdir, False, True)
    before = _weight_bits(model)
    pr.predict(model, ds, members=paths[1:])
    after = _weight_bits(model)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    params = read_weights_file(paths[2])
    dropped = sorted(params)[len(params) // 2]
    del params[dropped]
    short = str(workdir / "weights_short_0001.npz")
    write_weights_file(short, params)
    for fn, kw in ((pr.predict, {}), (ev.evaluate, dict(out_dir=str(workdir), verbose=0))):
        with pytest.raises(ValueError, match=r"member 1 lacks 1 layer\(s\) of the network: \['%s'\]" % dropped):
            fn(model, ds, members=[paths[1], short, paths[2]], **kw)
        after = _weight_bits(model)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # one member of a soft head: the decode of fl32(log softmax(z)) in the place of z, so the plain estimate up to that rounding and no
    # further -- |logp| 2^-24 on a weight, over an eigen-gap of order 1: far inside 1e-5 rad, the project's bound for the soft head
    a, b = pr.predict(model, ds), pr.predict(model, ds, members=[paths[0]])
    assert np.array_equal(a.loc_est, b.loc_est) and np.all(P.angle(a.q_est, b.q_est) <= 1e-5)


def test_submission_of_the_ensemble_and_the_size_refusal(workdir):
    from ursonet_amd import predict as pr, submission as sub
    from ursonet_amd.dataset import SyntheticPoses
    cfg, model, ds, paths = _setup(workdir, False, True)
    virt, real = SyntheticPoses(5, 128, 192, cfg, seed=6), SyntheticPoses(4, 128, 192, cfg, seed=7)
    for data, tag in ((virt, "v"), (real, "r")):
        data.ori_histogram_map = ds.ori_histogram_map
        for i, info in enumerate(data.image_info):
            info["path"] = "images/%s%06d.jpg" % (tag, 900 - 7 * i)
    rv, rr = sub.test_and_submit(model, virt, real, out_dir=str(workdir), suffix="ens", members=paths)
    want = sub.SubmissionWriter()
    for row in sub.submission_rows(pr.predict(model, virt, members=paths), virt, cfg):
        want.append_test(*row)
    for row in sub.submission_rows(pr.predict(model, real, members=paths), real, cfg):
        want.append_real_test(*row)
    ref = want.export(out_dir=str(workdir), suffix="ens_ref")
    assert (workdir / "submission_ens.csv").read_bytes() == open(ref, "rb").read()
    sub.test_and_submit(model, virt, real, out_dir=str(workdir), suffix="plain")
    assert (workdir / "submission_ens.csv").read_bytes() != (workdir / "submission_plain.csv").read_bytes()
    assert rv.n_members == rr.n_members == 3 and len(rv.image_ids) == 5 and len(rr.image_ids) == 4
    # 7 images x 512 bins x 8 bytes and the small tables: 0.000 GiB; the message names the figure and the limit
    before = _weight_bits(model)
    with pytest.raises(ValueError, match=r"accumulators of 7 images \(512 orientation and 0 location bins in fp64, 3 members' rows\) need 0\.000 GiB "
                                         r"on the device, more than max_gb = 1e-09"):
        pr.predict(model, ds, members=paths, max_gb=1e-9)
    assert np.array_equal(before[0], _weight_bits(model)[0])
