"""Conformal bounds on the GPU: urso_conf_score / urso_conf_bound through the C ABI against their statement in NumPy
(ursonet_amd.conformal.score64 / bound64; cases: tests/confref.py) -- integer columns and keys bit for bit, BOUND / ERR to 4 ulp (acos;
sqrt bit for bit) -- special rows, invariance, and conformal() / predict / evaluate with conformal=... end to end on the small model and
dataset of tests/test_calibrate_gpu.py.

The one place where device and NumPy may differ is exp (both good to 1 ulp): confref.fragile counts, per row, the bins whose
exp(d) 2^34 lies within 4 ulp of a rounding boundary, F.  Rows with F > 0 leave the bit comparison (|W - W_ref| <= F, the selected key
the reference's or a neighbouring distinct key); at most 2 % of the rows of a case may.  The seeds of confref.case have F = 0 on every row."""
import math

import numpy as np
import pytest
import torch

import confref as R
from ursonet_amd import calibrate as Cal
from ursonet_amd import conformal as Cf

pytestmark = pytest.mark.gpu
NAN = float("nan")
METRICS = (Cf.ANGLE, Cf.EUCLID)


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


class _Case(object):
    """The device buffers of one case, NaN wherever the kernels must neither read nor write: B rows of logits ld apart, `misalign`
    floats behind a 16-byte boundary; est in columns [3, 3 + D) of a table of 12 columns whose rows row0 .. hold the batch; the truth
    [B, D]; the out table with guard rows in front of row0 and behind row0 + n."""

    def __init__(self, K, metric, B, n, row0, ld, misalign):
        self.K, self.metric, self.B, self.n, self.row0, self.D = K, metric, B, n, row0, R.D[metric]
        self.rows = row0 + B + 1
        self.zstore = torch.full((B * ld + 8,), NAN, dtype=torch.float32, device="cuda")
        self.logits = self.zstore[misalign:misalign + B * ld].view(B, ld)[:, :K]
        assert self.logits.data_ptr() % 16 == 4 * (misalign % 4)
        self.table = torch.full((self.rows, 12), NAN, dtype=torch.float64, device="cuda")
        self.est = self.table[:, 3:3 + self.D]
        self.ref = torch.full((B, self.D), NAN, dtype=torch.float64, device="cuda")
        self.out = torch.full((self.rows, Cf.COLS), NAN, dtype=torch.float64, device="cuda")

    def load(self, z, m, est, ref):
        self.logits[:self.n] = _dev(z)
        self.map = _dev(m)
        self.est[self.row0:self.row0 + self.n] = _dev(est)
        self.ref[:self.n] = _dev(ref)
        return self

    def _rows(self):
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        keep = np.ones(self.rows, dtype=bool)
        keep[self.row0:self.row0 + self.n] = False
        assert np.all(np.isnan(out[keep])), "a row outside [row0, row0 + n) was written"
        return out[self.row0:self.row0 + self.n].copy()

    def score(self):
        from ursonet_amd import hip
        self.out.fill_(NAN)
        hip.conf_score(self.B, self.n, self.row0, self.metric, self.logits, self.map, self.est, self.ref, self.out)
        return self._rows()

    def bound(self, q):
        from ursonet_amd import hip
        self.out.fill_(NAN)
        hip.conf_bound(self.B, self.n, self.row0, self.metric, q, self.logits, self.map, self.est, self.out)
        return self._rows()


def _check_score(got, want, F):
    exact = F == 0
    assert np.array_equal(R.bits(got[exact][:, [Cf.SCORE, Cf.C_MASS, Cf.W_SUM, Cf.KEY_REF, Cf.NEAR, 6, 7]]),
                          R.bits(want[exact][:, [Cf.SCORE, Cf.C_MASS, Cf.W_SUM, Cf.KEY_REF, Cf.NEAR, 6, 7]]))
    assert np.array_equal(R.bits(got[:, [Cf.KEY_REF, Cf.NEAR]]), R.bits(want[:, [Cf.KEY_REF, Cf.NEAR]]))       # these do not depend on exp
    assert np.all(np.abs(got[:, Cf.W_SUM] - want[:, Cf.W_SUM]) <= F) and np.all(np.abs(got[:, Cf.C_MASS] - want[:, Cf.C_MASS]) <= F)
    return R.ulps(got[:, Cf.ERR], want[:, Cf.ERR]).max()


def _check_bound(got, want, F, metric, keys):
    exact = F == 0
    cols = [Cf.KEY, Cf.MASS, Cf.COUNT, Cf.BOUND_W, 5, 6, 7]
    assert np.array_equal(R.bits(got[exact][:, cols]), R.bits(want[exact][:, cols]))
    for b in np.flatnonzero(~exact):                               # the reference's key or a neighbouring distinct one
        distinct = np.unique(Cf.ranks(metric, keys[b]))
        pos = [int(np.searchsorted(distinct, Cf.ranks(metric, np.array([k]))[0])) for k in (got[b, Cf.KEY], want[b, Cf.KEY])]
        assert abs(got[b, Cf.BOUND_W] - want[b, Cf.BOUND_W]) <= F[b] and (np.isnan(want[b, Cf.KEY]) or abs(pos[0] - pos[1]) <= 1)
    return R.ulps(got[:, Cf.BOUND], want[:, Cf.BOUND]).max()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K", R.KS)
def test_kernels_against_the_numpy_statement(K, metric):
    """Both kernels on seeded normal logits (sigma 2 .. 6), rows at ld = K + 1 off the 16-byte boundary and at ld = K, B > n, row0 = 5,
    every buffer NaN around the valid elements; the levels 1e-12, 0.5, 0.9, 1, +inf and every row's own score (where it is > 0: the entry
    point refuses q = 0)."""
    B, n, row0 = R.rows_of(K)
    z, m, est, ref = R.case(K, metric)
    F = R.fragile(z)
    assert np.sum(F > 0) <= 0.02 * n, F
    keys = Cf.keys64(metric, m, est)
    want_s = Cf.score64(z, m, est, ref, metric)
    qs = R.QS + tuple(float(x) for x in want_s[:, Cf.SCORE] if x > 0)
    want_b = dict((q, Cf.bound64(z, m, est, metric, q)) for q in qs)
    worst = 0.0
    for ld, mis in ((K + 1, 1), (K, 0)):
        case = _Case(K, metric, B, n, row0, ld, mis).load(z, m, est, ref)
        worst = max(worst, _check_score(case.score(), want_s, F))
        for q in qs:
            worst = max(worst, _check_bound(case.bound(q), want_b[q], F, metric, keys))
        pad = case.zstore.cpu().numpy().copy()
        body = pad[mis:mis + B * ld].reshape(B, ld)[:n, :K]
        assert np.array_equal(body.view(np.int32), z.view(np.int32)), "the logits were written"
        body[...] = NAN
        assert np.all(np.isnan(pad)), "the padding of the logits was written"
    print("K=%d metric=%d: F=%s, BOUND / ERR worst %.3g ulp over %d levels" % (K, metric, F.tolist(), worst, len(qs)))
    assert worst <= (4 if metric == Cf.ANGLE else 0)


@pytest.mark.parametrize("metric", METRICS)
def test_special_rows(metric):
    """All logits equal; one finite logit among -inf; a NaN logit, a +inf logit, an all -inf row, a NaN in est and an inf in ref (only
    those rows become NaN); est on a map entry (the key clamps to 1 / is 0: bound 0); the map of confref has duplicate and flipped entries."""
    K, n = 27, 8
    z, m, est, ref = R.case(K, metric, seed=3)
    z[0, :] = 1.5
    z[1, :] = -np.inf
    z[1, 11] = -3.0
    z[2, 3], z[3, 0], z[4, :] = np.nan, np.inf, -np.inf
    est[5, 2], ref[6, 1] = np.nan, np.inf
    est[7] = m[4].astype(np.float64) * (1.0 + 2.0 ** -20 if metric == Cf.ANGLE else 1.0)   # (an fp32 unit vector's norm is 1 to 2^-24 only)
    ref[7] = est[7]
    case = _Case(K, metric, n + 1, n, 2, K + 1, 1).load(z, m, est, ref)
    want = Cf.score64(z, m, est, ref, metric)
    got = case.score()
    assert np.all(np.isnan(got[[2, 3, 4, 5, 6]])) and np.all(np.isfinite(got[[0, 1, 7]]))
    assert np.array_equal(R.bits(got[[0, 1, 7]][:, [0, 1, 2, 3, 5, 6, 7]]), R.bits(want[[0, 1, 7]][:, [0, 1, 2, 3, 5, 6, 7]]))
    assert got[0, Cf.W_SUM] == K * 2.0 ** 34 and got[1, Cf.W_SUM] == 2.0 ** 34 and got[7, Cf.ERR] == 0 and got[7, Cf.SCORE] == 0
    for q in (1e-12, 0.5, 1.0):
        want, got = Cf.bound64(z, m, est, metric, q), case.bound(q)
        assert np.all(np.isnan(got[[2, 3, 4, 5]])) and np.all(np.isfinite(got[[0, 1, 6, 7]][:, [Cf.MASS, Cf.COUNT, Cf.BOUND_W]]))
        ok = [0, 1, 6, 7]
        assert np.array_equal(R.bits(got[ok][:, 1:]), R.bits(want[ok][:, 1:])) and R.ulps(got[ok, 0], want[ok, 0]).max() <= 4
        if q < 1:
            assert got[1, Cf.MASS] == 1 and R.bits(got[1, Cf.KEY]) == R.bits(Cf.keys64(metric, m, est[1:2])[0, 11])
        if q == 1e-12:
            assert got[7, Cf.BOUND] == 0 and got[7, Cf.KEY] == (1.0 if metric == Cf.ANGLE else 0.0) and got[7, Cf.COUNT] >= 2    # m[4] has a copy


@pytest.mark.parametrize("K", [27, 4099])
def test_a_row_gives_the_same_bits_wherever_it_lies(K):
    """Two launches give equal bits; every row of a batch of 8 in padded, misaligned rows and the same row alone at (B, n, row0) =
    (1, 1, 0), packed and aligned, give equal bits."""
    for metric in METRICS:
        z, m, est, ref = R.case(K, metric, seed=4)
        n = len(z)
        batch = _Case(K, metric, n + 2, n, 5, K + 1, 3).load(z, m, est, ref)
        s0, b0 = batch.score(), batch.bound(0.9)
        assert np.array_equal(R.bits(s0), R.bits(batch.score())) and np.array_equal(R.bits(b0), R.bits(batch.bound(0.9)))
        for r in (0, n // 2, n - 1):
            alone = _Case(K, metric, 1, 1, 0, K, 0).load(z[r:r + 1], m, est[r:r + 1], ref[r:r + 1])
            assert np.array_equal(R.bits(alone.score()[0]), R.bits(s0[r])) and np.array_equal(R.bits(alone.bound(0.9)[0]), R.bits(b0[r])), (metric, r)


def test_refusals_launch_nothing():
    """Every URSO_EINVAL of tests/test_conformal_cpu.py's list comes before the launch: with real buffers, the out table stays NaN."""
    import ctypes as C
    from ursonet_amd import hip
    K, metric = 27, Cf.ANGLE
    z, m, est, ref = R.case(K, metric)
    case = _Case(K, metric, 9, 8, 0, K + 1, 1).load(z, m, est, ref)
    case.out.fill_(NAN)
    lib = hip.side_lib("infer")

    def args(cls, **kw):
        a = cls()
        a.B, a.n, a.row0, a.K, a.metric = 9, 8, 0, K, metric
        a.logits, a.ld_z = hip._rows(case.logits)
        a.est, a.ld_est = hip._rows(case.est)
        a.map, a.out = hip.ptr(case.map), hip.ptr(case.out)
        if cls is hip.ConfScoreArgs:
            a.ref, a.ld_ref = hip._rows(case.ref)
        else:
            a.q = 0.9
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    common = [dict(logits=None), dict(map=None), dict(est=None), dict(out=None), dict(n=-1), dict(n=10), dict(row0=-1), dict(K=0), dict(K=2 ** 18 + 1),
              dict(ld_z=K - 1), dict(metric=2), dict(ld_est=3), dict(logits=case.logits.data_ptr() + 2), dict(est=case.est.data_ptr() + 4),
              dict(out=case.out.data_ptr() + 4), dict(map=case.map.data_ptr() + 8)]
    for kw in common + [dict(ref=None), dict(ld_ref=3), dict(ref=case.ref.data_ptr() + 4)]:
        assert lib.urso_conf_score(C.byref(args(hip.ConfScoreArgs, **kw)), hip.stream_ptr()) == -1, kw
    for kw in common + [dict(q=0.0), dict(q=-1.0), dict(q=NAN)]:
        assert lib.urso_conf_bound(C.byref(args(hip.ConfBoundArgs, **kw)), hip.stream_ptr()) == -1, kw
    assert lib.urso_conf_score(C.byref(args(hip.ConfScoreArgs, n=0)), hip.stream_ptr()) == 0
    assert lib.urso_conf_bound(C.byref(args(hip.ConfBoundArgs, n=0)), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(case.out).all()), "a refused call or n = 0 wrote"


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("conformal")


def _setup(workdir, regress_loc):
    from test_calibrate_gpu import _setup as setup
    return setup(workdir, regress_loc)


EKEYS = ("image_ids", "loc_est", "q_est", "loc_err", "ori_err", "esa", "dist", "loc_encoded_err", "ori_encoded_err")
PKEYS = ("image_ids", "loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda")


def _same(a, b, keys):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), k


def test_conformal_then_evaluate_covers_its_own_images(workdir, capsys):
    """Soft orientation head and location classification (8^3 and 4^3 bins, 7 images, engine batch 3).  conformal() followed by
    evaluate(conformal=cf) on the same images covers at least k = ceil((n + 1)(1 - alpha)) of them -- exactly, by the equivalence
    SCORE <= q <=> covered -- and the covered flag is the comparison of the keys; predict(conformal=cf) gives the same bound bits; the
    scores are score64 of the engine's own logits; conformal=None is the code of before, bit for bit; a line is printed."""
    from ursonet_amd import evaluate as ev, predict as pr
    from test_calibrate_gpu import _engine_logits
    cfg, model, ds = _setup(workdir, False)
    alpha, n = 0.4, 7
    k = math.ceil((n + 1) * (1 - alpha))
    assert k == 5
    cf = Cf.conformal(model, ds, alpha=alpha)
    assert cf.ori_kind == cf.loc_kind == "pmf" and cf.k_ori == 512 and cf.k_loc == 64 and cf.n_images == 7 and cf.ori_beta is None
    assert cf.ori_q == cf.ori_scores[k - 1] and cf.loc_q == cf.loc_scores[k - 1]
    for sub in ("e0", "e1"):
        (workdir / sub).mkdir()
    capsys.readouterr()
    e0 = ev.evaluate(model, ds, out_dir=str(workdir / "e0"))
    lines0 = capsys.readouterr().out.splitlines()
    e = ev.evaluate(model, ds, out_dir=str(workdir / "e1"), conformal=cf)
    lines = capsys.readouterr().out.splitlines()
    _same(e0, e, EKEYS)
    _same(e0, ev.evaluate(model, ds, out_dir=str(workdir / "e0"), verbose=0, conformal=None), EKEYS)
    assert e0.ori_bound is None and e0.ori_covered is None and e0.loc_region_bins is None
    assert len(lines0) == 4 and len(lines) == 5 and lines[:4] == lines0 and lines[4] == cf.line(e)
    assert lines[4].startswith("Conformal: target coverage 0.6 on 7 calibration images; orientation coverage ")
    print(lines[4])
    # the scores are those of the engine's logits around the table's estimates
    loc_z, ori_z = _engine_logits(model, ds)
    q_gt = np.stack([np.asarray(ds.load_quaternion(i), dtype=np.float64) for i in ds.image_ids])
    loc_gt = np.stack([np.asarray(ds.load_location(i), dtype=np.float64) for i in ds.image_ids])
    hq, lmap = np.ascontiguousarray(ds.ori_histogram_map, dtype=np.float32), np.asarray(ds.histogram_3D_map, dtype=np.float64)
    for head, z, m, est, gt, metric, err in (("ori", ori_z, hq, e.q_est, q_gt, Cf.ANGLE, e.ori_err), ("loc", loc_z, lmap, e.loc_est, loc_gt, Cf.EUCLID, e.loc_err)):
        F = R.fragile(z)
        s, q = Cf.score64(z, m, est, gt, metric), getattr(cf, head + "_q")
        b = Cf.bound64(z, m, est, metric, q)
        scores = getattr(cf, head + "_scores")
        if not F.any():
            assert scores == sorted(s[:, Cf.SCORE].tolist()), head
            assert np.array_equal(R.bits(getattr(e, head + "_bound")), R.bits(b[:, Cf.BOUND])) or R.ulps(getattr(e, head + "_bound"), b[:, Cf.BOUND]).max() <= 4
            assert np.array_equal(getattr(e, head + "_region_bins"), b[:, Cf.COUNT]) and np.array_equal(getattr(e, head + "_region_mass"), b[:, Cf.MASS])
        covered = getattr(e, head + "_covered")
        print(head, "level", q, "covered", int(covered.sum()), "of", n, "bounds", getattr(e, head + "_bound"), "errors", err)
        assert covered.sum() >= k, head
        assert np.array_equal(covered, np.array([(kr >= kb if metric == Cf.ANGLE else kr <= kb) for kr, kb in zip(s[:, Cf.KEY_REF], b[:, Cf.KEY])])) or F.any()
        assert np.allclose(s[:, Cf.ERR], err, rtol=1e-9, atol=0)                   # the value of the truth's key is the error the table reports
    # predict: the same bounds, and nothing else changes
    p0, p = pr.predict(model, ds), pr.predict(model, ds, conformal=cf)
    _same(p0, p, PKEYS)
    _same(p0, pr.predict(model, ds, conformal=None), PKEYS)
    assert p0.ori_bound is None and p0.loc_region_mass is None
    for f in ("ori_bound", "loc_bound", "ori_region_bins", "loc_region_bins", "ori_region_mass", "loc_region_mass"):
        assert np.array_equal(R.bits(getattr(p, f)), R.bits(getattr(e, f))), f
    # a Conformal file comes back and applies; another alpha from the same scores
    again = Cf.Conformal.load(cf.save(str(workdir / "cf.json")))
    assert again == cf
    wide = pr.predict(model, ds, conformal=again.at(0.2))                          # k = 7 of 7: the largest score
    assert np.all(wide.ori_bound >= p.ori_bound) and np.all(wide.loc_bound >= p.loc_bound)
    everything = pr.predict(model, ds, conformal=again.at(0.05))                   # k = 8 > n: the level is +inf
    assert np.all(everything.ori_bound == 180) and np.all(np.isinf(everything.loc_bound)) and np.all(everything.ori_region_bins == 512)


def test_calibration_and_conformal_go_together_or_not_at_all(workdir):
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds = _setup(workdir, False)
    cal = Cal.Calibration(ori_beta=2.0, loc_beta=0.5)
    plain, under = Cf.conformal(model, ds, alpha=0.4), Cf.conformal(model, ds, alpha=0.4, calibration=cal)
    assert (under.ori_beta, under.loc_beta) == (2.0, 0.5) and under.ori_scores != plain.ori_scores
    e = ev.evaluate(model, ds, out_dir=str(workdir), verbose=0, calibration=cal, conformal=under)
    assert e.ori_covered.sum() >= 5 and e.loc_covered.sum() >= 5
    assert np.array_equal(e.q_est, pr.predict(model, ds, calibration=cal).q_est)
    with pytest.raises(ValueError, match=r"fitted under the calibration betas \(ori None, loc None\), but calibration= gives \(ori 2.0, loc 0.5\)"):
        pr.predict(model, ds, calibration=cal, conformal=plain)
    with pytest.raises(ValueError, match=r"fitted under the calibration betas \(ori 2.0, loc 0.5\), but calibration= gives \(ori None, loc None\)"):
        ev.evaluate(model, ds, out_dir=str(workdir), verbose=0, conformal=under)
    with pytest.raises(ValueError, match="whose orientation head has 4096 bins, this model's has 512 bins"):
        d = plain.to_dict()
        d["k_ori"] = 4096
        pr.predict(model, ds, conformal=Cf.Conformal(**d))


def test_a_regression_head_gets_the_constant_quantile(workdir):
    """REGRESS_LOC: the location scores are the errors of the EVAL table, the bound is the host quantile for every image, and the
    orientation head keeps its PMF bound."""
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds = _setup(workdir, True)
    e0 = ev.evaluate(model, ds, out_dir=str(workdir), verbose=0)
    cf = Cf.conformal(model, ds, alpha=0.4)
    assert cf.loc_kind == "error" and cf.ori_kind == "pmf" and cf.k_loc == 0 and cf.loc_scores == sorted(e0.loc_err.tolist())
    assert cf.loc_q == Cf.quantile(e0.loc_err, 0.4) == sorted(e0.loc_err.tolist())[4]
    e, p = ev.evaluate(model, ds, out_dir=str(workdir), verbose=0, conformal=cf), pr.predict(model, ds, conformal=cf)
    for r in (e, p):
        assert np.all(r.loc_bound == cf.loc_q) and r.loc_bound.shape == (7,) and r.loc_region_bins is None and r.loc_region_mass is None
        assert r.ori_region_bins is not None and np.all(r.ori_bound >= 0)
    assert np.array_equal(e.loc_covered, e0.loc_err <= cf.loc_q) and e.loc_covered.sum() == 5 and e.ori_covered.sum() >= 5
    few = Cf.conformal(model, ds, alpha=0.4, nr_images=4)
    assert few.n_images == 4 and few.loc_scores == sorted(e0.loc_err[:4].tolist()) and few.loc_q == sorted(e0.loc_err[:4].tolist())[2]
