"""Domain-shift scores on the GPU: urso_feat_pool / urso_feat_gram_add / urso_feat_maha through the C ABI against their statements in
NumPy (ursonet_amd.domain.pool64 / gram_add64 / maha64), bit for bit -- no transcendental function is involved, so no row is excused and
there is no tolerance -- and fit_domain() / predict / evaluate with domain=... end to end on the small model of
tests/test_calibrate_gpu.py (inference ResNet-18 at 128 x 192, fp32, engine batch 3, bottleneck 32: features of 2 x 3 cells) over 40
images, which ends in a tail batch of one.  Buffers are NaN wherever a kernel must neither read nor write, with guard rows in front of
row0 and behind row0 + n."""
import numpy as np
import pytest
import torch

from ursonet_amd import calibrate as Cal
from ursonet_amd import conformal as Cf
from ursonet_amd import domain as Dm
from util import make_config

pytestmark = pytest.mark.gpu
NAN = float("nan")
DS = (1, 3, 64, 65, 130, 512)
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def _same_bits(got, want, what=""):
    assert np.array_equal(bits(got), bits(want)), what


# ------------------------------------------------------------------ pool
def _grids(h, w):
    return [(gh, gw) for gh in range(1, h + 1) if h % gh == 0 for gw in range(1, w + 1) if w % gw == 0]


@pytest.mark.parametrize("dt", sorted(TORCH_DT))
@pytest.mark.parametrize("geo", [(2, 3, 32), (2, 3, 5), (8, 10, 128), (4, 4, 33)])
def test_pool_is_pool64(geo, dt):
    """Every grid that divides, (1, 1) and (h, w) included (a grid whose D exceeds 4096 is refused and writes nothing); n in {1, B - 1, B}
    for B = 3 and 32; row0 = 2 in a table with a padded leading dimension; the batch rows behind n are NaN and must not show up."""
    from ursonet_amd import hip
    h, w, Cc = geo
    rng = np.random.RandomState(h * 100 + Cc)
    full = torch.as_tensor((rng.randn(32, h, w, Cc) * 10 ** rng.uniform(-2, 2, (32, h, w, Cc))).astype(np.float32)).to(TORCH_DT[dt]).cuda()
    host = full.float().cpu().numpy()                                               # the conversion to fp32 (and on to fp64) is exact
    launches = 0
    for grid in _grids(h, w):
        D = grid[0] * grid[1] * Cc
        if D > Dm.MAX_D:
            tab = _nan(4, D)
            with pytest.raises(hip.UrsoHipError, match="need 1 <= D <= 4096"):
                hip.feat_pool(3, 3, 0, grid, full[:3].contiguous(), tab)
            assert bool(torch.isnan(tab).all())
            continue
        want = Dm.pool64(host, grid)
        for B in (3, 32):
            for n in sorted({1, B - 1, B}):
                row0 = 2
                act = full[:B].clone()
                act[n:] = NAN                                                       # stale rows of a tail batch
                store = _nan(row0 + B + 1, D + 3)
                hip.feat_pool(B, n, row0, grid, act, store[:, :D])
                got = store.cpu().numpy()
                launches += 1
                _same_bits(got[row0:row0 + n, :D], want[:n], (grid, B, n))
                got[row0:row0 + n, :D] = NAN
                assert np.all(np.isnan(got)), ("written outside the valid rows and columns", grid, B, n)
    print(geo, dt, launches, "launches")


def test_pool_passes_non_finite_values_through():
    from ursonet_amd import hip
    rng = np.random.RandomState(2)
    host = rng.randn(3, 4, 4, 8).astype(np.float32)
    host[0, 1, 2, 3], host[2, 3, 3, 7], host[1, 0, 0, 0] = np.nan, np.inf, -np.inf
    for grid in ((1, 1), (2, 2), (4, 4)):
        out = _nan(3, grid[0] * grid[1] * 8)
        hip.feat_pool(3, 3, 0, grid, torch.as_tensor(host).cuda(), out)
        want = Dm.pool64(host, grid)
        got = out.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
        assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])


# ------------------------------------------------------------------ gram
class _Gram(object):
    """The accumulators of one case: s [D], G in a store [D, D + 2] whose strict lower triangle and padding are NaN and whose upper
    triangle starts at given values; a non-zero centre."""

    def __init__(self, D, seed):
        rng = np.random.RandomState(seed)
        self.D = D
        self.centre = rng.randn(D) + 2.0
        self.s0, self.G0 = rng.randn(D), np.triu(rng.randn(D, D))
        store = np.full((D, D + 2), NAN)
        store[:, :D] = np.where(np.triu(np.ones((D, D), dtype=bool)), self.G0, NAN)
        self.store, self.s, self.c = _dev(store), _dev(self.s0), _dev(self.centre)
        self.s_ref, self.G_ref = self.s0.copy(), self.G0.copy()

    def add(self, X, B, row0=2):
        """n = len(X) valid rows of a batch of B, in a table with guard rows and a padded leading dimension, NaN around the valid rows."""
        from ursonet_amd import hip
        n = len(X)
        x = _nan(row0 + B + 1, self.D + 1)
        x[row0:row0 + n, :self.D] = _dev(X)
        hip.feat_gram_add(B, n, row0, x[:, :self.D], self.c, self.s, self.store[:, :self.D])
        Dm.gram_add64(X, self.centre, self.s_ref, self.G_ref)
        return self

    def check(self, what=""):
        torch.cuda.synchronize()
        got, D = self.store.cpu().numpy(), self.D
        up = np.triu(np.ones((D, D), dtype=bool))
        assert np.all(np.isnan(got[:, D:])) and np.all(np.isnan(got[:, :D][~up])), ("the strict lower triangle or the padding was written", what)
        assert np.array_equal(bits(got[:, :D][up]), bits(self.G_ref[up])), ("G", what)
        assert np.array_equal(bits(self.s.cpu().numpy()), bits(self.s_ref)), ("s", what)
        return got[:, :D][up], self.s.cpu().numpy()


@pytest.mark.parametrize("D", DS)
def test_gram_add_is_gram_add64(D):
    """Three calls with n in {B, B - 1, 1} into one accumulator (B = 5, and B = 37: more than one stage of 32 rows)."""
    for B in (5, 37):
        rng = np.random.RandomState(D + B)
        case = _Gram(D, seed=D)
        for n in (B, B - 1, 1):
            case.add(rng.randn(n, D) * 3.0 + 2.0, B).check((D, B, n))


@pytest.mark.parametrize("D", DS)
def test_gram_add_does_not_depend_on_the_batching(D):
    """The same 7 rows added as 3 + 3 + 1 and as 7 give the same bits."""
    X = np.random.RandomState(D).randn(7, D) + 1.0
    a, b = _Gram(D, seed=1), _Gram(D, seed=1)
    a.add(X[:3], 3).add(X[3:6], 3).add(X[6:], 3)
    b.add(X, 7)
    ga, sa = a.check()
    gb, sb = b.check()
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(sa), bits(sb))


@pytest.mark.parametrize("D", [3, 65, 130])
def test_a_nan_feature_poisons_exactly_what_it_touches(D):
    X = np.random.RandomState(D).randn(6, D)
    k = D // 2
    X[4, k] = NAN
    case = _Gram(D, seed=2).add(X, 8)
    torch.cuda.synchronize()
    got = case.store.cpu().numpy()[:, :D]
    want = np.zeros((D, D), dtype=bool)
    want[k, k:], want[:k + 1, k] = True, True
    up = np.triu(np.ones((D, D), dtype=bool))
    assert np.array_equal(np.isnan(got) & up, want) and np.array_equal(np.isnan(case.s.cpu().numpy()), np.arange(D) == k)
    keep = up & ~want
    assert np.array_equal(bits(got[keep]), bits(case.G_ref[keep]))


# ------------------------------------------------------------------ maha
def _maha_case(D, n, seed):
    rng = np.random.RandomState(seed)
    W = np.tril(rng.randn(D, D)) / np.sqrt(D)
    return rng.randn(n, D) * 2.0 + 1.0, rng.randn(D) + 1.0, W + np.triu(np.full((D, D), NAN), 1)


def _maha(X, mean, W, B, row0=3, slot0=0):
    """urso_feat_maha on the rows X placed at the batch slots slot0 .. of a batch of B (NaN elsewhere; n = slot0 + len(X), the slots in front
    of slot0 hold finite filler), W transposed into a store with a padded leading dimension; -> the out rows of X's slots."""
    from ursonet_amd import hip
    D, n = len(mean), slot0 + len(X)
    x = _nan(B, D + 1)
    x[:slot0, :D] = 0.5
    x[slot0:n, :D] = _dev(X)
    wt = _nan(D, D + 3)
    wt[:, :D] = _dev(np.asarray(W).T)
    out = _nan(row0 + B + 1, Dm.COLS)
    hip.feat_maha(B, n, row0, x[:, :D], _dev(mean), wt[:, :D], out)
    got = out.cpu().numpy()
    rows = got[row0 + slot0:row0 + n].copy()
    got[row0:row0 + n] = NAN
    assert np.all(np.isnan(got)), "a row outside [row0, row0 + n) was written"
    return rows


@pytest.mark.parametrize("D", DS)
def test_maha_is_maha64(D):
    """All four columns bit for bit, a random lower-triangular W with NaN above the diagonal; B = 11 (two workgroups of 8 rows), n in
    {B, B - 1, 1}; a non-finite row gives four NaNs and leaves its neighbours alone; a row's result does not depend on its slot."""
    X, mean, W = _maha_case(D, 11, seed=D)
    want = Dm.maha64(X, mean, W)
    assert np.all(np.isfinite(want))
    for n in (11, 10, 1):
        _same_bits(_maha(X[:n], mean, W, 11), want[:n], (D, n))
    Xb = X.copy()
    Xb[2, D // 2], Xb[9, D - 1] = np.inf, NAN
    got = _maha(Xb, mean, W, 11)
    ok = [r for r in range(11) if r not in (2, 9)]
    assert np.all(np.isnan(got[[2, 9]]))
    _same_bits(got[ok], want[ok], "the neighbours of a non-finite row")
    alone = _maha(X[5:6], mean, W, 1, row0=0)
    late = _maha(X[5:6], mean, W, 16, slot0=13)
    _same_bits(alone, want[5:6], "slot 0 of 1")
    _same_bits(late, want[5:6], "slot 13 of 16")


def test_maha_tie_returns_the_lower_index():
    D = 70
    d = np.zeros((2, D))
    d[0, [3, 40, 69]] = -2.0, 2.0, 2.0
    d[1, [68, 69]] = 1.5, -1.5
    got = _maha(d + 1.0, np.ones(D), np.eye(D), 2)
    assert got[0].tolist() == [12.0, 12.0, 2.0, 3.0] and got[1].tolist() == [4.5, 4.5, 1.5, 68.0]
    _same_bits(got, Dm.maha64(d + 1.0, np.ones(D), np.eye(D)))


def test_refusals_launch_nothing():
    import ctypes as C
    from ursonet_amd import hip
    lib = hip.side_lib("feat")
    D = 8
    x, mean, wt, out, s, g = _nan(4, D), _nan(D), _nan(D, D), _nan(6, Dm.COLS), _nan(D), _nan(D, D)
    act, tab = torch.full((4, 2, 2, 2), NAN, device="cuda"), _nan(6, D)
    cases = []
    for kw in (dict(n=5), dict(n=-1), dict(row0=-1), dict(D=0), dict(ld_x=7), dict(ld_w=7), dict(out=None), dict(x=x.data_ptr() + 4)):
        a = hip.FeatMahaArgs(B=4, n=4, row0=0, D=D, pad=0, ld_x=D, ld_w=D, x=x.data_ptr(), mean=mean.data_ptr(), wt=wt.data_ptr(), out=out.data_ptr())
        cases.append((lib.urso_feat_maha, a, kw))
    for kw in (dict(n=5), dict(row0=-1), dict(D=4097), dict(ld_g=7), dict(s=None), dict(g=g.data_ptr() + 4)):
        a = hip.FeatGramArgs(B=4, n=4, row0=0, D=D, pad=0, ld_x=D, ld_g=D, x=x.data_ptr(), centre=mean.data_ptr(), s=s.data_ptr(), g=g.data_ptr())
        cases.append((lib.urso_feat_gram_add, a, kw))
    for kw in (dict(n=5), dict(row0=-1), dict(gh=3), dict(gw=0), dict(dtype=7), dict(ld=7), dict(act=None), dict(out=tab.data_ptr() + 4)):
        a = hip.FeatPoolArgs(B=4, n=4, row0=0, h=2, w=2, C=2, gh=2, gw=2, dtype=hip.F32, ld=D, act=act.data_ptr(), out=tab.data_ptr())
        cases.append((lib.urso_feat_pool, a, kw))
    for fn, a, kw in cases:
        for k, v in kw.items():
            setattr(a, k, v)
        assert fn(C.byref(a), hip.stream_ptr()) == -1, kw
        if "n" not in kw:
            a.n = 0
            assert fn(C.byref(a), hip.stream_ptr()) == -1, kw                       # the refusals come in front of n == 0
    torch.cuda.synchronize()
    for t in (out, s, g, tab):
        assert bool(torch.isnan(t).all()), "a refused call wrote"


# ------------------------------------------------------------------ end to end
_CACHE = {}
N_IMAGES, N_HOLDOUT = 40, 10


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("domain")


def _setup(workdir):
    """(cfg, model, dataset, holdout, X, Xh): the model of tests/test_calibrate_gpu.py (both heads classify), 40 images and 10 held-out ones,
    and their feature tensors [N, 2, 3, 32] read from Engine.features() batch by batch at predict()'s batch composition."""
    if "m" in _CACHE:
        return _CACHE["m"]
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.feeder import eval_batch_plan
    cfg = make_config("resnet18", 128, 192, batch=3, regress_ori=False, regress_loc=False, ori_bins=8, loc_bins=4, dtype="float32")
    cfg.NAME = "syn"
    d = workdir / "m"
    d.mkdir()
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(d))
    path = str(d / "weights_a_0001.npz")
    tr.save_weights(path)
    del tr
    model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(d))
    model.load_weights(path, path, by_name=True)
    ds, hold = SyntheticPoses(N_IMAGES, 128, 192, cfg, seed=3), SyntheticPoses(N_HOLDOUT, 128, 192, cfg, seed=9)
    eng = model._engine
    feats = []
    for data in (ds, hold):
        acts = []
        for _row0, n, slots in eval_batch_plan(data.image_ids, eng.B):
            model.detect([data.load_image(i) for i in slots])
            f = eng.features()
            assert tuple(f.shape) == (3, 2, 3, 32) and f.dtype == torch.float32
            acts.append(f[:n].cpu().numpy().copy())
        feats.append(np.concatenate(acts))
    _CACHE["m"] = (cfg, model, ds, hold, feats[0], feats[1])
    return _CACHE["m"]


def _state_bits(model):
    eng = model._engine
    loc, ori = eng.outputs()
    return [t.detach().cpu().numpy().view(np.int32).copy() for t in (eng.flat_w, eng.flat_stats, loc.contiguous(), ori.contiguous())]


def _statement(acts, grid, shrink="oas"):
    X = Dm.pool64(acts, grid)
    D = X.shape[1]
    s, G = np.zeros(D), np.zeros((D, D))
    for r0 in range(0, len(X), 3):
        Dm.gram_add64(X[r0:r0 + 3], X[0], s, G)
    return (X,) + Dm.settle(X[0], s, G, len(X), shrink)


PKEYS = ("image_ids", "loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda", "loc_spread", "ori_spread", "view_lambda", "n_views",
         "ori_bound", "loc_bound", "ori_region_bins", "ori_region_mass", "loc_region_bins", "loc_region_mass")
EKEYS = ("image_ids", "loc_est", "q_est", "loc_err", "ori_err", "esa", "dist", "loc_encoded_err", "ori_encoded_err", "ori_bound", "loc_bound",
         "ori_covered", "loc_covered")
DKEYS = ("domain_score", "domain_dist2", "domain_zmax", "domain_zarg", "domain_p")


def _same(a, b, keys):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("grid", [(1, 1), (2, 3)])
def test_fit_domain_is_the_statement_on_the_engines_features(workdir, grid):
    cfg, model, ds, hold, acts, hacts = _setup(workdir)
    before = _state_bits(model)[:2]
    dom = Dm.fit_domain(model, ds, holdout=hold, grid=grid)
    X, mean, cov, rho, W = _statement(acts, grid)
    assert dom.n == N_IMAGES and dom.grid == grid and dom.geometry == (2, 3, 32) and dom.D == grid[0] * grid[1] * 32 and dom.shrink == rho
    _same_bits(dom.centre, X[0], "centre")
    _same_bits(dom.mean, mean, "mean")
    _same_bits(dom.cov, cov, "cov")
    _same_bits(dom.W, W, "W")
    want = np.sort(Dm.maha64(Dm.pool64(hacts, grid), mean, W)[:, Dm.SCORE])
    _same_bits(dom.holdout_scores, want, "holdout scores")
    assert len(dom.holdout_scores) == N_HOLDOUT and np.all(np.isfinite(want)) and np.all(want > 0)
    for a, b in zip(before, _state_bits(model)[:2]):
        assert np.array_equal(a, b), "fit_domain changed the weights or the BN statistics"
    # the first images only; no holdout: no p-values
    few = Dm.fit_domain(model, ds, nr_images=7, grid=grid, shrink=0.5)
    X7, mean7, cov7, rho7, W7 = _statement(acts[:7], grid, 0.5)
    assert few.n == 7 and few.shrink == 0.5 and few.holdout_scores is None
    _same_bits(few.mean, mean7)
    _same_bits(few.cov, cov7)
    _same_bits(few.W, W7)
    _CACHE[grid] = dom


def test_predict_and_evaluate_with_a_domain(workdir, capsys):
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds, hold, acts, hacts = _setup(workdir)
    for grid in ((1, 1), (2, 3)):
        dom = _CACHE.get(grid) or Dm.fit_domain(model, ds, holdout=hold, grid=grid)
        p0 = pr.predict(model, ds)
        s0 = _state_bits(model)
        p = pr.predict(model, ds, domain=dom)
        s1 = _state_bits(model)
        for a, b in zip(s0, s1):
            assert np.array_equal(a, b), "weights, BN statistics or the engine's outputs differ"
        _same(p0, p, PKEYS)
        _same(p0, pr.predict(model, ds, domain=None), PKEYS + DKEYS)
        assert all(getattr(p0, k) is None for k in DKEYS)
        want = Dm.maha64(Dm.pool64(acts, grid), dom.mean, dom.W)
        _same_bits(p.domain_score, want[:, Dm.SCORE], "score")
        _same_bits(p.domain_dist2, want[:, Dm.DIST2], "dist2")
        _same_bits(p.domain_zmax, want[:, Dm.ZMAX], "zmax")
        assert np.array_equal(p.domain_zarg, want[:, Dm.ZARG].astype(np.int32)) and p.domain_zarg.dtype == np.int32
        assert np.array_equal(p.domain_p, dom.p_value(want[:, Dm.SCORE])) and np.all((p.domain_p > 0) & (p.domain_p <= 1))
        # the held-out source images against themselves: the k-th largest score has k holdout scores >= it, p = (1 + k) / (m + 1)
        ph = pr.predict(model, hold, domain=dom)
        assert sorted(ph.domain_p.tolist()) == [(1.0 + k) / (N_HOLDOUT + 1.0) for k in range(1, N_HOLDOUT + 1)]
        # evaluate: the same columns and one more line
        for sub in ("e0%d" % grid[0], "e1%d" % grid[0]):
            (workdir / sub).mkdir()
        capsys.readouterr()
        e0 = ev.evaluate(model, ds, out_dir=str(workdir / ("e0%d" % grid[0])))
        lines0 = capsys.readouterr().out.splitlines()
        e = ev.evaluate(model, ds, out_dir=str(workdir / ("e1%d" % grid[0])), domain=dom)
        lines = capsys.readouterr().out.splitlines()
        _same(e0, e, EKEYS)
        _same(p, e, DKEYS)
        assert all(getattr(e0, k) is None for k in DKEYS)
        assert len(lines) == len(lines0) + 1 and lines[:-1] == lines0 and lines[-1] == dom.line(e)
        assert lines[-1].startswith("Domain: score median %s, 95th percentile %s, p < 0.05 for " % (np.median(e.domain_score), np.percentile(e.domain_score, 95)))
        assert "Spearman's rho of the score with ori_err %s, with loc_err %s" % (Dm.spearman(e.domain_score, e.ori_err), Dm.spearman(e.domain_score, e.loc_err)) in lines[-1]
        print(lines[-1])
        # the Domain file comes back and applies; a domain without a holdout has no p-values
        again = Dm.Domain.load(dom.save(str(workdir / ("dom%d.npz" % grid[0]))))
        assert again == dom
        _same(p, pr.predict(model, ds, domain=again), PKEYS + DKEYS)
        again.holdout_scores = None
        assert pr.predict(model, ds, domain=again).domain_p is None


def test_domain_calibration_and_conformal_go_together(workdir):
    """domain= together with calibration= and conformal= gives the bits each gives alone."""
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds, hold, acts, hacts = _setup(workdir)
    dom = _CACHE.get((1, 1)) or Dm.fit_domain(model, ds, holdout=hold)
    cal = Cal.Calibration(ori_beta=2.0, loc_beta=0.5)
    cf = Cf.conformal(model, hold, alpha=0.4, calibration=cal)
    both = pr.predict(model, ds, calibration=cal, conformal=cf)
    alone = pr.predict(model, ds, domain=dom)
    every = pr.predict(model, ds, calibration=cal, conformal=cf, domain=dom)
    _same(both, every, PKEYS)
    _same(alone, every, DKEYS)
    (workdir / "all").mkdir()
    e_both = ev.evaluate(model, ds, out_dir=str(workdir / "all"), verbose=0, calibration=cal, conformal=cf)
    e_every = ev.evaluate(model, ds, out_dir=str(workdir / "all"), verbose=0, calibration=cal, conformal=cf, domain=dom)
    _same(e_both, e_every, EKEYS)
    _same(alone, e_every, DKEYS)


def test_a_domain_of_another_geometry_is_refused(workdir):
    from ursonet_amd import predict as pr
    cfg, model, ds, hold, acts, hacts = _setup(workdir)
    D = 32
    other = Dm.Domain(10, (1, 1), (8, 10, D), np.zeros(D), np.zeros(D), np.eye(D), 0.0, np.eye(D))
    with pytest.raises(ValueError, match="predict: the domain was fitted on bottleneck features of 8 x 10 cells with 32 channels"):
        pr.predict(model, ds, domain=other)
    with pytest.raises(ValueError, match="does not divide the model's feature map of 2 x 3 cells"):
        Dm.fit_domain(model, ds, grid=(2, 2))
