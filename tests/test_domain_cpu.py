"""Domain-shift scores without a GPU (fit_domain(), predict / evaluate with domain=..., domain_gap(), ursonet_amd/domain.py): pool64
against a per-element loop, gram_add64 + settle against np.cov, the order of the accumulation, the trace identity of the in-sample
scores, the OAS weight, the whitening matrix, domain_gap, the p-values, the Domain file, every refusal of the public interface before
torch, the engine or the library is touched, the surface of liburso_feat.so against header and bindings, and the three entry points'
argument checks (they run before any launch).

Bounds.  The data is Gaussian with a prescribed spectrum of condition number kappa <= 1e3 in D <= 512 dimensions; covariances, the
whitening identity and the trace identity are held to 1e-9 relative: kappa * D * 2^-53 = 6e-11 at the largest case, with room to spare."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from libsurface import header_symbols
from ursonet_amd import domain as Dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_feat.h")
FEAT_NAMES = {"urso_feat_pool", "urso_feat_gram_add", "urso_feat_maha"}
REL = 1e-9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def gaussian(n, D, kappa=1e3, seed=0, shift=0.0):
    """n rows of a D-dimensional Gaussian whose covariance has the eigenvalues geomspace(1, 1 / kappa) in a random basis, mean 3 + shift."""
    rng = np.random.RandomState(seed)
    ev = np.geomspace(1.0, 1.0 / kappa, D) if D > 1 else np.ones(1)
    Q = np.linalg.qr(rng.randn(D, D))[0]
    return (rng.randn(n, D) * np.sqrt(ev)) @ Q.T + 3.0 + shift


def fit(X, shrink="oas"):
    """A Domain of the rows of X through the module's statements: centre = X[0], one gram_add64 per batch of 7, settle."""
    n, D = X.shape
    s, G = np.zeros(D), np.zeros((D, D))
    for r0 in range(0, n, 7):
        Dm.gram_add64(X[r0:r0 + 7], X[0], s, G)
    mean, cov, rho, W = Dm.settle(X[0], s, G, n, shrink)
    return Dm.Domain(n, (1, 1), (1, 1, D), X[0], mean, cov, rho, W)


# ------------------------------------------------------------------ the statements
@pytest.mark.parametrize("geo,grid", [((2, 3, 5), (1, 1)), ((2, 3, 5), (2, 3)), ((4, 6, 3), (2, 2)), ((4, 6, 3), (1, 3)), ((8, 10, 4), (4, 5))])
def test_pool64_is_the_row_major_cell_mean(geo, grid):
    h, w, Cc = geo
    rng = np.random.RandomState(1)
    act = (rng.randn(3, h, w, Cc) * 10 ** rng.uniform(-3, 3, (3, h, w, Cc))).astype(np.float32)
    got = Dm.pool64(act, grid)
    gh, gw = grid
    ch, cw = h // gh, w // gw
    assert got.shape == (3, gh * gw * Cc) and got.dtype == np.float64
    for b in range(3):
        for gy in range(gh):
            for gx in range(gw):
                for c in range(Cc):
                    s = 0.0
                    for y in range(gy * ch, (gy + 1) * ch):
                        for x in range(gx * cw, (gx + 1) * cw):
                            s = s + float(act[b, y, x, c])
                    assert bits(got[b, (gy * gw + gx) * Cc + c]) == bits(s / (ch * cw)), (b, gy, gx, c)
    act[1, 0, 0, 0], act[2, h - 1, w - 1, Cc - 1] = np.nan, np.inf                    # non-finite values pass through, into their cell only
    bad = Dm.pool64(act, grid)
    assert np.isnan(bad[1, 0]) and np.isinf(bad[2, -1]) and np.isfinite(bad).sum() == bad.size - 2
    for g in ((3, 1), (1, 4), (0, 1), (h + 1, 1)):
        if h % max(g[0], 1) or w % max(g[1], 1) or 0 in g:
            with pytest.raises(ValueError, match="does not divide"):
                Dm.pool64(act, g)


@pytest.mark.parametrize("D,n", [(1, 5), (3, 40), (32, 100), (512, 600)])
def test_gram_and_settlement_give_np_cov(D, n):
    X = gaussian(n, D, seed=D)
    dom = fit(X, shrink=0.0)
    ref = np.cov(X, rowvar=False).reshape(D, D)
    scale = np.abs(ref).max()
    err = np.abs(dom.cov - ref).max() / scale
    merr = np.abs(dom.mean - X.mean(axis=0)).max() / np.abs(X).max()
    print("D=%d n=%d: cov rel %.3g, mean rel %.3g" % (D, n, err, merr))
    assert err <= REL and merr <= REL and np.array_equal(dom.cov, dom.cov.T) and dom.shrink == 0.0
    assert np.array_equal(bits(dom.centre), bits(X[0]))


def test_the_accumulation_order_is_part_of_the_statement():
    """The same rows in any batching give the same bits; a version that adds the rows in another order, or the batch's sum at once, does not."""
    X = gaussian(40, 16, seed=5)
    c = X[0]
    s0, G0 = Dm.gram_add64(X, c, np.zeros(16), np.zeros((16, 16)))
    s1, G1 = np.zeros(16), np.zeros((16, 16))
    for lo, hi in ((0, 3), (3, 6), (6, 7), (7, 40)):
        Dm.gram_add64(X[lo:hi], c, s1, G1)
    assert np.array_equal(bits(s0), bits(s1)) and np.array_equal(bits(G0), bits(G1))
    assert np.all(np.tril(G0, -1) == 0)                                             # nothing below the diagonal
    s2, G2 = Dm.gram_add64(X[::-1], c, np.zeros(16), np.zeros((16, 16)))            # descending rows
    d = X - c
    G3 = np.triu(d.T @ d)                                                           # one matrix product: another summation order
    assert not np.array_equal(bits(G0), bits(G2)) and not np.array_equal(bits(G0), bits(G3)) and not np.array_equal(bits(s0), bits(s2))
    assert np.allclose(G0, G2, rtol=1e-12) and np.allclose(G0, G3, rtol=1e-12)
    Xn = X.copy()
    Xn[4, 2] = np.nan                                                               # a NaN poisons what it touches: row and column 2 of the upper triangle
    sn, Gn = Dm.gram_add64(Xn, c, np.zeros(16), np.zeros((16, 16)))
    want = np.zeros((16, 16), dtype=bool)
    want[2, 2:], want[:3, 2] = True, True
    assert np.array_equal(np.isnan(Gn), want) and np.array_equal(np.isnan(sn), np.arange(16) == 2)


def test_maha64_is_the_sequential_rule():
    rng = np.random.RandomState(3)
    D, n = 9, 6
    X, mean = rng.randn(n, D), rng.randn(D)
    W = np.tril(rng.randn(D, D))
    Wn = W + np.triu(np.full((D, D), np.nan), 1)                                    # nothing above the diagonal is read
    got = Dm.maha64(X, mean, Wn)
    for b in range(n):
        d = X[b] - mean
        score = dist2 = 0.0
        zmax, zarg = -1.0, 0
        for i in range(D):
            acc = 0.0
            for j in range(i + 1):
                acc = acc + W[i, j] * d[j]
            score, dist2 = score + acc * acc, dist2 + d[i] * d[i]
            if abs(acc) > zmax:
                zmax, zarg = abs(acc), i
        assert np.array_equal(bits(got[b]), bits([score, dist2, zmax, float(zarg)])), b
    # a tie in |y_i| returns the lower index: W = I and d = (1, -2, 2, 0.5)
    tie = Dm.maha64(np.array([[1.0, -2.0, 2.0, 0.5]]), np.zeros(4), np.eye(4))
    assert tie[0].tolist() == [9.25, 9.25, 2.0, 1.0]
    X[2, 4] = np.inf
    X[4, 0] = np.nan
    bad = Dm.maha64(X, mean, Wn)
    assert np.all(np.isnan(bad[[2, 4]])) and np.array_equal(bits(bad[[0, 1, 3, 5]]), bits(got[[0, 1, 3, 5]]))


@pytest.mark.parametrize("D,n", [(32, 100), (512, 600)])
def test_trace_identity_and_whitening(D, n):
    """shrink = 0 and n > D: the in-sample scores sum to (n - 1) D, and W S' W^T = I."""
    X = gaussian(n, D, seed=7)
    dom = fit(X, shrink=0.0)
    scores = Dm.maha64(X, dom.mean, dom.W)[:, Dm.SCORE]
    rel = abs(scores.sum() - (n - 1) * D) / ((n - 1) * D)
    eye = np.abs(dom.W @ dom.cov @ dom.W.T - np.eye(D)).max()
    print("D=%d n=%d: trace identity rel %.3g, |W S W^T - I| %.3g" % (D, n, rel, eye))
    assert rel <= REL and eye <= REL and np.all(np.triu(dom.W, 1) == 0)
    oas = fit(X)                                                                    # with shrinkage the identity is for S'
    Sp = (1 - oas.shrink) * oas.cov + oas.shrink * np.trace(oas.cov) / D * np.eye(D)
    assert 0 < oas.shrink < 1 and np.abs(oas.W @ Sp @ oas.W.T - np.eye(D)).max() <= REL


def test_oas_rho_by_hand():
    # S = diag(1, 3), n = 5: tr = 4, tr(S^2) = 10, D = 2 -> ((1 - 1) 10 + 16) / ((5 + 1 - 1) (10 - 8)) = 1.6 -> 1
    assert Dm.oas_rho(np.diag([1.0, 3.0]), 5) == 1.0
    # n = 21: 16 / (21 * 2) = 8 / 21
    assert abs(Dm.oas_rho(np.diag([1.0, 3.0]), 21) - 8.0 / 21.0) <= 1e-15
    # S = [[2, 1], [1, 2]] (D = 2, tr = 4, tr(S^2) = 10), n = 41: 16 / (41 * 2) = 8 / 41
    assert abs(Dm.oas_rho(np.array([[2.0, 1.0], [1.0, 2.0]]), 41) - 8.0 / 41.0) <= 1e-15
    # D = 3, S = diag(1, 2, 3), n = 10: tr = 6, tr2 = 14: ((1/3) 14 + 36) / ((11 - 2/3) (14 - 12)) = (122/3) / (62/3) -> 1;  n = 100: (122/3) / ((101 - 2/3) 2)
    assert Dm.oas_rho(np.diag([1.0, 2.0, 3.0]), 10) == 1.0
    assert abs(Dm.oas_rho(np.diag([1.0, 2.0, 3.0]), 100) - (122.0 / 3.0) / ((101.0 - 2.0 / 3.0) * 2.0)) <= 1e-15
    assert Dm.oas_rho(np.array([[4.0]]), 7) == 1.0 and Dm.oas_rho(np.eye(3), 50) == 1.0          # D = 1; a denominator of 0
    X = gaussian(5, 1, seed=1)
    assert fit(X).shrink == 1.0
    with pytest.raises(ValueError, match="at least 2 images"):
        Dm.settle(X[0], np.zeros(1), np.zeros((1, 1)), 1)
    with pytest.raises(ValueError, match="not positive definite: raise shrink"):
        fit(gaussian(4, 8, seed=2), shrink=0.0)                                     # n < D without shrinkage
    assert fit(gaussian(4, 8, seed=2)).shrink > 0                                   # and OAS mends it
    for bad in ("ledoit", -0.1, 1.5, float("nan"), None, True):
        with pytest.raises(ValueError, match=r"shrink is 'oas' or a number in \[0, 1\]"):
            Dm.settle(X[0], np.zeros(1), np.zeros((1, 1)), 5, bad)


def test_domain_gap():
    D = 24
    a, b = fit(gaussian(200, D, seed=1), 0.0), fit(gaussian(150, D, seed=2, shift=0.5), 0.0)
    same = Dm.domain_gap(a, a)
    assert same["mean_term"] == 0 and abs(same["frechet"]) <= REL * np.trace(a.cov) and same["frechet"] == same["cov_term"]
    ab, ba = Dm.domain_gap(a, b), Dm.domain_gap(b, a)
    assert set(ab) == {"frechet", "mean_term", "cov_term"} and ab["frechet"] == ab["mean_term"] + ab["cov_term"]
    assert ab["mean_term"] == ba["mean_term"] and abs(ab["cov_term"] - ba["cov_term"]) <= REL * (np.trace(a.cov) + np.trace(b.cov))
    assert ab["frechet"] > 0.2 * D and ab["cov_term"] >= -REL * np.trace(a.cov)
    # diagonal covariances: sum (sqrt a_i - sqrt b_i)^2
    va, vb = np.linspace(0.5, 3.0, D), np.linspace(2.0, 0.1, D)
    da = Dm.Domain(10, (1, 1), (1, 1, D), np.zeros(D), np.zeros(D), np.diag(va), 0.0, np.diag(1 / np.sqrt(va)))
    db = Dm.Domain(10, (1, 1), (1, 1, D), np.zeros(D), np.ones(D), np.diag(vb), 0.0, np.diag(1 / np.sqrt(vb)))
    g = Dm.domain_gap(da, db)
    assert g["mean_term"] == D and abs(g["cov_term"] - np.sum((np.sqrt(va) - np.sqrt(vb)) ** 2)) <= REL * (va.sum() + vb.sum())
    with pytest.raises(ValueError, match="differ in geometry or grid"):
        Dm.domain_gap(a, da.__class__(10, (1, 1), (1, 1, 3), np.zeros(3), np.zeros(3), np.eye(3), 0.0, np.eye(3)))
    with pytest.raises(ValueError, match="needs two domain.Domain"):
        Dm.domain_gap(a, None)


def test_p_values_and_the_file(tmp_path):
    X = gaussian(30, 6, seed=4)
    dom = fit(X)
    with pytest.raises(ValueError, match="needs holdout scores"):
        dom.p_value([1.0])
    dom.holdout_scores = np.array([1.0, 2.0, 2.0, 3.0])                             # m = 4
    p = dom.p_value([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, np.nan])
    assert p[:7].tolist() == [1.0, 1.0, 0.8, 0.8, 0.4, 0.4, 0.2] and np.isnan(p[7])  # ties count as >=; both ends
    unsorted = Dm.Domain(dom.n, dom.grid, dom.geometry, dom.centre, dom.mean, dom.cov, dom.shrink, dom.W, [3.0, 1.0, 2.0, 2.0])
    assert unsorted == dom
    back = Dm.Domain.load(dom.save(str(tmp_path / "dom.npz")))
    assert back == dom and back.n == 30 and back.grid == (1, 1) and back.geometry == (1, 1, 6) and back.D == 6
    for k in ("centre", "mean", "cov", "W", "holdout_scores"):
        assert np.array_equal(bits(getattr(back, k)), bits(getattr(dom, k))), k
    assert bits(back.shrink) == bits(dom.shrink)
    dom.holdout_scores = None
    again = Dm.Domain.load(dom.save(str(tmp_path / "dom2.npz")))
    assert again == dom and again.holdout_scores is None and again != back
    with pytest.raises(ValueError, match=r"cov has shape \(5, 5\), D = 6"):
        Dm.Domain(3, (1, 1), (1, 1, 6), dom.centre, dom.mean, np.eye(5), 0.0, dom.W)


def test_spearman_uses_average_ranks():
    assert Dm.spearman([1, 2, 3, 4], [10, 20, 30, 40]) == 1.0 and Dm.spearman([1, 2, 3, 4], [4, 3, 2, 1]) == -1.0
    # ranks of (1, 2, 2, 3) are (1, 2.5, 2.5, 4); against (1, 2, 3, 4): cov = 4.5, var = 4.5 and 5
    assert abs(Dm.spearman([1, 2, 2, 3], [1, 2, 3, 4]) - 4.5 / np.sqrt(4.5 * 5.0)) <= 1e-15
    assert np.isnan(Dm.spearman([1, 1, 1], [1, 2, 3]))


# ------------------------------------------------------------------ refusals
def test_interface_refuses_before_torch_the_engine_or_the_library():
    code = """
import os, sys
sys.path.insert(0, "tests")
sys.modules["torch"] = None                              # poisoned: any import of torch raises
import numpy as np
import pytest
from util import make_config
from ursonet_amd import domain, evaluate, predict
class Boom(object):
    def __getattr__(self, name):
        raise AssertionError("touched %s" % name)
class Data(object):
    def __init__(self, n):
        self.image_ids = list(range(n))
class Model(object):
    _dp, _world = None, 1
    _engine = property(lambda self: Boom().engine)
    def __init__(self, mode="inference", **kw):
        self.mode, self.config = mode, make_config("resnet18", 128, 192, batch=3, **kw)
assert domain.feature_geometry(Model().config) == (2, 3, 32)
assert domain.feature_geometry(make_config("resnet50", 512, 640, bottleneck=128)) == (8, 10, 128)
for grid in ((2, 2), (3, 3), (1, 2), (0, 1), (4, 6)):
    with pytest.raises(ValueError, match="fit_domain: the grid .* does not divide the model's feature map of 2 x 3 cells"):
        domain.fit_domain(Model(), Data(10), grid=grid)
with pytest.raises(ValueError, match="fit_domain: grid must be a pair"):
    domain.fit_domain(Model(), Data(10), grid=2)
with pytest.raises(ValueError, match=r"gives D = 6144 features, more than URSO_FEAT_MAX_D = 4096"):
    domain.fit_domain(Model(bottleneck=1024), Data(10), grid=(2, 3))
need = 8 * (192 * 192 + 3 * 192 + 3 * 192) + 8 * 4 * 10
with pytest.raises(ValueError, match=r"the accumulators for D = 192 features need %d bytes \\(.* GiB\\), more than max_gb = 0.0001 GiB" % need):
    domain.fit_domain(Model(), Data(10), grid=(2, 3), max_gb=1e-4)
with pytest.raises(ValueError, match="fit_domain needs a model created in inference mode"):
    domain.fit_domain(Model("training"), Data(10))
with pytest.raises(ValueError, match="a covariance needs at least 2 images"):
    domain.fit_domain(Model(), Data(1))
with pytest.raises(ValueError, match="nr_images must be >= 2"):
    domain.fit_domain(Model(), Data(10), nr_images=1)
with pytest.raises(ValueError, match="shrink is 'oas' or a number"):
    domain.fit_domain(Boom(), Boom(), shrink=2.0)
D = 32
dom = domain.Domain(10, (1, 1), (2, 3, D), np.zeros(D), np.zeros(D), np.eye(D), 0.0, np.eye(D))
other = domain.Domain(10, (1, 1), (8, 10, D), np.zeros(D), np.zeros(D), np.eye(D), 0.0, np.eye(D))
dom.check_model(Model(), "predict")
with pytest.raises(ValueError, match="predict: the domain was fitted on bottleneck features of 8 x 10 cells with 32 channels, this model's have 2 x 3 cells with 32"):
    other.check_model(Model(), "predict")
class Maps(object):
    image_ids, histogram_3D_map, ori_histogram_map = [], 1, 1
for fn, who in ((predict.predict, "predict"), (evaluate.evaluate, "evaluate")):
    for kw, msg in ((dict(domain=0.5), "domain must be a domain.Domain"),
                    (dict(domain=dom, members=[{"a": {}}]), "domain=... cannot be combined with members=... or views=..."),
                    (dict(domain=dom, views=[[0, 0, 5]]), "domain=... cannot be combined with members=... or views=...")):
        with pytest.raises(ValueError) as err:
            fn(Boom(), Boom(), **kw)
        assert msg in str(err.value) and str(err.value).startswith(who), err.value
    with pytest.raises(ValueError, match="%s: the domain was fitted on bottleneck features of 8 x 10" % who):
        fn(Model(), Maps(), domain=other)
os.environ["WORLD_SIZE"] = "2"
with pytest.raises(ValueError, match="fit_domain is not supported under a data-parallel launcher"):
    domain.fit_domain(Boom(), Boom())
for fn, who in ((predict.predict, "predict"), (evaluate.evaluate, "evaluate")):
    with pytest.raises(ValueError, match="%s: domain=... is not supported under a data-parallel launcher" % who):
        fn(Boom(), Boom(), domain=dom)
del os.environ["WORLD_SIZE"]
class Ranked(Model):
    _world = 2
with pytest.raises(ValueError, match="fit_domain is not supported under a data-parallel launcher"):
    domain.fit_domain(Ranked(), Data(10))
assert sys.modules["torch"] is None and "ursonet_amd.hip" not in sys.modules and "ursonet_amd.engine" not in sys.modules
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["feat"]) == FEAT_NAMES and build.SIDE_SOURCES["feat"] == ["feat.hip"]
    for macro, v in (("MAX_D", Dm.MAX_D), ("COLS", Dm.COLS), ("MAHA_ROWS", Dm.MAHA_ROWS), ("SCORE", Dm.SCORE), ("DIST2", Dm.DIST2),
                     ("ZMAX", Dm.ZMAX), ("ZARG", Dm.ZARG)):
        assert re.search(r"#define\s+URSO_FEAT_%s\s+%d\b" % (macro, v), txt), macro
        assert getattr(hip, "FEAT_" + macro) == v
    # the argument structs are the header's: field order and sizes
    fields = {"urso_feat_pool_args": (hip.FeatPoolArgs, ["B", "n", "row0", "h", "w", "C", "gh", "gw", "dtype", "ld", "act", "out"], 64),
              "urso_feat_gram_args": (hip.FeatGramArgs, ["B", "n", "row0", "D", "pad", "ld_x", "ld_g", "x", "centre", "s", "g"], 72),
              "urso_feat_maha_args": (hip.FeatMahaArgs, ["B", "n", "row0", "D", "pad", "ld_x", "ld_w", "x", "mean", "wt", "out"], 72)}
    for struct, (cls, order, size) in fields.items():
        assert [f[0] for f in cls._fields_] == order and C.sizeof(cls) == size, struct
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
        declared = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"\b(const|int32_t|int64_t|float|double|void)\b|\*", " ", body))
        assert declared == order, struct
    assert hip.FeatPoolArgs.ld.offset == 40 and hip.FeatPoolArgs.act.offset == 48 and hip.FeatGramArgs.ld_x.offset == 24 and hip.FeatMahaArgs.x.offset == 40


def test_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "feat_abi.c"
    src.write_text('#include "ursonet_feat.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\n'
                   "fn table[] = { (fn)urso_feat_pool, (fn)urso_feat_gram_add, (fn)urso_feat_maha };\n"
                   "size_t sizes(void) { return sizeof(urso_feat_pool_args) + sizeof(urso_feat_gram_args) + sizeof(urso_feat_maha_args) + URSO_FEAT_COLS; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "feat_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_without_gpu():
    """Every refusal of the three entry points.  Device pointers are made up and never dereferenced: each call is refused before a launch,
    or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("feat")
    P = [0x1000000 * k for k in range(1, 6)]

    def call(fn, cls, base, kw):
        a = cls()
        for k, v in dict(base, **kw).items():
            setattr(a, k, v)
        return fn(C.byref(a), None)
    pool_base = dict(B=4, n=3, row0=0, h=4, w=6, C=8, gh=2, gw=3, dtype=hip.BF16, ld=48, act=P[0], out=P[1])
    gram_base = dict(B=4, n=3, row0=0, D=48, pad=0, ld_x=48, ld_g=48, x=P[0], centre=P[1], s=P[2], g=P[3])
    maha_base = dict(B=4, n=3, row0=0, D=48, pad=0, ld_x=48, ld_w=48, x=P[0], mean=P[1], wt=P[2], out=P[3])
    rows = [(dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"), (dict(B=-1, n=0), "0 <= n <= B"), (dict(row0=-1), "row0 must be >= 0")]
    pool_bad = rows + [(dict(act=None), "null pointer"), (dict(out=None), "null pointer"), (dict(h=0), "need h, w, C >= 1"), (dict(C=0), "need h, w, C >= 1"),
                       (dict(gh=3), "the grid (3, 3) does not divide the feature map (4, 6)"), (dict(gw=4), "does not divide"), (dict(gh=0), "does not divide"),
                       (dict(gw=-1), "does not divide"), (dict(C=1024, gh=4, gw=6, ld=1 << 20), "need 1 <= D <= 4096 (got 24576)"),
                       (dict(dtype=3), "unknown dtype 3"), (dict(dtype=-1), "unknown dtype -1"), (dict(ld=47), "ld 47 < D 48"),
                       (dict(act=P[0] + 1), "act must be 2-byte aligned"), (dict(dtype=hip.F32, act=P[0] + 2), "act must be 4-byte aligned"),
                       (dict(out=P[1] + 4), "out must be 8-byte aligned")]
    gram_bad = rows + [(dict(x=None), "null pointer"), (dict(centre=None), "null pointer"), (dict(s=None), "null pointer"), (dict(g=None), "null pointer"),
                       (dict(D=0), "need 1 <= D <= 4096 (got 0)"), (dict(D=4097, ld_x=4097, ld_g=4097), "need 1 <= D <= 4096 (got 4097)"),
                       (dict(ld_x=47), "ld_x 47 < D 48"), (dict(ld_g=47), "ld_g 47 < D 48"), (dict(x=P[0] + 4), "must be 8-byte aligned"),
                       (dict(centre=P[1] + 4), "must be 8-byte aligned"), (dict(s=P[2] + 2), "must be 8-byte aligned"), (dict(g=P[3] + 4), "must be 8-byte aligned")]
    maha_bad = rows + [(dict(x=None), "null pointer"), (dict(mean=None), "null pointer"), (dict(wt=None), "null pointer"), (dict(out=None), "null pointer"),
                       (dict(D=0), "need 1 <= D <= 4096 (got 0)"), (dict(D=-5), "need 1 <= D <= 4096 (got -5)"), (dict(ld_x=47), "ld_x 47 < D 48"),
                       (dict(ld_w=47), "ld_w 47 < D 48"), (dict(x=P[0] + 4), "must be 8-byte aligned"), (dict(mean=P[1] + 4), "must be 8-byte aligned"),
                       (dict(wt=P[2] + 4), "must be 8-byte aligned"), (dict(out=P[3] + 4), "must be 8-byte aligned")]
    for fn, cls, base, name, cases in ((lib.urso_feat_pool, hip.FeatPoolArgs, pool_base, "urso_feat_pool", pool_bad),
                                       (lib.urso_feat_gram_add, hip.FeatGramArgs, gram_base, "urso_feat_gram_add", gram_bad),
                                       (lib.urso_feat_maha, hip.FeatMahaArgs, maha_base, "urso_feat_maha", maha_bad)):
        for kw, msg in cases:
            assert call(fn, cls, base, kw) == -1, (name, kw)
            err = hip.last_error()
            assert err.startswith(name + ":") and msg in err, (kw, err)
        assert fn(None, None) == -1 and name + ": null argument struct" in hip.last_error()
        # n = 0 is valid and launches nothing (so it needs no GPU); the refusals come in front of it
        assert call(fn, cls, base, dict(n=0)) == 0 and call(fn, cls, base, dict(n=0, B=0)) == 0
        assert call(fn, cls, base, dict(n=0, row0=-1)) == -1
    assert call(lib.urso_feat_pool, hip.FeatPoolArgs, pool_base, dict(n=0, C=512, ld=4096, dtype=hip.F16)) == 0      # D = 3072
    assert call(lib.urso_feat_pool, hip.FeatPoolArgs, pool_base, dict(n=0, C=1024, ld=8192)) == -1                   # D = 6144
