"""Conformal bounds without a GPU (conformal(), predict / evaluate / test_and_submit with conformal=..., ursonet_amd/conformal.py):
weights64 / score64 / bound64 against a brute-force restatement with Python integers (tests/confref.py), the equivalence SCORE <= q <=>
covered, quantile's index rule, the coverage of exchangeable synthetic PMFs, the Conformal file, every refusal of the public interface
before torch, the engine or the library is touched, the surface of liburso_infer.so against header and bindings, and the two entry
points' argument checks (they run before any launch)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import confref as R
from libsurface import header_symbols
from ursonet_amd import conformal as Cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_infer.h")
CONF_NAMES = {"urso_conf_score", "urso_conf_bound"}
METRICS = (Cf.ANGLE, Cf.EUCLID)


# ------------------------------------------------------------------ the rule
def test_weights_are_the_rounded_scaled_exponentials():
    z = np.array([[0.0, -1.0, -np.inf, -30.0, -1e4], [5.0, 5.0, 5.0, 5.0, 5.0]], dtype=np.float32)
    w, W, ok = Cf.weights64(z)
    assert w.dtype == np.uint64 and ok.all()
    assert [int(x) for x in w[0]] == [2 ** 34, int(np.rint(math.exp(-1.0) * 2 ** 34)), 0, int(np.rint(math.exp(-30.0) * 2 ** 34)), 0]
    assert int(W[0]) == sum(int(x) for x in w[0]) and int(W[1]) == 5 * 2 ** 34
    big = np.zeros((1, Cf.MAX_K), dtype=np.float32)                                 # the largest W there is stays below 2^53
    assert int(Cf.weights64(big)[1][0]) == 2 ** 52 < 2 ** 53
    bad = np.array([[1.0, np.nan], [np.inf, 0.0], [-np.inf, -np.inf]], dtype=np.float32)
    assert not Cf.weights64(bad)[2].any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K", [1, 3, 5, 27, 1023])
def test_score64_and_bound64_against_brute_force(K, metric):
    z, m, est, ref = R.case(K, metric)
    s = Cf.score64(z, m, est, ref, metric)
    kref = Cf.ref_keys64(metric, est, ref)
    for b, (Cm, W, near) in enumerate(R.brute_score(z, m, est, ref, metric)):
        assert s[b, Cf.C_MASS] == Cm and s[b, Cf.W_SUM] == W and s[b, Cf.NEAR] == near and s[b, Cf.SCORE] == float(Cm) / float(W)
        assert R.bits(s[b, Cf.KEY_REF]) == R.bits(kref[b]) and np.all(s[b, 6:] == 0)
        want = math.degrees(2 * math.acos(kref[b])) if metric == Cf.ANGLE else math.sqrt(kref[b])
        assert R.ulps(s[b, Cf.ERR], want) <= 4
    for q in R.QS + tuple(float(x) for x in s[:, Cf.SCORE] if x > 0):
        got = Cf.bound64(z, m, est, metric, q)
        for b, (key, G, count, W) in enumerate(R.brute_bound(z, m, est, metric, q)):
            if key is None:
                assert q >= 1 and np.isnan(got[b, Cf.KEY]) and got[b, Cf.MASS] == 1 and got[b, Cf.COUNT] == K
                assert got[b, Cf.BOUND] == (180.0 if metric == Cf.ANGLE else np.inf) and got[b, Cf.BOUND_W] == W
                continue
            assert R.bits(got[b, Cf.KEY]) == R.bits(key) and got[b, Cf.MASS] == float(G) / float(W) and got[b, Cf.COUNT] == count
            assert got[b, Cf.BOUND_W] == W and got[b, Cf.MASS] > q and np.all(got[b, 5:] == 0)
            assert got[b, Cf.BOUND] == Cf.value(metric, key)


def _covered(metric, key_ref, key_bound):
    """The truth is at least as close as the bound's key (a NaN key: no key qualified, everything is covered)."""
    if np.isnan(key_bound):
        return True
    return key_ref >= key_bound if metric == Cf.ANGLE else key_ref <= key_bound


@pytest.mark.parametrize("metric", METRICS)
def test_score_at_most_q_is_covered_exactly(metric):
    """q just below, at and just above every row's own score, on random rows and on rows whose truth IS a map entry, a repeated one or
    (angle) a sign-flipped one: ties fall on the covered side, and SCORE <= q <=> key_ref at least as close as v*."""
    for K in (5, 27, 1023):
        z, m, est, ref = R.case(K, metric, seed=1)
        n = len(z)
        ties = m[[(3 * i + 1) % K for i in range(n)]].astype(np.float64)          # entries that have a copy or a flipped copy
        for truth in (ref, ties, -ties if metric == Cf.ANGLE else ties):
            s = Cf.score64(z, m, est, truth, metric)
            for b in range(n):
                sc = s[b, Cf.SCORE]
                for q in (np.nextafter(sc, -1), sc, np.nextafter(sc, 2), 0.5, 0.9, 1.0):
                    if not q > 0:
                        continue
                    bd = Cf.bound64(z[b:b + 1], m, est[b:b + 1], metric, q)[0]
                    assert _covered(metric, s[b, Cf.KEY_REF], bd[Cf.KEY]) == (sc <= q), (K, b, q, sc)
    # est on a map entry: the key clamps to 1 / is 0, and a q below the entry's own mass gives the bound 0
    z, m, est, ref = R.case(27, metric, seed=2)
    est = m[[0, 1, 3, 4, 6, 7, 9, 10]].astype(np.float64) * (1.0 + 2.0 ** -20 if metric == Cf.ANGLE else 1.0)   # (an fp32 unit vector's norm is 1 to 2^-24 only)
    bd = Cf.bound64(z, m, est, metric, 1e-12)
    assert np.all(bd[:, Cf.BOUND] == 0) and np.all(bd[:, Cf.KEY] == (1.0 if metric == Cf.ANGLE else 0.0)) and np.all(bd[:, Cf.COUNT] >= 1)


def test_rows_that_are_not_finite_are_nan():
    z, m, est, ref = R.case(27, Cf.ANGLE)
    z[1, 3], z[2, 0], z[3, :] = np.nan, np.inf, -np.inf
    est[4, 2], ref[5, 1] = np.nan, np.inf
    s, b = Cf.score64(z, m, est, ref, Cf.ANGLE), Cf.bound64(z, m, est, Cf.ANGLE, 0.5)
    assert np.all(np.isnan(s[[1, 2, 3, 4, 5]])) and np.all(np.isfinite(s[[0, 6, 7]]))
    assert np.all(np.isnan(b[[1, 2, 3, 4]])) and np.all(np.isfinite(b[[0, 5, 6, 7]]))
    one = np.full((1, 27), -np.inf, dtype=np.float32)                              # one finite logit among -inf: its bin has all the mass
    one[0, 11] = -3.0
    bd = Cf.bound64(one, m, est[:1], Cf.ANGLE, 0.999)[0]
    assert bd[Cf.MASS] == 1 and bd[Cf.BOUND_W] == 2 ** 34 and R.bits(bd[Cf.KEY]) == R.bits(Cf.keys64(Cf.ANGLE, m, est[:1])[0, 11])


def test_quantile_index_rule():
    for n, k in ((9, 9), (10, 10), (19, 18)):                                       # k = ceil((n + 1) 0.9)
        s = np.random.default_rng(n).permutation(n).astype(np.float64)
        assert Cf.quantile(s, 0.1) == k - 1, n
    assert Cf.quantile([0.3], 0.1) == np.inf and Cf.quantile(np.arange(8.0), 0.1) == np.inf       # k > n
    assert Cf.quantile([0.3], 0.5) == 0.3 and Cf.quantile(np.arange(19.0), 0.5) == 9 and Cf.quantile([], 0.5) == np.inf
    assert Cf.quantile(np.arange(10.0), 0.99) == 0.0                               # k = 1


def test_coverage_of_exchangeable_synthetic_pmfs():
    """200 calibration and 2000 test rows drawn alike: the truth is a jittered bin drawn from the row's own softmax, the estimate the
    jittered arg max.  The guarantee is P(covered) >= 0.9 marginally; with n = 200 the coverage of a test set spreads about 0.02 around
    k / (n + 1) = 0.9005 (the k-th of n uniform order statistics: sd sqrt(0.9 * 0.1 / 201) = 0.021, plus the test set's own 0.007), so
    [0.85, 0.95] is the binomial spread of the guarantee, not a measurement of the code: about one draw in fifty falls outside it by
    chance alone (of the seeds 0 .. 7, seed 5 does, at 0.823), which is why the seed is fixed."""
    rng = np.random.default_rng(0)
    K, n_cal, n_test = 64, 200, 2000
    m = rng.uniform(-1, 1, size=(K, 3))
    N = n_cal + n_test
    z = (rng.normal(size=(N, K)) * 2).astype(np.float32)
    p = np.exp(z.astype(np.float64) - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    truth_bin = np.array([rng.choice(K, p=p[i]) for i in range(N)])
    ref = m[truth_bin] + rng.normal(size=(N, 3)) * 0.01
    est = m[z.argmax(axis=1)] + rng.normal(size=(N, 3)) * 0.01
    s = Cf.score64(z, m, est, ref, Cf.EUCLID)
    cf = Cf.Conformal(0.1, "error", "pmf", np.zeros(n_cal), s[:n_cal, Cf.SCORE])
    assert cf.loc_q == np.sort(s[:n_cal, Cf.SCORE])[math.ceil(201 * 0.9) - 1]
    bd = Cf.bound64(z[n_cal:], m, est[n_cal:], Cf.EUCLID, cf.loc_q)
    covered = s[n_cal:, Cf.KEY_REF] <= bd[:, Cf.KEY]
    assert np.array_equal(covered, s[n_cal:, Cf.SCORE] <= cf.loc_q)                   # the equivalence, on 2000 rows
    assert np.array_equal(covered, s[n_cal:, Cf.ERR] <= bd[:, Cf.BOUND])               # (sqrt is monotone and correctly rounded)
    print("coverage %.4f, mean bound %.4f, mean region %.1f bins" % (covered.mean(), bd[:, Cf.BOUND].mean(), bd[:, Cf.COUNT].mean()))
    assert 0.85 <= covered.mean() <= 0.95


# ------------------------------------------------------------------ the file
def test_conformal_round_trip_is_bit_for_bit(tmp_path):
    rng = np.random.default_rng(0)
    ori, loc = rng.uniform(size=19), rng.uniform(0, 3, size=19)
    ori[3] = float(np.nextafter(0.5, 1))
    c = Cf.Conformal(0.1, "pmf", "error", ori, loc, k_ori=512, k_loc=0, n_images=19, ori_beta=np.pi / 3)
    assert c.ori_scores == sorted(ori.tolist()) and c.ori_q == sorted(ori.tolist())[17] and c.loc_q == sorted(loc.tolist())[17]
    d = Cf.Conformal.load(c.save(str(tmp_path / "cf.json")))
    assert d == c and [x.hex() for x in d.ori_scores] == [x.hex() for x in c.ori_scores] and d.ori_q.hex() == c.ori_q.hex()
    assert d.ori_beta.hex() == (np.pi / 3).hex() and d.loc_beta is None and d.k_ori == 512 and d.n_images == 19 and d.loc_kind == "error"
    half = c.at(0.5)
    assert half.alpha == 0.5 and half.ori_q == c.ori_scores[9] and half.ori_scores == c.ori_scores and c.at(0.01).ori_q == np.inf
    assert Cf.Conformal.load(c.at(0.01).save(str(tmp_path / "inf.json"))).loc_q == np.inf            # +inf survives the file
    assert c.line().startswith("Conformal: target coverage 0.9 on 19 calibration images; orientation level %s (pmf); location level" % c.ori_q)
    for bad in (0, 1, -0.1, 1.5, float("nan"), "x", True, None):
        with pytest.raises(ValueError, match=r"alpha must be a number in \(0, 1\)"):
            Cf.Conformal(bad, "pmf", "error", ori, loc)
    with pytest.raises(ValueError, match="a head's kind is 'pmf' or 'error'"):
        Cf.Conformal(0.1, "soft", "error", ori, loc)
    with pytest.raises(ValueError, match="ori_q = 0.25 is not the level of the scores"):
        Cf.Conformal(0.1, "pmf", "error", ori, loc, ori_q=0.25)
    c.check_model(512, 0)
    with pytest.raises(ValueError, match="whose orientation head has 512 bins, this model's has 4096 bins"):
        c.check_model(4096, 0)
    with pytest.raises(ValueError, match="whose location head has a regression output, this model's has 64 bins"):
        c.check_model(512, 64)


def test_interface_refuses_before_torch_the_engine_or_the_library():
    code = """
import os, sys
import pytest
from ursonet_amd import calibrate, conformal, evaluate, predict, submission
class Boom(object):
    def __getattr__(self, name):
        raise AssertionError("touched %s" % name)
class Empty(object):
    image_ids = []
class Model(object):
    mode, _dp, _world = "inference", None, 1
    config = property(lambda self: Boom().config)
    _engine = property(lambda self: Boom().engine)
cf = conformal.Conformal(0.1, "pmf", "error", [0.1, 0.2], [1.0, 2.0], k_ori=512, ori_beta=2.0)
same, other = calibrate.Calibration(ori_beta=2.0), calibrate.Calibration(ori_beta=3.0)
for fn, who in ((predict.predict, "predict"), (evaluate.evaluate, "evaluate")):
    for kw, msg in ((dict(conformal=0.9), "conformal must be a conformal.Conformal"),
                    (dict(conformal={"alpha": 0.1}), "conformal must be a conformal.Conformal"),
                    (dict(conformal=cf, calibration=same, members=[{"a": {}}]), "calibrate and predict each member on its own"),
                    (dict(conformal=cf, members=[{"a": {}}]), "cannot be combined with members=... or views=..."),
                    (dict(conformal=cf, calibration=same, views=[[0, 0, 5]]), "cannot be combined with members=... or views=..."),
                    (dict(conformal=cf), "fitted under the calibration betas (ori 2.0, loc None), but calibration= gives (ori None, loc None)"),
                    (dict(conformal=cf, calibration=other), "betas (ori 2.0, loc None), but calibration= gives (ori 3.0, loc None)")):
        with pytest.raises(ValueError) as err:
            fn(Boom(), Boom(), **kw)
        assert msg in str(err.value) and str(err.value).startswith(who), err.value
with pytest.raises(ValueError, match="evaluate: conformal=... cannot be combined with multimodal=True"):
    evaluate.evaluate(Boom(), Boom(), multimodal=True, conformal=cf, calibration=same)
with pytest.raises(ValueError, match="cannot be combined with members=... or views=..."):
    submission.test_and_submit(Boom(), Boom(), Boom(), views=[[0, 0, 5]], conformal=cf, calibration=same)
for kw in (dict(members=[{"a": {}}]), dict(views=[[0, 0, 5]])):
    with pytest.raises(ValueError, match="conformal: members=... and views=... are not supported"):
        conformal.conformal(Boom(), Boom(), **kw)
for bad in (0, 1, 1.5, -0.1, float("nan"), "x", None):
    with pytest.raises(ValueError, match="conformal: alpha must be a number in"):
        conformal.conformal(Boom(), Boom(), alpha=bad)
with pytest.raises(ValueError, match="conformal: calibration must be a calibrate.Calibration"):
    conformal.conformal(Model(), Empty(), calibration=2.0)
with pytest.raises(ValueError, match="conformal: the dataset has no labelled images"):
    conformal.conformal(Model(), Empty())
with pytest.raises(ValueError, match="conformal: nr_images must be >= 1"):
    conformal.conformal(Model(), Empty(), nr_images=0)
os.environ["WORLD_SIZE"] = "2"
with pytest.raises(ValueError, match="conformal is not supported under a data-parallel launcher"):
    conformal.conformal(Boom(), Boom())
assert "torch" not in sys.modules and "ursonet_amd.hip" not in sys.modules and "ursonet_amd.engine" not in sys.modules
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["infer"]) == CONF_NAMES and build.SIDE_SOURCES["infer"] == ["conformal.hip"]
    for macro, v in (("SHIFT", Cf.SHIFT), ("MAX_K", Cf.MAX_K), ("COLS", Cf.COLS), ("ANGLE", Cf.ANGLE), ("EUCLID", Cf.EUCLID), ("SCORE", Cf.SCORE),
                     ("C", Cf.C_MASS), ("W", Cf.W_SUM), ("KEY_REF", Cf.KEY_REF), ("ERR", Cf.ERR), ("NEAR", Cf.NEAR), ("BOUND", Cf.BOUND),
                     ("KEY", Cf.KEY), ("MASS", Cf.MASS), ("COUNT", Cf.COUNT), ("BW", Cf.BOUND_W), ("DIGIT", 11), ("PASSES", 6)):
        assert re.search(r"#define\s+URSO_CONF_%s\s+%d\b" % (macro, v), txt), macro
        assert getattr(hip, "CONF_" + macro) == v
    # the argument structs are the header's: field order and sizes
    assert [f[0] for f in hip.ConfScoreArgs._fields_] == ["B", "n", "row0", "K", "ld_z", "metric", "ld_est", "ld_ref", "pad", "logits", "map",
                                                          "est", "ref", "out"]
    assert [f[0] for f in hip.ConfBoundArgs._fields_] == ["B", "n", "row0", "K", "ld_z", "metric", "ld_est", "q", "logits", "map", "est", "out"]
    assert C.sizeof(hip.ConfScoreArgs) == 80 and C.sizeof(hip.ConfBoundArgs) == 72
    assert hip.ConfScoreArgs.logits.offset == 40 and hip.ConfBoundArgs.q.offset == 32 and hip.ConfBoundArgs.logits.offset == 40
    for struct, fields in (("urso_conf_score_args", hip.ConfScoreArgs._fields_), ("urso_conf_bound_args", hip.ConfBoundArgs._fields_)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
        declared = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"\b(const|int32_t|int64_t|float|double|void)\b|\*", " ", body))
        assert declared == [f[0] for f in fields], struct


def test_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "infer_abi.c"
    src.write_text('#include "ursonet_infer.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\nfn table[] = { (fn)urso_conf_score, (fn)urso_conf_bound };\n'
                   "size_t sizes(void) { return sizeof(urso_conf_score_args) + sizeof(urso_conf_bound_args) + URSO_CONF_COLS; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "infer_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_without_gpu():
    """Every refusal of the two entry points.  Device pointers are made up and never dereferenced: each call is refused before a launch,
    or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("infer")
    Z, M, E, RF, O = (0x1000000 * k for k in range(1, 6))

    def fill(a, base, kw):
        for k, v in dict(base, **kw).items():
            setattr(a, k, v)
        return a
    common = dict(B=4, n=3, row0=0, K=8, ld_z=8, metric=hip.CONF_ANGLE, ld_est=16, logits=Z, map=M, est=E, out=O)

    def score(**kw):
        a = fill(hip.ConfScoreArgs(), dict(common, ld_ref=4, pad=0, ref=RF), kw)
        return lib.urso_conf_score(C.byref(a), None)

    def bound(**kw):
        a = fill(hip.ConfBoundArgs(), dict(common, q=0.9), kw)
        return lib.urso_conf_bound(C.byref(a), None)
    nan, inf = float("nan"), float("inf")
    bad = [(dict(logits=None), "null pointer"), (dict(map=None), "null pointer"), (dict(est=None), "null pointer"), (dict(out=None), "null pointer"),
           (dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"), (dict(B=-1, n=0), "0 <= n <= B"), (dict(row0=-1), "row0 must be >= 0"),
           (dict(K=0, ld_z=0), "need 1 <= K <= 262144"), (dict(K=-3), "need 1 <= K <= 262144"), (dict(K=2 ** 18 + 1, ld_z=2 ** 18 + 1), "need 1 <= K <= 262144"),
           (dict(ld_z=7), "ld_z 7 < K 8"), (dict(metric=2), "unknown metric 2"), (dict(metric=-1), "unknown metric -1"),
           (dict(ld_est=3), "ld_est 3 < 4"), (dict(metric=hip.CONF_EUCLID, ld_est=2), "ld_est 2 < 3"),
           (dict(logits=Z + 2), "logits must be 4-byte aligned"), (dict(est=E + 4), "est and out must be 8-byte aligned"),
           (dict(out=O + 4), "est and out must be 8-byte aligned"), (dict(map=M + 8), "the map must be 16-byte aligned"),
           (dict(metric=hip.CONF_EUCLID, map=M + 4), "the map must be 8-byte aligned")]
    bad_score = bad + [(dict(ref=None), "null pointer"), (dict(ld_ref=3), "ld_ref 3 < 4"), (dict(metric=hip.CONF_EUCLID, ld_ref=2), "ld_ref 2 < 3"),
                       (dict(ref=RF + 4), "ref must be 8-byte aligned")]
    bad_bound = bad + [(dict(q=0.0), "q must be > 0"), (dict(q=-0.5), "q must be > 0"), (dict(q=nan), "q must be > 0"), (dict(q=-inf), "q must be > 0")]
    for fn, name, cases in ((score, "score", bad_score), (bound, "bound", bad_bound)):
        for kw, msg in cases:
            assert fn(**kw) == -1, kw
            err = hip.last_error()
            assert err.startswith("urso_conf_%s:" % name) and msg in err, (kw, err)
    for fn, name in ((lib.urso_conf_score, "score"), (lib.urso_conf_bound, "bound")):
        assert fn(None, None) == -1 and "urso_conf_%s: null argument struct" % name in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU); the refusals come in front of it
    assert score(n=0) == 0 and score(n=0, B=0) == 0 and bound(n=0) == 0 and bound(n=0, q=inf) == 0 and bound(n=0, q=1e-300) == 0
    assert score(n=0, K=2 ** 18, ld_z=2 ** 18, logits=Z + 4, metric=hip.CONF_EUCLID, map=M + 8, ld_est=3, ld_ref=3) == 0
    assert score(n=0, K=0) == -1 and bound(n=0, q=0.0) == -1 and bound(n=0, metric=7) == -1
