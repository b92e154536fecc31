"""BN recalibration without a GPU (recalibrate_bn, Config.BN_RECAL_BATCHES): the NumPy float64 rule of
ursonet_amd/bn_recal.py against pooled statistics in exact rational arithmetic within bounds counted from its roundings, the one-batch
case that is exact, the channel a NaN stays in, whole_batches, the key and its refusals, the refusal messages of the public call, the
report, and every refusal of the three entry points with made-up pointers that are never dereferenced."""
import ctypes
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

from ursonet_amd import bn_recal as R
from ursonet_amd.config import Config

U = 2.0 ** -53                                   # unit roundoff of float64
U32 = 2.0 ** -24                                 # unit roundoff of float32
TINY32 = 2.0 ** -150                             # half the smallest float32 subnormal: the absolute rounding error down there


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stats(T, N, seed, mean_spread=1.0):
    """T batches of N float32 (mu_b, v_b): channel scales across 2^-20 .. 2^20, zeros and subnormals among means and variances."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.integers(-20, 21, size=N)
    mu = (scale * (rng.normal(size=N) + mean_spread * rng.normal(size=(T, N)))).astype(np.float32)
    v = (scale ** 2 * rng.uniform(0.0, 2.0, size=(T, N))).astype(np.float32)
    mu[:, 0] = 0.0
    v[:, 1] = 0.0
    mu[:, 2] = (rng.integers(-50, 50, size=T) * 2.0 ** -149).astype(np.float32)          # subnormal means
    v[:, 3] = (rng.integers(0, 50, size=T) * 2.0 ** -149).astype(np.float32)             # subnormal variances
    mu[0, 4], v[0, 4] = 0.0, 0.0                                                         # one batch of a channel all zero
    return mu, v


def _fold(mu, v, M):
    acc = R.pool_zero(mu.shape[1])
    for t in range(mu.shape[0]):
        acc = R.pool_add64(acc, mu[t], v[t], M, t)
    return acc


def _exact(mu, v, M):
    """Per channel (mean, m2, var) of the pooled population as Fractions, from the same float32 batch statistics."""
    T, N = mu.shape
    out = []
    for c in range(N):
        ms = [Fraction(float(x)) for x in mu[:, c]]
        vs = [Fraction(float(x)) for x in v[:, c]]
        mean = sum(ms) / T
        m2 = sum(M * (vb + (mb - mean) ** 2) for mb, vb in zip(ms, vs))
        out.append((mean, m2, m2 / (T * M)))
    return out


# ------------------------------------------------------------------ against exact rationals
@pytest.mark.parametrize("M", [1, 3, 8, 1000, 2621440, 2 ** 22 + 1])
@pytest.mark.parametrize("T", [2, 5])
def test_fold_against_exact_rationals(T, M):
    """Bounds, counted per path (u = 2^-53, A = max |mu_b| of the channel; n, M, n1 = n + M and n * M are exact integers):

    mean.  Batch k computes d = fl(mu_k - mean), fl(fl(d * M) / n1) and fl(mean + .): three roundings on a step of size |d| M / n1 <=
    2 A / k and one on a value <= A.  The exact recurrence mean_k = mean_{k-1} (1 - 1/k) + mu_k / k does not amplify the error carried in,
    so E_T <= sum_k (3 * 2 A / k + A) u = (6 H_T + T) u A.

    m2.  A sum of non-negative terms v_k M + d^2 (n M / n1): each term takes 6 roundings (v M; d d; n M; the division; the product; the
    sum) and the running sum T more, a relative error (T + 6) u of the sum.  The term is formed with the computed d, which is off by at
    most E_{k-1} + u |d| <= E + 2 u A; |d_computed| + |d| <= 4 A and n M / n1 <= M, so that adds at most 4 A (E + 2 u A) M per batch,
    absolutely.

    settle.  One more float64 rounding for m2 / n, then the rounding to float32 (relative 2^-24, or half a subnormal step).
    A factor 1.01 covers the second-order terms."""
    N = 48
    mu, v = _stats(T, N, seed=100 * T + M % 97)
    mean, m2 = _fold(mu, v, M)
    mm, mv = R.pool_settle32((mean, m2), M, T)
    assert mean.dtype == m2.dtype == np.float64 and mm.dtype == mv.dtype == np.float32
    H = sum(1.0 / k for k in range(1, T + 1))
    worst = [0.0, 0.0]
    for c, (e_mean, e_m2, e_var) in enumerate(_exact(mu, v, M)):
        A = float(np.max(np.abs(mu[:, c])))
        E = 1.01 * (6 * H + T) * U * A
        absolute = 1.01 * T * M * 4 * A * (E + 2 * U * A)
        b_m2 = 1.01 * (T + 6) * U * (float(e_m2) + absolute) + absolute
        err_mean = abs(Fraction(float(mean[c])) - e_mean)
        err_m2 = abs(Fraction(float(m2[c])) - e_m2)
        assert err_mean <= E, (c, float(err_mean), E)
        assert err_m2 <= b_m2, (c, float(err_m2), b_m2)
        assert m2[c] >= 0.0
        b_mm = E + U32 * float(abs(e_mean)) + TINY32
        b_mv = b_m2 / (T * M) + (U + U32) * 1.01 * float(e_var) + TINY32
        assert abs(Fraction(float(mm[c])) - e_mean) <= b_mm, (c, float(mm[c]), float(e_mean), b_mm)
        assert abs(Fraction(float(mv[c])) - e_var) <= b_mv, (c, float(mv[c]), float(e_var), b_mv)
        if A > 0:
            worst[0] = max(worst[0], float(err_mean) / (U * A))
        if e_m2 > 0:
            worst[1] = max(worst[1], float(err_m2 / e_m2) / U)
    print("T=%d M=%d  worst mean error %.2f u A, worst m2 error %.2f u m2" % (T, M, worst[0], worst[1]))


def test_pooled_variance_is_not_the_mean_of_batch_variances():
    """Two batches with zero variance each and different means: the pooled variance is the spread of the means."""
    mu = np.array([[1.0], [3.0]], dtype=np.float32)
    v = np.zeros((2, 1), dtype=np.float32)
    mm, mv = R.pool_settle32(_fold(mu, v, 16), 16, 2)
    assert mm[0] == 2.0 and mv[0] == 1.0 and float(np.mean(v)) == 0.0


# ------------------------------------------------------------------ one batch is exact
@pytest.mark.parametrize("M", [1, 2, 3, 7, 4096, 2621440, 2 ** 22 - 1])
def test_one_batch_gives_its_statistics_back_bit_for_bit(M):
    """M < 2^22: mu_b * M and v_b * M are exact in float64 (24 + 22 bits), the divisions give the inputs back, and the float32
    conversion is exact.  (A mean of -0.0 would come back as +0.0: 0.0 + -0.0; the engine never produces one.)"""
    rng = np.random.default_rng(M)
    mu = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    v = np.abs(rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32).view(np.float32)).copy()
    keep = np.isfinite(mu) & np.isfinite(v) & ~((mu == 0) & np.signbit(mu))
    mu, v = mu[keep], v[keep]
    mu[:4] = np.array([0.0, 2.0 ** -149, -2.0 ** -149, np.finfo(np.float32).max], dtype=np.float32)
    v[:4] = np.array([2.0 ** -149, 0.0, np.finfo(np.float32).max, 0.0], dtype=np.float32)
    acc = R.pool_add64(R.pool_zero(mu.size), mu, v, M, 0)
    mm, mv = R.pool_settle32(acc, M, 1)
    assert np.array_equal(_bits(mm), _bits(mu)) and np.array_equal(_bits(mv), _bits(v))


def test_a_nan_stays_in_its_channel():
    mu, v = _stats(3, 16, seed=7)
    clean = R.pool_settle32(_fold(mu, v, 8), 8, 3)
    mu2, v2 = mu.copy(), v.copy()
    mu2[1, 5] = np.nan
    v2[2, 9] = np.inf
    mm, mv = R.pool_settle32(_fold(mu2, v2, 8), 8, 3)
    assert not np.isfinite(mm[5]) and not np.isfinite(mv[5]) and not np.isfinite(mv[9])
    others = np.ones(16, dtype=bool)
    others[[5, 9]] = False
    assert np.array_equal(_bits(mm[others]), _bits(clean[0][others])) and np.array_equal(_bits(mv[others]), _bits(clean[1][others]))
    assert np.array_equal(_bits(mm[9]), _bits(clean[0][9]))                  # an infinite variance leaves its channel's mean alone


def test_the_rule_refuses_bad_counts():
    acc = R.pool_zero(2)
    z = np.zeros(2, dtype=np.float32)
    for M in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="M must be"):
            R.pool_add64(acc, z, z, M, 0)
    for t in (-1, 0.5, True):
        with pytest.raises(ValueError, match="t must be"):
            R.pool_add64(acc, z, z, 4, t)
    with pytest.raises(ValueError, match="t must be an int >= 1"):
        R.pool_settle32(acc, 4, 0)
    with pytest.raises(ValueError, match="2\\^53"):
        R.pool_add64(acc, z, z, 2 ** 30, 2 ** 23)
    with pytest.raises(ValueError, match="2\\^53"):
        R.pool_settle32(acc, 2 ** 30, 2 ** 23 + 1)
    a2 = R.pool_add64(acc, z + 1, z, 4, 0)
    assert a2[0] is not acc[0] and not acc[0].any()                          # new arrays


# ------------------------------------------------------------------ helpers
def test_whole_batches():
    assert R.whole_batches(range(5), 2) == ([0, 1, 2, 3], 1)
    assert R.whole_batches([7, 8, 9], 3) == ([7, 8, 9], 0)
    assert R.whole_batches([7, 8], 3) == ([], 2)
    assert R.whole_batches([], 4) == ([], 0)
    assert R.whole_batches(np.arange(9), 4) == (list(range(8)), 1)
    for B in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="batch size"):
            R.whole_batches([1, 2], B)


def test_key_default_and_validation():
    assert Config().BN_RECAL_BATCHES == 0
    assert R.validate(Config()) == 0 and R.validate(object()) == 0 and not R.enabled(Config())
    assert R.validate(_cfg(BN_RECAL_BATCHES=0), world=8) == 0                # off: nothing to refuse under a launcher
    assert R.validate(_cfg(BN_RECAL_BATCHES=0, TRAIN_BN=False)) == 0
    on = _cfg(BN_RECAL_BATCHES=3, WEIGHT_EMA=0.99, TRAIN_BN=None)
    assert R.validate(on) == 3 and R.enabled(on, "training") and not R.enabled(on, "inference")
    assert R.validate(_cfg(BN_RECAL_BATCHES=np.int64(2), WEIGHT_EMA=0.9, TRAIN_BN=None)) == 2
    for bad in (True, False, -1, 1.0, "2", None, [1], np.True_, float("nan")):
        with pytest.raises(ValueError, match="BN_RECAL_BATCHES must be an int >= 0"):
            R.validate(_cfg(BN_RECAL_BATCHES=bad, WEIGHT_EMA=0.99, TRAIN_BN=None))
    with pytest.raises(ValueError, match="BN_RECAL_BATCHES = 2 needs WEIGHT_EMA"):
        R.validate(_cfg(BN_RECAL_BATCHES=2, TRAIN_BN=None))
    for frozen in (False, True):
        with pytest.raises(ValueError, match="needs batch-statistics BatchNorm \\(TRAIN_BN = None\\)"):
            R.validate(_cfg(BN_RECAL_BATCHES=2, WEIGHT_EMA=0.99, TRAIN_BN=frozen))
    with pytest.raises(ValueError, match="BN_RECAL_BATCHES.*data parallelism.*world size 2"):
        R.validate(on, world=2)


def test_the_public_call_refuses_other_models_with_the_way_to_one():
    ds = types.SimpleNamespace(image_ids=list(range(8)))
    howto = "UrsoNet\\('training', cfg\\).*TRAIN_BN = None.*load_weights.*recalibrate_bn.*save_weights"
    inference = types.SimpleNamespace(mode="inference", _engine=types.SimpleNamespace(train_bn=False, B=2), config=Config())
    frozen = types.SimpleNamespace(mode="training", _engine=types.SimpleNamespace(train_bn=False, B=2), config=Config())
    for model in (inference, frozen, types.SimpleNamespace(mode="training", _engine=None)):
        with pytest.raises(ValueError, match=howto):
            R.recalibrate_bn(model, ds)


def test_report_and_lines():
    slices = {("bn_a", "moving_mean"): (0, 3, (3,)), ("bn_a", "moving_variance"): (4, 3, (3,)),
              ("bn_b", "moving_mean"): (8, 2, (2,)), ("bn_b", "moving_variance"): (12, 2, (2,))}
    before = np.zeros(16, dtype=np.float32)
    after = np.zeros(16, dtype=np.float32)
    before[4:7], before[12:14] = 1.0, 4.0
    after[0:3], after[4:7] = [0.0, 2.0, -1.0], [1.0, 3.0, 0.5]
    after[8:10], after[12:14] = [4.0, 0.0], [4.0, 8.0]
    after[3] = after[7] = np.nan                                             # padding is not looked at
    rep = R.shift_report(slices, before, after, eps=0.0)
    assert list(rep) == ["bn_a", "bn_b"] and rep["bn_a"] == (2.0, 3.0) and rep["bn_b"] == (2.0, 2.0)
    res = R.BNRecalResult(4, 1, 2, rep)
    assert (res.images_used, res.images_dropped, res.batches) == (4, 1, 2) and res.layers == rep
    text = "\n".join(res.lines())
    assert "4 images in 2 batches" in text and "1 dropped" in text and "2 BN layers" in text and "bn_a" in text
    assert "dropped" not in "\n".join(R.BNRecalResult(4, 0, 2, rep).lines())


def test_module_imports_neither_torch_nor_the_library():
    code = "import sys; import ursonet_amd.bn_recal; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True).returncode == 0


# ------------------------------------------------------------------ the entry points' refusals
def test_argument_validation_without_gpu():
    """Every refusal of the three entry points.  Device pointers are made up and never dereferenced: each call is refused before the
    copy of the table or the launch."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("train")
    assert {"urso_bn_recal_plan", "urso_bn_recal_add", "urso_bn_recal_settle"} <= set(hip.SIDE_SYMBOLS["train"])
    assert ctypes.sizeof(hip.BnRecalLayer) == 48
    BM, BV, TAB, ACC, ST = (0x100000 * k for k in range(1, 6))

    def table(*rows):
        t = (hip.BnRecalLayer * len(rows))()
        for r, (m, v, N, M, om, ov) in zip(t, rows):
            r.bmean, r.bvar, r.N, r.M, r.off_mean, r.off_var = m, v, N, M, om, ov
        return t
    good = [(BM, BV, 5, 8, 0, 8), (BM + 64, BV + 64, 3, 2, 16, 20)]

    def changed(row, **kw):
        names = ("bmean", "bvar", "N", "M", "off_mean", "off_var")
        rows = [list(r) for r in good]
        for k, val in kw.items():
            rows[row][names.index(k)] = val
        return table(*[tuple(r) for r in rows])
    bad_tables = [(changed(0, bmean=None), "null"), (changed(1, bvar=None), "null"), (changed(0, bmean=BM + 2), "4-byte aligned"),
                  (changed(1, bvar=BV + 1), "4-byte aligned"), (changed(0, N=0), "N must be > 0"), (changed(1, N=-3), "N must be > 0"),
                  (changed(0, M=0), "M must be > 0"), (changed(1, M=-1), "M must be > 0"), (changed(0, off_mean=-4), "negative offset"),
                  (changed(1, off_var=-1), "negative offset"), (changed(1, off_var=22), "ends behind n_stats"),
                  (changed(0, off_var=4), "overlap"), (changed(1, off_mean=12), "overlap"), (changed(1, off_mean=2), "overlap"),
                  (changed(1, off_var=16), "overlap")]
    calls = {"urso_bn_recal_plan": lambda t, L=2, n=24, tab=TAB: lib.urso_bn_recal_plan(L, t, n, tab),
             "urso_bn_recal_add": lambda t, L=2, n=24, tab=TAB, acc=ACC, k=0: lib.urso_bn_recal_add(L, t, tab, n, acc, k, None),
             "urso_bn_recal_settle": lambda t, L=2, n=24, tab=TAB, acc=ACC, st=ST, k=1: lib.urso_bn_recal_settle(L, t, tab, n, acc, st, k, None)}
    ok = table(*good)
    for fn, call in calls.items():
        cases = [(lambda t=t: call(t), msg) for t, msg in bad_tables]
        cases += [(lambda: call(ok, L=0), "L must be"), (lambda: call(ok, L=-1), "L must be"), (lambda: call(ok, L=65536), "L must be"),
                  (lambda: call(None), "null"), (lambda: call(ok, tab=None), "null"), (lambda: call(ok, tab=TAB + 4), "8-byte aligned"),
                  (lambda: call(ok, n=0), "n_stats must be > 0"), (lambda: call(ok, n=22), "ends behind n_stats")]
        if fn != "urso_bn_recal_plan":
            cases += [(lambda: call(ok, acc=None), "null"), (lambda: call(ok, acc=ACC + 4), "8-byte aligned"),
                      (lambda: call(ok, k=-1), "t must be >= "), (lambda: call(ok, k=2 ** 53), "2^53"),
                      (lambda: call(changed(0, M=2 ** 40), k=2 ** 13 + 1), "2^53")]
        if fn == "urso_bn_recal_settle":
            cases += [(lambda: call(ok, k=0), "nothing was added"), (lambda: call(ok, st=None), "null"),
                      (lambda: call(ok, st=ST + 2), "4-byte aligned")]
        for run, msg in cases:
            assert run() == -1, (fn, msg)
            err = hip.last_error()
            assert err.startswith(fn + ":") and msg in err, (fn, msg, err)
