"""Temperature scaling without a GPU (calibrate(), predict / evaluate / test_and_submit with calibration=..., ursonet_amd/calibrate.py):
stats64 against a direct float64 restatement, the convexity the search relies on, fit64 on planted temperatures, its clamped / flat /
non-finite ends, the bounds of tests/tempref.py against simulated kernels with one wrong operation, the Calibration file, every
refusal of the public interface before torch, the engine or the library is touched, the surface of liburso_train.so against header and
bindings, and the three entry points' argument checks (they run before any launch)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tempref as R
from libsurface import header_symbols
from ursonet_amd import calibrate as Cal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_train.h")
TEMP_NAMES = {"urso_temp_stats", "urso_temp_reduce", "urso_temp_scale"}


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("K", [1, 2, 63, 257])
def test_stats64_is_the_cross_entropy_and_its_derivatives(K):
    """Against the definitions written out directly (no shift by the maximum, probabilities formed explicitly), and CE's derivatives
    against central differences of CE itself."""
    rng = np.random.default_rng(K)
    z = rng.normal(size=(3, K)).astype(np.float32) * 3
    y = rng.uniform(0.1, 1, size=(3, K)).astype(np.float32)
    betas = [0.3, 1.0, 2.5]
    rows = Cal.stats64(z, y, betas)
    z64, y64 = z.astype(np.float64), y.astype(np.float64)
    assert np.allclose(rows[:, Cal.SY], y64.sum(axis=1), rtol=1e-14) and np.allclose(rows[:, Cal.YZ], (y64 * z64).sum(axis=1), rtol=1e-12, atol=1e-12)
    ce, g, h, bad = Cal.row_terms(rows, betas)
    assert not bad.any()

    def direct(b):
        e = np.exp(b * z64)
        p = e / e.sum(axis=1, keepdims=True)
        return np.log(e.sum(axis=1)), (p * z64).sum(axis=1), (p * z64 ** 2).sum(axis=1) - (p * z64).sum(axis=1) ** 2, -(y64 * np.log(p)).sum(axis=1)
    for j, b in enumerate(betas):
        lse, m1, var, xent = direct(b)
        assert np.allclose(rows[:, Cal.LSE + 3 * j], lse, rtol=1e-12, atol=1e-12)
        assert np.allclose(rows[:, Cal.M1 + 3 * j], m1, rtol=1e-11, atol=1e-11)
        assert np.allclose(rows[:, Cal.VAR + 3 * j], var, rtol=1e-9, atol=1e-11)
        assert np.allclose(ce[:, j], xent, rtol=1e-11, atol=1e-11)           # CE = -sum y log softmax(beta z)
        step = 1e-5
        up, dn = direct(b + step)[3], direct(b - step)[3]
        assert np.allclose(g[:, j], (up - dn) / (2 * step), rtol=1e-6, atol=1e-7)
        assert np.allclose(h[:, j], (up - 2 * xent + dn) / step ** 2, rtol=1e-3, atol=1e-4)
    tot = Cal.reduce64(rows, betas)
    assert tot.shape == (3, 4) and np.allclose(tot[:, 0], ce.sum(axis=0)) and np.all(tot[:, 3] == 0)
    one = np.float32(3.25)
    assert np.array_equal(Cal.scale32(z, 1.0).view(np.int32), z.view(np.int32)) and Cal.scale32([one], 0.1)[0] == np.float32(float(one) * 0.1)


def test_degenerate_rows():
    z = np.array([[1, 2, -np.inf, 0.5], [1, np.nan, 0, 0], [np.inf, 0, 0, 0], [-np.inf] * 4, [2, 2, 2, 2]], dtype=np.float32)
    y = np.array([[0.5, 0.5, 0, 0], [0.25] * 4, [0.25] * 4, [0.25] * 4, [0, 0, 0, 0]], dtype=np.float32)
    rows = Cal.stats64(z, y, [0.5, 2.0])
    assert np.all(np.isfinite(rows[0])) and rows[0, Cal.YZ] == 1.5                # a -inf bin without weight vanishes from every sum
    assert np.all(np.isnan(rows[1:4]))                                             # NaN, +inf, all -inf: every column NaN
    assert np.all(rows[4, [Cal.SY, Cal.YZ, Cal.M1 + 0, Cal.VAR + 0, Cal.VAR + 3]] == [0, 0, 2, 0, 0])
    assert rows[4, Cal.LSE] == np.log(4.0) + 0.5 * 2 and rows[4, Cal.LSE + 3] == np.log(4.0) + 2.0 * 2
    tot = Cal.reduce64(rows, [0.5, 2.0])
    assert np.all(tot[:, 3] == 3) and np.all(np.isnan(tot[:, :3]))
    weighs_inf = Cal.stats64(z[:1], np.array([[0, 0, 1, 0]], dtype=np.float32), [1.0])
    assert weighs_inf[0, Cal.YZ] == -np.inf and Cal.reduce64(weighs_inf, [1.0])[0, 3] == 1


@pytest.mark.parametrize("K", R.KS)
def test_the_slope_does_not_decrease_over_the_grid(K):
    """Convexity: g over GRID is non-decreasing, for the kernel cases and for a planted one -- up to the rounding of g itself."""
    sets = [R.logits_and_targets(K, 1.0), R.planted(max(K, 2), 1.0)]
    for z, y in sets:
        ce, g, h, bad = Cal.row_terms(Cal.stats64(z, y, Cal.GRID), Cal.GRID)
        assert not bad.any() and np.all(h >= -R.tol(z.shape[1]) * np.abs(h).max())
        scale = R.tol(z.shape[1]) * (np.abs(z[np.isfinite(z)]).max() * np.abs(y).sum(axis=1, keepdims=True) + 1e-300)
        assert np.all(np.diff(g, axis=1) >= -2 * scale), (K, g)
        assert np.all(np.diff(g.sum(axis=0)) >= -2 * scale.sum())


# ------------------------------------------------------------------ the search
@pytest.mark.parametrize("b0", R.PLANT_B0)
@pytest.mark.parametrize("K", R.PLANT_KS)
def test_fit64_recovers_a_planted_temperature(K, b0):
    """Targets softmax64(b0 z) rounded to fp32: the fit gives b0 back to 1e-6 relative (the residue is the targets' fp32 rounding),
    within 16 passes, and the loss at the fit is not above the loss at beta = 1."""
    z, y = R.planted(K, b0)
    beta, info = Cal.fit64(z, y)
    print("K=%d b0=%g: beta %.12g, relative error %.3g, passes %d" % (K, b0, beta, abs(beta - b0) / b0, info["passes"]))
    assert info["converged"] and not info["clamped"] and not info["flat"] and info["passes"] <= Cal.MAX_PASSES
    assert abs(beta - b0) <= 1e-6 * b0
    assert info["nll_after"] <= info["nll_before"] * (1 + R.tol(K)) and (b0 == 1.0 or info["nll_after"] < info["nll_before"])   # (CE's own rounding)
    tight, tinfo = Cal.fit64(z, y, tol=R.REF_TOL)
    assert tinfo["converged"] and abs(beta - tight) <= R.beta_bound(z, y, tight)


def test_the_bracket_alone_converges_within_the_cap():
    """With Newton's point taken away (h reported as 0 makes every Newton point fall back to a subdivision point) the 8-fold shrink
    alone ends within 16 passes, from the grid and from the piece next to either bound."""
    for b0 in (1.3, 1.0 / 40, 40.0):
        z, y = R.planted(63, b0)

        def no_newton(betas):
            t = Cal.reduce64(Cal.stats64(z, y, betas), betas)
            t[:, 2] = 1e-300
            return t
        beta, info = Cal.search(no_newton, z.shape[0])
        print("b0=%g without Newton: beta %.12g passes %d bracket %r" % (b0, beta, info["passes"], info.get("bracket")))
        assert info["converged"] and info["passes"] <= Cal.MAX_PASSES and abs(beta - b0) <= 1e-6 * b0


def test_clamped_flat_and_not_finite():
    z, y = R.planted(63, 1.0)
    sharp = np.zeros_like(y)
    sharp[np.arange(len(z)), z.argmax(axis=1)] = 1                                # one-hot at the arg max: the loss falls for ever
    beta, info = Cal.fit64(z, sharp)
    assert beta == Cal.BETA_MAX and info["clamped"] and not info["flat"] and info["nll_after"] < info["nll_before"]
    blunt = np.full_like(y, 1.0 / y.shape[1])                                     # the uniform target: beta -> 0
    beta, info = Cal.fit64(z, blunt)
    assert beta == Cal.BETA_MIN and info["clamped"]
    beta, info = Cal.fit64(np.full_like(z, 0.75), y)
    assert beta == 1.0 and info["flat"] and not info["clamped"] and info["passes"] == 1 and info["nll_after"] == info["nll_before"]
    bad = z.copy()
    bad[3, 5] = np.nan
    bad[7, 0] = np.inf
    with pytest.raises(ValueError, match=r"2 of %d rows are not finite" % len(z)):
        Cal.fit64(bad, y)


# ------------------------------------------------------------------ the bounds reject a wrong kernel
@pytest.mark.parametrize("K", [2, 63, 4096])
def test_bounds_reject_a_kernel_with_one_wrong_operation(K):
    z, y = R.logits_and_targets(K, 1.0)
    betas = R.betas_of(8)
    good = Cal.stats64(z, y, betas)
    fig = R.check_stats(good, z, y, betas)
    assert max(fig.values()) == 0
    m = z.max(axis=1).astype(np.float64)
    no_shift = good.copy()                                                        # LSE without its beta_j m
    for j, b in enumerate(betas):
        no_shift[:, Cal.LSE + 3 * j] -= b * m
    assert R.check_stats(no_shift, z, y, betas)["LSE"] > 1e6
    no_square = good.copy()                                                       # VAR = Q / Z alone
    for j in range(len(betas)):
        no_square[:, Cal.VAR + 3 * j] += (good[:, Cal.M1 + 3 * j] - m) ** 2
    assert R.check_stats(no_square, z, y, betas)["VAR"] > 1e6
    in_fp32 = good.astype(np.float32).astype(np.float64)                          # a kernel that accumulates in fp32
    worst = R.check_stats(in_fp32, z, y, betas)
    assert max(worst.values()) > 1e3, worst


# ------------------------------------------------------------------ the file
def test_calibration_round_trip_is_bit_for_bit(tmp_path):
    fit = dict(nll_before=0.1 + 0.2, nll_after=1.0 / 3, passes=5, clamped=False, flat=False, converged=True, extra="dropped")
    c = Cal.Calibration(ori_beta=np.pi / 3, loc_beta=float(np.nextafter(1.0, 2.0)), k_ori=512, k_loc=64, n_images=7, ori_fit=fit, loc_fit=fit)
    p = c.save(str(tmp_path / "cal.json"))
    d = Cal.Calibration.load(p)
    assert d == c and d.ori_beta.hex() == (np.pi / 3).hex() and d.loc_beta.hex() == float(np.nextafter(1.0, 2.0)).hex()
    assert d.ori_nll_before.hex() == (0.1 + 0.2).hex() and d.loc_nll_after.hex() == (1.0 / 3).hex() and d.ori_passes == 5 and d.loc_clamped is False
    assert d.ori_temperature == 1.0 / (np.pi / 3) and d.k_ori == 512 and d.n_images == 7 and "extra" not in d.ori_fit
    hand = Cal.Calibration(ori_beta=2)
    assert hand.ori_beta == 2.0 and hand.loc_beta is None and hand.loc_temperature is None and hand.ori_passes is None and hand.k_ori is None
    assert Cal.Calibration.load(hand.save(str(tmp_path / "hand.json"))) == hand
    assert hand.line() == "Calibration: orientation T = 0.5 (beta 2.0)" and Cal.Calibration().line() == "Calibration: no head is scaled"
    for bad in (0, -1.0, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError, match="ori_beta must be a finite number > 0"):
            Cal.Calibration(ori_beta=bad)
    with pytest.raises(AttributeError):
        hand.no_such_field
    hand.check_model(512, 0)
    c.check_model(512, 64)
    with pytest.raises(ValueError, match="fitted on a ori head of 512 bins, the model's has 4096"):
        c.check_model(4096, 64)
    with pytest.raises(ValueError, match="ori_beta = 2.0, but the model's orientation head is a regression head"):
        hand.check_model(0, 64)


def test_size_check_names_the_figure():
    assert Cal.buffer_bytes(1000, 64 ** 3, 0) == 1000 * 64 ** 3 * 8 and Cal.check_size(1000, 64 ** 3, 27, 16) == 1000 * (64 ** 3 + 27) * 8
    with pytest.raises(ValueError, match=r"calibrate: the logits and targets of 1000 images \(262144 orientation and 0 location bins in fp32\) "
                                         r"need 1\.953 GiB on the device, more than max_gb = 1;"):
        Cal.check_size(1000, 64 ** 3, 0, 1)
    for bad in (0, -1, float("nan"), None, "x"):
        with pytest.raises(ValueError, match="max_gb must be a number > 0"):
            Cal.check_size(10, 8, 0, bad)


def test_interface_refuses_before_torch_the_engine_or_the_library():
    code = """
import os, sys
import pytest
from ursonet_amd import calibrate, evaluate, predict, submission
class Boom(object):
    def __getattr__(self, name):
        raise AssertionError("touched %s" % name)
class Cfg(object):
    REGRESS_ORI = REGRESS_LOC = True
    REGRESS_KEYPOINTS = False
class Model(object):
    mode, config, _dp, _world = "inference", Cfg(), None, 1
    _engine = property(lambda self: Boom().engine)
cal = calibrate.Calibration(ori_beta=2.0)
for fn, who in ((predict.predict, "predict"), (evaluate.evaluate, "evaluate")):
    for kw, msg in ((dict(calibration=2.0), "calibration must be a calibrate.Calibration"),
                    (dict(calibration={"ori_beta": 2.0}), "calibration must be a calibrate.Calibration"),
                    (dict(calibration=cal, members=[{"a": {}}]), "calibrate and predict each member on its own")):
        with pytest.raises(ValueError) as err:
            fn(Boom(), Boom(), **kw)
        assert msg in str(err.value) and str(err.value).startswith(who), err.value
with pytest.raises(ValueError, match="calibrate and predict each member on its own"):
    submission.test_and_submit(Boom(), Boom(), Boom(), members=[{"a": {}}], calibration=cal)
for kw in (dict(members=[{"a": {}}]), dict(views=[[0, 0, 5]])):
    with pytest.raises(ValueError, match="calibrate: members=... and views=... are not supported"):
        calibrate.calibrate(Boom(), Boom(), **kw)
with pytest.raises(ValueError, match="calibrate: the model has no classification head"):
    calibrate.calibrate(Model(), Boom())
os.environ["WORLD_SIZE"] = "2"
with pytest.raises(ValueError, match="calibrate is not supported under a data-parallel launcher"):
    calibrate.calibrate(Boom(), Boom())
assert "torch" not in sys.modules and "ursonet_amd.hip" not in sys.modules and "ursonet_amd.engine" not in sys.modules
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["train"]) and TEMP_NAMES <= names and len(names) == 13
    assert "calibrate.hip" in build.SIDE_SOURCES["train"]
    for macro, v in (("MAX_J", Cal.MAX_J), ("COLS", Cal.COLS), ("TOTALS", Cal.TOTALS), ("SY", Cal.SY), ("YZ", Cal.YZ), ("LSE", Cal.LSE),
                     ("M1", Cal.M1), ("VAR", Cal.VAR)):
        assert re.search(r"#define\s+URSO_TEMP_%s\s+%d\b" % (macro, v), txt), macro
        assert getattr(hip, "TEMP_" + macro) == v
    assert Cal.COLS == 2 + 3 * Cal.MAX_J and len(Cal.GRID) == Cal.MAX_J and Cal.GRID[3] == 1.0
    # the argument structs are the header's: field order and sizes
    assert [f[0] for f in hip.TempStatsArgs._fields_] == ["B", "n", "row0", "K", "ld_z", "ld_y", "J", "beta", "logits", "target", "out"]
    assert [f[0] for f in hip.TempReduceArgs._fields_] == ["N", "J", "pad", "beta", "rows", "totals"]
    assert [f[0] for f in hip.TempScaleArgs._fields_] == ["B", "n", "K", "ld_in", "ld_out", "pad", "beta", "in_", "out"]
    assert C.sizeof(hip.TempStatsArgs) == 120 and C.sizeof(hip.TempReduceArgs) == 96 and C.sizeof(hip.TempScaleArgs) == 48
    assert hip.TempStatsArgs.beta.offset == 32 and hip.TempReduceArgs.beta.offset == 16 and hip.TempScaleArgs.beta.offset == 24


def test_argument_validation_without_gpu():
    """Every refusal of the three entry points.  Device pointers are made up and never dereferenced: each call is refused before a
    launch, or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("train")
    Z, Y, O, T = (0x1000000 * k for k in range(1, 5))

    def fill(a, base, kw):
        for k, v in dict(base, **kw).items():
            if k == "beta" and not isinstance(v, float):
                for j, b in enumerate(v):
                    a.beta[j] = b
            else:
                setattr(a, k, v)
        return a

    def stats(**kw):
        a = fill(hip.TempStatsArgs(), dict(B=4, n=3, row0=0, K=8, ld_z=8, ld_y=8, J=2, beta=[0.5, 2.0], logits=Z, target=Y, out=O), kw)
        return lib.urso_temp_stats(C.byref(a), None)

    def reduce(**kw):
        a = fill(hip.TempReduceArgs(), dict(N=5, J=2, pad=0, beta=[0.5, 2.0], rows=O, totals=T), kw)
        return lib.urso_temp_reduce(C.byref(a), None)

    def scale(**kw):
        a = fill(hip.TempScaleArgs(), dict(B=4, n=3, K=8, ld_in=8, ld_out=8, pad=0, beta=2.0, in_=Z, out=Y), kw)
        return lib.urso_temp_scale(C.byref(a), None)
    nan, inf = float("nan"), float("inf")
    bad_betas = [(dict(J=0), "1 <= J <= 8"), (dict(J=9), "1 <= J <= 8"), (dict(J=-1), "1 <= J <= 8"), (dict(beta=[0.5, 0.0]), "beta[1] must be finite and > 0"),
                 (dict(beta=[-1.0, 2.0]), "beta[0] must be finite and > 0"), (dict(beta=[nan, 2.0]), "beta[0] must be finite"),
                 (dict(beta=[0.5, inf]), "beta[1] must be finite")]
    bad_stats = bad_betas + [(dict(logits=None), "null pointer"), (dict(target=None), "null pointer"), (dict(out=None), "null pointer"),
                             (dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"), (dict(B=-1, n=0), "0 <= n <= B"), (dict(row0=-1), "row0 must be >= 0"),
                             (dict(K=0), "K must be >= 1"), (dict(K=-3, ld_z=-3, ld_y=-3), "K must be >= 1"), (dict(ld_z=7), "ld_z 7 < K 8"),
                             (dict(ld_y=7), "ld_y 7 < K 8"), (dict(logits=Z + 2), "4-byte aligned"), (dict(target=Y + 1), "4-byte aligned"),
                             (dict(out=O + 4), "out must be 8-byte aligned")]
    for kw, msg in bad_stats:
        assert stats(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_temp_stats:") and msg in err, (kw, err)
    bad_reduce = bad_betas + [(dict(rows=None), "null pointer"), (dict(totals=None), "null pointer"), (dict(N=0), "N must be >= 1"),
                              (dict(N=-4), "N must be >= 1"), (dict(rows=O + 4), "8-byte aligned"), (dict(totals=T + 2), "8-byte aligned")]
    for kw, msg in bad_reduce:
        assert reduce(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_temp_reduce:") and msg in err, (kw, err)
    bad_scale = [(dict(in_=None), "null pointer"), (dict(out=None), "null pointer"), (dict(beta=0.0), "beta must be finite and > 0"),
                 (dict(beta=-2.0), "beta must be finite"), (dict(beta=nan), "beta must be finite"), (dict(beta=inf), "beta must be finite"),
                 (dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"), (dict(K=0), "K must be >= 1"), (dict(ld_in=7), "ld_in 7 < K 8"),
                 (dict(ld_out=7), "ld_out 7 < K 8"), (dict(in_=Z + 2), "4-byte aligned"), (dict(out=Y + 3), "4-byte aligned")]
    for kw, msg in bad_scale:
        assert scale(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_temp_scale:") and msg in err, (kw, err)
    for fn, name in ((lib.urso_temp_stats, "stats"), (lib.urso_temp_reduce, "reduce"), (lib.urso_temp_scale, "scale")):
        assert fn(None, None) == -1 and "urso_temp_%s: null argument struct" % name in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU), at any 4- / 8-byte alignment; the refusals come in front of it
    assert stats(n=0) == 0 and stats(n=0, B=0) == 0 and stats(n=0, logits=Z + 4, target=Y + 12, out=O + 8, ld_z=11, J=8, beta=list(Cal.GRID)) == 0
    assert scale(n=0) == 0 and scale(n=0, in_=Z + 4, out=Z + 4, beta=1.0) == 0
    assert stats(n=0, K=0) == -1 and scale(n=0, beta=0.0) == -1
