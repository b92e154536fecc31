"""Shared by tests/test_calibrate_cpu.py and tests/test_calibrate_gpu.py: the seeded cases the temperature kernels and the fit are run
on, their float64 reference (ursonet_amd.calibrate.stats64 / reduce64 / fit64) and the bounds, counted from the operations.

The bounds.  With eps = 2^-52: m is exact, and d = z - m, d * d and beta * d are single IEEE operations on the same operands, so the
device and the reference hand exp the same double; exp is within 1 ulp on either side, the products e * d and e * (d * d) are one
rounding each, and the sum of K terms of one sign adds <= K - 1 roundings on a path, whatever the order (K eps covers the device's order
and NumPy's pairwise one).  A is a sum of terms <= 0 and Q of terms >= 0: no cancellation.  So Z, A and Q --
and LSE - beta m = log Z, M1 - m = A / Z, Q / Z, which are one or two operations behind them -- take (K + 16) eps relative; LSE and M1
themselves take that of their two parts' magnitudes.  VAR = Q / Z - (A / Z)^2 is a difference and takes the bound times
(Q / Z + (A / Z)^2), absolute.  SY and YZ are sums of K products that are exact in fp64 (24 x 24 bits): K eps of sum |y_i z_i|.

The fitted beta.  Each search stops within TOL, relative, of the root of ITS g; the device's g differs from the exact one by at most
delta_g = tol(K) * sum_r (sy_r (|m_r| + |m1_r - m_r|) + sum_i |y_i z_i|), the bounds above put through g = sum_r (sy_r m1_r - yz_r),
and a root moves by delta_g / h, h = dg/dbeta.  beta_bound() is TOL * beta + delta_g / h from the reference's own terms; the reference
root it is compared with comes from fit64 at tol = 1e-13, whose own stopping error does not count beside it.
"""
import numpy as np

from ursonet_amd import calibrate as Cal

EPS = 2.0 ** -52
KS = (1, 2, 63, 64, 257, 4096)
BIG_K = 32768
JS = (1, 3, 8)
SCALES = (1.0, 30.0)
PLANT_B0 = (0.25, 1.0, 5.0)
PLANT_KS = (2, 63, 257, 4096, 32768)
REF_TOL = 1e-13


def tol(K):
    return (K + 16) * EPS


def betas_of(J):
    """J inverse temperatures spread over the fit's range, the identity among them for J = 8."""
    return {1: [0.7], 3: [1.0 / 64, 1.0, 64.0], 8: list(Cal.GRID)}[J]


def shape_of(K):
    """(B, n, row0, ld) of a case: a batch with a row past n, rows in front of it and padding behind the columns; the one large case is
    packed and starts at row 0."""
    return (2, 2, 0, K) if K == BIG_K else (3, 2, 5, K + 3)


def logits_and_targets(K, scale):
    """(z, y) fp32 [n, K], seeded by the case: normal logits of the given scale, targets a softmax of other logits (row 0) and an
    un-normalised positive vector (row 1).  Scale 1: row 0 has a -inf bin that the target gives no weight (K > 1).  Scale 30: row 1 has a
    NaN logit (K > 1), so every column of that row is NaN; and row 0's target is all zero."""
    n = shape_of(K)[1]
    rng = np.random.default_rng([K, int(scale), 7])
    z = (rng.normal(size=(n, K)) * scale).astype(np.float32)
    t = rng.normal(size=(n, K)) * 2
    y = np.exp(t - t.max(axis=1, keepdims=True))
    y[0] /= y[0].sum()
    y = y.astype(np.float32)
    if K > 1:
        if scale == 1.0:
            z[0, K // 2] = -np.inf
            y[0, K // 2] = 0.0
        else:
            z[1, K // 3] = np.nan
    if scale != 1.0:
        y[0] = 0.0
    return z, y


def check_stats(got, z, y, betas):
    """The figures (observed / bound, per quantity) of a device or simulated table `got` [n, 2 + 3 J] against stats64; rows whose
    reference is NaN must be NaN in every column and are left out of the figures."""
    z, y = np.asarray(z, dtype=np.float32), np.asarray(y, dtype=np.float32)
    K, J = z.shape[1], len(betas)
    ref = Cal.stats64(z, y, betas)
    got = np.asarray(got, dtype=np.float64)[:, :2 + 3 * J]
    nanrow = np.isnan(ref[:, Cal.LSE])
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern"
    assert np.all(np.isnan(ref[nanrow])), "a NaN row is NaN in every column"
    ok = ~nanrow
    fig = dict(SY=0.0, YZ=0.0, LSE=0.0, M1=0.0, VAR=0.0)
    if not ok.any():
        return fig
    g, r, z64, y64 = got[ok], ref[ok], z[ok].astype(np.float64), y[ok].astype(np.float64)
    t, one = tol(K), lambda a: np.where(a > 0, a, 1.0)             # noqa: E731
    with np.errstate(all="ignore"):
        m = z64.max(axis=1)
        ayz = np.where(y64 == 0, 0.0, np.abs(y64 * z64)).sum(axis=1)
    fig["SY"] = float((np.abs(g[:, Cal.SY] - r[:, Cal.SY]) / one(K * EPS * np.abs(y64).sum(axis=1))).max())
    fig["YZ"] = float((np.abs(g[:, Cal.YZ] - r[:, Cal.YZ]) / one(K * EPS * ayz)).max())
    for j, b in enumerate(betas):
        lse, m1, var = (r[:, c + 3 * j] for c in (Cal.LSE, Cal.M1, Cal.VAR))
        logz, az = lse - b * m, m1 - m                             # log Z >= 0, A / Z <= 0
        qz = var + az * az
        fig["LSE"] = max(fig["LSE"], float((np.abs(g[:, Cal.LSE + 3 * j] - lse) / one(t * (np.abs(logz) + np.abs(b * m)))).max()))
        fig["M1"] = max(fig["M1"], float((np.abs(g[:, Cal.M1 + 3 * j] - m1) / one(t * (np.abs(az) + np.abs(m)))).max()))
        fig["VAR"] = max(fig["VAR"], float((np.abs(g[:, Cal.VAR + 3 * j] - var) / one(t * (qz + az * az))).max()))
    return fig


def planted(K, b0, rows=None):
    """(z, y): logits of scale 2 and the targets softmax64(b0 z) rounded to fp32 -- the fit must give b0 back."""
    rows = rows if rows is not None else (6 if K >= 4096 else 24)
    rng = np.random.default_rng([K, int(b0 * 100), 3])
    z = (rng.normal(size=(rows, K)) * 2).astype(np.float32)
    x = b0 * z.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return z, (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def beta_bound(z, y, beta):
    """TOL * beta + delta_g / h at the reference's root `beta` (see the module's text)."""
    z, y = np.asarray(z, dtype=np.float32), np.asarray(y, dtype=np.float32)
    K = z.shape[1]
    rows = Cal.stats64(z, y, [beta])
    _ce, _g, h, _bad = Cal.row_terms(rows, [beta])
    z64, y64 = z.astype(np.float64), y.astype(np.float64)
    m = z64.max(axis=1)
    ayz = np.where(y64 == 0, 0.0, np.abs(y64 * z64)).sum(axis=1)
    delta_g = tol(K) * (np.abs(rows[:, Cal.SY]) * (np.abs(m) + np.abs(rows[:, Cal.M1] - m)) + ayz).sum()
    return Cal.TOL * beta + delta_g / h.sum()
