"""Shared by tests/test_explain_cpu.py and tests/test_explain_gpu.py: the seeded cases urso_occl_score is run on, their float64
reference (ursonet_amd.explain.score64) and the bounds, counted from the operations.

The bound, for ONE evaluation (the kernel's or NumPy's) against exact arithmetic on the fp32 logits; two evaluations differ by at most
twice that, which is what the gates below allow.  eps = 2^-52.
  * d_k = z_k - max is exact in fp64 (fp32 operands within the cases' range), so nothing enters there.
  * e_k = exp(d_k): 1 ulp, relative eps.
  * Z = sum_k e_k: K positive terms, at most K - 1 roundings on a path whatever the order (the kernel's thread / butterfly / wave order and
    NumPy's pairwise one alike), plus the terms' own eps: relative (K + 1) eps.
  * p_k = e_k / Z: eps + (K + 1) eps + the division's: relative P(K) = (K + 3) eps.
  * log Z: 1 ulp of |log Z| <= log K, plus Z's relative error, which enters a logarithm absolutely: EL(K) = (K + 1 + log K) eps; it
    enters every lp_k = d_k - log Z absolutely, beside the subtraction's own rounding |lp_k| eps / 2.
  * KL = sum_k p0_k (lp0_k - lp_k).  With L = the largest |lp| over the bins that count (p0_k > 0) in either row, the difference carries
    2 EL + L eps (two lp's) + 2 L eps / 2 (its own rounding, |difference| <= 2 L); times p0_k and summed (sum p0 = 1): 2 EL + 2 L eps.  The
    terms' own relative errors -- p0's P(K), the product's eps, the sum's K eps -- apply to A = sum_k |term_k| <= 2 L:
    KL_ABS(K, L) = (2 (K + 1 + log K) + 2 L + 2 L (2 K + 4)) eps.
  * TV = 0.5 sum_k |p0_k - p_k|: each difference (p0_k + p_k) P(K) + eps / 2 of itself, summed (sum (p0 + p) = 2), plus the sum's K eps of
    sum |.| <= 2, halved: TV_ABS(K) = (2 K + 4) eps.
  * DROP = p0[k0] - p[k0]: (p0 + p) P(K) + its own rounding: DROP_ABS(K) = (2 K + 7) eps.
ARGMAX (and k0) are compared exactly: the cases' top two logits differ in every row (top_two_differ, asserted by the CPU test).  A bin
with p0_k > 0 and p_k == 0 makes KL +inf on both sides and a NaN row makes the four columns NaN on both sides: compared exactly; no exp
of the cases comes near underflow (no_underflow, asserted by the CPU test), so both sides agree on which p are 0.

D_ORI = 2 acos(min(1, |q0 . q|)) in degrees.  acos is ill-conditioned at 1, so the angle is gated as tests/poseref.py gates one: the dot
product's error is bounded (four products and three sums: 4 eps sum |a_i b_i|) and any value between the angles at both ends of that
interval is accepted, widened by ANGLE_ULPS ulps of the result for acos and the conversion to degrees.  D_LOC is three products, two
sums and a square root: LOC_REL relative."""
import numpy as np

from ursonet_amd import explain as X

EPS = 2.0 ** -52
KS = (1, 2, 63, 64, 257, 4096, 32768)
SCALES = (1.0, 30.0)
ANGLE_ULPS = 8
LOC_REL = 4 * EPS
B, N, ROW0 = 5, 4, 2                                             # a batch with a row past n, rows in front of row0


def p_rel(K):
    return (K + 3) * EPS


def kl_abs(K, L):
    return (2 * (K + 1 + np.log(K)) + 2 * L + 2 * L * (2 * K + 4)) * EPS


def tv_abs(K):
    return (2 * K + 4) * EPS


def drop_abs(K):
    return (2 * K + 7) * EPS


def head_cases(K, scale):
    """[(name, z0 [K], z [N, K])] fp32, seeded by (K, scale).  "plain": a finite baseline against a random row, a row with -inf bins (in z_i
    only), a NaN row and the baseline itself.  "holes" (K >= 2): a baseline with -inf bins against a finite row (-inf in z0 only), a row
    with the same -inf bins (both), a row with one more -inf bin, where p0 > 0 (KL = +inf), and the baseline itself.  K = 1: finite rows,
    a NaN row and the baseline."""
    rng = np.random.default_rng([K, int(scale), 7])
    z0 = (rng.normal(size=K) * scale).astype(np.float32)
    z = (rng.normal(size=(N, K)) * scale).astype(np.float32)
    z[2, K // 3] = np.nan
    z[3] = z0
    if K == 1:
        return [("plain", z0, z)]
    holes = [K - 1] if K == 2 else [K // 2, K - 1]
    z[1, holes] = -np.inf
    h0 = z0.copy()
    h0[holes] = -np.inf
    hz = (rng.normal(size=(N, K)) * scale).astype(np.float32)
    hz[1, holes] = -np.inf
    hz[2, holes] = -np.inf
    hz[2, 0] = -np.inf
    hz[3] = h0
    return [("plain", z0, z), ("holes", h0, hz)]


def top_two_differ(z):
    """The premise of the exact ARGMAX: in every row that has one (no NaN, a finite maximum) the largest logit is attained once."""
    z = np.atleast_2d(z)
    ok = True
    for row in z:
        if np.isnan(row).any() or len(row) < 2 or not np.isfinite(row.max()):
            continue
        s = np.sort(row)
        ok = ok and s[-1] > s[-2]
    return ok


def no_underflow(z):
    """The premise of the exact zeros: every finite z - max stays far above exp's underflow at -745."""
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    with np.errstate(all="ignore"):
        d = z - np.where(np.isnan(z), -np.inf, z).max(axis=1, keepdims=True)
    return bool(np.all(d[np.isfinite(d)] > -700))


def lp_max(z0, z):
    """L of the bound: the largest |lp| of either row over the bins with p0 > 0 and p > 0."""
    with np.errstate(all="ignore"):
        p0, lp0 = X._pmf64(z0)
        p1, lp1 = X._pmf64(z)
    use = (p0 > 0) & (p1 > 0)
    return float(max(np.abs(lp0[use]).max(), np.abs(lp1[use]).max())) if use.any() else 0.0


def check_head(got, z0, z):
    """got [n, 4] (KL, TV, DROP, ARGMAX) against head64 of every row -> {name: worst observed / bound}; > 1 fails.  NaN rows, +inf and
    ARGMAX are compared exactly (a mismatch reports inf)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    K = len(z0)
    fig = {"kl": 0.0, "tv": 0.0, "drop": 0.0, "exact": 0.0}
    for r in range(len(got)):
        ref = X.head64(z0, z[r])
        if np.isnan(ref).any():
            if not np.all(np.isnan(got[r])):
                fig["exact"] = np.inf
            continue
        if np.isnan(got[r]).any() or got[r, 3] != ref[3] or np.isinf(ref[0]) != np.isinf(got[r, 0]) or (np.isinf(ref[0]) and got[r, 0] != ref[0]):
            fig["exact"] = np.inf
            continue
        if np.isfinite(ref[0]):
            fig["kl"] = max(fig["kl"], abs(got[r, 0] - ref[0]) / (2 * kl_abs(K, lp_max(z0, z[r]))))
        fig["tv"] = max(fig["tv"], abs(got[r, 1] - ref[1]) / (2 * tv_abs(K)))
        fig["drop"] = max(fig["drop"], abs(got[r, 2] - ref[2]) / (2 * drop_abs(K)))
    return fig


def angle_interval(q0, q):
    """[lo, hi] degrees: every D_ORI a correct evaluation may give for the two quaternions."""
    a, b = np.asarray(q0, dtype=np.float64), np.asarray(q, dtype=np.float64)
    d = abs(float(np.sum(a * b)))
    err = 4 * EPS * float(np.sum(np.abs(a * b)))
    hi = 2 * np.arccos(min(1.0, max(0.0, d - err))) * 180 / np.pi
    lo = 2 * np.arccos(min(1.0, d + err)) * 180 / np.pi
    return lo * (1 - ANGLE_ULPS * EPS), hi * (1 + ANGLE_ULPS * EPS)


def check_pose(got, dec0, dec):
    """got [n, >= 2] (D_ORI, D_LOC) against the DEC rows -> {name: worst observed / bound}: D_ORI 0 inside its interval, else inf."""
    got = np.asarray(got, dtype=np.float64)
    fig = {"d_ori": 0.0, "d_loc": 0.0}
    for r in range(len(got)):
        lo, hi = angle_interval(dec0[X.DEC_Q_EST:X.DEC_Q_EST + 4], dec[r, X.DEC_Q_EST:X.DEC_Q_EST + 4])
        if not lo <= got[r, X.D_ORI] <= hi:
            fig["d_ori"] = np.inf
        ref = X.pose64(dec0, dec[r])[1]
        fig["d_loc"] = max(fig["d_loc"], abs(got[r, X.D_LOC] - ref) / (LOC_REL * ref) if ref > 0 else (0.0 if got[r, X.D_LOC] == 0 else np.inf))
    return fig


def dec_rows(n, seed=0):
    """(dec0 [DEC_COLS], dec [n, DEC_COLS]): random unit quaternions and locations; row 0 of dec is dec0 itself, row 1 its antipode."""
    rng = np.random.default_rng([seed, 11])
    dec = rng.normal(size=(n + 1, X.DEC_COLS))
    q = dec[:, X.DEC_Q_EST:X.DEC_Q_EST + 4]
    dec[:, X.DEC_Q_EST:X.DEC_Q_EST + 4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    dec[1] = dec[0]
    if n > 1:
        dec[2] = dec[0]
        dec[2, X.DEC_Q_EST:X.DEC_Q_EST + 4] *= -1
    return dec[0].copy(), dec[1:].copy()
