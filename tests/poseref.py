"""Float64 NumPy references of the pose decode, written from the formulas and independent of ursonet_amd's kernels and of oracle/pose_math.py
(tests/test_poseref_cpu.py pins them against both): the soft-argmax scatter and its top eigenvector (urso_quat_wavg_decode), the
conversions of urso_pose_eval / urso_pose_decode (se3lib.SO32quat, euler2SO3_left, the angle-axis branch of pose_estimator.py:397-403,
the keypoint solve of :355-369 by Kabsch / SVD where the kernel uses Horn's quaternion method), and the location reductions.  The only
rounding points are those of the kernels' INPUTS (fp32 logits, fp32 bin map, the one fp32 subtraction z - max).

Also here, shared by the CPU and the GPU test file: the gates of tests/test_pose_decode_exact_gpu.py as plain functions of (result,
reference) that return observed / bound (<= 1 passes), the seeded case generators with each row's family name, and an fp32 emulation of
quat_wavg_kernel's summation order (with injectable defects) on which the CPU test proves that the gates accept the arithmetic and
reject mistakes.

Conventions: eps = 2^-24; "angle" = rotation angle = twice the angle between unit 4-vectors taken up to sign; lambda1 >= lambda2 are the two
largest eigenvalues of the float64 reference matrix; quaternions are [x, y, z, w]."""
import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]            # the kernel's 10 unique entries, in its order


# ------------------------------------------------------------------------------------------------ scatter and eigenvector
def fmax_rows(z):
    """Row maximum with fmaxf's rule (a NaN is dropped unless the whole row is NaN)."""
    return np.fmax.reduce(np.asarray(z, dtype=F32), axis=1)


def scatter(z, hq):
    """z fp32 [B,K], hq fp32 [K,4] -> (A, M) float64 [B,4,4]: d = z - max z as ONE fp32 subtraction, w = exp(float64(d)),
    A = sum w h h^T / sum w, M = sum w |h_i h_j| / sum w over the fp32 map values widened to float64."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(invalid="ignore"):
        d = z - fmax_rows(z)[:, None]
        assert d.dtype == F32
        w = np.exp(d.astype(np.float64))
        h = np.asarray(hq, dtype=F32).astype(np.float64)
        P = (h[:, :, None] * h[:, None, :]).reshape(-1, 16)
        den = w.sum(axis=1)[:, None]
        A, M = (w @ P) / den, (w @ np.abs(P)) / den
    return A.reshape(-1, 4, 4), M.reshape(-1, 4, 4)


def sign_rule(v):
    """The project's sign: the component of largest magnitude is positive (rows)."""
    v = np.array(v, dtype=np.float64, copy=True)
    v2 = np.atleast_2d(v)
    im = np.argmax(np.abs(v2), axis=1)
    s = np.where(v2[np.arange(len(v2)), im] < 0, -1.0, 1.0)
    return (v2 * s[:, None]).reshape(v.shape)


def top_vector(A):
    """A [...,4,4] symmetric float64 -> (unit eigenvector of lambda1 with the sign rule, gap = lambda1 - lambda2, spread = lambda1 - lambda4)."""
    A = np.asarray(A, dtype=np.float64)
    lam, V = np.linalg.eigh(A)
    v = sign_rule(V[..., :, -1])
    return v, lam[..., 3] - lam[..., 2], lam[..., 3] - lam[..., 0]


def scatter_tol(K, A, M):
    """Gate (a): T_ij = (ceil(K/256) + 24) eps (M_ij + |A_ij|) + 1e-45 -- one rounding per term of a thread's sequential sum, 6 shuffle
    levels + 4 wave partials, two product roundings, expf at up to 2 ulp, the denominator's own sum, one division."""
    return (-(-int(K) // 256) + 24) * EPS * (M + np.abs(A)) + 1e-45


def angle(a, b):
    """Rotation angle [rad] between quaternion rows a and b up to sign, accurate near 0."""
    a, b = np.atleast_2d(np.asarray(a, np.float64)), np.atleast_2d(np.asarray(b, np.float64))
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    s = np.where(np.sum(a * b, axis=1) < 0, -1.0, 1.0)[:, None]
    return 4 * np.arcsin(np.minimum(1.0, np.linalg.norm(a - s * b, axis=1) / 2))


# ------------------------------------------------------------------------------------------------ gates: observed / bound, <= 1 passes
def sign_ambiguous(v, tol=2.0 ** -22):
    """Rows whose two largest magnitudes differ by less than tol: either sign is accepted there."""
    m = np.sort(np.abs(np.atleast_2d(v)), axis=1)
    return m[:, 3] - m[:, 2] < tol


def signed_diff(q, ref):
    """q - ref per row; where ref's sign is ambiguous the closer of +ref / -ref is taken."""
    q, ref = np.atleast_2d(np.asarray(q, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    d, dm = q - ref, q + ref
    flip = sign_ambiguous(ref) & (np.abs(dm).max(axis=1) < np.abs(d).max(axis=1))
    return np.where(flip[:, None], dm, d)


def gate_scatter(a, A, M, K):
    """(a): max |a - A| / T, asymmetry (must be 0 -> reported as inf when not) and |trace - 1| / (4 max T)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 4, 4)
    T = scatter_tol(K, A, M)
    if not np.all(np.isfinite(a)):
        return np.inf
    r = float((np.abs(a - A) / T).max())
    if not np.array_equal(a, np.swapaxes(a, 1, 2)):
        return np.inf
    tr = np.abs(np.trace(a, axis1=1, axis2=2) - 1.0) / (4 * np.trace(T, axis1=1, axis2=2))
    return max(r, float(tr.max()))


def gate_planted(q, h, tol=2.0 ** -23):
    """(b): q against the sign-normalised fp32 map row (or +-normalise(h1 - h2)), per component."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    if not np.all(np.isfinite(q)):
        return np.inf
    return float(np.abs(signed_diff(q, sign_rule(h))).max() / tol)


def gate_solver(q, a):
    """(c) on the kernel's OWN scatter a (fp32 values, widened): returns (worst ratio, rows with gap < 1e-6).
    gap >= 1e-6: ||q - v|| <= 2^-23 + 1e-14 / gap.  All rows: finite, | ||q|| - 1 | <= 2^-22, lambda1 - Rayleigh(q) <= 1e-12 spread + 1e-15,
    and the sign rule unless the two largest magnitudes are within 2^-22."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    a = np.asarray(a, dtype=np.float64).reshape(-1, 4, 4)
    if not (np.all(np.isfinite(q)) and np.all(np.isfinite(a))):
        return np.inf, np.zeros(len(q), bool)
    v, gap, spread = top_vector(a)
    lam1 = np.linalg.eigvalsh(a)[:, 3]
    ok = gap >= 1e-6
    r = [0.0]
    if ok.any():
        dv = np.linalg.norm(signed_diff(q[ok], v[ok]), axis=1)
        r.append(float((dv / (2.0 ** -23 + 1e-14 / gap[ok])).max()))
    nq = np.linalg.norm(q, axis=1)
    r.append(float((np.abs(nq - 1) / 2.0 ** -22).max()))
    ray = np.einsum("bi,bij,bj->b", q, a, q) / (nq * nq)
    r.append(float(((lam1 - ray) / (1e-12 * spread + 1e-15)).max()))
    im = np.argmax(np.abs(q), axis=1)
    bad_sign = (q[np.arange(len(q)), im] < 0) & ~sign_ambiguous(q)
    if bad_sign.any():
        r.append(np.inf)
    return max(r), ~ok


def decode_bound(K, A, M):
    """(d): (bound [rad], gap, excluded rows).  Davis-Kahan on the tolerance of (a): angle <= 2 asin(min(1, |T|_F / (gap - |T|_F))) + 2^-21;
    rows with gap <= 4 |T|_F are excluded."""
    _, gap, _ = top_vector(A)
    tf = np.linalg.norm(scatter_tol(K, A, M).reshape(-1, 16), axis=1)
    excl = gap <= 4 * tf
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 2 * np.arcsin(np.minimum(1.0, np.where(excl, 1.0, tf / (gap - tf)))) + 2.0 ** -21
    return b, gap, excl


def gate_decode(q, K, A, M):
    """(d): (worst observed / bound over the rows kept, excluded rows)."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    b, _, excl = decode_bound(K, A, M)
    if not np.all(np.isfinite(q)):
        return np.inf, excl
    keep = ~excl
    if not keep.any():
        return 0.0, excl
    v, _, _ = top_vector(A[keep])
    return float((angle(q[keep], v) / b[keep]).max()), excl


def gate_quat(q, ref, tol):
    """max over rows of min(|q - ref|, |q + ref|)_max / tol."""
    q, ref = np.atleast_2d(np.asarray(q, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    if not np.all(np.isfinite(q)):
        return np.inf
    return float(np.minimum(np.abs(q - ref).max(axis=1), np.abs(q + ref).max(axis=1)).max() / tol)


def gate_rotation(q, R_ref, tol):
    """max |R(q) - R_ref| / tol over rows (independent of the quaternion's sign and of the branch taken)."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    if not np.all(np.isfinite(q)):
        return np.inf
    return float(max(np.abs(quat_to_so3(qi) - Ri).max() for qi, Ri in zip(q, R_ref)) / tol)


# ------------------------------------------------------------------------------------------------ conversions
def euler_to_so3(pitch, yaw, roll):
    """se3lib.euler2SO3_left, degrees."""
    p, y, r = (np.float64(a) * np.pi / 180 for a in (pitch, yaw, roll))
    cp, sp, cy, sy, cr, sr = np.cos(p), np.sin(p), np.cos(y), np.sin(y), np.cos(r), np.sin(r)
    return np.array([[cy * cr, sp * sy * cr - cp * sr, cp * sy * cr + sp * sr],
                     [cy * sr, sp * sy * sr + cp * cr, cp * sy * sr - sp * cr],
                     [-sy, sp * cy, cp * cy]])


def so3_branch_margin(R):
    """Distance of the branch comparisons that decide so3_to_quat(R) from a tie (0 = exactly on one)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    m = [abs(tr)]
    if not tr > 0:
        m += [abs(R[0, 0] - R[1, 1]), abs(R[0, 0] - R[2, 2])]
        if not (R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]):
            m.append(abs(R[1, 1] - R[2, 2]))
    return min(m)


def so3_to_quat(R, variant=None):
    """se3lib.SO32quat restated: (q [x,y,z,w], branch 0..3).  variant "ge": R00 > R11 replaced by >=; "w4": the last branch's w with its
    operands swapped (both for the CPU test's rejected-mistake checks)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    first = (R[0, 0] >= R[1, 1]) if variant == "ge" else (R[0, 0] > R[1, 1])
    if tr > 0:
        Z = np.sqrt(tr + 1) * 2
        return np.array([(R[1, 2] - R[2, 1]) / Z, (R[2, 0] - R[0, 2]) / Z, (R[0, 1] - R[1, 0]) / Z, 0.25 * Z]), 0
    if first and R[0, 0] > R[2, 2]:
        Z = np.sqrt(1.0 + 2 * R[0, 0] - tr) * 2
        return np.array([0.25 * Z, (R[0, 1] + R[1, 0]) / Z, (R[0, 2] + R[2, 0]) / Z, (R[1, 2] - R[2, 1]) / Z]), 1
    if R[1, 1] > R[2, 2]:
        Z = np.sqrt(1.0 + 2 * R[1, 1] - tr) * 2
        return np.array([(R[0, 1] + R[1, 0]) / Z, 0.25 * Z, (R[1, 2] + R[2, 1]) / Z, (R[2, 0] - R[0, 2]) / Z]), 2
    Z = np.sqrt(1.0 + 2 * R[2, 2] - tr) * 2
    w = (R[1, 0] - R[0, 1]) / Z if variant == "w4" else (R[0, 1] - R[1, 0]) / Z
    return np.array([(R[0, 2] + R[2, 0]) / Z, (R[1, 2] + R[2, 1]) / Z, 0.25 * Z, w]), 3


def quat_to_so3(q):
    """se3lib.quat2SO3."""
    x, y, z, w = (np.float64(c) for c in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * (x * y + z * w), 2 * (x * z - y * w)],
                     [2 * (x * y - z * w), 1 - 2 * x * x - 2 * z * z, 2 * (y * z + x * w)],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * x * x - 2 * y * y]])


def angle_axis_to_quat(v):
    """pose_estimator.py:397-403: theta = |v|, axis 0 below the reference's 1e-6 cut, [axis sin(theta/2), cos(theta/2)]."""
    v = np.asarray(v, dtype=np.float64)
    th = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    ax = np.zeros(3) if th < 1e-6 else v / th
    return np.append(ax * np.sin(th / 2), np.cos(th / 2))


P1 = np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 0.0], [3.0, 0.0, 0.0]])      # columns (0,0,3), (0,3,0), (0,0,0)


def _centred(k1, k2, loc):
    P2 = np.stack([np.asarray(k1, np.float64), np.asarray(k2, np.float64), np.asarray(loc, np.float64)], axis=1)
    return P1 - P1.mean(axis=1, keepdims=True), P2 - P2.mean(axis=1, keepdims=True)


def keypoints_to_quat(k1, k2, loc, correct_reflection=True):
    """pose_estimator.py:355-369 the way the reference writes it: Kabsch by SVD of H = (P1 - C1)(P2 - C2)^T with the determinant correction,
    then so3_to_quat(R^T).  Deliberately NOT Horn's method (the kernel's), so that the two derivations check each other."""
    X, Y = _centred(k1, k2, loc)
    U, _, Vh = np.linalg.svd(X @ Y.T)
    D = np.eye(3)
    if correct_reflection:
        D[2, 2] = np.linalg.det(U) * np.linalg.det(Vh.T)
    R = U @ D @ Vh
    return so3_to_quat(R.T)[0]


def horn_gap(k1, k2, loc):
    """Relative top gap g = (lambda1 - lambda2) / max |lambda| of Horn's 4x4 matrix of the keypoint problem: the conditioning of the solve."""
    X, Y = _centred(k1, k2, loc)
    S = X @ Y.T
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    lam = np.linalg.eigvalsh(N)
    top = np.abs(lam).max()
    return 0.0 if top == 0 else float((lam[3] - lam[2]) / top)


def encode_as_keypoints(q, c):
    """utils.py:220-227: k1 = R(q) e_z + c, k2 = R(q) e_y + c."""
    R = quat_to_so3(q)
    return R[:, 2] + np.asarray(c, np.float64), R[:, 1] + np.asarray(c, np.float64)


# ------------------------------------------------------------------------------------------------ location
def loc_softmax(z, loc_map):
    """softmax(z) @ loc_map with w = exp(float64(z) - float64(max z)): (loc_est [B,3], peak probability [B])."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(invalid="ignore"):
        w = np.exp(z.astype(np.float64) - fmax_rows(z).astype(np.float64)[:, None])
        den = w.sum(axis=1)
        return (w @ np.asarray(loc_map, np.float64)) / den[:, None], 1.0 / den


def peak(z):
    """Largest probability of the float64 softmax of the fp32 logits."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(invalid="ignore"):
        return 1.0 / np.exp(z.astype(np.float64) - fmax_rows(z).astype(np.float64)[:, None]).sum(axis=1)


def first_moment(p, loc_map):
    return np.asarray(p, dtype=F32).astype(np.float64) @ np.asarray(loc_map, np.float64)


def pmf_scatter(p, hq):
    """A = sum p h h^T in float64 from the fp32 PMF and map (the encoded target of ORI_ENC_ERR; no normalisation, as the kernel)."""
    h = np.asarray(hq, dtype=F32).astype(np.float64)
    return (np.asarray(p).astype(np.float64) @ (h[:, :, None] * h[:, None, :]).reshape(-1, 16)).reshape(-1, 4, 4)


# ------------------------------------------------------------------------------------------------ case generators
KS = (1, 3, 255, 256, 257, 512, 1728, 13824, 32768)
K_BIG = 262144
_MAPS = {}


def bin_map(K):
    """fp32 [K,4]: OrientationCodec(n, 6.0).H_quat for K = n^3, else the first K rows of the n = 8 map."""
    if K not in _MAPS:
        from ursonet_amd.pose import OrientationCodec
        n = int(round(K ** (1.0 / 3)))
        _MAPS[K] = OrientationCodec(n, 6.0).H_quat if n ** 3 == K else np.ascontiguousarray(OrientationCodec(8, 6.0).H_quat[:K])
    return _MAPS[K]


def random_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _peak_row(rng, hq, height):
    """ReLU background (what a trained head's last layer leaves) + an encoded peak of the given height around a random pose."""
    K = len(hq)
    var = (6.0 / max(2.0, round(K ** (1.0 / 3)))) ** 2 / 12
    d = np.abs(hq.astype(np.float64) @ random_quats(rng, 1)[0])
    pr = np.exp(-2 * (np.arccos(np.minimum(1.0, d)) / np.pi) ** 2 / var)
    return np.maximum(0.0, 0.3 * rng.standard_normal(K)) + height * pr / pr.max()


def logit_cases(K, seed=0, big=False):
    """(z fp32 [B,K], family name per row).  Families: normal, peak3 / peak6 / peak12, equal, range200, neginf.  big: one row each of
    peak3, peak12 and equal (the B = 3 launch at K = 262,144)."""
    rng = np.random.default_rng(1000 + seed + K)
    hq = bin_map(K)
    rows, fam = [], []

    def add(name, r):
        rows.append(np.asarray(r, dtype=np.float64)); fam.append(name)
    if big:
        add("peak3", _peak_row(rng, hq, 3)); add("peak12", _peak_row(rng, hq, 12)); add("equal", np.full(K, 0.7))
    else:
        for _ in range(2):
            add("normal", rng.standard_normal(K))
        for h in (3, 6, 12):
            add("peak%d" % h, _peak_row(rng, hq, h))
        add("equal", np.full(K, 0.7))
        add("equal", np.full(K, -31.5))
        for _ in range(2):
            add("range200", rng.uniform(-100.0, 100.0, K))
        for _ in range(2):
            r = rng.standard_normal(K)
            r[rng.random(K) < 0.3] = -np.inf
            r[rng.integers(K)] = 0.25                                     # at least one finite entry
            add("neginf", r)
    return np.stack(rows).astype(F32), fam


def planted_bins(K):
    ks = [0, 63, 64, 255, 256, K - 257, K - 1] + ([K - K % 256] if K % 256 else [])
    return sorted({k for k in ks if 0 <= k < K})


def planted_cases(K):
    """(z, bins): row r is -200 everywhere except z[r, bins[r]] = 0 (exp(-200) vanishes in fp32 and is 1.4e-87 in float64)."""
    ks = planted_bins(K)
    z = np.full((len(ks), K), -200.0, dtype=F32)
    z[np.arange(len(ks)), ks] = 0.0
    return z, ks


def antipodal_cases(K, seed=0, rows=6):
    """(z, pairs): two planted bins of equal weight whose map quaternions have a negative dot product.  For each first bin the partner is the
    bin of most negative dot product, and only pairs with h1 . h2 <= -0.5 are kept: A = (h1 h1^T + h2 h2^T) / 2 has the top vector
    normalise(h1 - h2) with the gap |h1 . h2|, and the fp32 error of A (<= 2 eps in Frobenius norm) divided by that gap must stay
    inside the gate's 2^-22.  May return no rows (K = 1, 3)."""
    rng = np.random.default_rng(2000 + seed + K)
    h = bin_map(K).astype(np.float64)
    pairs = []
    for i in ([0, K - 1] + list(rng.integers(0, K, size=rows)))[:rows + 2]:
        d = h @ h[i]
        j = int(np.argmin(d))
        if d[j] <= -0.5 and j != i and (i, j) not in pairs:
            pairs.append((int(i), j))
    z = np.full((len(pairs), K), -200.0, dtype=F32)
    for r, (i, j) in enumerate(pairs):
        z[r, i] = z[r, j] = 0.0
    return z, pairs


def euler_cases(seed=0):
    """fp32 [N,3] (pitch, yaw, roll): the 30-degree grid in [-180, 180] (yaw = +-90 included) + 64 random triples."""
    g = np.arange(-180, 181, 30, dtype=np.float64)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rnd = np.random.default_rng(3000 + seed).uniform(-180, 180, size=(64, 3))
    return np.concatenate([grid, rnd]).astype(F32)


def angle_axis_cases():
    th = [0.0, 5e-7, 9.99e-7, 1.01e-6, 1e-3, np.pi - 1e-6, np.pi, 2 * np.pi, 7.0, 100.0]
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.48, -0.6, 0.64]])
    return np.concatenate([t * axes for t in th]).astype(F32)


def cube_group():
    """The 24 proper signed permutation matrices (nine 180-degree rotations among them): integer entries, so their keypoints are exact in fp32."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = sg
            if np.linalg.det(R) > 0:
                out.append(R)
    return out


def keypoint_poses(seed=0, n=64):
    """(q [24 + n, 4], loc [24 + n, 3], exact [24 + n] bool) float64.  The first 24 rows are the cube group at locations that are multiples of
    1/8: their keypoints R e_z + c, R e_y + c are exact in fp32 (exact = True).  Then n random poses, the first 8 of them 180-degree
    rotations (w = 0); their keypoints are rounded to fp32 when they are fed to the kernel."""
    rng = np.random.default_rng(4000 + seed)
    q = random_quats(rng, n)
    q[:8, 3] = 0.0
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    loc = rng.uniform(-1, 1, size=(n, 3)) * [2.0, 2.0, 10.0] + [0, 0, 15.0]
    cq = np.array([so3_to_quat(R)[0] for R in cube_group()])
    cl = np.round((rng.uniform(-1, 1, size=(24, 3)) * [2.0, 2.0, 10.0] + [0, 0, 15.0]) * 8) / 8
    return np.concatenate([cq, q]), np.concatenate([cl, loc]), np.arange(24 + n) < 24


def keypoint_cases(seed=0):
    """(dict name -> (k1, k2, loc) fp32 [N,3], q [N,4], exact [N]): exact encodings, noisy ones (sigma 1e-3, 0.3, 3), and k - loc rescaled by
    1e-3 / 1e3 around loc = 0."""
    rng = np.random.default_rng(5000 + seed)
    q, loc, exact = keypoint_poses(seed)
    k = np.array([encode_as_keypoints(qi, ci) for qi, ci in zip(q, loc)])
    out = {"exact": (k[:, 0], k[:, 1], loc)}
    for s in (1e-3, 0.3, 3.0):
        out["noise%g" % s] = (k[:, 0] + s * rng.standard_normal((len(q), 3)), k[:, 1] + s * rng.standard_normal((len(q), 3)), loc)
    k0 = np.array([encode_as_keypoints(qi, np.zeros(3)) for qi in q])
    for s in (1e-3, 1e3):
        out["scale%g" % s] = (k0[:, 0] * s, k0[:, 1] * s, np.zeros_like(loc))
    return {n: tuple(np.asarray(a, dtype=F32) for a in v) for n, v in out.items()}, q, exact


def keypoint_input_bound(k1, k2, loc):
    """Bound [rad] on the rotation between the pose and the best fit of its fp32-ROUNDED keypoints: each coordinate moves by at most
    2^-24 |c|, so each of the two unit arms k - loc by at most sqrt(3) 2^-23 cmax; an arm of length 1 turns by at most that, and the frame
    fitted to two arms by at most the sum of both, doubled for the arms' non-orthogonality after rounding."""
    cmax = max(np.abs(k1).max(), np.abs(k2).max(), np.abs(loc).max())
    return 4 * np.sqrt(3.0) * 2.0 ** -23 * cmax


# ------------------------------------------------------------------------------------------------ fp32 emulation of quat_wavg_kernel
def jacobi_top(S, sweeps=30, sign=True):
    """The kernel's solver in float64: cyclic Jacobi, stop at off^2 < 1e-30, the column of the largest diagonal entry, normalised, signed."""
    A = np.array(S, dtype=np.float64)
    V = np.eye(4)
    for _ in range(sweeps):
        if sum(A[i, j] ** 2 for i in range(4) for j in range(i + 1, 4)) < 1e-30:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                if abs(A[p, q]) < 1e-300:
                    continue
                th = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if th >= 0 else -1.0) / (abs(th) + np.sqrt(th * th + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                kp, kq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * kp - s * kq, s * kp + c * kq
                pk, qk = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * pk - s * qk, s * pk + c * qk
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    v = V[:, int(np.argmax(np.diag(A)))]
    v = v / np.linalg.norm(v)
    return sign_rule(v) if sign else v


def emulate_wavg(z, hq, defect=None):
    """quat_wavg_kernel in NumPy fp32, in its order: thread t adds bins t, t + 256, ... sequentially, 6 xor-shuffle levels per wave, the 4
    wave partials in order, one division; expf rounded correctly; the solver in float64.  -> (q fp32 [B,4], a fp32 [B,16]).
    defect: None | "tail_drop" (first bin of the ragged tail) | "wave_drop" (wave 3's partial) | "map_fp16" | "max256" | "no_sign" |
    "one_sweep"."""
    z = np.asarray(z, dtype=F32)
    hq = np.asarray(hq, dtype=F32)
    B, K = z.shape
    if defect == "map_fp16":
        hq = hq.astype(np.float16).astype(F32)
    n = -(-K // 256)
    mx = fmax_rows(z[:, :256] if defect == "max256" else z)
    zp = np.full((B, n * 256), -np.inf, dtype=F32)
    zp[:, :K] = z
    if defect == "tail_drop" and K % 256:
        zp[:, K - K % 256] = -np.inf
    hp = np.zeros((n * 256, 4), dtype=F32)
    hp[:K] = hq
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((zp - mx[:, None]).astype(np.float64)).astype(F32).reshape(B, n, 256)
        hp = hp.reshape(n, 256, 4)
        acc = np.zeros((B, 256, 11), dtype=F32)
        for i in range(n):
            wi = w[:, i, :]
            acc[:, :, 10] += wi
            for t, (r, c) in enumerate(PAIRS):
                acc[:, :, t] += (wi * hp[i, :, r][None]) * hp[i, :, c][None]
        v = acc.reshape(B, 4, 64, 11)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ o, :]
        part = v[:, :, 0, :]
        tot = np.zeros((B, 11), dtype=F32)
        for wv in range(3 if defect == "wave_drop" else 4):
            tot = tot + part[:, wv, :]
        a10 = tot[:, :10] / tot[:, 10:11]
    assert a10.dtype == F32
    a = np.zeros((B, 4, 4), dtype=F32)
    for t, (r, c) in enumerate(PAIRS):
        a[:, r, c] = a[:, c, r] = a10[:, t]
    q = np.full((B, 4), np.nan, dtype=F32)
    for b in range(B):
        if np.all(np.isfinite(a[b])):
            q[b] = jacobi_top(a[b].astype(np.float64), sweeps=1 if defect == "one_sweep" else 30, sign=defect != "no_sign").astype(F32)
    return q, a.reshape(B, 16)
