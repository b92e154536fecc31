"""NumPy float64 references of detect_dataset's pictures, written independently of ursonet_amd/detect.py and of the kernels: the slice
sheet of urso_pmf_sheet_u8 (geometry and value rule of include/ursonet_hip.h) pixel by pixel, the near-tie rule its estimate row is
compared under, and the primitives of detect.detect_prims with np.matrix as the reference writes utils.visualize_axes."""
import math

import numpy as np

TIE_MARGIN = 1e-12          # relative: covers a 1-ulp exp (2.2e-16) with three orders to spare
TIE_MAX_FRACTION = 1e-3


# ---------------------------------------------------------------- sheet
def values(p, estimate):
    """fp64 value of every bin of one source row [K]: GT p / max p (negative or NaN p counts as 0; max 0: all 0), estimate
    exp(z - max z)."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if estimate:
            v = np.exp(p - np.nanmax(p))
            return np.where(np.isnan(v), 0.0, v)
        p = np.where(p > 0, p, 0.0)
        m = p.max()
        return p / m if m > 0 else np.zeros_like(p)


def indices(v):
    return np.minimum(255, np.floor(256.0 * v)).astype(np.int64)


def near_tie(v):
    """Boolean [K]: floor(256 v (1 +- 1e-12)) gives different indices."""
    return indices(v * (1 - TIE_MARGIN)) != indices(v * (1 + TIE_MARGIN))


def shape(n, cell, gap, rows):
    return rows * n * cell + (rows + 1) * gap, n * n * cell + (n + 1) * gap


def cell_map(n, cell, gap, rows):
    """int64 [SH,SW]: r * n^3 + bin of the bin a pixel shows, -1 for the background; a loop over rows, slices and cells."""
    SH, SW = shape(n, cell, gap, rows)
    m = np.full((SH, SW), -1, dtype=np.int64)
    for r in range(rows):
        y0 = gap + r * (n * cell + gap)
        for z in range(n):
            x0 = gap + z * (n * cell + gap)
            for j in range(n):
                for i in range(n):
                    m[y0 + j * cell:y0 + (j + 1) * cell, x0 + i * cell:x0 + (i + 1) * cell] = r * n ** 3 + i * n * n + j * n + z
    return m


def sources(gt, logits):
    return [(s, est) for s, est in ((gt, False), (logits, True)) if s is not None]


def sheet(gt, logits, n, cell, gap, lut, bg):
    """One image: gt / logits [K] or None -> uint8 [SH,SW,3]."""
    src = sources(gt, logits)
    idx = np.concatenate([indices(values(s, est)) for s, est in src])
    m = cell_map(n, cell, gap, len(src))
    lut = np.asarray(lut, dtype=np.uint8).reshape(256, 3)
    out = np.empty(m.shape + (3,), dtype=np.uint8)
    out[:] = np.asarray(bg, dtype=np.uint8)
    out[m >= 0] = lut[idx[m[m >= 0]]]
    return out


def check_sheet(got, gt, logits, n, cell, gap, lut, bg):
    """The comparison rule of the sheet: the GT row and the background byte for byte; an estimate cell byte for byte unless it is a
    near-tie, where either neighbouring index's colour will do.  -> (near-tie bins, differing pixels); raises AssertionError."""
    src = sources(gt, logits)
    ref = sheet(gt, logits, n, cell, gap, lut, bg)
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.uint8, (got.shape, ref.shape, got.dtype)
    vs = [values(s, est) for s, est in src]
    tie = np.concatenate([near_tie(v) if est else np.zeros(v.shape, dtype=bool) for v, (s, est) in zip(vs, src)])
    lo = np.concatenate([indices(v * (1 - TIE_MARGIN)) for v in vs])
    hi = np.concatenate([indices(v * (1 + TIE_MARGIN)) for v in vs])
    m = cell_map(n, cell, gap, len(src))
    lut = np.asarray(lut, dtype=np.uint8).reshape(256, 3)
    bad = (got != ref).any(axis=2)
    allowed = (m >= 0) & tie[np.maximum(m, 0)]
    assert not (bad & ~allowed).any(), "pixels differ outside near-ties: %s" % (np.argwhere(bad & ~allowed)[:8],)
    ys, xs = np.nonzero(bad)
    for y, x in zip(ys, xs):
        k = m[y, x]
        assert tuple(got[y, x]) in (tuple(lut[lo[k]]), tuple(lut[hi[k]])), (y, x, got[y, x], lo[k], hi[k])
    n_est = sum(v.size for v, (s, est) in zip(vs, src) if est)
    assert int(tie.sum()) <= TIE_MAX_FRACTION * max(n_est, 1), "near-ties: %d of %d estimate bins" % (tie.sum(), n_est)
    return int(tie.sum()), int(bad.sum())


# ---------------------------------------------------------------- primitives
def quat2SO3_matrix(q):
    return np.matrix([[1 - 2 * q[1] ** 2 - 2 * q[2] ** 2, 2 * (q[0] * q[1] + q[2] * q[3]), 2 * (q[0] * q[2] - q[1] * q[3])],
                      [2 * (q[0] * q[1] - q[2] * q[3]), 1 - 2 * q[0] ** 2 - 2 * q[2] ** 2, 2 * (q[1] * q[2] + q[0] * q[3])],
                      [2 * (q[0] * q[2] + q[1] * q[3]), 2 * (q[1] * q[2] - q[0] * q[3]), 1 - 2 * q[0] ** 2 - 2 * q[1] ** 2]])


def arrows(q, C, K, length=100.0):
    """utils.visualize_axes' (c, v) as the reference states them, np.matrix and all -> c [2], v [2,3]."""
    C = np.asarray(C, dtype=np.float64)
    P_r = quat2SO3_matrix(np.asarray(q, dtype=np.float64)) * np.matrix([[1, 0, 0], [0, -1, 0], [0, 0, 1]])
    P_t = np.asarray(P_r) + np.transpose([C])
    p = np.matrix(K) * (P_t / P_t[-1, :])
    c = np.matrix(K) * np.matrix(C / C[-1]).transpose()
    v = p - c
    v = length * v / np.linalg.norm(v)
    return np.asarray(c)[:2, 0], np.asarray(v)[:2, :]


def centre(loc, fx, fy, w0, h0):
    loc = np.asarray(loc, dtype=np.float64).ravel()
    return np.array([loc[0] / loc[2] * fx + w0 / 2, h0 / 2 + loc[1] / loc[2] * fy])


def _rint(x):
    return int(np.rint(x))


def _ok(*xs):
    return all(math.isfinite(x) and abs(_rint(x)) <= 16384 for x in xs)


def _arrow(c, t, thick, colour):
    """Shaft c -> t and the two head strokes: tip + 0.1 |t - c| (cos, sin)(a +- pi / 4), a the direction from the tip back to c."""
    rows = [[0, c[0], c[1], t[0], t[1], thick] + list(colour)]
    d = 0.1 * math.sqrt((c[0] - t[0]) ** 2 + (c[1] - t[1]) ** 2)
    a = math.atan2(c[1] - t[1], c[0] - t[0])
    for s in (+1, -1):
        ex, ey = t[0] + d * math.cos(a + s * math.pi / 4), t[1] + d * math.sin(a + s * math.pi / 4)
        if _ok(ex, ey):
            rows.append([0, _rint(ex), _rint(ey), t[0], t[1], thick] + list(colour))
    return rows


def axes_prims(q, loc, K, scale, speed=False):
    q = np.asarray(q, dtype=np.float64)
    if speed:
        q = np.array([-q[0], -q[1], -q[2], q[3]])
    with np.errstate(all="ignore"):
        c, v = arrows(q, loc, K)
    rows = []
    thick = max(1, _rint(2 * scale))
    for i, colour in enumerate(((255, 0, 0), (0, 255, 0), (0, 0, 255))):
        xs = (c[0] * scale, c[1] * scale, (c[0] + v[0, i]) * scale, (c[1] + v[1, i]) * scale)
        if _ok(*xs):
            rows += _arrow((_rint(xs[0]), _rint(xs[1])), (_rint(xs[2]), _rint(xs[3])), thick, colour)
    return np.asarray(rows, dtype=np.int32).reshape(-1, 9)


def overlap_prims(loc_est, loc_gt, loc_encoded, K, scale):
    K = np.asarray(K, dtype=np.float64)
    rows = []
    for loc, radius, colour in ((loc_encoded, 7, (0, 0, 255)), (loc_gt, 15, (255, 0, 0)), (loc_est, 10, (0, 255, 0))):
        if loc is None:
            continue
        with np.errstate(all="ignore"):
            p = centre(loc, K[0, 0], K[1, 1], 2 * K[0, 2], 2 * K[1, 2]) * scale
        if _ok(p[0], p[1]):
            rows.append([1, _rint(p[0]), _rint(p[1]), 0, 0, max(1, _rint(radius * scale))] + list(colour))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 9)
