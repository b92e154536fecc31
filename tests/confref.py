"""Cases and a brute-force restatement for the conformal kernels (urso_conf_score / urso_conf_bound; ursonet_amd/conformal.py is the
specification).  brute_score / brute_bound sort the bins and cumulate with Python integers; fragile() counts, per row, the bins at which
two exp implementations that are both good to 1 ulp may round the weight differently."""
import numpy as np

from ursonet_amd import conformal as Cf

KS = (1, 3, 4, 5, 27, 1023, 4099, 32768)                          # 4099 = 4 * 1024 + 3: the second lap plus the ragged group
QS = (1e-12, 0.5, 0.9, 1.0, float("inf"))
D = {Cf.ANGLE: 4, Cf.EUCLID: 3}


def rows_of(K):
    """(B, n, row0): n = 3 rows at 32768, up to 8 elsewhere; B > n; rows in front of row0."""
    n = 3 if K >= 32768 else (8 if K >= 27 else 4)
    return n + 2, n, 5


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def bin_map(K, metric, seed=0):
    """ANGLE: fp32 unit quaternions [K, 4], every third one the sign flip or the copy of its neighbour (groups of equal keys); EUCLID:
    fp64 points [K, 3] of a jittered grid with every fifth a duplicate."""
    rng = np.random.default_rng(1000 + seed)
    if metric == Cf.ANGLE:
        m = _unit(rng.normal(size=(K, 4))).astype(np.float32)
        for i in range(2, K, 3):
            m[i] = -m[i - 1] if i % 2 else m[i - 1]
        return m
    m = rng.uniform(-2, 2, size=(K, 3)) + np.array([0.0, 0.0, 10.0])
    for i in range(4, K, 5):
        m[i] = m[i - 1]
    return m


def case(K, metric, seed=0):
    """-> z fp32 [n, K] (normal logits, sigma 2 .. 6 by row), bin map, est fp64 [n, D], ref fp64 [n, D]."""
    _B, n, _row0 = rows_of(K)
    rng = np.random.default_rng(7 * K + 3 * metric + seed)
    sigma = np.linspace(2.0, 6.0, n)[:, None]
    z = (rng.normal(size=(n, K)) * sigma).astype(np.float32)
    m = bin_map(K, metric, seed)
    if metric == Cf.ANGLE:
        est, ref = _unit(rng.normal(size=(n, 4))), _unit(rng.normal(size=(n, 4)))
    else:
        est = rng.uniform(-2, 2, size=(n, 3)) + np.array([0.0, 0.0, 10.0])
        ref = est + rng.normal(size=(n, 3))
    return z, m, est, ref


def fragile(z, ulps=4):
    """F [n]: the bins whose exp(d) 2^34 lies within `ulps` ulp of a rounding boundary (an integer plus one half)."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = z.astype(np.float64) - z.max(axis=1).astype(np.float64)[:, None]
        s = np.exp(d) * float(2 ** Cf.SHIFT)
        s = np.where(np.isfinite(s), s, 0.0)
        near = np.abs(s - (np.floor(s) + 0.5)) <= ulps * np.spacing(np.maximum(s, 0.5))
    return near.sum(axis=1)


def _int_weights(z_row):
    w, _W, _ok = Cf.weights64(z_row[None, :])
    return [int(x) for x in w[0]]


def brute_score(z, m, est, ref, metric):
    """score64's integer columns by a Python loop: -> list of (C, W, near) per row."""
    keys = Cf.keys64(metric, m, est)
    kref = Cf.ref_keys64(metric, est, ref)
    out = []
    for b in range(len(z)):
        w = _int_weights(z[b])
        closer = (keys[b] > kref[b]) if metric == Cf.ANGLE else (keys[b] < kref[b])
        out.append((sum(w[i] for i in np.flatnonzero(closer)), sum(w), int(closer.sum())))
    return out


def brute_bound(z, m, est, metric, q):
    """bound64's selection by sorting the bins and cumulating Python integers: -> list of (key or None, G, count, W) per row."""
    keys = Cf.keys64(metric, m, est)
    out = []
    for b in range(len(z)):
        w = _int_weights(z[b])
        W = sum(w)
        order = sorted(range(len(w)), key=lambda i: -keys[b, i] if metric == Cf.ANGLE else keys[b, i])
        G, found, i = 0, None, 0
        while i < len(order):
            j = i
            while j < len(order) and keys[b, order[j]] == keys[b, order[i]]:
                G += w[order[j]]
                j += 1
            if float(G) / float(W) > q:
                found = (float(keys[b, order[i]]), G, j, W)
                break
            i = j
        out.append(found if found is not None else (None, W, len(w), W))
    return out


def ulps(a, b):
    """|a - b| in units of the spacing of b (0 where both are equal, infinities included)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.abs(b)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
