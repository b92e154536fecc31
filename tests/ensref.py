"""Shared by tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py: the seeded cases the two ensemble kernels are run on, their
float64 reference (ursonet_amd.ensemble.add64 / settle64) and the bounds, counted from the operations.

The bound.  With eps = 2^-52, one member's p_i = e_i / Z carries: exp at <= 1 ulp on either side, the sum Z of K positive terms
(<= K - 1 roundings on a path, whatever the order: K eps covers the device's order and NumPy's pairwise one), one division and one
accumulation -- (K + 16) eps relative per member added, M (K + 16) eps for M members.  H_MEAN, H_MEMBERS and PEAK are sums / maxima of such
terms and take the same relative bound; MI is a difference of two of them and takes the bound times (H_MEAN + H_MEMBERS), absolute.
logp = fl32(log(pbar)): the fp64 error is ~1e-5 of an fp32 ulp, so the device's value is the reference's except where log(pbar) falls that
close to a rounding boundary -- one ulp there, nowhere more.  CAP is the share of elements, over all cases together, that may differ at all
(a case with a handful of elements cannot be held to a share of its own)."""
import numpy as np

from ursonet_amd import ensemble as E

EPS = 2.0 ** -52
KS = (1, 2, 63, 64, 257, 4096)
BIG_K = 32768
MS = (1, 2, 5)
SCALES = (1.0, 30.0)
CAP = 1e-3


def all_cases():
    """(K, M, scale) of every kernel case."""
    return [(K, M, s) for K in KS + (BIG_K,) for M in (MS if K != BIG_K else (2,)) for s in SCALES]


def tol(K, M):
    return (K + 16) * EPS * M


def shape_of(K):
    """(B, n, row0, ld) of a case: a batch with a row past n, rows in front of it and padding behind the columns; the one large case is
    packed and starts at row 0."""
    return (2, 2, 0, K) if K == BIG_K else (3, 2, 5, K + 3)


def member_logits(K, M, scale):
    """[M, n, K] fp32, seeded by the case: normal logits of the given scale.  Scale 1: row 0 has a -inf bin in member 0 and, for K > 1,
    in every member at another column.  Scale 30: row 1 has a NaN in the last member (K > 1), so that row is NaN in every output."""
    n = shape_of(K)[1]
    rng = np.random.default_rng([K, M, int(scale)])
    z = (rng.normal(size=(M, n, K)) * scale).astype(np.float32)
    if K > 1:
        if scale == 1.0:
            z[0, 0, K // 2] = -np.inf
            z[:, 0, K - 1] = -np.inf
        else:
            z[M - 1, 1, K // 3] = np.nan
    return z


def reference(z):
    """(acc [n, K], stat [n, 4], logp fp32 [n, K], table [n, 8]) of members z [M, n, K]."""
    acc = stat = None
    for zj in z:
        acc, stat = E.add64(zj, acc, stat)
    logp, table = E.settle64(acc, stat, len(z))
    return acc, stat, logp, table


def logp_flips(acc, M, K):
    """How many elements of fl32(log(acc / M)) change when acc moves by the bound either way: the premise of CAP for a seed."""
    with np.errstate(all="ignore"):
        base = E.settle64(acc, np.zeros((len(acc), 4)), M)[0]
        lo = E.settle64(acc * (1 - tol(K, M)), np.zeros((len(acc), 4)), M)[0]
        hi = E.settle64(acc * (1 + tol(K, M)), np.zeros((len(acc), 4)), M)[0]
    fin = np.isfinite(base)
    return int(((lo != base) | (hi != base))[fin].sum()), int(fin.sum())
