"""The kernel-level layout of the LAMB tests, shared by tests/test_lamb_cpu.py (which checks, on the NumPy rule alone, that the layout
claims what the GPU test needs) and tests/test_lamb_gpu.py (which runs the kernels over it).  NumPy only.

Ten tensors in one flat buffer at the sizes where the kernels take another path, a NaN-payload sentinel in all padding and guards of all
five buffers, one tensor with g = 0 and zero moments, one with w = 0, two that do not adapt; non-trivial m, v >= 0, vhat >= 0 on both
sides of v, and the hyper / state of t = 3."""
import numpy as np

from ursonet_amd import lamb as B

SIZES = [1, 3, 4, 5, 255, 1023, 4096, 4097, 2 * 4096 + 4, 3 * 4096]
ZERO_G, ZERO_W, PLAIN = 5, 6, (2, 7)           # tensor indices: g == 0 and zero moments | w == 0 | the two that do not adapt
SENTINEL = 0x7FA5A5A5                          # a NaN with a payload: an arithmetic pass over the padding would show, and so would a store
GUARD = 64                                     # floats in front of and behind the tensors (the buffers stay 16-byte aligned)
NAMES = ("w", "g", "m", "v", "vhat")
CLIPS = (0.0, 1e9, 1e4)                        # clip = 0 and 1e9: c = 1 (no clip, and one out of reach); 1e4: c < 1
ETA, EPS = 1.0, 1e-8

_cache = {}


def hyper_state(clip, t=3):
    """Adam's 8 floats and the state after t ticks from {1, 1, 0} (lr 0.001, b1 0.9, b2 0.999, eps 1e-7)."""
    hyper = np.array([0.001, 0.9, 0.999, 1e-7, clip, 0.0, 1.0 - 0.9, 1.0 - 0.999], dtype=np.float32)
    state = np.array(B.STATE_INIT, dtype=np.float32)
    for _ in range(t):
        hyper, state = B.tick32(hyper, state)
    return hyper, state


def layout():
    """Computed once and shared; the tests copy what they change."""
    if not _cache:
        rng = np.random.default_rng(20)
        tensors, off = [], GUARD
        for t, n in enumerate(SIZES):
            tensors.append((off, n, t not in PLAIN))
            off += -(-n // 4) * 4 + (8 if t == 3 else 0)                     # (one wider gap: offsets need not be dense)
        total = off + GUARD
        used = np.zeros(total, dtype=bool)
        bufs = {}
        for name in NAMES:
            x = np.full(total, SENTINEL, dtype=np.uint32).view(np.float32).copy()
            for o, n, _a in tensors:
                x[o:o + n] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
                used[o:o + n] = True
            bufs[name] = x
        for t, (o, n, _a) in enumerate(tensors):
            s = slice(o, o + n)
            bufs["g"][s] *= np.float32(10.0 ** ((t % 5) - 2))                # gradient scales over four decades
            bufs["w"][s] *= np.float32(10.0 ** ((t % 3) - 2))                # weight scales over three: LAMB_CLIP sees both sides of its min
            bufs["v"][s] = np.square(bufs["v"][s])                           # second moments: >= 0
            bufs["vhat"][s] = bufs["v"][s] * rng.uniform(0.5, 2.0, n).astype(np.float32)      # on both sides of v
        o, n, _a = tensors[ZERO_G]
        for name in ("g", "m", "v", "vhat"):
            bufs[name][o:o + n] = 0
        o, n, _a = tensors[ZERO_W]
        bufs["w"][o:o + n] = 0
        _cache.update(tensors=tensors, total=total, used=used, normsq=np.float32(np.square(bufs["g"][used].astype(np.float64)).sum()), **bufs)
    return _cache


def reference(clip, clip_mode, steps=1, guard=False, normsq=None, **kw):
    """lamb.step32 over the layout, `steps` times with the same gradient: the list of its results."""
    lay = layout()
    hyper, state = hyper_state(clip)
    w, m, v, vhat = (lay[k] for k in ("w", "m", "v", "vhat"))
    out = []
    for _ in range(steps):
        res = B.step32(w, lay["g"], m, v, vhat, lay["tensors"], hyper, state, lay["normsq"] if normsq is None else normsq, ETA, EPS,
                       clip_mode, guard, **kw)
        w, m, v, vhat, hyper, state = res[:6]
        out.append(res)
    return out
