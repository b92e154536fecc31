"""Layer-wise adaptive rate scaling for SGD with momentum, on the device (Config.LARS): the configuration rules,
which tensors adapt, and `slot_sums32` / `norms64` / `trust32` / `update32` / `step32`, the written specification of the device kernels
behind urso_lars_norms, urso_lars_trust and urso_lars_sgd (include/ursonet_ext.h).

  Config.LARS        None (default: off, the step is launch for launch what it is without this module) | the trust coefficient eta, a
                     float > 0 (0.001 is the usual value)
  Config.LARS_EPS    1e-8, a float >= 0: added to the denominator of the trust ratio
  Config.LARS_CLIP   False | True = the "clip" mode of LARC: the effective rate of a tensor never exceeds the global one

A tensor adapts when its shape has two or more dimensions (conv and Dense kernels); biases, BN gamma / beta and the two loss-weight scalars
keep trust 1.  With g the finalised flat gradient (weight decay inside, the mean of GRAD_ACCUM_STEPS taken, unscaled under LOSS_SCALE),
lr / mom / clip the three floats of `hyper` and normsq the squared global norm of g:

    norm = sqrtf(normsq);  c = (clip > 0 and norm >= clip) ? clip / norm : 1                  float32, as the plain SGD launch computes it
    per tensor t, float64:   nw = sqrt(sum w^2), ng = sqrt(sum g^2)                           sums: see below
                             q = 1 if nw == 0 or ng == 0 else eta * nw / (c * ng + LARS_EPS)
                             q = min(q / lr, 1) when LARS_CLIP
                             trust = fl32(q)
    per element, float32:    step = (lr * c) * trust;  v = mom * v - step * g;  w = w + v     every operation rounded once

The sums.  A tensor of n elements is cut into chunks(n) chunks of CHUNK = 4096 elements (the last one short); a chunk yields two float32
slots, the sum of w^2 and the sum of g^2, in the order of one block of 256 threads: thread t owns the 16-byte groups t, 256 + t, 512 + t,
768 + t of the chunk and adds their squares (each rounded once) to a running sum from 0.0f, groups in order, x y z w each; the 64 lanes
of a wave are added by the xor shuffle (offsets 32, 16, 8, 4, 2, 1); the four wave sums are added in wave order from 0.0f.  Elements past
the tensor's end contribute nothing.  A tensor's slots are then added in index order in float64.  So every value is a function of the
inputs alone, and NumPy reproduces the bits: all float64 operations are + * / sqrt and a comparison.

Because weight decay is already inside g, ng is the norm of (gradient + decay * w): the LARC form, not the LARS paper's
eta * |w| / (|grad| + decay * |w|).

No GPU and no torch needed here."""
import math

import numpy as np

KEY, KEY_EPS, KEY_CLIP = "LARS", "LARS_EPS", "LARS_CLIP"
CHUNK = 4096                   # URSO_LARS_CHUNK: elements per block and slot pair
THREADS = 256                  # threads per block: four waves of 64
GROUPS = CHUNK // (4 * THREADS)          # 16-byte groups per thread
WAVE_ORDER = (0, 1, 2, 3)

_f32, _f64 = np.float32, np.float64


def validate(config, world=1):
    """Validate the three keys and return (eta, eps, clip) -- or None when Config.LARS is None (a config without the key is off).
    ValueError: a bool, a non-float or a non-positive (or non-finite) LARS; a negative or non-finite LARS_EPS; a non-bool LARS_CLIP; LARS
    with an optimizer other than SGD; LARS in a data-parallel run (world > 1)."""
    eta = getattr(config, KEY, None)
    eps = getattr(config, KEY_EPS, 1e-8)
    clip = getattr(config, KEY_CLIP, False)
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, (int, float, np.integer, np.floating)) or not math.isfinite(eps) or eps < 0:
        raise ValueError("%s must be a finite float >= 0, got %r" % (KEY_EPS, eps))
    if not isinstance(clip, (bool, np.bool_)):
        raise ValueError("%s must be a bool, got %r" % (KEY_CLIP, clip))
    if eta is None:
        return None
    if isinstance(eta, (bool, np.bool_)) or not isinstance(eta, (float, np.floating)) or not math.isfinite(eta) or eta <= 0:
        raise ValueError("%s must be None or the trust coefficient, a float > 0, got %r" % (KEY, eta))
    opt = str(getattr(config, "OPTIMIZER", "SGD")).upper()
    if opt != "SGD":
        raise ValueError("%s needs OPTIMIZER = 'SGD' (got %r): the Adam form, LAMB, is not built; leave %s = None" % (KEY, opt, KEY))
    if int(world) > 1:
        raise ValueError("%s is not supported under data parallelism (world size %d): the optimizer launches behind the all-reduce do not "
                         "carry it yet; train on one GPU or leave %s = None" % (KEY, int(world), KEY))
    return float(eta), float(eps), bool(clip)


def enabled(config, mode="training"):
    """True when `config` asks for LARS and `mode` trains: an inference model ignores the keys."""
    return mode == "training" and validate(config) is not None


def adapts(shape):
    """A tensor adapts when its shape has two or more dimensions: conv and Dense kernels.  Everything else has trust 1."""
    return len(tuple(shape)) >= 2


def chunks(n):
    """The chunks, blocks and slot pairs of a tensor of n elements: ceil(n / CHUNK); 0 for n = 0."""
    n = int(n)
    if n < 0:
        raise ValueError("chunks: n must be >= 0, got %d" % n)
    return (n + CHUNK - 1) // CHUNK


def slot_sums32(x, n=None, wave_order=WAVE_ORDER):
    """The float32 slots of the first n elements of x (default: all): [chunks(n)] sums of squares in the documented order, bit for bit
    what a block of urso_lars_norms writes.  wave_order is the order in which the four wave sums are added; the device's is (0, 1, 2, 3),
    and any other is another function (the tests use one to show that the comparison sees the order)."""
    x = np.asarray(x, dtype=_f32).reshape(-1)
    n = x.size if n is None else int(n)
    assert 0 <= n <= x.size
    nc = chunks(n)
    pad = np.zeros(nc * CHUNK, dtype=_f32)             # (adding the square of a padding zero, +0, changes no bit of a sum that began at +0)
    pad[:n] = x[:n]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = (pad * pad).astype(_f32).reshape(nc, GROUPS, THREADS, 4)
        acc = np.zeros((nc, THREADS), dtype=_f32)
        for j in range(GROUPS):                        # the thread's groups in order, x y z w each
            for e in range(4):
                acc = (acc + sq[:, j, :, e]).astype(_f32)
        v = acc.reshape(nc, THREADS // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):                 # the xor shuffle: every lane adds its partner's value
            v = (v + v[:, :, lane ^ o]).astype(_f32)
        out = np.zeros(nc, dtype=_f32)
        for wv in wave_order:
            out = (out + v[:, wv, 0]).astype(_f32)
    return out


def norms64(slots):
    """sqrt of the float64 sum of a tensor's float32 slots, added in index order from 0.0."""
    s = _f64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(slots, dtype=_f32).reshape(-1):
            s = s + _f64(x)
        return np.sqrt(s)


def clip_factor32(normsq, clip):
    """c, the global-norm clip factor, in float32 as sgd_kernel (csrc/pool_loss_optim.hip) computes it."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = np.sqrt(_f32(normsq))
        clip = _f32(clip)
        return _f32(clip / norm) if (clip > 0 and norm >= clip) else _f32(1.0)


def trust64(nw, ng, eta, eps, clip_mode, lr, c, adapt=True):
    """q of one tensor in float64 (before its one rounding to float32)."""
    nw, ng = _f64(nw), _f64(ng)
    if not adapt or nw == 0 or ng == 0:
        return _f64(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = _f64(eta) * nw / (_f64(_f32(c)) * ng + _f64(eps))
        if clip_mode:
            q = q / _f64(_f32(lr))
            q = q if q < 1.0 else _f64(1.0)
    return q


def trust32(nw, ng, eta, eps, clip_mode, lr, c, adapt=True):
    """trust = fl32(q), rounded once: bit for bit what urso_lars_trust writes."""
    with np.errstate(over="ignore"):
        return _f32(trust64(nw, ng, eta, eps, clip_mode, lr, c, adapt))


def update32(w, g, v, lr, mom, c, trust):
    """One tensor's update in float32, every operation rounded once: step = (lr * c) * trust; v = mom * v - step * g; w = w + v.
    Returns (w, v), new arrays."""
    w, g, v = (np.asarray(a, dtype=_f32) for a in (w, g, v))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        step = _f32(_f32(_f32(lr) * _f32(c)) * _f32(trust))
        a = (_f32(mom) * v).astype(_f32)
        b = (step * g).astype(_f32)
        v2 = (a - b).astype(_f32)
        return (w + v2).astype(_f32), v2


def step32(w, g, v, tensors, hyper, normsq, eta, eps=1e-8, clip_mode=False, guard=False):
    """The whole step over flat float32 buffers.  tensors: [(offset, numel, adapt)], hyper: (lr, mom, clip), normsq: the squared global
    norm the engine computed.  guard: the loss-scaled form -- a non-finite normsq changes nothing.
    Returns (w, v, trust[T] float32, stat[T][3] float64 = nw, ng, q) -- or (w, v, None, None) for a skipped step.  Floats between the
    tensors (padding) keep their bits."""
    w, v = np.array(w, dtype=_f32, copy=True), np.array(v, dtype=_f32, copy=True)
    g = np.asarray(g, dtype=_f32)
    if guard and not np.isfinite(_f32(normsq)):
        return w, v, None, None
    lr, mom, clip = (_f32(x) for x in hyper)
    c = clip_factor32(normsq, clip)
    trust = np.ones(len(tensors), dtype=_f32)
    stat = np.zeros((len(tensors), 3), dtype=_f64)
    for t, (o, n, adapt) in enumerate(tensors):
        o, n = int(o), int(n)
        nw, ng = norms64(slot_sums32(w[o:o + n])), norms64(slot_sums32(g[o:o + n]))
        q = trust64(nw, ng, eta, eps, clip_mode, lr, c, adapt)
        with np.errstate(over="ignore"):
            trust[t] = _f32(q)
        stat[t] = (nw, ng, q)
        w[o:o + n], v[o:o + n] = update32(w[o:o + n], g[o:o + n], v[o:o + n], lr, mom, c, trust[t])
    return w, v, trust, stat


def summary(report):
    """{"min", "median", "max", "tensors"} of the trust column of an Engine.lars_report() ({key: (nw, ng, trust)}), for the log line.
    train() passes the adapting tensors alone (lars_report(adapting_only=True)): the trust 1 of every bias and BN vector would drown the
    median.  None for an empty report."""
    vals = sorted(float(r[2]) for r in report.values())
    if not vals:
        return None
    m = len(vals)
    med = vals[m // 2] if m % 2 else 0.5 * (vals[m // 2 - 1] + vals[m // 2])
    return {"min": vals[0], "median": med, "max": vals[-1], "tensors": m}
