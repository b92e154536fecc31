"""LAMB: layer-wise trust ratios for Adam(amsgrad) with global-norm clip, on the device (Config.LAMB): the
configuration rules and `tick32` / `moments32` / `direction32` / `trust64` / `trust32` / `apply32` / `step32`, the written specification of
the device kernels behind urso_lamb_moments, urso_lamb_trust and urso_lamb_apply (include/ursonet_opt.h).

  Config.LAMB        None (default: off, the step is launch for launch what it is without this module) | the trust coefficient eta, a
                     float > 0 (1.0 is the usual value)
  Config.LAMB_EPS    1e-8, a finite float >= 0: added to the denominator of the trust ratio
  Config.LAMB_CLIP   False | True = a tensor's rate never exceeds plain Adam's: q = min(q, 1)

Which tensors adapt is lars.adapts: two or more dimensions (conv and Dense kernels); biases, BN gamma / beta and the two loss-weight scalars
keep trust 1.  With g the finalised flat gradient (weight decay inside, the mean of GRAD_ACCUM_STEPS taken, unscaled under LOSS_SCALE),
hyper Adam's 8 floats {lr, b1, b2, eps, clip, t, c1, c2}, state the 3 floats {p1, p2, kt} ({1, 1, 0} before the first step) and normsq the
squared global norm of g, every float32 operation rounded once:

    tick, one thread:        t = t + 1;  p1 = p1 * b1;  p2 = p2 * b2;  kt = sqrtf(1 - p2) / (1 - p1)
    per element, float32:    c = clip_factor(clip, normsq);  gi = g * c
                             m = b1 * m + c1 * gi;  v = b2 * v + c2 * (gi * gi);  vhat = max(vhat, v)
                             a = kt * m;  den = sqrtf(vhat) + eps;  r = a / den
    per tensor, float64:     nw = sqrt(sum w^2), nr = sqrt(sum r^2)          the sums of lars.py (slot_sums32, norms64), w before the step
                             q = 1 if not adapting or nw == 0 or nr == 0 else eta * nw / (nr + LAMB_EPS)
                             q = min(q, 1) when LAMB_CLIP;  trust = fl32(q)
    per element, float32:    step = lr * trust;  w = w - step * r            r recomputed from the stored m and vhat: the same bits

The products p1, p2 stand in for powf(b, t) on purpose: powf has no bit-exact host counterpart, while * - / and sqrtf are rounded
correctly on both sides (lars.clip_factor32 already relies on that).  kt therefore differs from Keras's sqrt(1 - b2^t) / (1 - b1^t) by a
few ulp.  The clip factor does not appear in the trust ratio: it is inside r.

Weight decay reaches r through g and the moments: the reference's L2 form, not the LAMB paper's decoupled r + lambda w.

A step that LOSS_SCALE marks as overflowed (a non-finite normsq under `guard`) keeps every bit: w, m, v, vhat, t, the state, the slots,
trust and stat.

No GPU and no torch needed here."""
import math

import numpy as np

from . import lars
from .lars import adapts, summary          # the same tensors adapt; the same min / median / max of a report's trust column

KEY, KEY_EPS, KEY_CLIP = "LAMB", "LAMB_EPS", "LAMB_CLIP"
STATE_INIT = (1.0, 1.0, 0.0)               # {p1, p2, kt} before the first step
T_INDEX = 5                                # hyper[5] = t

_f32, _f64 = np.float32, np.float64


def validate(config, world=1):
    """Validate the three keys and return (eta, eps, clip) -- or None when Config.LAMB is None (a config without the key is off).
    ValueError: a bool, a non-float or a non-positive (or non-finite) LAMB; a negative or non-finite LAMB_EPS; a non-bool LAMB_CLIP; LAMB
    with OPTIMIZER = 'SGD'; LAMB together with LARS; LAMB in a data-parallel run (world > 1)."""
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
    if getattr(config, lars.KEY, None) is not None:
        raise ValueError("%s and %s are two rules for one step: set one of them (LARS is SGD's, LAMB is Adam's)" % (KEY, lars.KEY))
    opt = str(getattr(config, "OPTIMIZER", "SGD")).upper()
    if opt == "SGD":
        raise ValueError("%s needs an OPTIMIZER other than 'SGD' (Adam): the SGD form is Config.LARS; leave %s = None" % (KEY, KEY))
    if int(world) > 1:
        raise ValueError("%s is not supported under data parallelism (world size %d): the optimizer launches behind the all-reduce do not "
                         "carry it yet; train on one GPU or leave %s = None" % (KEY, int(world), KEY))
    return float(eta), float(eps), bool(clip)


def enabled(config, mode="training"):
    """True when `config` asks for LAMB and `mode` trains: an inference model ignores the keys."""
    return mode == "training" and validate(config) is not None


def tick32(hyper, state):
    """The tick: (hyper, state) after it, new float32 arrays.  t = t + 1; p1 = p1 * b1; p2 = p2 * b2; kt = sqrtf(1 - p2) / (1 - p1)."""
    hyper, state = np.array(hyper, dtype=_f32, copy=True), np.array(state, dtype=_f32, copy=True)
    b1, b2 = hyper[1], hyper[2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        hyper[T_INDEX] = _f32(hyper[T_INDEX] + _f32(1.0))
        p1 = _f32(state[0] * b1)
        p2 = _f32(state[1] * b2)
        a = _f32(_f32(1.0) - p2)
        b = _f32(_f32(1.0) - p1)
        state[:] = (p1, p2, _f32(np.sqrt(a) / b))
    return hyper, state


def moments32(g, m, v, vhat, hyper, c):
    """One tensor's moments in float32, every operation rounded once.  c: the clip factor.  Returns (m, v, vhat), new arrays."""
    g, m, v, vhat = (np.asarray(a, dtype=_f32) for a in (g, m, v, vhat))
    b1, b2, c1, c2 = (_f32(hyper[i]) for i in (1, 2, 6, 7))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        gi = (g * _f32(c)).astype(_f32)
        m2 = ((b1 * m).astype(_f32) + (c1 * gi).astype(_f32)).astype(_f32)
        gg = (gi * gi).astype(_f32)
        v2 = ((b2 * v).astype(_f32) + (c2 * gg).astype(_f32)).astype(_f32)
        return m2, v2, np.fmax(vhat, v2).astype(_f32)          # fmax: the device's fmaxf returns the other operand for a NaN


def direction32(m, vhat, kt, eps):
    """r = (kt * m) / (sqrtf(vhat) + eps) in float32, every operation rounded once."""
    m, vhat = np.asarray(m, dtype=_f32), np.asarray(vhat, dtype=_f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        a = (_f32(kt) * m).astype(_f32)
        den = (np.sqrt(vhat).astype(_f32) + _f32(eps)).astype(_f32)
        return (a / den).astype(_f32)


def trust64(nw, nr, eta, eps, clip_mode, adapt=True):
    """q of one tensor in float64 (before its one rounding to float32)."""
    nw, nr = _f64(nw), _f64(nr)
    if not adapt or nw == 0 or nr == 0:
        return _f64(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = _f64(eta) * nw / (nr + _f64(eps))
        if clip_mode:
            q = q if q < 1.0 else _f64(1.0)
    return q


def trust32(nw, nr, eta, eps, clip_mode, adapt=True):
    """trust = fl32(q), rounded once: bit for bit what urso_lamb_trust writes."""
    with np.errstate(over="ignore"):
        return _f32(trust64(nw, nr, eta, eps, clip_mode, adapt))


def apply32(w, r, lr, trust):
    """One tensor's update in float32: step = lr * trust; w = w - step * r.  Returns w, a new array."""
    w, r = np.asarray(w, dtype=_f32), np.asarray(r, dtype=_f32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        step = _f32(_f32(lr) * _f32(trust))
        return (w - (step * r).astype(_f32)).astype(_f32)


def step32(w, g, m, v, vhat, tensors, hyper, state, normsq, eta, eps=1e-8, clip_mode=False, guard=False, wave_order=lars.WAVE_ORDER,
           intermediates=None):
    """The whole step over flat float32 buffers.  tensors: [(offset, numel, adapt)], hyper: Adam's 8 floats, state: {p1, p2, kt}, normsq:
    the squared global norm the engine computed.  guard: the loss-scaled form -- a non-finite normsq changes nothing.
    Returns (w, m, v, vhat, hyper, state, trust[T] float32, stat[T][3] float64 = nw, nr, q) -- trust and stat None for a skipped step.
    Floats between the tensors (padding) keep their bits.  wave_order: see lars.slot_sums32 (the device's is the default).
    intermediates: a list that receives every float32 array the kernels hold in between (gi, the products, r, step * r, the slots)."""
    w, m, v, vhat = (np.array(a, dtype=_f32, copy=True) for a in (w, m, v, vhat))
    g = np.asarray(g, dtype=_f32)
    hyper, state = np.array(hyper, dtype=_f32, copy=True), np.array(state, dtype=_f32, copy=True)
    if guard and not np.isfinite(_f32(normsq)):
        return w, m, v, vhat, hyper, state, None, None
    hyper, state = tick32(hyper, state)
    lr, eps_a, kt = hyper[0], hyper[3], state[2]
    c = lars.clip_factor32(normsq, hyper[4])
    trust = np.ones(len(tensors), dtype=_f32)
    stat = np.zeros((len(tensors), 3), dtype=_f64)
    for t, (o, n, adapt) in enumerate(tensors):
        o, n = int(o), int(n)
        s = slice(o, o + n)
        w_slots = lars.slot_sums32(w[s], wave_order=wave_order)
        m0, v0 = m[s].copy(), v[s].copy()
        m[s], v[s], vhat[s] = moments32(g[s], m[s], v[s], vhat[s], hyper, c)
        r = direction32(m[s], vhat[s], kt, eps_a)
        r_slots = lars.slot_sums32(r, wave_order=wave_order)
        nw, nr = lars.norms64(w_slots), lars.norms64(r_slots)
        q = trust64(nw, nr, eta, eps, clip_mode, adapt)
        with np.errstate(over="ignore"):
            trust[t] = _f32(q)
        stat[t] = (nw, nr, q)
        w2 = apply32(w[s], r, lr, trust[t])
        if intermediates is not None:
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                gi = (g[s] * c).astype(_f32)
                intermediates += [gi, (hyper[1] * m0).astype(_f32), (hyper[6] * gi).astype(_f32), (gi * gi).astype(_f32),
                                  (hyper[7] * (gi * gi).astype(_f32)).astype(_f32), (hyper[2] * v0).astype(_f32), m[s].copy(), v[s].copy(),
                                  vhat[s].copy(), (kt * m[s]).astype(_f32), np.sqrt(vhat[s]).astype(_f32), r,
                                  (w[s] * w[s]).astype(_f32), (r * r).astype(_f32), w_slots, r_slots,
                                  (_f32(lr * trust[t]) * r).astype(_f32), w2, np.array([_f32(lr * trust[t]), trust[t]], dtype=_f32)]
        w[s] = w2
    return w, m, v, vhat, hyper, state, trust, stat
