"""SAM: sharpness-aware minimization on the device (Config.SAM; Foret et al. 2021): the configuration rules and
`scale32` / `ascend32` / `descend32` / `settle32`, the written specification of the device kernels behind urso_sam_ascend,
urso_sam_descend and urso_sam_settle (include/ursonet_train.h).  The optimizer steps with the gradient taken at w + rho g / |g|, not at w.

  Config.SAM         None (default: off, every launch and every bit is what it is without this module) | rho, the radius of the ascent, a
                     finite float > 0 (0.05 is the usual value)
  Config.SAM_EPS     1e-12, a finite float >= 0: added to the norm in the denominator

g1 is what the backward pass leaves in flat_g at w: finalised (weight decay, BN gamma / beta and the loss-weight slots inside, unscaled under
LOSS_SCALE).  N is the float32 squared norm of all of flat_g by the unfused urso_sqnorm launch (the bits of hip.sqnorm; padding between
the slices is zero and adds nothing).  state is URSO_SAM_STATE = 8 floats {rho, eps, normsq, scale, applied, applied_total, pending, 0};
the host sets rho and eps, the norm launch writes normsq.  Every float32 operation is rounded once (the library is built with
-ffp-contract=off; sqrtf and / are correctly rounded on both sides):

    applied = isfinite(N) and N > 0
    s       = rho / (sqrtf(N) + eps)       if applied else 0             three float32 operations
    ascend:   w0 = w (the bits);  if applied:  w = w + (s * g1)          the product rounded, then the sum
              one thread: scale = s;  applied = 1 | 0;  applied_total += applied;  pending += applied
    (prep, forward, losses, backward at w + e: g2 in flat_g)
    descend:  w = w0 (the bits)
    (the optimizer's launches on g2, unchanged)

A tensor whose gradient is zero -- a frozen layer -- does not move (a -0.0 weight reads +0.0 during the second pass and gets its bits back
from w0).  A NaN, infinite or zero norm moves nothing.

The skipped step.  Under LOSS_SCALE the optimizer skips a step whose squared norm (of g2; under GRAD_ACCUM_STEPS of the mean it closes with)
is not finite.  Such a step leaves applied_total as it was: behind the optimizer's norm one thread settles the count,

    settle:   if not isfinite(normsq):  applied_total -= pending          (guard: the loss-scaled form, the only one the engine launches)
              pending = 0

so `pending` holds the ascents since the last settled optimizer step (one, or up to GRAD_ACCUM_STEPS of them).  Without LOSS_SCALE no step
is skipped, nothing settles, and `pending` is a count nobody reads.  The counts are float32 and exact up to 2^24.

No GPU and no torch needed here."""
import math

import numpy as np

KEY, KEY_EPS = "SAM", "SAM_EPS"
RHO, EPS, NORMSQ, SCALE, APPLIED, APPLIED_TOTAL, PENDING = 0, 1, 2, 3, 4, 5, 6      # the fields of the device state
STATE_LEN = 8                                                                       # URSO_SAM_STATE
STATE_INIT = (0.0,) * STATE_LEN                # before the first step; initial_state() puts rho and eps in

_f32 = np.float32
_NUM = (int, float, np.integer, np.floating)


def validate(config, world=1):
    """Validate the two keys and return (rho, eps) -- or None when Config.SAM is None (a config without the key is off).
    ValueError: a bool, a string, a non-float, a non-finite or non-positive SAM; a bool, non-number, negative or non-finite SAM_EPS; SAM
    in a data-parallel run (world > 1)."""
    rho = getattr(config, KEY, None)
    eps = getattr(config, KEY_EPS, 1e-12)
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, _NUM) or not math.isfinite(eps) or eps < 0:
        raise ValueError("%s must be a finite float >= 0, got %r" % (KEY_EPS, eps))
    if rho is None:
        return None
    if isinstance(rho, (bool, np.bool_)) or not isinstance(rho, (float, np.floating)) or not math.isfinite(rho) or rho <= 0:
        raise ValueError("%s must be None or rho, the radius of the ascent, a finite float > 0, got %r" % (KEY, rho))
    if int(world) > 1:
        raise ValueError("%s is not supported under data parallelism (world size %d): the step behind the all-reduce has one backward pass; "
                         "train on one GPU or leave %s = None" % (KEY, int(world), KEY))
    return float(rho), float(eps)


def enabled(config, mode="training"):
    """True when `config` asks for SAM and `mode` trains: an inference model ignores the keys."""
    return mode == "training" and validate(config) is not None


def initial_state(rho, eps):
    """The URSO_SAM_STATE floats before the first step."""
    st = list(STATE_INIT)
    st[RHO], st[EPS] = float(rho), float(eps)
    return tuple(st)


def scale32(normsq, rho, eps):
    """(s, applied): s = rho / (sqrtf(N) + eps) in float32, every operation rounded once, and whether the ascent moves anything."""
    n = _f32(normsq)
    if not (np.isfinite(n) and n > 0):
        return _f32(0.0), False
    with np.errstate(over="ignore", divide="ignore"):
        root = _f32(np.sqrt(n))
        den = _f32(root + _f32(eps))
        return _f32(_f32(rho) / den), True


def ascend32(w, g, normsq, rho, eps):
    """(w_new, w0, s, applied): w0 the bits of w, w_new = w + (s * g) where applied, else the bits of w.  New arrays."""
    w = np.asarray(w, dtype=_f32)
    g = np.asarray(g, dtype=_f32)
    s, applied = scale32(normsq, rho, eps)
    w0 = w.copy()
    if not applied:
        return w.copy(), w0, s, False
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        e = (s * g).astype(_f32)
        return (w + e).astype(_f32), w0, s, True


def descend32(w, w0):
    """w after the way back: the bits of w0, whatever w holds."""
    return np.asarray(w0, dtype=_f32).copy()


def ascend_state32(state):
    """The state behind urso_sam_ascend, a new float32 array: scale, applied, applied_total and pending from rho, eps and normsq."""
    st = np.array(state, dtype=_f32, copy=True)
    s, applied = scale32(st[NORMSQ], st[RHO], st[EPS])
    a = _f32(1.0 if applied else 0.0)
    st[SCALE], st[APPLIED] = s, a
    st[APPLIED_TOTAL] = _f32(st[APPLIED_TOTAL] + a)
    st[PENDING] = _f32(st[PENDING] + a)
    return st


def settle32(state, normsq, guard=True):
    """The state behind urso_sam_settle, a new float32 array: a skipped step (guard and a non-finite normsq) takes its ascents out of
    applied_total; pending = 0 either way."""
    st = np.array(state, dtype=_f32, copy=True)
    if guard and not np.isfinite(_f32(normsq)):
        st[APPLIED_TOTAL] = _f32(st[APPLIED_TOTAL] - st[PENDING])
    st[PENDING] = _f32(0.0)
    return st
