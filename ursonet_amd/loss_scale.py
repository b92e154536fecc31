"""Loss scaling for 16-bit training (Config.LOSS_SCALE): the configuration rules, the layout of the device-side
state buffer and `next_state`, the written specification of the device kernel urso_loss_scale_update (include/ursonet_loss_scale.h).

  Config.LOSS_SCALE                  None (default: off, the step is launch for launch what it is without this module) |
                                     a positive power of two (static scale) | "dynamic"
  Config.LOSS_SCALE_INIT             first scale of the dynamic mode (power of two), default 2**15
  Config.LOSS_SCALE_GROWTH_INTERVAL  finite steps in a row after which the dynamic scale doubles, default 2000
  Config.LOSS_SCALE_MIN / _MAX       bounds of the dynamic scale (powers of two), defaults 1 and 2**24

No GPU and no torch needed here."""
import math

# fields of the fp32 state buffer (URSO_LS_* of include/ursonet_loss_scale.h)
SCALE, INV_SCALE, GOOD_STEPS, GROWTH_INTERVAL, MIN, MAX, SKIPPED_TOTAL, LAST_SKIPPED = range(8)
FIELDS = 8
FIELD_NAMES = ("scale", "inv_scale", "good_steps", "growth_interval", "min", "max", "skipped_total", "last_step_skipped")

DEFAULT_INIT = 2.0 ** 15
DEFAULT_GROWTH_INTERVAL = 2000
DEFAULT_MIN = 1.0
DEFAULT_MAX = 2.0 ** 24
FP32_MIN_SCALE, FP32_MAX_SCALE = 2.0 ** -126, 2.0 ** 126


def is_power_of_two(x):
    """True for a finite positive float whose mantissa is exactly 1/2 (2**k, k any integer)."""
    if isinstance(x, (str, bytes)):
        return False
    try:
        x = float(x)
    except (TypeError, ValueError):
        return False
    if not (x > 0.0) or math.isinf(x) or math.isnan(x):
        return False
    return math.frexp(x)[0] == 0.5


def _pow2(name, v):
    if isinstance(v, bool) or not is_power_of_two(v):
        raise ValueError("%s must be a positive power of two, got %r" % (name, v))
    # the state is fp32: the scale and its reciprocal must both be normal there (2**127 has a subnormal reciprocal, 2**-127 is one itself)
    if not (FP32_MIN_SCALE <= float(v) <= FP32_MAX_SCALE):
        raise ValueError("%s must lie in [2**-126, 2**126] (the device state is fp32 and holds the reciprocal too), got %r" % (name, v))
    return float(v)


def initial_state(config, world=1):
    """Validate the LOSS_SCALE keys of `config` and return the initial state as a list of FIELDS floats, or None when loss scaling is off.
    ValueError: a scale that is not a positive power of two, inconsistent bounds, or a data-parallel run (world > 1)."""
    ls = getattr(config, "LOSS_SCALE", None)
    if ls is None:
        return None
    if int(world) > 1:
        raise ValueError("LOSS_SCALE is not supported under data parallelism (world size %d): the bucketed gradient exchange and the "
                         "two-phase rel_loss would have to carry the scale; train 16-bit runs on one GPU or leave LOSS_SCALE = None" % int(world))
    if getattr(config, "DP_EXACT_REL_LOSS", False):
        raise ValueError("LOSS_SCALE is not supported with DP_EXACT_REL_LOSS (the two-phase rel_loss has no scaled form)")
    if isinstance(ls, str):
        if ls != "dynamic":
            raise ValueError("LOSS_SCALE must be None, a positive power of two or \"dynamic\", got %r" % (ls,))
        init = _pow2("LOSS_SCALE_INIT", getattr(config, "LOSS_SCALE_INIT", DEFAULT_INIT))
        lo = _pow2("LOSS_SCALE_MIN", getattr(config, "LOSS_SCALE_MIN", DEFAULT_MIN))
        hi = _pow2("LOSS_SCALE_MAX", getattr(config, "LOSS_SCALE_MAX", DEFAULT_MAX))
        interval = getattr(config, "LOSS_SCALE_GROWTH_INTERVAL", DEFAULT_GROWTH_INTERVAL)
        if isinstance(interval, bool) or int(interval) != interval or not (1 <= int(interval) < 2 ** 24):
            raise ValueError("LOSS_SCALE_GROWTH_INTERVAL must be an integer in [1, 2**24), got %r" % (interval,))
        if not (lo <= init <= hi):
            raise ValueError("need LOSS_SCALE_MIN <= LOSS_SCALE_INIT <= LOSS_SCALE_MAX, got %r, %r, %r" % (lo, init, hi))
        return [init, 1.0 / init, 0.0, float(int(interval)), lo, hi, 0.0, 0.0]
    scale = _pow2("LOSS_SCALE", ls)
    return [scale, 1.0 / scale, 0.0, 0.0, scale, scale, 0.0, 0.0]          # growth_interval 0 = static


def next_state(state, norm_is_finite):
    """The state after a step whose squared gradient norm was finite (True) or not (False): what urso_loss_scale_update leaves in the
    buffer, field for field.  Every value is exact in fp32 (powers of two; counters below 2**24)."""
    s = [float(v) for v in state]
    assert len(s) == FIELDS
    dynamic = s[GROWTH_INTERVAL] > 0.0
    if not norm_is_finite:
        if dynamic:
            s[SCALE] = max(s[SCALE] * 0.5, s[MIN])
        s[GOOD_STEPS] = 0.0
        s[SKIPPED_TOTAL] += 1.0
        s[LAST_SKIPPED] = 1.0
    else:
        s[GOOD_STEPS] = min(s[GOOD_STEPS] + 1.0, 2.0 ** 24)       # (where an fp32 counter stops; only a static scale ever gets there)
        s[LAST_SKIPPED] = 0.0
        if dynamic and s[GOOD_STEPS] >= s[GROWTH_INTERVAL]:
            s[SCALE] = min(2.0 * s[SCALE], s[MAX])
            s[GOOD_STEPS] = 0.0
    s[INV_SCALE] = 1.0 / s[SCALE]
    return s


def as_dict(state):
    """{scale, skipped_total, last_step_skipped, good_steps} of a state (the form Engine.loss_scale() returns)."""
    return {"scale": float(state[SCALE]), "skipped_total": int(state[SKIPPED_TOTAL]), "last_step_skipped": bool(state[LAST_SKIPPED]),
            "good_steps": int(state[GOOD_STEPS])}
