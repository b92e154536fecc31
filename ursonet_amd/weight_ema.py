"""An exponential moving average of the weights, kept on the device (Config.WEIGHT_EMA): the configuration rules, the
layout of the device-side state buffer, and `next_state` / `update32`, the written specification of the device kernels behind
urso_ema_update (include/ursonet_ext.h).

  Config.WEIGHT_EMA         None (default: off, the step is launch for launch what it is without this module) | a float in (0, 1), the decay
  Config.WEIGHT_EMA_WARMUP  True (default): the decay of update t + 1 is min(decay, (1 + t) / (10 + t)), TensorFlow's num_updates schedule,
                            so that the average forgets its starting point quickly; False: the configured decay from the first update on

After every optimizer step that was performed (a step skipped by loss scaling is not one):
    ema = ema + (1 - d) * (w - ema)          three float32 operations, each rounded once
over the flat parameter buffer, with d the state's NEXT_DECAY; then the state advances.  The reference has no such average (Keras 2.1).

No GPU and no torch needed here."""
import numpy as np

# fields of the fp32 state buffer (URSO_EMA_* of include/ursonet_ext.h); 4..7 are reserved and zero
DECAY, WARMUP, UPDATES, NEXT_DECAY = range(4)
FIELDS = 8
FIELD_NAMES = ("decay", "warmup", "updates", "next_decay")
MAX_UPDATES = 2.0 ** 24                      # where an fp32 counter stops

_f32 = np.float32


def enabled(config, mode="training"):
    """True when `config` asks for the average and `mode` keeps one: an inference model ignores the key."""
    return mode == "training" and getattr(config, "WEIGHT_EMA", None) is not None


def _schedule(decay, warmup, t):
    """The decay of the update after t performed ones, in float32 arithmetic (one rounding per operation)."""
    decay, t = _f32(decay), _f32(t)
    if not warmup:
        return decay
    return min(decay, (_f32(1.0) + t) / (_f32(10.0) + t))


def initial_state(config, world=1):
    """Validate the WEIGHT_EMA keys of `config` and return the initial state as a list of FIELDS floats, or None when the key is off.
    ValueError: a decay that is no float in (0, 1) (bools included), or a data-parallel run (world > 1)."""
    decay = getattr(config, "WEIGHT_EMA", None)
    if decay is None:
        return None
    if isinstance(decay, (bool, np.bool_, str, bytes)):
        raise ValueError("WEIGHT_EMA must be None or a float in (0, 1), got %r" % (decay,))
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError("WEIGHT_EMA must be None or a float in (0, 1), got %r" % (decay,))
    d32 = float(_f32(d))
    if not (0.0 < d < 1.0) or not (0.0 < d32 < 1.0):        # (also NaN; and a value that float32 rounds to 0 or 1)
        raise ValueError("WEIGHT_EMA must be None or a float in (0, 1) (and stay inside it as a float32), got %r" % (decay,))
    warmup = getattr(config, "WEIGHT_EMA_WARMUP", True)
    if not isinstance(warmup, (bool, np.bool_)):
        raise ValueError("WEIGHT_EMA_WARMUP must be True or False, got %r" % (warmup,))
    if int(world) > 1:
        raise ValueError("WEIGHT_EMA is not supported under data parallelism (world size %d): the swap around validation and the rank-0 "
                         "checkpoint of the average are not built yet; train on one GPU or leave WEIGHT_EMA = None" % int(world))
    return [d32, 1.0 if warmup else 0.0, 0.0, float(_schedule(d32, bool(warmup), 0.0)), 0.0, 0.0, 0.0, 0.0]


def next_state(state, skipped=False):
    """The state after one step: what the one-thread kernel behind urso_ema_update leaves in the buffer, field for field, in numpy.float32
    arithmetic.  skipped = the optimizer did not perform the step (loss scaling's LAST_SKIPPED): nothing moves."""
    s = [float(_f32(v)) for v in state]
    assert len(s) == FIELDS
    if skipped:
        return s
    t = min(_f32(s[UPDATES]) + _f32(1.0), _f32(MAX_UPDATES))
    s[UPDATES] = float(t)
    s[NEXT_DECAY] = float(_schedule(s[DECAY], s[WARMUP] != 0.0, t))
    return s


def update32(ema, w, d):
    """ema + (1 - d) * (w - ema) in float32 with one rounding per operation: bit for bit what urso_ema_update writes.  Returns a new array."""
    ema, w = np.asarray(ema, dtype=np.float32), np.asarray(w, dtype=np.float32)
    c = _f32(1.0) - _f32(d)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (w - ema).astype(np.float32)
        prod = (c * diff).astype(np.float32)
        return (ema + prod).astype(np.float32)


def as_dict(state):
    """{decay, warmup, updates, next_decay} of a state (the form Engine.weight_ema() returns)."""
    return {"decay": float(state[DECAY]), "warmup": bool(state[WARMUP]), "updates": int(state[UPDATES]), "next_decay": float(state[NEXT_DECAY])}
