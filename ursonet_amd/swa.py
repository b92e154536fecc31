"""Stochastic weight averaging and SWAG-diagonal, kept on the device (Config.SWA): the configuration rules, the layout
of the device-side state buffer, and `next_state` / `collect32` / `philox4x32_10` / `normals` / `sample32`, the written specification of
the device kernels behind urso_swa_update and urso_swag_sample (include/ursonet_train.h).

  Config.SWA                None (default: off, the step is launch for launch what it is without this module) | an int c > 0: collect the
                            weights every c performed optimizer steps (the low points of Config.CLR's cycle: c = 2 * CLR_STEP_SIZE)
  Config.SWA_START          0 (default) | an int >= 0: the number of performed optimizer steps before the counting begins
  Config.SWA_VARIANCE       False (default) | True: also keep the mean of w * w (SWAG-diagonal: a Gaussian over the weights to sample from)
  Config.SWA_RECAL_BATCHES  0 (default) | an int k > 0, with SWA and TRAIN_BN = None: train() pools the BN statistics of k training batches
                            under the averaged weights before it writes the averaged file (BN_RECAL_BATCHES stays WEIGHT_EMA's)

After every optimizer step that was performed (a step skipped by loss scaling is not one) the state ticks; where it collects, with n the
new number of models, over the flat parameter buffer in float32, one rounding per operation:
    n == 1:  mean = w (the bits)                   sq = fl(w * w)
    n >  1:  r = fl32(1 / n)
             mean = mean + (w - mean) * r          sq = sq + (fl(w * w) - sq) * r
A weight that never moves keeps mean == w and sq == fl(w * w) bit for bit, so its sampled standard deviation is exactly 0.  The reference
has no such average (Keras 2.1).

No GPU and no torch needed here."""
import math

import numpy as np

KEY = "SWA"
# fields of the int32 state buffer (URSO_SWA_* of include/ursonet_train.h); 6 and 7 are reserved and zero
PERIOD, START, TICKS, MODELS, COLLECTED, VARIANCE = range(6)
FIELDS = 8
FIELD_NAMES = ("period", "start", "ticks", "models", "collected", "variance")
MAX_TICKS = 2 ** 31 - 1                      # where the int32 step counter stops
MAX_MODELS = 2 ** 24                         # the last n that float32 holds exactly: no model is collected past it
REFUSED = -1                                 # COLLECTED after an update whose sq buffer contradicts VARIANCE: nothing else moved

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI = 6.283185307179586                   # the float64 nearest 2 pi

_f32 = np.float32


def enabled(config, mode="training"):
    """True when `config` asks for the average and `mode` keeps one: an inference model ignores the key."""
    return mode == "training" and getattr(config, KEY, None) is not None


def _int(name, value, low, what):
    """`value` as an int >= low that an int32 holds, or ValueError: bools, strings, non-finite and non-integral values are no ints."""
    msg = "%s must be %s, got %r" % (name, what, value)
    if isinstance(value, (bool, np.bool_, str, bytes)) or value is None:
        raise ValueError(msg)
    try:
        f = float(value)
    except (TypeError, ValueError):
        raise ValueError(msg)
    if not math.isfinite(f) or f != math.floor(f) or not (low <= f <= MAX_TICKS):
        raise ValueError(msg)
    return int(f)


def validate(config, world=1):
    """Validate the SWA keys of `config`.  None when Config.SWA is off (the other keys must still be well formed), otherwise
    (period, start, variance, recal_batches).  ValueError: a key of the wrong kind, SWA_RECAL_BATCHES > 0 without SWA or with a frozen BN,
    or SWA in a data-parallel run (world > 1)."""
    period = getattr(config, KEY, None)
    if period is not None:
        period = _int(KEY, period, 1, "None or an int > 0 (collect every that many performed optimizer steps)")
    start = _int("SWA_START", getattr(config, "SWA_START", 0), 0, "an int >= 0 (performed optimizer steps before the counting begins)")
    variance = getattr(config, "SWA_VARIANCE", False)
    if not isinstance(variance, (bool, np.bool_)):
        raise ValueError("SWA_VARIANCE must be True or False, got %r" % (variance,))
    k = _int("SWA_RECAL_BATCHES", getattr(config, "SWA_RECAL_BATCHES", 0), 0, "an int >= 0 (training batches pooled under the averaged weights)")
    if k > 0 and period is None:
        raise ValueError("SWA_RECAL_BATCHES = %d needs SWA: it recalibrates the BN statistics of the averaged weights before train() writes "
                         "swa_weights_*.h5; set SWA or leave SWA_RECAL_BATCHES = 0" % k)
    if k > 0 and getattr(config, "TRAIN_BN", None) is not None:
        raise ValueError("SWA_RECAL_BATCHES = %d needs TRAIN_BN = None (batch-statistics BN): a frozen BN has no batch statistics to pool, "
                         "got TRAIN_BN = %r" % (k, getattr(config, "TRAIN_BN", None)))
    if period is None:
        return None
    if int(world) > 1:
        raise ValueError("SWA is not supported under data parallelism (world size %d): the swap around validation and the rank-0 "
                         "checkpoint of the average are not built yet; train on one GPU or leave SWA = None" % int(world))
    return period, start, bool(variance), k


def initial_state(config, world=1):
    """Validate the SWA keys of `config` and return the initial state as a list of FIELDS ints, or None when the key is off."""
    keys = validate(config, world)
    if keys is None:
        return None
    period, start, variance, _k = keys
    return [period, start, 0, 0, 0, 1 if variance else 0, 0, 0]


def collects(state):
    """(ticks, collect) of the step that the state stands in front of: the gate every thread of urso_swa_update evaluates."""
    period, start, models = int(state[PERIOD]), int(state[START]), int(state[MODELS])
    ticks = min(int(state[TICKS]) + 1, MAX_TICKS)
    return ticks, period > 0 and ticks > start and (ticks - start) % period == 0 and models < MAX_MODELS


def next_state(state, skipped=False):
    """The state after one step: what the one-thread kernel behind urso_swa_update leaves in the buffer, field for field.
    skipped = the optimizer did not perform the step (loss scaling's LAST_SKIPPED): nothing moves, COLLECTED included."""
    s = [int(v) for v in state]
    assert len(s) == FIELDS
    if skipped:
        return s
    ticks, collect = collects(s)
    s[TICKS] = ticks
    s[MODELS] += 1 if collect else 0
    s[COLLECTED] = 1 if collect else 0
    return s


def collect32(mean, sq, w, n):
    """Model number n >= 1 into the running mean (and, where sq is not None, the running mean of squares) in float32 with one rounding per
    operation: bit for bit what urso_swa_update writes.  Returns new arrays (mean, sq); sq is None where it was."""
    n = int(n)
    assert 1 <= n <= MAX_MODELS
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ww = (w * w).astype(np.float32)
        if n == 1:
            return w.copy(), (None if sq is None else ww)
        mean = np.asarray(mean, dtype=np.float32)
        r = _f32(1.0 / n)

        def step(avg, x):
            diff = (x - avg).astype(np.float32)
            prod = (diff * r).astype(np.float32)
            return (avg + prod).astype(np.float32)
        return step(mean, w), (None if sq is None else step(np.asarray(sq, dtype=np.float32), ww))


def as_dict(state):
    """{period, start, ticks, models, collected, variance} of a state (the form Engine.swa() returns)."""
    return {"period": int(state[PERIOD]), "start": int(state[START]), "ticks": int(state[TICKS]), "models": int(state[MODELS]),
            "collected": bool(int(state[COLLECTED]) == 1), "variance": bool(state[VARIANCE])}


# ---------------------------------------------------------------------------------------------------- sampling (SWAG-diagonal)
def philox4x32_10(counter, key):
    """Philox-4x32 with 10 rounds (Salmon et al., SC'11; Random123) in NumPy integers.  counter: [..., 4] and key: [..., 2] words
    (broadcast against each other); returns uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xffffffff)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xffffffff)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    for rnd in range(10):
        if rnd:
            k0 = (k0 + np.uint64(PHILOX_W0)) & mask
            k1 = (k1 + np.uint64(PHILOX_W1)) & mask
        p0 = np.uint64(PHILOX_M0) * c0                 # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def normals64(n, seed, sample, first=0):
    """The float64 normals of elements [first, first + n) of the flat buffer, before their rounding to float32.  Elements 4i .. 4i + 3 use
    the words x0 .. x3 of counter (i & 0xffffffff, i >> 32, sample, 0) under key (seed & 0xffffffff, seed >> 32):
        u = (x + 0.5) * 2^-32  (exact);  (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1);  (z2, z3) likewise from u2, u3.
    The index is the absolute element index, so the values do not depend on how a range is cut."""
    n, first, seed, sample = int(n), int(first), int(seed), int(sample)
    assert n >= 0 and first >= 0 and 0 <= seed < 2 ** 64 and 0 <= sample < 2 ** 31
    b0, b1 = first // 4, (first + n + 3) // 4
    i = np.arange(b0, b1, dtype=np.uint64)
    ctr = np.stack([i & np.uint64(0xffffffff), i >> np.uint64(32), np.full_like(i, sample), np.zeros_like(i)], axis=-1)
    x = philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = TWO_PI * u[:, 1], TWO_PI * u[:, 3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1).reshape(-1)
    return z[first - 4 * b0:first - 4 * b0 + n]


def normals(n, seed, sample, first=0):
    """normals64 rounded to float32: what urso_swag_sample leaves in z_out (within the float64 functions' last bits)."""
    return normals64(n, seed, sample, first).astype(np.float32)


def scale32(var_scale=0.5):
    """s = fl32(sqrt(var_scale)), computed on the host.  var_scale: a finite float >= 0 (0.5 in the SWAG paper).  ValueError otherwise."""
    if isinstance(var_scale, (bool, np.bool_, str, bytes)) or not isinstance(var_scale, (int, float, np.integer, np.floating)):
        raise ValueError("var_scale must be a finite float >= 0, got %r" % (var_scale,))
    v = float(var_scale)
    if not math.isfinite(v) or v < 0.0 or math.sqrt(v) > float(np.finfo(np.float32).max):
        raise ValueError("var_scale must be a finite float >= 0, got %r" % (var_scale,))
    return float(_f32(math.sqrt(v)))


def sample32(mean, sq, z, s):
    """mean + (s * sd) * z with sd = sqrtf(max(sq - fl(mean * mean), 0)) in float32, one rounding per operation: bit for bit what
    urso_swag_sample writes from its own z.  (max: d where d > 0, else 0 -- a NaN difference counts as 0.)"""
    mean, sq, z = (np.asarray(a, dtype=np.float32) for a in (mean, sq, z))
    s = _f32(s)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        mm = (mean * mean).astype(np.float32)
        d = (sq - mm).astype(np.float32)
        sd = np.sqrt(np.where(d > 0, d, _f32(0.0)).astype(np.float32)).astype(np.float32)
        t = (s * sd).astype(np.float32)
        p = (t * z).astype(np.float32)
        return (mean + p).astype(np.float32)
