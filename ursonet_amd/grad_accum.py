"""Gradient accumulation over micro-batches, on the device (Config.GRAD_ACCUM_STEPS): the configuration rules, the
launch role of every micro-step, and `first32` / `add32` / `close32`, the written specification of the device kernels behind
urso_grad_accum and urso_grad_accum_close (include/ursonet_ext.h).

  Config.GRAD_ACCUM_STEPS   1 (default: off, the step is launch for launch what it is without this module) | an int k >= 2: one optimizer
                            step consumes k micro-batches of IMAGES_PER_GPU images

With g_j what the backward pass of micro-batch j leaves in the flat gradient buffer (finalised: weight decay, BN gamma / beta and the two
loss-weight slots included, and already unscaled under LOSS_SCALE):
    j = 1:        acc = g_1                       the bits
    1 < j < k:    acc = acc + g_j                 one float32 add, rounded once
    j = k:        g   = (acc + g_k) * c           one add and one multiply, each rounded once; c = inv32(k) = fl32(1 / k)
and the unchanged optimizer launches follow on g, the mean gradient.  Multiplying by c is exact for a power of two; otherwise c is 1 / k
rounded once, so the product is off from the quotient (acc + g_k) / k by at most that one more rounding (relative 2^-24) -- stated here as
the stagnation of the weights' average is stated in weight_ema.py: the price of one multiply per element instead of a division.  The
reference has no accumulation (Keras 2.1).

No GPU and no torch needed here."""
import numpy as np

KEY = "GRAD_ACCUM_STEPS"
ROLES = ("first", "add", "close")

_f32 = np.float32


def validate(config, world=1):
    """Validate Config.GRAD_ACCUM_STEPS and return k (1 = off; a config without the key is off).
    ValueError: a bool, a non-int (2.0 and "2" included), k < 1, or k > 1 in a data-parallel run (world > 1)."""
    k = getattr(config, KEY, 1)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError("%s must be an int >= 1, got %r" % (KEY, k))
    k = int(k)
    if k < 1:
        raise ValueError("%s must be an int >= 1, got %r" % (KEY, k))
    if k > 1 and int(world) > 1:
        raise ValueError("%s = %d is not supported under data parallelism (world size %d): the gradient exchange would have to move into the "
                         "closing micro-step, which is not built yet; train on one GPU or leave %s = 1" % (KEY, k, int(world), KEY))
    return k


def enabled(config, mode="training"):
    """True when `config` asks for accumulation and `mode` trains: an inference model ignores the key."""
    return mode == "training" and validate(config) > 1


def roles(k):
    """The launch role of micro-step i = 0 .. k - 1 of an optimizer step: ["first", "add", ..., "close"]; k = 1 has no roles."""
    k = int(k)
    if k < 2:
        return []
    return ["first"] + ["add"] * (k - 2) + ["close"]


def inv32(k):
    """c = fl32(1 / k) as the engine passes it to urso_grad_accum_close: one float32 division."""
    return _f32(1.0) / _f32(k)


def first32(g):
    """acc after the first micro-step: the bits of g.  Returns a new array."""
    return np.array(g, dtype=np.float32, copy=True)


def add32(acc, g):
    """acc + g in float32, rounded once: bit for bit what urso_grad_accum(first = 0) writes.  Returns a new array."""
    acc, g = np.asarray(acc, dtype=np.float32), np.asarray(g, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc + g).astype(np.float32)


def close32(acc, g, c):
    """(acc + g) * c in float32, each operation rounded once: bit for bit what urso_grad_accum_close writes.  Returns a new array."""
    acc, g = np.asarray(acc, dtype=np.float32), np.asarray(g, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = (acc + g).astype(np.float32)
        return (s * _f32(c)).astype(np.float32)


def accumulate32(gs):
    """The whole recurrence over the gradients gs = [g_1, ..., g_k], k >= 2: what flat_g holds in front of the optimizer."""
    k = len(gs)
    assert k >= 2
    acc = first32(gs[0])
    for g in gs[1:-1]:
        acc = add32(acc, g)
    return close32(acc, gs[-1], inv32(k))


def fold_history(rows, k):
    """rows: [steps * k, n] per-micro-batch values in order -> [steps, n], the mean of each optimizer step's k rows (float64 mean, returned
    in the dtype of `rows`).  k = 1 returns the rows unchanged."""
    rows = np.asarray(rows)
    k = int(k)
    if k == 1:
        return rows
    if rows.ndim != 2 or rows.shape[0] % k:
        raise ValueError("fold_history: %r rows do not fold by %d" % (rows.shape, k))
    return rows.reshape(rows.shape[0] // k, k, rows.shape[1]).astype(np.float64).mean(axis=1).astype(rows.dtype)
