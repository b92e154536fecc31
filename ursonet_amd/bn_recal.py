"""Re-estimate the BatchNorm population statistics on the device (recalibrate_bn, Config.BN_RECAL_BATCHES; AdaBN,
Li et al. 2016; `update_bn` in other stacks): the configuration rules, `pool_add64` / `pool_settle32` / `whole_batches`, the written
specification of the device kernels behind urso_bn_recal_add and urso_bn_recal_settle (include/ursonet_train.h), and the public call.

With TRAIN_BN = None the moving mean and variance matter only at inference, where they are folded into the filters; training trails them
behind the raw weights with Keras' momentum 0.99.  recalibrate_bn replaces them by the statistics of the model AS IT IS on the frames it
is shown -- unlabelled frames of the target domain, or training frames under the averaged weights (Config.WEIGHT_EMA) -- and keeps every
weight.

  Config.BN_RECAL_BATCHES   0 (default: off, nothing changes) | an int k > 0, with WEIGHT_EMA and TRAIN_BN = None: before train() writes an
                            ema_weights_*.h5 it takes k batches from the training feeder, recalibrates under the averaged weights, writes
                            the file with those statistics and puts the raw ones back bit for bit.  One GPU only.

The rule is the pooled population statistic over all pixels of all batches seen, by the law of total variance: not a moving average, and not
the mean of the batch variances, which loses the spread of the batch means.  Per BN channel two float64 accumulators, mean and m2; one more
batch has float32 statistics mu_b, v_b (biased variance) over M pixels; n = t * M pixels have been pooled before it, t the number of batches
already added.  Every float64 operation is rounded once, in this order:

    n1    = n + M
    d     = mu_b - mean
    mean' = mean + (d * M) / n1
    m2'   = m2 + (v_b * M + (d * d) * ((n * M) / n1))
    settle:  moving_mean = (float) mean      moving_variance = (float) (m2 / n)          n = t * M, t >= 1

From the zero state one batch gives its own statistics back bit for bit (M < 2^22: the products with M are exact; a mean of -0.0 comes
back as +0.0).  A batch statistic that is not finite makes that channel's result not finite and touches no other channel.  Only whole
batches are pooled: a padded tail batch would weight its repeated image twice, so a tail of fewer than B images is dropped and reported.

Only TRAIN_BN = None is covered: a frozen-BN training engine and an inference engine fold the statistics into the filters and never
materialise the tensor whose statistics these are.

No GPU and no torch needed for the specification; recalibrate_bn imports them when it is called."""
from collections import OrderedDict

import numpy as np

KEY = "BN_RECAL_BATCHES"
MAX_PIXELS = 2 ** 53                           # t * M stays an exact float64

_f64 = np.float64

HOWTO = ("build UrsoNet('training', cfg) with cfg.TRAIN_BN = None, load_weights(...), recalibrate_bn(model, dataset), save_weights(...)")


def validate(config, world=1):
    """Validate Config.BN_RECAL_BATCHES and return it as an int (0 = off; a config without the key is off).
    ValueError: not a non-negative int (bools included); > 0 without WEIGHT_EMA, with a frozen BN (TRAIN_BN other than None) or in a
    data-parallel run (world > 1)."""
    k = getattr(config, KEY, 0)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 0:
        raise ValueError("%s must be an int >= 0 (0 = off), got %r" % (KEY, k))
    k = int(k)
    if k == 0:
        return 0
    if getattr(config, "WEIGHT_EMA", None) is None:
        raise ValueError("%s = %d needs WEIGHT_EMA: it recalibrates the BN statistics of the averaged weights before train() writes "
                         "ema_weights_*.h5; set WEIGHT_EMA or leave %s = 0" % (KEY, k, KEY))
    if getattr(config, "TRAIN_BN", False) is not None:
        raise ValueError("%s = %d needs batch-statistics BatchNorm (TRAIN_BN = None), got TRAIN_BN = %r: a frozen BN layer is folded into its "
                         "filter and leaves no batch statistics to pool" % (KEY, k, getattr(config, "TRAIN_BN", False)))
    if int(world) > 1:
        raise ValueError("%s is not supported under data parallelism (world size %d): each rank would pool its own shard; train on one GPU "
                         "or leave %s = 0" % (KEY, int(world), KEY))
    return k


def enabled(config, mode="training"):
    """True when `config` asks train() for the recalibration and `mode` trains: an inference model ignores the key."""
    return mode == "training" and validate(config) > 0


# ------------------------------------------------------------------ the specification
def pool_zero(n):
    """The zero state of n channels: (mean, m2), float64."""
    return np.zeros(n, dtype=_f64), np.zeros(n, dtype=_f64)


def _check_count(M, t, least):
    if isinstance(M, (bool, np.bool_)) or int(M) != M or int(M) <= 0:
        raise ValueError("M must be an int > 0, got %r" % (M,))
    if isinstance(t, (bool, np.bool_)) or int(t) != t or int(t) < least:
        raise ValueError("t must be an int >= %d, got %r" % (least, t))
    return int(M), int(t)


def pool_add64(acc, mu_b, v_b, M, t):
    """acc = (mean, m2) after one more batch with float32 statistics mu_b, v_b over M pixels, t batches having been added before: new
    float64 arrays, bit for bit what urso_bn_recal_add leaves in the accumulator."""
    M, t = _check_count(M, t, 0)
    if (t + 1) * M > MAX_PIXELS:
        raise ValueError("(t + 1) * M = %d exceeds 2^53" % ((t + 1) * M))
    mean, m2 = (np.asarray(a, dtype=_f64) for a in acc)
    mu = np.asarray(mu_b, dtype=np.float32).astype(_f64)
    v = np.asarray(v_b, dtype=np.float32).astype(_f64)
    n, Md = _f64(t * M), _f64(M)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        n1 = n + Md
        d = mu - mean
        mean1 = mean + (d * Md) / n1
        m21 = m2 + (v * Md + (d * d) * ((n * Md) / n1))
    return mean1, m21


def pool_settle32(acc, M, t):
    """(moving_mean, moving_variance) float32 from acc = (mean, m2) after t >= 1 batches of M pixels: what urso_bn_recal_settle writes."""
    M, t = _check_count(M, t, 1)
    if t * M > MAX_PIXELS:
        raise ValueError("t * M = %d exceeds 2^53" % (t * M))
    mean, m2 = (np.asarray(a, dtype=_f64) for a in acc)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return mean.astype(np.float32), (m2 / _f64(t * M)).astype(np.float32)


def whole_batches(ids, B):
    """(the ids of the whole batches of B, in order; the number of trailing ids dropped).  Never padded."""
    if isinstance(B, (bool, np.bool_)) or int(B) != B or int(B) <= 0:
        raise ValueError("the batch size must be an int > 0, got %r" % (B,))
    ids = list(ids)
    used = len(ids) // int(B) * int(B)
    return ids[:used], len(ids) - used


def shift_report(slices, before, after, eps):
    """{layer: (max |mean_new - mean_old| / sqrt(var_old + eps), max var_new / var_old)} from the statistics buffer before and after;
    slices: {(layer, "moving_mean" | "moving_variance"): (offset, numel, shape)} as Engine.stat_slices."""
    out = OrderedDict()
    b, a = np.asarray(before, dtype=_f64), np.asarray(after, dtype=_f64)
    for (ln, wn), (o, n, _shape) in slices.items():
        if wn != "moving_mean":
            continue
        vo, vn, _ = slices[(ln, "moving_variance")]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            dm = np.abs(a[o:o + n] - b[o:o + n]) / np.sqrt(b[vo:vo + vn] + _f64(eps))
            ratio = a[vo:vo + vn] / b[vo:vo + vn]
        out[ln] = (float(np.max(dm)), float(np.max(ratio)))
    return out


class BNRecalResult(object):
    """What recalibrate_bn did: images_used, images_dropped (the tail of fewer than a batch), batches, and per BN layer
    layers[name] = (max over channels of |mean_new - mean_old| / sqrt(var_old + eps), max over channels of var_new / var_old), computed on
    the host from the statistics before and after."""

    def __init__(self, images_used, images_dropped, batches, layers):
        self.images_used, self.images_dropped, self.batches = int(images_used), int(images_dropped), int(batches)
        self.layers = OrderedDict(layers)

    def lines(self):
        """A short summary, one string per line."""
        out = ["BN recalibration: %d images in %d batches%s, %d BN layers" % (
            self.images_used, self.batches, " (%d dropped: less than a batch)" % self.images_dropped if self.images_dropped else "",
            len(self.layers))]
        if self.layers:
            ln_m = max(self.layers, key=lambda k: self.layers[k][0])
            ln_v = max(self.layers, key=lambda k: self.layers[k][1])
            shifts = np.array([v[0] for v in self.layers.values()])
            out.append("  mean shift / sigma_old   median %.3e  max %.3e (%s)" % (float(np.median(shifts)), self.layers[ln_m][0], ln_m))
            out.append("  var_new / var_old        max %.3e (%s)" % (self.layers[ln_v][1], ln_v))
        return out


def check_model(model):
    """ValueError unless `model` is a training-mode model on one GPU whose engine runs batch-statistics BatchNorm."""
    eng = getattr(model, "_engine", None)
    if getattr(model, "mode", None) != "training" or eng is None or not getattr(eng, "train_bn", False):
        raise ValueError("recalibrate_bn needs a training-mode model with batch-statistics BatchNorm (TRAIN_BN = None): only that plan "
                         "leaves every BN layer's batch mean and variance on the device -- " + HOWTO)
    from .dp import launcher_world
    world = max(int(getattr(model, "_world", 1)), int(launcher_world()[2]))
    if world > 1 or getattr(model, "_dp", None) is not None:
        raise ValueError("recalibrate_bn is not supported under a data-parallel launcher (world size %d): each rank would pool its own "
                         "frames; run it in a plain process" % world)
    return eng


def recalibrate_bn(model, dataset, nr_images=None, workers=None, cache=None, ema=False):
    """Replace every BN layer's moving mean and variance by the pooled statistics of the model as it is over `dataset.image_ids` (the
    first nr_images of them), in whole batches of the engine's size -> BNRecalResult.  The dataset needs image_ids, load_image and
    image_info; no label loader is called.  Nothing but the statistics changes: no weight, no optimizer state.  ema=True
    (Config.WEIGHT_EMA): the pass runs under the averaged weights, whose statistics these then are.  cache: as in predict().
    ValueError: a model that is not a training-mode one with TRAIN_BN = None; a data-parallel launcher; less than one whole batch;
    ema=True without WEIGHT_EMA.  If a settled statistic is not finite, or anything raises in mid-pass, the statistics from before the
    call are back bit for bit and the error is raised."""
    eng = check_model(model)
    if ema and getattr(eng, "flat_ema", None) is None:
        raise ValueError("recalibrate_bn(ema=True) needs Config.WEIGHT_EMA")
    ids = list(dataset.image_ids)
    if nr_images is not None:
        if isinstance(nr_images, (bool, np.bool_)) or int(nr_images) != nr_images or int(nr_images) < 0:
            raise ValueError("nr_images must be None or an int >= 0, got %r" % (nr_images,))
        ids = ids[:int(nr_images)]
    used, dropped = whole_batches(ids, eng.B)
    if not used:
        raise ValueError("recalibrate_bn needs at least one whole batch of %d images, got %d: a padded batch would count its repeated "
                         "image twice" % (eng.B, len(ids)))
    import torch
    from .feeder import EvalFeeder
    from .graph import BN_EPS
    from .infer import Subset, loader_workers
    cfg = model.config
    before = eng.flat_stats.detach().cpu().numpy().copy()

    def run():
        feed = EvalFeeder(model, Subset(dataset, used), cfg, workers=loader_workers(cfg, workers), labels=False, cache=cache)
        eng.bn_recal_begin()
        try:
            for bt in feed:
                assert bt.n == eng.B
                if bt.images.dtype == torch.uint8:             # by dtype, as infer.PosePass.run uploads
                    eng.load_batch_u8(bt.images)
                else:
                    eng.set_input_u8(False)
                    eng.load_batch(bt.images)
                eng.bn_recal_add()
            eng.bn_recal_end()
            after = eng.flat_stats.detach().cpu().numpy().copy()
            bad = [ln for (ln, wn), (o, n, _s) in eng.stat_slices.items() if not np.all(np.isfinite(after[o:o + n]))]
            if bad:
                raise FloatingPointError("recalibrate_bn: statistics that are not finite in %d BN layers (first: %s); the statistics "
                                         "from before the call are back" % (len(set(bad)), bad[0]))
            return after
        except BaseException:
            eng.bn_recal_abort()
            raise
        finally:
            feed.close()

    if ema:
        with model.ema_weights():
            after = run()
    else:
        after = run()
    return BNRecalResult(len(used), dropped, len(used) // eng.B, shift_report(eng.stat_slices, before, after, BN_EPS))
