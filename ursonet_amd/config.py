"""Configuration object of the drop-in: same attribute names, defaults and derived
fields as the reference's `Config` (config.py:13-196), so that pose_estimator.py's
field-by-field mutation (pose_estimator.py:815-872) works unchanged.

Additions (all optional, never required by a reference caller):
  COMPUTE_DTYPE  "float32" (default; "float16" when F16) | "bfloat16" | "float16" --
                 storage type of activations / MFMA inputs on the MI355X; accumulation,
                 master weights, gradients of parameters and the optimizer are fp32.
  DP_EXACT_REL_LOSS  False: per-rank `rel_loss_graph` (what a tower-parallel Keras model
                 would compute); True: the two squared norms are summed over the ranks between
                 forward and backward, i.e. the loss and its gradient are those of the one global batch.
  LOSS_SCALE     None (default) | a power of two | "dynamic": loss scaling for 16-bit training, with LOSS_SCALE_INIT,
                 LOSS_SCALE_GROWTH_INTERVAL, LOSS_SCALE_MIN and LOSS_SCALE_MAX (ursonet_amd/loss_scale.py).
  LEARNABLE_LOSS_WEIGHTS  a reference field that the reference leaves without effect (its formula is commented out, net.py:709-760).
                 True: in training mode each of the loc / ori losses is w (L exp(-s) + s) with s a trainable scalar of the layer
                 `loss_weights` (ori_weight -2.3, loc_weight 0.0), learnt by the same optimizer launch (ursonet_amd/loss_weights.py).
                 One GPU; refused with REGRESS_KEYPOINTS and DP_EXACT_REL_LOSS.
"""
import json
import os

import numpy as np


class Config(object):
    GPU_COUNT = 1
    IMAGES_PER_GPU = 2
    STEPS_PER_EPOCH = 1000
    VALIDATION_STEPS = 50
    BACKBONE = "resnet101"
    BOTTLENECK_WIDTH = 128
    BRANCH_SIZE = 1024
    IMAGE_RESIZE_MODE = "pad64"
    IMAGE_MIN_DIM = 480
    IMAGE_MAX_DIM = 512
    IMAGE_MIN_SCALE = 0
    NR_IMAGE_CHANNELS = 3
    MEAN_PIXEL = np.array([123.7, 116.8, 103.9])
    LEARNING_RATE = 0.001
    LEARNING_MOMENTUM = 0.9
    CLR = False
    MAX_LEARNING_RATE = 0.0005
    BASE_LEARNING_RATE = 0.0001
    CLR_STEP_SIZE = 4000
    REGRESS_ORI = True
    REGRESS_LOC = True
    REGRESS_KEYPOINTS = False
    ROT_AUG = True
    SIM2REAL_AUG = False
    ROT_IMAGE_AUG = False
    ORIENTATION_PARAM = 'quaternion'
    DECOUPLE_ORIENTATION = False
    LOC_BINS_PER_DIM = 16
    ORI_BINS_PER_DIM = 32
    BETA = 6.0
    OPTIMIZER = 'SGD'
    WEIGHT_DECAY = 0.0001
    F16 = False
    LEARNABLE_LOSS_WEIGHTS = False
    LOSS_WEIGHTS = {"loc_loss": 1., "ori_loss": 1., "k2_loss": 1., "k3_loss": 1.}
    TRAIN_BN = False
    GRADIENT_CLIP_NORM = 5.0
    # Not a reference field: True = uint8 RGB frames of one size are rescaled and padded on the GPU (augment.resize_images, byte-exact to
    # utils.resize_image) by the feeders, detect() and evaluate(); False = the host path (utils.resize_image), call for call as before.
    DEVICE_RESIZE = False
    # Not a reference field: > 0 = budget in GiB of a device-resident cache of RAW frames (ursonet_amd/frame_cache.py).  Every frame that
    # takes the DEVICE_RESIZE path is decoded and uploaded once and served from HBM from the second epoch on; needs DEVICE_RESIZE = True
    # (ValueError otherwise) and a dataset whose load_image(i) always returns the same frame.  The budget is spent in whole slabs of 1 GiB,
    # each holding either grey frames (one plane) or RGB frames: give a dataset that has both at least 2.  The budget is PER FEEDER:
    # UrsoNet.train owns a training and a validation feeder, so up to 2 x DEVICE_CACHE_GB of HBM per rank.  0 = off: nothing changes.
    DEVICE_CACHE_GB = 0
    # Not reference fields: loss scaling for 16-bit training (ursonet_amd/loss_scale.py).  None = off (nothing changes);
    # a positive power of two = a static scale; "dynamic" = start at LOSS_SCALE_INIT, halve on an overflowed (skipped) step down to
    # LOSS_SCALE_MIN, double after LOSS_SCALE_GROWTH_INTERVAL finite steps in a row up to LOSS_SCALE_MAX.  One GPU only.
    LOSS_SCALE = None
    LOSS_SCALE_INIT = 2.0 ** 15
    LOSS_SCALE_GROWTH_INTERVAL = 2000
    LOSS_SCALE_MIN = 1.0
    LOSS_SCALE_MAX = 2.0 ** 24
    # Not reference fields: an exponential moving average of the weights kept on the device (ursonet_amd/weight_ema.py).
    WEIGHT_EMA = None             # None = off (nothing changes) | the decay, a float in (0, 1): train() also validates and saves the average.  One GPU only.
    WEIGHT_EMA_WARMUP = True      # the decay of update t + 1 is min(WEIGHT_EMA, (1 + t) / (10 + t)); False = WEIGHT_EMA from the first update on
    # Not a reference field: gradient accumulation on the device (ursonet_amd/grad_accum.py).
    GRAD_ACCUM_STEPS = 1          # 1 = off (nothing changes) | an int k >= 2: one optimizer step consumes k micro-batches of IMAGES_PER_GPU images.  One GPU only.
    # Not reference fields: layer-wise adaptive rate scaling for SGD on the device (ursonet_amd/lars.py).
    LARS = None                   # None = off (nothing changes) | the trust coefficient, a float > 0 (usually 0.001): every conv / Dense kernel steps at lr * LARS * |w| / (c |g| + LARS_EPS).  SGD and one GPU only.
    LARS_EPS = 1e-8               # a float >= 0, added to the denominator of the trust ratio
    LARS_CLIP = False             # True = LARC's "clip" mode: a tensor's effective rate never exceeds the global one (trust = min(ratio / lr, 1))
    # Not reference fields: LAMB, layer-wise trust ratios for Adam on the device (ursonet_amd/lamb.py).
    LAMB = None                   # None = off (nothing changes) | the trust coefficient, a float > 0 (usually 1.0): every conv / Dense kernel steps at lr * LAMB * |w| / (|r| + LAMB_EPS), r the Adam direction.  Adam and one GPU only; not together with LARS.
    LAMB_EPS = 1e-8               # a finite float >= 0, added to the denominator of the trust ratio
    LAMB_CLIP = False             # True = a tensor's rate never exceeds plain Adam's (trust = min(ratio, 1))
    # Not reference fields: SAM, sharpness-aware minimization on the device (ursonet_amd/sam.py).
    SAM = None                    # None = off (nothing changes) | rho, a finite float > 0 (usually 0.05): the optimizer steps with the gradient taken at w + rho g / |g|; every step runs its forward and backward pass twice.  One GPU only.
    SAM_EPS = 1e-12               # a finite float >= 0, added to the norm in the denominator
    # Not a reference field: BN statistics of their own for the averaged checkpoints (ursonet_amd/bn_recal.py).  The same
    # module's recalibrate_bn(model, dataset) re-estimates the statistics of any TRAIN_BN = None model on unlabelled frames and needs no key.
    BN_RECAL_BATCHES = 0          # 0 = off (nothing changes) | an int k > 0: before train() writes ema_weights_*.h5 it pools the BN statistics of k training batches under the averaged weights into that file; the raw statistics come back bit for bit.  Needs WEIGHT_EMA and TRAIN_BN = None.  One GPU only.
    # Not reference fields: stochastic weight averaging and SWAG-diagonal on the device (ursonet_amd/swa.py).
    SWA = None                    # None = off (nothing changes) | an int c > 0: every c performed optimizer steps the weights go into an equal-weight running mean (with CLR: c = 2 * CLR_STEP_SIZE, the low points of the cycle); train() also validates and saves the average.  One GPU only.
    SWA_START = 0                 # an int >= 0: the number of performed optimizer steps before the counting begins
    SWA_VARIANCE = False          # True = also keep the running mean of w * w (SWAG-diagonal): swag_weights() samples weight sets from N(mean, var_scale * diag(sq - mean^2))
    SWA_RECAL_BATCHES = 0         # 0 = off | an int k > 0: before train() writes swa_weights_*.h5 it pools the BN statistics of k training batches under the averaged weights into that file; the raw statistics come back bit for bit.  Needs SWA and TRAIN_BN = None.

    def update(self):
        """Derived fields (config.py:151-166)."""
        self.BATCH_SIZE = self.IMAGES_PER_GPU * self.GPU_COUNT
        if self.IMAGE_RESIZE_MODE == "crop":
            self.IMAGE_SHAPE = np.array([self.IMAGE_MIN_DIM, self.IMAGE_MIN_DIM, self.NR_IMAGE_CHANNELS])
        elif self.IMAGE_RESIZE_MODE == "pad64":
            self.IMAGE_SHAPE = np.array([self.IMAGE_MIN_DIM, self.IMAGE_MAX_DIM, self.NR_IMAGE_CHANNELS])
        else:
            self.IMAGE_SHAPE = np.array([self.IMAGE_MAX_DIM, self.IMAGE_MAX_DIM, self.NR_IMAGE_CHANNELS])
        self.IMAGE_META_SIZE = 1 + self.NR_IMAGE_CHANNELS + 3 + 4 + 1

    def __init__(self):
        self.LOSS_WEIGHTS = dict(type(self).LOSS_WEIGHTS)
        self.update()

    def display(self):
        print("\nConfigurations:")
        for a in dir(self):
            if not a.startswith("__") and not callable(getattr(self, a)):
                print("{:30} {}".format(a, getattr(self, a)))
        print("\n")

    def write_to_file(self, filepath):
        """JSON dump of every non-array attribute (config.py:180-196)."""
        d = {}
        for a in dir(self):
            v = getattr(self, a)
            if not a.startswith("__") and not callable(v) and not isinstance(v, np.ndarray):
                d[a] = v
        directory = os.path.dirname(filepath)
        if directory and not os.path.isdir(directory):
            os.makedirs(directory)
        with open(filepath, 'w+') as f:
            f.write(json.dumps(d))


def compute_dtype_name(config):
    """Resolve the activation storage dtype: explicit COMPUTE_DTYPE wins, else F16 (net.py:590-593)."""
    name = getattr(config, "COMPUTE_DTYPE", None)
    if name is None:
        name = "float16" if getattr(config, "F16", False) else "float32"
    if name not in ("float32", "bfloat16", "float16"):
        raise ValueError("COMPUTE_DTYPE must be float32, bfloat16 or float16, got %r" % (name,))
    return name
