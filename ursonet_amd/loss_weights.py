"""Learnable loss weights (Config.LEARNABLE_LOSS_WEIGHTS): the configuration rules, the parameter layer that holds the
two trainable log-variances, and which of them belongs to which loss.

The reference creates `ori_weight` (-2.3) and `loc_weight` (0.0) and appends them to the trainable weights (net.py:648-654, 685-686), but its
formula `loss / exp(weight) + weight` is commented out in every loss (net.py:709-760).  Here, in training mode, each of the two losses is
    reported = w (L exp(-s) + s)        w = LOSS_WEIGHTS[name], L = the batch-mean loss without w
with s an ordinary trainable fp32 scalar of the flat parameter buffer (include/ursonet_ext.h: the urso_*_lw entry points).

No GPU and no torch needed here."""
from collections import OrderedDict

LAYER = "loss_weights"
KIND = "loss_weights"
# weight name -> (initial value (net.py:649-650), the loss it belongs to, its slot in Engine.loss_buf)
WEIGHTS = OrderedDict((("ori_weight", (-2.3, "ori_loss", 1)), ("loc_weight", (0.0, "loc_loss", 0))))
WEIGHT_OF_LOSS = {loss: wn for wn, (_, loss, _) in WEIGHTS.items()}


def enabled(config, mode="training"):
    """True when `config` asks for the feature and `mode` has it: an inference model has no such layer."""
    return mode == "training" and bool(getattr(config, "LEARNABLE_LOSS_WEIGHTS", False))


def validate(config, world=1):
    """ValueError for what the feature does not cover: keypoint regression (three MSE losses, no loc / ori pair), the two-phase exact
    rel_loss of data parallelism, and a data-parallel run (world > 1).  Nothing to check when the key is off."""
    if not bool(getattr(config, "LEARNABLE_LOSS_WEIGHTS", False)):
        return
    if getattr(config, "REGRESS_KEYPOINTS", False):
        raise ValueError("LEARNABLE_LOSS_WEIGHTS is not supported with REGRESS_KEYPOINTS (the keypoint losses have no loc / ori weight pair)")
    if getattr(config, "DP_EXACT_REL_LOSS", False):
        raise ValueError("LEARNABLE_LOSS_WEIGHTS is not supported with DP_EXACT_REL_LOSS (the two-phase rel_loss has no learnable-weight form)")
    if int(world) > 1:
        raise ValueError("LEARNABLE_LOSS_WEIGHTS is not supported under data parallelism (world size %d): the two scalars' gradients are not "
                         "part of the gradient exchange yet; train on one GPU or leave LEARNABLE_LOSS_WEIGHTS = False" % int(world))


def add_layer(graph):
    """Append the parameter layer to a Graph (ursonet_amd/graph.py): its weights join the flat buffers like any other layer's."""
    graph.params[LAYER] = OrderedDict((wn, (1,)) for wn in WEIGHTS)
    graph.kinds[LAYER] = KIND
    return graph


def initial_values():
    """{weight name: float32 array of shape (1,)} at the reference's initial values."""
    import numpy as np
    return OrderedDict((wn, np.full((1,), init, dtype=np.float32)) for wn, (init, _, _) in WEIGHTS.items())
