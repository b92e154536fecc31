"""Static execution plan of the UrsoNet hot path on one MI355X.

The reference runs its graph through Keras/TensorFlow sessions (net.py:1152-1163 fit_generator,
net.py:1251 predict).  Here the graph (ursonet_amd/graph.py) is lowered ONCE into a flat list of
C-ABI kernel launches over pre-allocated HBM buffers -- weight prep (BN folding), forward, fused
loss+gradient, backward (dgrad/wgrad), parameter-gradient finalisation, global-norm clip + momentum
SGD -- and the whole step is captured into a hipGraph and replayed (no per-step Python, no
allocator, no host sync).  PyTorch is used only for device memory, streams and graph capture.

Data layout in HBM: activations NHWC in the compute dtype; all trainable parameters live in ONE
flat fp32 buffer (Keras layouts, forward layer order) with matching flat gradient / momentum
buffers, so that the data-parallel all-reduce works on contiguous slices (ursonet_amd/dp.py)
and the optimizer is two launches.
"""
import math
import os
import re
from collections import OrderedDict

import numpy as np
import torch

from . import bn_recal, grad_accum, hip, lamb, lars, loss_scale, loss_weights, sam, swa, weight_ema
from .config import compute_dtype_name
from .graph import BN_EPS, build_graph, conv_flops
from .plan_state import _Act, _Conv, _Launch, _PendingLaunches, _round_up
from .train_state import weights_location

BN_MOMENTUM = 0.99          # Keras BatchNormalization default (net.py:60-76 passes none)

_DT = {"float32": hip.F32, "bfloat16": hip.BF16, "float16": hip.F16}


_SIDE_STREAMS = {}


def _side_stream(device):
    """One second stream per device for the process, shared by every Engine: engines come and go (tests build dozens), and a replay of a forked
    graph segfaulted inside hipGraphLaunch (ROCm 7.2) in a process where earlier engines' side streams had been destroyed with them."""
    key = torch.device(device).index or 0
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


class _no_gc(object):
    """Collect garbage now and keep the cyclic collector off inside the block.  An Engine is full of reference cycles (its op lists are
    closures over itself), so an engine that went out of scope dies whenever the collector happens to run -- and if that is in the
    middle of another engine's stream capture, destroying the old engine's hipGraph / events there aborts the process."""

    def __enter__(self):
        import gc
        gc.collect()
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
        return False


def _checked_params(graph, params, strict, only=None):
    """(layer, weight, host float32 tensor) of every tensor of `graph` that params {layer: {weight: array}} holds, in the graph's order,
    as the loaders copy them.  A missing layer is a KeyError if strict and skipped otherwise; a wrong shape is a ValueError.  only: a
    container of (layer, weight) outside which tensors are passed over unread (Engine.slices: the trainable ones)."""
    for ln, ws in graph.params.items():
        if ln not in params:
            if strict:
                raise KeyError("missing layer %r" % ln)
            continue
        for wn, shape in ws.items():
            if only is not None and (ln, wn) not in only:
                continue
            a = np.asarray(params[ln][wn], dtype=np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("layer %s weight %s: shape %s != expected %s" % (ln, wn, a.shape, shape))
            yield ln, wn, torch.from_numpy(np.ascontiguousarray(a))


class _StandIn(object):
    """Context manager of Engine.ema_weights() / swa_weights() / swag_weights(): `enter` puts another set of weights into flat_w, `leave`
    brings the raw ones back -- also after an exception inside the block, which goes on to the caller.  Yields the engine."""

    def __init__(self, eng, enter, leave):
        self.eng, self.enter, self.leave = eng, enter, leave

    def __enter__(self):
        self.enter()
        return self.eng

    def __exit__(self, *exc):
        self.leave()
        return False


class Engine(object):
    def __init__(self, config, mode, batch=None, seed=1234, device=None, randomize_bn=False, grad_bucket_bytes=1 << 40):
        assert mode in ("training", "inference")
        # gradient buckets: one batched reduction / finalisation per bucket.  One GPU: ONE bucket (round 5: the 128 MiB default cut ResNet-50's
        # 128.0 MiB of gradients into a big bucket and a two-layer tail: three more launches, 25 us; 32 MiB: 13 launches and 0.52 ms, 8 MiB: 41 and
        # 0.68 ms); ursonet_amd/dp.py re-plans with 32 MiB buckets, which the all-reduces overlap behind
        self.grad_bucket_bytes = int(grad_bucket_bytes)
        self.grad_tail_bytes = 0                       # > 0: the last bucket (stem side) is capped at this size; set by ursonet_amd/dp.py (plan_buckets)
        self.no_fused_sqnorm = self.no_wgrad_fork = False     # set by ursonet_amd/dp.py
        if not torch.cuda.is_available():
            raise RuntimeError("ursonet_amd.Engine needs an AMD GPU (MI355X / gfx950); there is no CPU fallback")
        self.config, self.mode = config, mode
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.dt_name = compute_dtype_name(config)
        self.dt = _DT[self.dt_name]
        self.tdt = hip.TORCH_DT[self.dt]
        self.B = int(batch if batch is not None else config.BATCH_SIZE)
        self.graph = build_graph(config)
        # Config.LEARNABLE_LOSS_WEIGHTS: the two log-variances are one more parameter layer of the training graph, so
        # they lie in flat_w / flat_g / the optimizer state and everything that walks graph.params or the flat buffers covers them
        self.learn_lw = loss_weights.enabled(config, mode)
        if self.learn_lw:
            loss_weights.validate(config, self.world_size_hint())
            loss_weights.add_layer(self.graph)
        self.H, self.W = int(config.IMAGE_SHAPE[0]), int(config.IMAGE_SHAPE[1])
        self.layer_trainable = {n: True for n in self.graph.params}
        self.world_size = 1
        self._graphs = None
        # state that outlives a re-plan (set_trainable, ursonet_amd/dp.py); halo_ws: its first 4 KiB of flags must stay zero
        self.plan_version, self.halo_ws, self.rel_scale = 0, None, None
        # the persistent training state: train_state() lists it, _plan_device_state() creates the small states once,
        # _stand_in says which set of weights lies in flat_w.  None / 1 / [] = the feature is off and none of it exists
        self.hyper = self.flat_v2 = self.flat_vhat = None
        self._state_init = {}                          # attribute of a small device state -> the initial values it last started from
        self._stand_in = None                          # None | "ema" | "swa" | "swag": what stands in flat_w for the raw weights right now
        self.ls_state = None                           # Config.LOSS_SCALE
        self.flat_ema = self.ema_state = None          # Config.WEIGHT_EMA (section 17)
        self.flat_acc, self.accum_k, self.accum_micro, self.accum_ops, self._accum_roles = None, 1, 0, [], []      # GRAD_ACCUM_STEPS (section 18)
        self.lars_plan = None                          # Config.LARS (section 19): hip.LarsPlan, rebuilt with every plan
        self.lamb_plan, self.lamb_state = None, None   # Config.LAMB (section 20): hip.LambPlan likewise, and its state {p1, p2, kt}
        self.sam_state, self._sam_keys, self.flat_w0, self.sam_loss, self.sam_stats, self.sam_ops = None, None, None, None, None, []   # Config.SAM (section 21)
        self._recal_plan = self._recal_stats = None    # BN_RECAL_BATCHES (section 22): (plan_version, hip.BnRecalPlan), the clone of flat_stats
        self.flat_swa = self.flat_swa_sq = self.swa_state = self._swag_hold = None     # Config.SWA (section 23); _swag_hold: the raw weights under a sample
        if mode == "training":                         # a bad key is a ValueError before anything is allocated: the first one in this order
            if weight_ema.enabled(config, mode):
                weight_ema.initial_state(config, self.world_size_hint())
            for feature in (swa, grad_accum, lars, lamb, sam, bn_recal):
                feature.validate(config, self.world_size_hint())
        self.input_u8, self.in_images_u8, self.adam = False, None, False
        self.wgrad_stream, self._single_chain, self._single_chain_always, self.fork_checks = None, False, False, 0
        self._alloc_params(seed, randomize_bn)
        self._build_plan()

    @staticmethod
    def world_size_hint():
        """The launcher's world size (1 in a plain process): ursonet_amd/dp.py wraps the engine only after it is built."""
        from .dp import launcher_world
        return launcher_world()[2]

    # ------------------------------------------------------------------ parameters
    def _alloc_params(self, seed, randomize_bn):
        g = self.graph
        off, soff = 0, 0
        self.slices = OrderedDict()        # (layer, weight) -> (offset, numel, shape) in the flat trainable buffer
        self.stat_slices = OrderedDict()   # (layer, weight) -> ... in the BN statistics buffer
        for ln, ws in g.params.items():
            for wn, shape in ws.items():
                n = int(np.prod(shape))
                if wn in ("moving_mean", "moving_variance"):
                    self.stat_slices[(ln, wn)] = (soff, n, shape); soff += _round_up(n, 4)
                else:
                    self.slices[(ln, wn)] = (off, n, shape); off += _round_up(n, 4)
        self.n_flat = off
        dev = self.device
        self.flat_w = torch.zeros(max(off, 4), dtype=torch.float32, device=dev)
        self.flat_stats = torch.zeros(max(soff, 4), dtype=torch.float32, device=dev)
        if self.mode == "training":
            self.flat_g = torch.zeros_like(self.flat_w)
            self.flat_v = torch.zeros_like(self.flat_w)
            if weight_ema.enabled(self.config, self.mode):
                self.flat_ema = torch.zeros_like(self.flat_w)          # set_weights below fills it: the average starts at the weights
            if swa.enabled(self.config, self.mode):                    # (the first collected model is copied in: zeros until then)
                self.flat_swa = torch.zeros_like(self.flat_w)
                if getattr(self.config, "SWA_VARIANCE", False):
                    self.flat_swa_sq = torch.zeros_like(self.flat_w)
        self.set_weights(initial_weights(g, seed, randomize_bn))

    def wview(self, ln, wn, buf=None):
        if (ln, wn) in self.slices:
            o, n, shape = self.slices[(ln, wn)]
            base = self.flat_w if buf is None else buf
        else:
            o, n, shape = self.stat_slices[(ln, wn)]
            base = self.flat_stats
        return base[o:o + n].view(shape)

    def gview(self, ln, wn):
        return self.wview(ln, wn, self.flat_g)

    def set_weights(self, params, strict=True):
        """params: {layer: {weight: array}} in Keras layouts.  Missing layers are skipped unless strict.  With Config.WEIGHT_EMA the values
        go into the average as well: a model that loads a checkpoint starts its average there (set_ema_weights loads another one).  With
        Config.SWA the collection starts afresh (ticks = models = 0): the models collected so far belong to other weights."""
        stand_in = getattr(self, "_stand_in", None)    # (getattr: tests/test_loss_weights_cpu.py calls this on a host stand-in of its own)
        assert stand_in != "ema", "set_weights while the average is swapped in (swap_ema / ema_weights)"
        assert stand_in not in ("swa", "swag"), \
            "set_weights while the SWA average or a SWAG sample stands in for the weights (swap_swa / swa_weights / swag_weights)"
        if getattr(self, "swa_state", None) is not None:
            self.reset_swa()
        ema = getattr(self, "flat_ema", None)
        for ln, wn, t in _checked_params(self.graph, params, strict):
            self.wview(ln, wn).copy_(t)
            if ema is not None and (ln, wn) in self.slices:
                self.wview(ln, wn, ema).copy_(self.wview(ln, wn))

    def set_ema_weights(self, params, strict=True):
        """Load params (as set_weights takes them) into the average alone; the BN statistics, which both sets share, are not touched."""
        assert self.flat_ema is not None, "Config.WEIGHT_EMA is off"
        assert self._stand_in != "ema", "set_ema_weights while the average is swapped in (swap_ema / ema_weights)"
        self._load_trainable(params, self.flat_ema, strict)

    def _load_trainable(self, params, buf, strict):
        """params' trainable tensors into the flat buffer `buf` (an average's: set_ema_weights, set_swa_weights); BN statistics are skipped."""
        for ln, wn, t in _checked_params(self.graph, params, strict, only=self.slices):
            self.wview(ln, wn, buf).copy_(t)

    # what stands in flat_w, as the three yes / no facts callers and tests ask for; _stand_in alone holds it
    ema_swapped = property(lambda self: self._stand_in == "ema", doc="flat_w holds the EMA average right now (swap_ema)")
    swa_swapped = property(lambda self: self._stand_in == "swa", doc="flat_w holds the SWA mean right now (swap_swa)")
    _swag_active = property(lambda self: self._stand_in == "swag", doc="flat_w holds a SWAG sample right now (swag_weights)")

    def get_weights(self, ema=False, swa=False):
        """{layer: {weight: array}}.  ema=True: the averaged parameters (Config.WEIGHT_EMA) beside the BN statistics, which both sets share.
        swa=True: the SWA mean (Config.SWA) likewise; swa="sq": the running mean of squares (SWA_VARIANCE) under the same names.
        Every set is found wherever it lies (train_state.weights_location): inside ema_weights() / swa_weights() two buffers have changed
        places.  Inside swag_weights() the plain call returns the sample, which is then the model (so that save_weights() writes a sampled model)."""
        if ema:
            assert self.flat_ema is not None, "Config.WEIGHT_EMA is off"
        if swa:
            assert not ema, "ema and swa are two sets: ask for one"
            assert self.flat_swa is not None, "Config.SWA is off"
            if swa == "sq":
                assert self.flat_swa_sq is not None, "Config.SWA_VARIANCE is off"
        which = ("sq" if swa == "sq" else "swa") if swa else ("ema" if ema else "raw")
        where = weights_location(self._stand_in, which, self.flat_ema is not None)
        buf = getattr(self, where) if where is not None else None
        out = OrderedDict()
        for ln, ws in self.graph.params.items():
            out[ln] = OrderedDict((wn, self.wview(ln, wn, buf).detach().cpu().numpy().copy()) for wn in ws)
        return out

    def get_grads(self):
        out = OrderedDict()
        for (ln, wn) in self.slices:
            out.setdefault(ln, OrderedDict())[wn] = self.gview(ln, wn).detach().cpu().numpy().copy()
        return out

    def trainable_ranges(self):
        """[(begin, end)] element ranges of the flat parameter / gradient buffers that belong to trainable layers."""
        return [(o, o + n) for (ln, _), (o, n, _) in self.slices.items() if self.layer_trainable.get(ln, False)]

    def set_trainable(self, layer_regex):
        """net.py:1030-1066: layer.trainable = fullmatch(regex, layer.name).  Rebuilds the plan."""
        self.layer_trainable = {n: bool(re.fullmatch(layer_regex, n)) for n in self.graph.params}
        self._graphs = None
        self._build_plan()

    # ------------------------------------------------------------------ plan construction
    def _ptr_or_none(self, ln, wn):
        if ln is None or (ln, wn) not in self.slices and (ln, wn) not in self.stat_slices:
            return None
        return self.wview(ln, wn).reshape(-1)

    def _plan_device_state(self, attr, init, dtype):
        """The rule of a feature's small device-side state (ls_state, ema_state, swa_state), "created once, like hyper": init None (the
        keys are off) drops it; the first plan that has the keys creates it from `init`; a later plan keeps the buffer -- the counts go on
        across set_trainable() -- unless the keys changed, and then the new values are copied into the SAME buffer."""
        if init is None:
            setattr(self, attr, None)
            self._state_init.pop(attr, None)
            return
        if getattr(self, attr) is None:
            setattr(self, attr, torch.tensor(init, dtype=dtype, device=self.device))
        elif init != self._state_init[attr]:
            getattr(self, attr).copy_(torch.tensor(init, dtype=dtype))
        self._state_init[attr] = init

    def _build_plan(self):
        training = self.mode == "training"
        self.plan_version += 1                         # ursonet_amd/dp.py re-derives its graph cuts when this moves
        # split counts, partial workspaces and grouped / paired weight-gradient launches are sized here from these kernel-policy options; the
        # library re-derives some of them at launch time, so a step under other values would reduce a different number of partials than it wrote
        self._plan_options = self._planning_options()
        # the plan's environment switches; tests build the non-default plans as references
        self._env_winograd = os.environ.get("URSO_WINOGRAD", "0") == "1"                # 1: 3x3 / stride-1 forward layers as Winograd (slower)
        self._env_compact_grad = os.environ.get("URSO_COMPACT_GRAD", "1") != "0"        # 0: dense stage-boundary gradients (_plan_compact_gradients)
        self._env_sampled_outputs = os.environ.get("URSO_SAMPLED_OUTPUTS", "1") != "0"  # 0: block outputs at every pixel (_sample_block_output)
        self._env_wgrad_group = int(os.environ.get("URSO_WGRAD_GROUP", "8"))            # layers per shared weight-gradient launch; 0: one each
        self._env_fuse_sqnorm = os.environ.get("URSO_FUSE_SQNORM", "1") != "0"          # 0: gradient norm by a pass of its own (_plan_buckets)
        self._env_wgrad_stream = int(os.environ.get("URSO_WGRAD_STREAM", "0"))          # 2: forked weight gradients (_fork_weight_gradients)
        # TRAIN_BN = None ("Train BN layers", net.py:60-76): batch statistics while training -- the BN is not folded, the conv
        # writes its raw output and separate stats / apply / backward kernels run (csrc/bn_train.hip).  Inference and
        # TRAIN_BN = False use the moving statistics folded into the filters.
        self.train_bn = training and self.config.TRAIN_BN is None
        # Config.LOSS_SCALE: None = every launch below is the one it is without the feature.  Set: the losses multiply
        # their gradients by the scale in front of the rounding to the engine dtype, every finalisation that writes flat_g divides it out again
        # before weight decay / BN derivation / squared norm, the optimizer skips a step whose norm is not finite and one more launch moves the scale
        if training:
            self._plan_device_state("ls_state", loss_scale.initial_state(self.config, self.world_size), torch.float32)
        if training and self.learn_lw:
            loss_weights.validate(self.config, self.world_size)
        # Config.WEIGHT_EMA: None = no launch and no buffer.  Set: one more launch at the end of opt_ops (_plan_optimizer).
        # Changed keys start the schedule afresh; the average stays
        if training:
            self._plan_device_state("ema_state", weight_ema.initial_state(self.config, self.world_size), torch.float32)
            if self.ema_state is not None and self.flat_ema is None:       # the key was set after the engine was built: the average starts
                self.flat_ema = self.flat_w.clone()                        # at the weights of now
        # Config.SWA: None = no launch and no buffer.  Set: one more launch, the last of opt_ops (_plan_optimizer).
        # Changed keys start the collection afresh
        if training:
            init = swa.initial_state(self.config, self.world_size)
            if init is not None:
                if self.flat_swa is None:              # the key was set after the engine was built
                    self.flat_swa = torch.zeros_like(self.flat_w)
                if bool(init[swa.VARIANCE]) != (self.flat_swa_sq is not None):
                    self.flat_swa_sq = torch.zeros_like(self.flat_w) if init[swa.VARIANCE] else None
            self._plan_device_state("swa_state", init, torch.int32)
        # Config.GRAD_ACCUM_STEPS: 1 = no launch and no buffer.  k > 1: one launch behind the backward pass of the
        # micro-steps that do not close (accum_ops) and one in front of the optimizer of the one that does (_plan_optimizer); a new plan
        # starts a new optimizer step
        self.accum_ops, self.accum_micro, self._accum_role = [], 0, None
        if training:
            self.accum_k = grad_accum.validate(self.config, self.world_size)
            self._accum_roles = grad_accum.roles(self.accum_k)
            if self.accum_k == 1:
                self.flat_acc = None
            elif self.flat_acc is None:
                self.flat_acc = torch.zeros_like(self.flat_w)
        self.acts = {}
        self.prep_ops, self.fwd_ops, self.loss_ops, self.bwd_ops, self.opt_ops = [], [], [], [], []      # lists of _Launch (plan_state.py)
        self.wino_ws = None
        self.n_entry_dgrad2 = 0
        self.n_wgrad_groups = 0
        self._cleared_once = []    # gradient buffers cleared at plan time only (scattered data gradients): (layer, buffer, H, W, C, sy, sx)
        self.loss_pre_ops = []     # DP_EXACT_REL_LOSS: the part of the loss that precedes the cross-rank sum of the two norms
        self.convs = OrderedDict()
        self._descs = []                           # hip.ParamDesc of every non-stem weight layer
        self._fused_pools = {}                     # id(pool node) -> the stem conv whose kernel also pools
        self._plan_input()
        for node in self.graph.nodes:
            if node.op == "pool":
                self._plan_pool(node)
            else:
                self._plan_conv(node)
        self._fuse_pointwise_pairs()
        self._fuse_entry_shortcuts()
        self._fuse_dense_heads()
        self._plan_forward_workspaces()
        self.out_loc = self.acts[self.graph.outputs["loc"].id]
        self.out_ori = self.acts[self.graph.outputs["ori"].id] if "ori" in self.graph.outputs else None      # keypoint mode has no orientation head
        self._build_heads_io()
        if not training:
            for X in list(self.acts.values()):
                self._sample_block_output(X)
            return
        self._plan_stem_workspaces()
        self._build_losses()
        self._plan_relu_bitmasks()
        self._plan_backward()
        self._resolve_bucket_ops()
        self._plan_optimizer()
        self._plan_sam()
        self.flat_g.zero_()
        self._fork_weight_gradients()

    @property
    def labels(self):
        """{pass: [label of every launch, in launch order]}: for profiles, tools and tests.  The plan itself never reads a label."""
        out = {"prep": [l.label for l in self.prep_ops], "fwd": [l.label for l in self.fwd_ops],
               "loss": [l.label for l in self.loss_pre_ops + self.loss_ops], "bwd": [l.label for l in self.bwd_ops],
               "opt": [l.label for l in self.opt_ops]}
        if self.accum_ops:                             # Config.GRAD_ACCUM_STEPS > 1: what a micro-step that does not close runs in place of "opt"
            out["accum"] = [l.label for l in self.accum_ops]
        if self.sam_ops:                               # Config.SAM: norm and ascent between the two passes (prep ... bwd run twice), the way back behind them
            out["sam"] = [l.label for l in self.sam_ops]
        return out

    def _act(self, spec, numel=None):
        if spec.id not in self.acts:
            self.acts[spec.id] = _Act(self, spec, numel if numel is not None else self.B * spec.h * spec.w * spec.c, self.tdt)
        return self.acts[spec.id]

    # ---------------------------------------------------------------- forward
    def _plan_input(self):
        """Two input forms: molded float32 frames (the reference's generator format) or raw uint8 frames whose mean subtraction
        (mold_image, net.py:1337-1348) happens in the molding kernel -- 4x fewer bytes over PCIe (ursonet_amd/feeder.py)."""
        B, dt, dev = self.B, self.dt, self.device
        self.in_images = torch.zeros(B, self.H, self.W, 3, dtype=torch.float32, device=dev)
        mp = np.asarray(self.config.MEAN_PIXEL, dtype=np.float32)
        self.mean3 = torch.tensor(mp if mp.size == 3 else np.full(3, float(mp.mean()), dtype=np.float32), device=dev)
        x0 = self._act(self.graph.tensors[0], B * self.H * self.W * 4)     # channels padded 3 -> 4, viewed as pixel pairs
        self.fwd_ops.append(_Launch(lambda: hip.mold_images(B, self.H, self.W, self.in_images_u8 if self.input_u8 else self.in_images,
                                                            self.mean3 if self.input_u8 else None, dt, x0.data), "mold"))

    def _plan_pool(self, node):
        if id(node) in self._fused_pools:      # computed by the stem's own kernel (urso_stem_conv_pool): no launch, no conv1 output
            return
        B, dt = self.B, self.dt
        src, dst = self._act(node.src), self._act(node.dst)
        am = torch.empty(dst.numel, dtype=torch.uint8, device=self.device)
        h, w, c = node.src.h, node.src.w, node.src.c
        self.fwd_ops.append(_Launch(lambda s=src, d=dst, am=am, h=h, w=w, c=c: hip.maxpool_fwd(B, h, w, c, dt, s.data, d.data, am), "maxpool"))
        node._am = am

    def _plan_conv(self, node):
        """One conv / Dense layer: geometry, weight-prep descriptor and forward launch."""
        B, dt, dev = self.B, self.dt, self.device
        training = self.mode == "training"
        c = _Conv(node)
        c.src = self._act(node.src) if not node.stem else self.acts[self.graph.tensors[0].id]
        out_elt = torch.float32 if node.out_f32 else self.tdt
        if node.dst.id not in self.acts:
            self.acts[node.dst.id] = _Act(self, node.dst, B * node.dst.h * node.dst.w * c.npad, out_elt)
        c.dst = self.acts[node.dst.id]
        c.res = self._act(node.residual) if node.residual is not None else None
        c.xin = c.src.data                         # the tensor the forward pass and the weight gradient read (c.gf describes it)
        if node.stem:
            c.gf = hip.geom(B, self.H, self.W // 2, 8, node.dst.h, node.dst.w, c.npad, 7, 4, 2, 1, 3, 2)
            c.K_raw = 7 * 4 * 8
        elif node.dense:
            c.gf = hip.geom(B, 1, 1, node.cin, 1, 1, c.npad, 1, 1)
            c.gd = hip.geom(B, 1, 1, c.npad, 1, 1, node.cin, 1, 1)
            c.K_raw = node.cin
        else:
            s, (pt, pl) = node.stride, node.pad
            c.gf = hip.geom(B, node.src.h, node.src.w, node.cin, node.dst.h, node.dst.w, c.npad, node.kh, node.kw, s, s, pt, pl)
            if node.kh == 1 and node.kw == 1 and s > 1:
                # compact data gradient: GEMM over the forward-output pixels, scattered to every s-th pixel
                # of the (pre-zeroed) input-gradient buffer instead of a 4x wasteful gather over all pixels
                c.gd = hip.geom(B, node.dst.h, node.dst.w, c.npad, node.dst.h, node.dst.w, node.cin, 1, 1,
                                FH=node.src.h, FW=node.src.w, OSH=s, OSW=s)
                c.gd_scatter = True
                c.gd_scatter_stride = s
            else:
                c.gd = hip.geom(B, node.dst.h, node.dst.w, c.npad, node.src.h, node.src.w, node.cin, node.kh, node.kw,
                                1, 1, node.kh - 1 - pt, node.kw - 1 - pl, s, s)
            c.K_raw = node.kh * node.kw * node.cin
            if (node.kh == 1 and node.kw == 1 and s == 2 and dt != hip.F32 and node.src.h % 2 == 0 and node.src.w % 2 == 0 and
                    (node.cin * 2) % 16 == 0):
                self._plan_compact_input(c)
        VE = 16 // (4 if dt == hip.F32 else 2)
        if node.cin % VE and not node.stem:
            raise ValueError("layer %s: %d input channels is not a multiple of %d" % (node.name, node.cin, VE))
        kelems = c.npad * c.K_raw
        c.wf = torch.empty(kelems, dtype=self.tdt, device=dev)
        need_dgrad = training and not node.stem
        c.wd = torch.empty(kelems, dtype=self.tdt, device=dev) if need_dgrad else None
        c.biasf = torch.empty(c.npad, dtype=torch.float32, device=dev)
        c.scale = torch.empty(c.npad, dtype=torch.float32, device=dev)
        c.w = self.wview(node.name, "kernel").reshape(-1)
        c.b = self._ptr_or_none(node.name, "bias") if node.bias else None
        c.gamma = self._ptr_or_none(node.bn, "gamma") if node.bn else None
        c.beta = self._ptr_or_none(node.bn, "beta") if node.bn else None
        c.mean = self._ptr_or_none(node.bn, "moving_mean") if node.bn else None
        c.var = self._ptr_or_none(node.bn, "moving_variance") if node.bn else None
        c.batch_bn = bool(self.train_bn and node.bn)
        if c.batch_bn:
            # unfolded conv: the BN tensors move to the bn_* fields, the conv itself is a plain conv + bias
            assert c.npad == c.N and not node.out_f32
            c.bn_gamma, c.bn_beta, c.bn_mmean, c.bn_mvar = c.gamma, c.beta, c.mean, c.var
            c.gamma = c.beta = c.mean = c.var = None
            c.Mpix = B * node.dst.h * node.dst.w
            c.z = torch.empty(c.Mpix * c.N, dtype=self.tdt, device=dev)
            c.dz = torch.empty(c.Mpix * c.N, dtype=self.tdt, device=dev)
            c.bmean, c.bvar = torch.empty(c.N, dtype=torch.float32, device=dev), torch.empty(c.N, dtype=torch.float32, device=dev)
            c.dbeta, c.dgamma = torch.empty(c.N, dtype=torch.float32, device=dev), torch.empty(c.N, dtype=torch.float32, device=dev)
        self.convs[node.name] = c
        # -- weight prep (per step in training; once in inference): the stem has its own packing kernel, every other
        #    layer gets a descriptor and ONE batched launch covers them all (urso_param_batch_run)
        if node.stem:
            self.prep_ops.append(_Launch(lambda c=c: hip.stem_weight_pack(c.N, dt, c.w, c.b, c.gamma, c.beta, c.mean, c.var, BN_EPS,
                                                                          c.wf, c.biasf, c.scale), "prep", "prep:" + node.name))
        else:
            d = hip.ParamDesc()
            c.splits = hip.conv_wgrad_splits(c.gf, dt) if training else 1
            hip.param_desc_init(d, node.kh if not node.dense else 1, node.kw if not node.dense else 1, node.cin, c.N, c.npad,
                                max(c.splits, 1), BN_EPS, float(self.config.WEIGHT_DECAY))
            for f, t in (("w", c.w), ("b", c.b), ("gamma", c.gamma), ("beta", c.beta), ("mean", c.mean), ("var", c.var),
                         ("wf", c.wf), ("wd", c.wd), ("biasf", c.biasf), ("scale", c.scale)):
                setattr(d, f, hip.ptr(t))
            c.desc_id = len(self._descs)
            c.desc = d
            self._descs.append(d)
        self._plan_conv_forward(c)

    def _plan_compact_input(self, c):
        """A stage's stride-2 entry layers (branch2a and the projection shortcut, net.py:121-126) read every second pixel of every
        second row of the previous stage's output: the strided source mapping costs the DMA kernel 20-35 us per layer against
        the same GEMM on a dense tensor (and keeps the layer off the register-filter kernels), forward and in the weight
        gradient.  The sampled pixels are gathered ONCE per step (urso_rows_subsample2) and both layers -- forward and weight
        gradient -- run as plain pointwise layers on that compact tensor."""
        node, B, dt = c.node, self.B, self.dt
        X = c.src
        if X.data_compact is None:
            X.data_compact = torch.empty(X.numel // 4, dtype=self.tdt, device=self.device)
            # ... by the layer that produces X where that is a stage-closing c -> 4c layer on the register-filter kernel
            # (urso_conv_pointwise_sampled: a second store from the LDS tile that holds the output rows), else by a gather pass
            P = [cc_ for cc_ in self.convs.values() if cc_.dst is X]
            Pc = P[0] if len(P) == 1 else None
            if (Pc is not None and not Pc.batch_bn and Pc.fwd is not None and hip.get_option("pair") and
                    hip.conv_pointwise_sampled_ok(Pc.gf, dt, Pc.fwd_flags | hip.EPI_EMIT_BITS, Pc.res is not None)):
                Pc.fwd.run = (lambda Pc=Pc, X=X: hip.conv_pointwise_sampled(
                    Pc.gf, dt, Pc.fwd_flags | (hip.EPI_EMIT_BITS if Pc.dst.bits is not None else 0), Pc.xin, Pc.wf, Pc.biasf,
                    Pc.res.data if Pc.res is not None else None, Pc.dst.data, Pc.dst.bits, X.data_compact))
                Pc.fwd.kind, Pc.fwd.label = "fwd+sampled", "fwd:%s+sampled" % Pc.name
            else:
                X.gather = _Launch(lambda X=X, hh=node.src.h, ww=node.src.w, rb=node.cin * 2:
                                   hip.rows_subsample2(B, hh, ww, rb, X.data, X.data_compact), "subsample", "subsample:T%d" % node.src.id)
                self.fwd_ops.append(X.gather)
        c.gf = hip.geom(B, node.dst.h, node.dst.w, node.cin, node.dst.h, node.dst.w, c.npad, 1, 1)
        c.xin = X.data_compact

    def _plan_conv_forward(self, c):
        node, dt, dev = c.node, self.dt, self.device
        training = self.mode == "training"
        flags = (hip.EPI_RELU if node.relu else 0) | (hip.EPI_OUT_F32 if node.out_f32 else 0)
        # split-K workspace (tiny-grid / deep-K layers: bottleneck_layer, Dense heads); 0 = not split
        c.ws_f = hip.conv_igemm_ws_bytes(c.gf, dt)
        c.ws_d = hip.conv_igemm_ws_bytes(c.gd, dt) if (c.gd is not None and training) else 0
        c.fwd_flags = flags
        # 3x3 layers taken by the halo-tile kernel get its stream-K hand-over workspace (dedicated: its first 4 KiB are flags that
        # must stay zero between launches, include/ursonet_hip.h)
        # (a batch-statistics layer launches the bare conv: no ReLU, no residual -- those belong to its bn_apply)
        c.halo_f = dt != hip.F32 and (hip.conv_igemm_halo_ok(c.gf, dt, 0, False) if c.batch_bn else
                                      hip.conv_igemm_halo_ok(c.gf, dt, flags, c.res is not None))
        c.halo_d = bool(c.gd is not None and training and dt != hip.F32 and hip.conv_igemm_halo_ok(c.gd, dt, 0, False))
        if (c.halo_f or c.halo_d) and self.halo_ws is None:
            self.halo_ws = torch.zeros(hip.conv_igemm_halo_ws_bytes() // 4 + 16, dtype=torch.float32, device=dev)
        if c.batch_bn:
            self.fwd_ops += [
                _Launch(lambda c=c: hip.conv_igemm_ex(c.gf, dt, 0, c.xin, c.wf, c.biasf, None, None, c.z, None, self.forward_workspace(c)),
                        "fwd", "fwd:" + node.name, fwd=(node.name,)),
                _Launch(lambda c=c: hip.bn_batch_stats(c.Mpix, c.N, dt, c.z, self.bn_ws, c.bmean, c.bvar, c.bn_mmean, c.bn_mvar, BN_MOMENTUM, BN_EPS),
                        "bn_stats", "bn_stats:" + node.name),
                _Launch(lambda c=c, n=node: hip.bn_apply(c.Mpix, c.N, dt, c.z, c.bmean, c.bvar, c.bn_gamma, c.bn_beta, BN_EPS,
                                                         c.res.data if c.res is not None else None, n.relu, c.dst.data),
                        "bn_apply", "bn_apply:" + node.name)]
            return
        elif (self._env_winograd and dt != hip.F32 and not node.stem and not node.dense and node.kh == 3 and node.kw == 3 and
              node.stride == 1 and tuple(node.pad) == (1, 1) and c.res is None and not (flags & ~hip.EPI_RELU) and c.npad == c.N and
              hip.conv_winograd_ws_bytes(c.gf, dt) > 0):
            # opt-in: the 3x3 / stride-1 layers through the Winograd F(2x2, 3x3) evaluation (conv_winograd.hip; north_star names it; slower
            # than the direct kernels on MI355X).  One shared workspace, sized for the largest layer.
            need_ws = hip.conv_winograd_ws_bytes(c.gf, dt) // 4 + 64
            if self.wino_ws is None or self.wino_ws.numel() < need_ws:
                self.wino_ws = torch.empty(need_ws, dtype=torch.float32, device=dev)
            c.fwd = _Launch(lambda c=c, f=flags: hip.conv_winograd_fwd(c.gf, dt, f, c.xin, c.wf, c.biasf, c.dst.data, self.wino_ws),
                            "fwd", "fwd:" + node.name, fwd=(node.name,))
            c.winograd = True
        elif (pool := self._stem_pool_node(self.graph, node, c, dt)) is not None:
            # conv1 + ReLU + the max-pool behind it in one kernel: conv1's output (the largest tensor of the net, read by the pool
            # alone) is neither written nor read; its _Act keeps no storage
            self._fused_pools[id(pool)] = c
            pdst = self._act(pool.dst)
            pool._am = torch.empty(pdst.numel, dtype=torch.uint8, device=dev)
            c.dst.data = torch.empty(0, dtype=self.tdt, device=dev)      # (frees the 335 MB; any later read raises: _Act.data)
            c.dst.fused_pool = True
            c.fwd = _Launch(lambda c=c, d=pdst, am=pool._am: hip.stem_conv_pool(c.gf, dt, c.xin, c.wf, c.biasf, d.data, am),
                            "fwd+maxpool", "fwd:%s+maxpool" % node.name, fwd=(node.name,))
        else:
            c.fwd = _Launch(lambda c=c, f=flags: hip.conv_igemm_ex(
                c.gf, dt, f | (hip.EPI_EMIT_BITS if c.dst.bits is not None else 0), c.xin, c.wf, c.biasf,
                c.res.data if c.res is not None else None, None, c.dst.data, c.dst.bits, self.forward_workspace(c)), "fwd", "fwd:" + node.name,
                fwd=(node.name,))
        self.fwd_ops.append(c.fwd)

    def forward_workspace(self, c):
        """The workspace of layer c's forward conv launch: the halo-tile kernel's dedicated hand-over workspace where that kernel takes the
        layer (never the split-K one: it would read the partials of other layers as its flags), else the split-K workspace where the layer splits."""
        return self.halo_ws if c.halo_f else (self.igemm_ws if c.ws_f else None)

    def _plan_forward_workspaces(self):
        """The workspaces the forward launches share (sized for the largest layer) and the batched weight prep."""
        convs, dev = list(self.convs.values()), self.device
        max_igemm_ws = max([0] + [max(c.ws_f, c.ws_d) for c in convs])
        max_bn_ws = max([0] + [hip.bn_ws_bytes(c.Mpix, c.N) for c in convs if c.batch_bn])
        self.igemm_ws = torch.empty(max_igemm_ws // 4 + 16, dtype=torch.float32, device=dev)
        self.bn_ws = torch.empty(max_bn_ws // 8 + 32, dtype=torch.float64, device=dev) if max_bn_ws else None
        if self._descs:
            self.prep_ops.append(_Launch(lambda: self.pbatch.run(hip.PB_PREP, "all", self.dt), "prep", "prep:batched[%d layers]" % len(self._descs),
                                         bucket="all"))
        if self.mode != "training":
            self._upload_param_table()

    def _plan_stem_workspaces(self):
        """The stem's weight-gradient and finalisation workspaces (every other layer has a split workspace of its own)."""
        stems = [c for c in self.convs.values() if c.node.stem]
        max_ws = max([0] + [hip.conv_wgrad_ws_bytes(c.gf, self.dt) for c in stems])
        max_fin_ws = max([0] + [hip.param_grad_finalize_ws_bytes(147, c.N) for c in stems])
        self.ws = torch.empty(max_ws // 4 + 64, dtype=torch.float32, device=self.device)
        self.fin_ws = torch.empty(max_fin_ws // 4 + 64, dtype=torch.float32, device=self.device)

    # ---------------------------------------------------------------- backward
    def _plan_buckets(self):
        """Gradient buckets (contiguous slices of the flat gradient buffer, in the order the backward pass completes them):
        the split reduction + finalisation of all layers of a bucket is three batched launches issued once the last of
        their weight-gradient partials is enqueued; ursonet_amd/dp.py starts the bucket's all-reduce right after."""
        from .dp import plan_buckets
        ext = {}
        for (ln, wn), (o, n, _) in self.slices.items():
            s0, e0 = ext.get(ln, (o, o))
            ext[ln] = (min(s0, o), max(e0, o + _round_up(n, 4)))
        self.buckets = plan_buckets(sorted(((ln, s0, e0) for ln, (s0, e0) in ext.items()), key=lambda t: t[1]), self.grad_bucket_bytes,
                                    tail_bytes=self.grad_tail_bytes)
        # Global gradient norm without a pass of its own: with ONE gradient bucket and nothing between finalisation and optimizer (no all-reduce,
        # no batch-statistics BN writing gamma / beta gradients elsewhere) every gradient slice is written by a finalisation launch, and each of
        # their blocks leaves the sum of squares of what it stored (urso_param_batch_run_sq): urso_sqnorm_final adds the slots (-24 us of reading
        # the 134 MB buffer back).  ursonet_amd/dp.py sets no_fused_sqnorm: there the norm is that of the all-reduced gradient.  Under
        # GRAD_ACCUM_STEPS > 1 the finalisations' slots would hold the norm of the last micro-batch's gradient alone: the plan is the
        # unfused one and the close launch writes the slots of the mean gradient instead (_plan_optimizer).
        self.fused_sqnorm = (self._env_fuse_sqnorm and not self.no_fused_sqnorm and self.accum_k == 1 and
                             len(self.buckets) == 1 and not any(c_.batch_bn for c_ in self.convs.values()))
        self._sq_slots = 0
        bucket_of = {ln: k for k, (_, _, names) in enumerate(self.buckets) for ln in names}
        groups = OrderedDict()                      # bucket index -> [conv names], backward order
        for node in self._backward_order():
            if node.op == "pool" or node.stem:
                continue
            folded_bn = node.bn and not self.convs[node.name].batch_bn      # batch-statistics BN finalises its own gamma/beta
            if self.layer_trainable[node.name] or (folded_bn and self.layer_trainable[node.bn]):
                groups.setdefault(bucket_of[node.name], []).append(node.name)
        self._last_of_group = {names[-1]: k for k, names in groups.items()}
        self._bucket_groups = groups                # (param_pass_bytes: what the batched parameter-sized launches of a bucket move)

    def _plan_needed_gradients(self):
        """Which activation gradients are needed at all: a tensor's gradient only if a trainable parameter lies at or upstream of its
        producer.  With layers='heads' / '4+' / '5+' (net.py:1086-1095) the data-gradient chain stops at the earliest trainable
        layer instead of running through the frozen backbone (TF prunes those gradients too)."""
        g = self.graph
        need = {g.tensors[0].id: False}
        for node in g.nodes:
            if node.op == "pool":
                need[node.dst.id] = need.get(node.src.id, False)
            else:
                own = self.layer_trainable[node.name] or bool(node.bn and self.layer_trainable[node.bn])
                need[node.dst.id] = (own or (not node.stem and need.get(node.src.id, False)) or
                                     (node.residual is not None and need.get(node.residual.id, False)))
        self.grad_needed = need

    def _plan_backward(self):
        dt = self.dt
        # Grouped pointwise weight gradients (urso_wgrad_group_run): a layer launched alone is cut into ~2 blocks per CU whatever its
        # size, so it writes -- and the bucket's split reduction re-reads -- CUs x 128 KiB of fp32 partials (32 MB a layer, as much as
        # its operands in stages 4-5), in a burst at the end of the launch that nothing overlaps.  Up to URSO_WGRAD_GROUP consecutive
        # pointwise layers of a bucket share one launch instead: each gets 1/n of the splits, its blocks run n times longer.
        q = _PendingLaunches(self, self._env_wgrad_group if dt != hip.F32 else 0)
        self._plan_buckets()
        self._plan_needed_gradients()
        need = self.grad_needed
        self._plan_compact_gradients(need)
        # Data gradients of the Dense heads (urso_dense_multi): the layers of one depth behind the bottleneck features share a launch, and the
        # two gradients into a tensor both branches read (loc_dense_0 / ori_dense_0 -> the bottleneck features) are the two reduction
        # segments of ONE layer instead of a launch that writes and a launch that accumulates in place
        dense_lv = self._dense_levels() if self.dense_multi else {}
        for node in self._backward_order():
            lvl_n = dense_lv.get(node.name) if node.op != "pool" else None
            q.at_node(lvl_n)
            if not need[node.dst.id]:
                continue                                   # nothing trainable at or below this node
            if node.op == "pool":
                self._plan_pool_backward(node)
                continue
            c = self.convs[node.name]
            assert c.dst.grad_written or c.dst.grad is not None, "no gradient reaches %s" % node.name
            G = c.dst.grad                             # compact tensors: [B, H/2, W/2, N] (see _plan_compact_gradients)
            tr = self.layer_trainable[node.name]
            bn_tr = self.layer_trainable[node.bn] if node.bn else False
            Gsum = G                                   # gradient w.r.t. (BN output + residual): what a residual branch receives
            if c.batch_bn:
                ggam, gbet = self.gview(node.bn, "gamma").reshape(-1), self.gview(node.bn, "beta").reshape(-1)
                self.bwd_ops.append(_Launch(lambda c=c, G=G, bn_tr=bn_tr, ggam=ggam, gbet=gbet:
                                            hip.bn_backward(c.Mpix, c.N, dt, G, c.z, c.bmean, c.bvar, c.bn_gamma, BN_EPS, self.bn_ws, c.dbeta, c.dgamma,
                                                            bn_tr, gbet, ggam, c.dz, ls=self.ls_state), "bn_bwd", "bn_bwd:" + node.name, done=(node.name,)))
                G = c.dz                               # the conv itself sees the gradient w.r.t. its raw output
                bn_tr = False                          # gamma/beta gradients are done; the finalisation treats the layer as a plain conv
            # -- weight gradient + finalisation (skipped for fully frozen layers; their grads stay zero)
            if (tr or bn_tr) and node.stem:
                self._plan_stem_wgrad(c, G, tr, bn_tr)
            elif tr or bn_tr:
                self._plan_wgrad(c, G, tr, bn_tr, q, lvl_n)
            self._plan_residual_handover(c, Gsum)
            self._plan_dgrad(c, G, q, lvl_n)
        q.flush()

    def _plan_pool_backward(self, node):
        if not self.grad_needed[node.src.id]:
            return
        B, dt = self.B, self.dt
        src, dst = self.acts[node.src.id], self.acts[node.dst.id]
        h, w, cc = node.src.h, node.src.w, node.src.c
        assert dst.grad_written
        # the pool behind the stem: its backward pass would write the gradient of conv1's output (335 MB at cfg2) for conv1's weight
        # gradient alone (the image needs no data gradient) -- that kernel rebuilds the tiles it needs from dst.grad and the
        # arg-max bytes instead (urso_stem_wgrad_pooled): no launch here, no tensor
        prod = [cc_ for cc_ in self.convs.values() if cc_.dst is src]
        if (len(prod) == 1 and prod[0].node.stem and not prod[0].batch_bn and dt != hip.F32 and hip.get_option("stem") and cc == 64 and
                h % 2 == 0 and w % 2 == 0 and (self.layer_trainable[prod[0].node.name] or bool(prod[0].node.bn and self.layer_trainable[prod[0].node.bn]))):
            prod[0].pooled_grad = (dst, node._am)
            src.grad_written = True
            return
        gsrc = src.grad_buf()
        self.bwd_ops.append(_Launch(lambda d=dst, gs=gsrc, am=node._am, h=h, w=w, cc=cc:
                                    hip.maxpool_bwd(B, h, w, cc, dt, d.data, d.grad, am, 1, gs), "maxpool_bwd"))
        src.grad_written = True

    def _plan_stem_wgrad(self, c, G, tr, bn_tr):
        node, cfg, dt, dev = c.node, self.config, self.dt, self.device
        done = (node.name,)
        c.dw_raw = torch.empty(c.K_raw * c.npad, dtype=torch.float32, device=dev)
        c.colsum = torch.empty(c.npad, dtype=torch.float32, device=dev)
        if c.pooled_grad is not None:
            self.bwd_ops.append(_Launch(lambda c=c, pg=c.pooled_grad: hip.stem_wgrad_pooled(c.gf, dt, c.src.data, pg[0].grad, pg[1], self.ws,
                                                                                            c.dw_raw, c.colsum),
                                        "wgrad", "wgrad:%s+maxpool_bwd" % node.name, wgrad=done, done=done))
        else:
            self.bwd_ops.append(_Launch(lambda c=c, G=G: hip.conv_wgrad(c.gf, dt, c.src.data, G, self.ws, c.dw_raw, c.colsum),
                                        "wgrad", "wgrad:" + node.name, wgrad=done, done=done))
        c.dw_unp = torch.empty(147 * c.N, dtype=torch.float32, device=dev)
        self.bwd_ops.append(_Launch(lambda c=c: hip.stem_wgrad_unpack(c.N, c.dw_raw, c.dw_unp), "unpack", "unpack:" + node.name, done=done))
        gw = self.gview(node.name, "kernel").reshape(-1)
        gb = self.gview(node.name, "bias").reshape(-1) if node.bias else None
        gg = self.gview(node.bn, "gamma").reshape(-1) if (node.bn and not c.batch_bn) else None
        gbe = self.gview(node.bn, "beta").reshape(-1) if (node.bn and not c.batch_bn) else None
        if self.ls_state is not None:
            s0 = s1 = 0
            if self.fused_sqnorm:
                s0 = self._sq_slots
                s1 = self._sq_slots = s0 + hip.param_grad_finalize_sq_slots(147, c.N)
            run = (lambda c=c, gw=gw, gb=gb, gg=gg, gbe=gbe, tr=tr, bn_tr=bn_tr, s0=s0, s1=s1:
                   hip.param_grad_finalize_ls(147, c.N, c.N, c.dw_unp, c.colsum, c.w, c.b, c.gamma, c.mean, c.var, BN_EPS,
                                              float(cfg.WEIGHT_DECAY), tr, bn_tr, gw, gb, gg, gbe, self.fin_ws,
                                              self.sqpart[s0:s1] if s1 > s0 else None, self.ls_state))
        elif self.fused_sqnorm:
            s0 = self._sq_slots
            s1 = self._sq_slots = s0 + hip.param_grad_finalize_sq_slots(147, c.N)
            run = (lambda c=c, gw=gw, gb=gb, gg=gg, gbe=gbe, tr=tr, bn_tr=bn_tr, s0=s0, s1=s1:
                   hip.param_grad_finalize_sq(147, c.N, c.N, c.dw_unp, c.colsum, c.w, c.b, c.gamma, c.mean, c.var, BN_EPS,
                                              float(cfg.WEIGHT_DECAY), tr, bn_tr, gw, gb, gg, gbe, self.fin_ws, self.sqpart[s0:s1]))
        else:
            run = (lambda c=c, gw=gw, gb=gb, gg=gg, gbe=gbe, tr=tr, bn_tr=bn_tr:
                   hip.param_grad_finalize(147, c.N, c.N, c.dw_unp, c.colsum, c.w, c.b, c.gamma, c.mean, c.var, BN_EPS,
                                           float(cfg.WEIGHT_DECAY), tr, bn_tr, gw, gb, gg, gbe, self.fin_ws))
        self.bwd_ops.append(_Launch(run, "finalize", "finalize:" + node.name, done=done))

    def _plan_wgrad(self, c, G, tr, bn_tr, q, lvl_n):
        """Weight gradient of a non-stem layer: the split workspace and finalisation fields of its descriptor, and the launch that writes
        its partials -- its own, a shared one (q), or none where a fused data-gradient launch writes them.  Closes the layer's bucket."""
        node, d, B, dt, dev = c.node, c.desc, self.B, self.dt, self.device
        gf_w = c.gf_compact or c.gf
        # a 64 -> 256 pointwise layer outside the pairs (the stage-2 projection shortcut) whose data gradient is the first
        # contribution to its input's gradient: both gradients in one pass over dz (urso_conv_dgrad_wgrad_pw)
        Xs = c.src
        Ms = B * node.dst.h * node.dst.w
        c.solo = (hip.get_option("pair") == 1 and dt != hip.F32 and not node.dense and node.kh == 1 and node.kw == 1 and node.stride == 1 and
                  node.cin == 64 and c.npad == 256 and c.N == 256 and not c.batch_bn and self.grad_needed[Xs.spec.id] and
                  not c.wgrad_by_pair and not c.dgrad_done_by_pair and
                  c.gf_compact is None and c.dst.compact is None and Xs.compact is None and not c.gd_scatter and
                  not Xs.grad_written and Xs.pending is None and self.pair_first.get(node.name) is None and node.name not in self._last_of_group and
                  hip.conv_pair_wgrad_splits(Ms, dt) > 1)
        if c.solo:
            c.splits = c.desc.splits = hip.conv_pair_wgrad_splits(Ms, dt)
        n_part = c.splits * (c.K_raw * c.npad + hip.WGRAD_PART_PAD)
        by_pair = c.wgrad_by_pair or c.solo         # partials written by a fused launch (the pair of the layer above / below)
        c.wg_npart = n_part
        c.wg_ws = torch.empty((n_part + c.splits * c.npad if by_pair else hip.conv_wgrad_ws_bytes(gf_w, dt) // 4) + 64,
                              dtype=torch.float32, device=dev)
        c.dw_raw = torch.empty(c.K_raw * c.npad, dtype=torch.float32, device=dev) if c.splits > 1 else None
        c.colsum = torch.empty(c.npad, dtype=torch.float32, device=dev) if c.splits > 1 else None
        c.dotpart = torch.empty(d.ks * c.N + 16, dtype=torch.float32, device=dev)
        d.part, d.colpart = c.wg_ws.data_ptr(), c.wg_ws.data_ptr() + 4 * n_part
        d.dw_raw, d.colsum, d.dotpart = hip.ptr(c.dw_raw), hip.ptr(c.colsum), hip.ptr(c.dotpart)
        d.trainable, d.bn_trainable = int(tr), int(bn_tr)
        d.gw = hip.ptr(self.gview(node.name, "kernel").reshape(-1))
        d.gb = hip.ptr(self.gview(node.name, "bias").reshape(-1)) if node.bias else None
        d.ggamma = hip.ptr(self.gview(node.bn, "gamma").reshape(-1)) if (node.bn and not c.batch_bn) else None
        d.gbeta = hip.ptr(self.gview(node.bn, "beta").reshape(-1)) if (node.bn and not c.batch_bn) else None
        if not by_pair:
            xw = c.xin if gf_w is c.gf else c.src.data
            if q.wg_max > 1 and gf_w.KH * gf_w.KW * gf_w.C == c.K_raw and gf_w.N == c.npad and hip.conv_wgrad_pair_splits(gf_w, gf_w, dt):
                # a 3x3 layer of the register-resident kernel: two of them share a launch and the CUs (urso_conv_wgrad_partial2)
                q.add_wgrad_pair((c, node.name, xw, G, gf_w))
            elif q.wg_max > 1 and hip.wgrad_group_fits(gf_w, dt) and gf_w.KH * gf_w.KW * gf_w.C == c.K_raw and gf_w.N == c.npad:
                # a layer of the general kernel: its weight gradient waits for company (_PendingLaunches.flush_wgrads); every tensor has a
                # gradient buffer of its own, so G is still there when the launch comes
                q.add_wgrad_group((c, node.name, xw, G, gf_w))
            elif lvl_n is not None and c.splits == 1 and gf_w is c.gf and self._dense_multi_ok(c):
                q.add_dense_wgrad(dict(name=node.name, x=xw, dz=G, part=c.wg_ws, colpart=c.wg_ws[c.wg_npart:], M=B, K=c.K_raw, N=c.npad))
            else:
                q.emit_wgrad(c, node.name, xw, G, gf_w)
        if node.name in self._last_of_group:
            q.flush_bucket()                       # the bucket's reduction reads every partial of the bucket
            k = self._last_of_group[node.name]
            for kind in self._BUCKET_PHASES:       # (run: filled in by _resolve_bucket_ops)
                self.bwd_ops.append(_Launch(None, kind, "%s:bucket%d" % (kind, k), done=tuple(self._bucket_groups[k]), bucket=k))

    def _plan_residual_handover(self, c, Gsum):
        """Residual branch: its gradient IS Gsum (Add); fold it into the next dgrad (post-ReLU tensors) or alias it."""
        if c.res is None or not self.grad_needed[c.res.spec.id]:
            return
        B, node = self.B, c.node
        R = c.res
        if R.grad_written or R.pending is not None:
            raise AssertionError("unexpected second residual consumer for %s" % node.name)
        if R.spec.relu and c.dst.compact is not None and c.dst.residual_needs_dense:
            # no fused pair on the residual side: hand over the dense form (zeros written once, by the expansion)
            # (the dense form is zero off the even grid in every step and nothing else writes it: cleared once, here; a step rewrites
            # the even pixels only -- urso_rows_scatter2, a quarter of the bytes of the full expansion urso_rows_expand2)
            c.dst.grad_dense = torch.zeros(c.dst.numel, dtype=self.tdt, device=self.device)
            self.bwd_ops.append(_Launch(lambda X=c.dst: hip.rows_scatter2(B, X.compact[0], X.compact[1], X.spec.c * 2, X.grad, X.grad_dense),
                                        "expand", "expand:" + node.name))
            R.pending = c.dst.grad_dense
        elif R.spec.relu:
            R.pending = Gsum
            R.pending_hw = c.dst.compact           # (H, W) when Gsum holds only the even rows / columns, else None
        else:
            assert c.dst.compact is None
            R.grad, R.grad_written = Gsum, True

    def _plan_dgrad(self, c, G, q, lvl_n):
        """Data gradient into the conv input, in the first of these forms that applies: with the weight gradient (solo), over a compact
        gradient, as a fused backward pair, as a Dense head of a shared launch, or as a plain (possibly scattered) launch."""
        node = c.node
        if c.dgrad_done_by_pair or node.stem or not self.grad_needed[c.src.spec.id]:
            return                                 # (dgrad_done_by_pair: written by the fused launch of the layer above, _dgrad_pair)
        B, dt = self.B, self.dt
        X = c.src
        add = X.grad if X.grad_written else X.pending
        if c.solo:
            assert add is None
            dstg = X.grad_buf()
            self.bwd_ops.append(_Launch(lambda c=c, G=G, X=X, dstg=dstg, Ms=B * node.dst.h * node.dst.w:
                                        hip.conv_dgrad_wgrad_pw(Ms, dt, G, c.wd, X.data, X.spec.relu, dstg, c.wg_ws, c.wg_ws[c.wg_npart:],
                                                                c.K_raw * c.npad + hip.WGRAD_PART_PAD),
                                        "dgrad+wgrad", "dgrad+wgrad:" + node.name, dgrad=(node.name,), wgrad=(node.name,), done=(node.name,)))
            X.grad_written = True
            return
        if X.compact is not None:
            self._dgrad_compact(c, G, X)
            return
        A = self.pair_first.get(node.name)         # this layer is the second of a fused forward pair (A = the block-closing 2c)
        if (A is not None and X.spec.relu and X.bits is not None and X.pending is not None and not X.grad_written and
                self.grad_needed[A.src.spec.id] and A.src.spec.relu and A.src.bits is None and not A.src.grad_written and A.src.pending is None):
            self._dgrad_pair(c, A, G, X, add)
            return
        assert X.pending_hw is None or X.grad_written, "compact residual gradient reached a non-fused data gradient (%s)" % node.name
        dstg = X.grad_buf()
        mask = (X.bits if X.bits is not None else X.data) if X.spec.relu else None
        mflag = hip.EPI_MASK_BITS if (X.spec.relu and X.bits is not None) else 0
        if lvl_n is not None and mflag == 0 and not c.gd_scatter and self._dense_multi_ok(c):
            q.add_dense_dgrad(dict(names=(node.name,), level=lvl_n, src0=G, wgt0=c.wd, K0=c.npad, N=node.cin, M=B, add=add, mask=mask, dst=dstg, flags=0))
            X.grad_written, X.pending = True, None
            return
        if c.gd_scatter:
            if add is None:
                self._clear_scattered_dgrad(c, X, dstg)
            elif add is not dstg:
                raise AssertionError("scattered dgrad into %s needs an in-place accumulate" % node.name)
        self._emit_dgrad(lambda c=c, G=G, add=add, mask=mask, dstg=dstg, mflag=mflag:
                         hip.conv_igemm_ex(c.gd, dt, mflag, G, c.wd, None, add, mask, dstg, None,
                                           self.halo_ws if (c.halo_d and add is None and not mflag) else (self.igemm_ws if c.ws_d else None)), (node.name,))
        X.grad_written, X.pending = True, None

    def _emit_dgrad(self, run, dgrad, wgrad=()):
        """A data-gradient launch of the layers `dgrad` that also writes the weight-gradient partials of the layers `wgrad` (a tail of dgrad)."""
        label = "dgrad:" + "+".join(dgrad) + ("+wgrad:" + "+".join(wgrad) if wgrad else "")
        self.bwd_ops.append(_Launch(run, "dgrad", label, dgrad=dgrad, wgrad=wgrad))
        return self.bwd_ops[-1]

    def _dgrad_compact(self, c, G, X):
        """Stride-2 pointwise consumer of a block output whose gradient is kept compact: a plain pointwise GEMM over the
        sampled pixels (no scatter, no zero fill of a dense tensor), masked with the sampled rows of X's ReLU bit mask."""
        B, dt, node = self.B, self.dt, c.node
        if not X.grad_written and not X.fwd_sampled:          # (a sampled block output wrote the compact mask in its forward pass)
            self.bwd_ops.append(_Launch(lambda X=X: hip.rows_subsample2(B, X.compact[0], X.compact[1], X.spec.c // 8, X.bits, X.bits_compact),
                                        "bits_subsample"))
        gq = c.gd_compact
        first = X._compact_first
        if (first is not None and X.grad_written and
                hip.conv_pointwise2_ok(B, gq.OH, gq.OW, first[1].npad, c.npad, node.cin, dt, hip.EPI_MASK_BITS)):
            # the SECOND stride-2 consumer of X (a stage's first block: the projection shortcut and branch2a, net.py:121-126, 148-157):
            # both data gradients in ONE launch with two reduction segments (urso_conv_pointwise2) -- dL/dX is written once and
            # rounded once instead of written by the first launch, read back and rewritten by this one.  The first launch leaves
            # the plan (its operands -- the block output's gradient, its filter -- outlive it: every tensor has its own gradient
            # buffer); the sum runs in the same order (shortcut first).
            launch0, c0, G0 = first
            self.bwd_ops.remove(launch0)
            self._emit_dgrad(lambda c=c, c0=c0, G0=G0, G=G, X=X, gq=gq, N=node.cin:
                             hip.conv_pointwise2(B, gq.OH, gq.OW, c0.npad, c.npad, N, dt, hip.EPI_MASK_BITS, G0, c0.wd, G, c.wd, None,
                                                 X.bits_compact, X.grad), (c0.name, node.name))
            X._compact_first = None
            self.n_entry_dgrad2 += 1
            return
        launch = self._emit_dgrad(lambda c=c, G=G, X=X, add=(X.grad if X.grad_written else None):
                                  hip.conv_igemm_ex(c.gd_compact, dt, hip.EPI_MASK_BITS, G, c.wd, None, add, X.bits_compact, X.grad, None, None),
                                  (node.name,))
        X._compact_first = (launch, c, G) if not X.grad_written else None       # (None: a third writer, no merge)
        X.grad_written = True

    def _dgrad_pair(self, c, A, G, X, add):
        """Data gradient of this layer into X (+ residual gradient, ReLU bit mask) and, from the LDS copy of that result,
        the data gradient of layer A into ITS input: X.grad crosses HBM once (conv_pair.hip)."""
        dt, node = self.dt, c.node
        dstg, dst2 = X.grad_buf(), A.src.grad_buf()
        a_tr = self.layer_trainable[A.name] or bool(A.node.bn and not A.batch_bn and self.layer_trainable[A.node.bn])
        wsplits = hip.conv_pair_wgrad_splits(A.Mpix, dt) if (A.node.cin == 64 and hip.get_option("pair") == 1) else 0
        if a_tr and wsplits > 1 and A.gf_compact is None:
            # ... and, stage 2, the weight gradient of layer A as well: both of its operands (X.grad, A's input) are in
            # LDS in that launch (conv_pairw.hip); one fp32 partial per block lands in A's split workspace, allocated
            # when the loop reaches A -- its reduction and finalisation stay where they are
            A.splits = A.desc.splits = wsplits
            A.wgrad_by_pair = True
            Sc = self._pair_entry_shortcut(A, X)
            if Sc is not None:
                # the stage's first block: X's gradient is read by nothing but this pair and the projection shortcut (A's residual
                # operand, a conv without activation): its data and weight gradient join the launch and dL/dX stays on chip
                Sc.splits = Sc.desc.splits = wsplits
                Sc.wgrad_by_pair = Sc.dgrad_done_by_pair = True
                dxin = Sc.src.grad_buf()
                Sc.src.grad_written = True
                dstg.zero_()                   # dL/dX never reaches memory in this form: the buffer stays what it is (zeros, not whatever the allocator left)
                dstg._urso_on_chip = True      # (tests/test_layerwise_gpu.py skips what it cannot read; the shortcut's gradient aliases this buffer)
                self._emit_dgrad(lambda c=c, A=A, Sc=Sc, G=G, add=add, X=X, dst2=dst2, dxin=dxin:
                                 hip.conv_pair_wgrad_entry(A.Mpix, dt, G, c.wd, add, X.bits, A.wd, A.src.data, dst2, Sc.wd, Sc.src.data, Sc.src.spec.relu, dxin,
                                                           A.wg_ws, A.wg_ws[A.wg_npart:], Sc.wg_ws, Sc.wg_ws[Sc.wg_npart:],
                                                           A.K_raw * A.npad + hip.WGRAD_PART_PAD), (node.name, A.name, Sc.name), (A.name, Sc.name))
            else:
                self._emit_dgrad(lambda c=c, A=A, G=G, add=add, X=X, dstg=dstg, dst2=dst2, hw=X.pending_hw:
                                 hip.conv_pair_wgrad(A.Mpix, dt, G, c.wd, add, X.bits, dstg, A.wd, A.src.data, dst2,
                                                     A.wg_ws, A.wg_ws[A.wg_npart:], A.K_raw * A.npad + hip.WGRAD_PART_PAD, add_hw=hw),
                                 (node.name, A.name), (A.name,))
        else:
            self._emit_dgrad(lambda c=c, A=A, G=G, add=add, X=X, dstg=dstg, dst2=dst2, hw=X.pending_hw:
                             hip.conv_pair(A.Mpix, A.node.cin, dt, 1, G, c.wd, None, add, X.bits, dstg, A.wd, None, A.src.data, dst2,
                                           add_hw=hw), (node.name, A.name))
        X.grad_written, X.pending = True, None
        A.src.grad_written = True
        A.dgrad_done_by_pair = True

    def _pair_entry_shortcut(self, A, X):
        """The projection shortcut whose data and weight gradient can join A's fused backward pair (conv_pairw.hip's entry form), or None."""
        S = [cc for cc in self.convs.values() if A.res is not None and cc.dst is A.res]
        Sc = S[0] if len(S) == 1 else None
        if Sc is None:
            return None
        sn = Sc.node
        entry = (X.pending_hw is None and not sn.stem and not sn.dense and sn.kh == 1 and sn.kw == 1 and
                 sn.stride == 1 and sn.cin == 64 and Sc.npad == 256 and Sc.N == 256 and not Sc.batch_bn and not sn.relu and
                 (self.layer_trainable[sn.name] or bool(sn.bn and self.layer_trainable[sn.bn])) and
                 self.grad_needed[Sc.src.spec.id] and Sc.src.compact is None and not Sc.gd_scatter and
                 Sc.gf_compact is None and not Sc.src.grad_written and Sc.src.pending is None and
                 sn.name not in self._last_of_group and self.pair_first.get(sn.name) is None)
        return Sc if entry else None

    def _clear_scattered_dgrad(self, c, X, dstg):
        """First (and only) contribution of a scattered data gradient: everything off the sampled grid is zero -- and STAYS zero: the
        scattered data gradient writes nothing but the sampled pixels, the tensor has a gradient buffer of its own and no other launch
        writes it, so the buffer is cleared ONCE, here, instead of by a fill launch in every step (rounds 2-4: three launches, 33 us per
        cfg2 step, 150 MB written for nothing)."""
        g = self.graph
        dstg.zero_()
        # (only when EVERY launch that writes this buffer is such a scattered data gradient: a dense one accumulating in place
        # behind this one would leave its values off the grid for the next step to find)
        writers = [cc for cc in self.convs.values() if cc.src is X and cc.gd is not None]
        once = (all(cc.gd_scatter for cc in writers) and not any(cc.res is X for cc in self.convs.values())
                # ... nor a max-pool reading X (urso_maxpool_bwd writes X.grad densely) or X being a network output
                and not any(n.op == "pool" and n.src.id == X.spec.id for n in g.nodes)
                and not any(t.id == X.spec.id for t in g.outputs.values()))
        if not once:
            self.bwd_ops.append(_Launch(lambda t=dstg: hip.zero_fill(t), "zero", "zero:" + c.name))
        else:
            # URSO_CHECK_CLEARED=1 (debugging; check_cleared_once()): the pixels no step writes must still be zero after any
            # number of steps -- a tool that writes gradient buffers (teacher-forced tests, dumps) would break that silently
            st = c.gd_scatter_stride
            self._cleared_once.append((c.name, dstg, X.spec.h, X.spec.w, X.spec.c, st, st))

    # ---------------------------------------------------------------- tail
    _BUCKET_PHASES = OrderedDict((("reduce", hip.PB_REDUCE), ("finalize_mat", hip.PB_FINALIZE_MAT), ("finalize_vec", hip.PB_FINALIZE_VEC)))

    def _resolve_bucket_ops(self):
        """The descriptor table is complete: upload it, plan the block maps and resolve the batched placeholders of the buckets (each
        finalisation block of a fused-norm plan gets a slot of sqpart for the sum of squares of what it stores)."""
        dt = self.dt
        self._upload_param_table()
        for launch in [l for l in self.bwd_ops if l.run is None]:
            ph, k = self._BUCKET_PHASES[launch.kind], launch.bucket
            nb_ = self.pbatch.plan(ph, k, [self.convs[nm].desc_id for nm in self._bucket_groups[k]])
            if nb_ == 0:
                self.bwd_ops.remove(launch)                    # nothing to launch (e.g. no split layer in the bucket)
            elif self.fused_sqnorm and ph in (hip.PB_FINALIZE_MAT, hip.PB_FINALIZE_VEC):
                s0 = self._sq_slots
                s1 = self._sq_slots = s0 + nb_
                launch.run = (lambda ph=ph, k=k, s0=s0, s1=s1: self.pbatch.run(ph, k, dt, sqpart=self.sqpart[s0:s1], ls=self.ls_state))
            else:
                launch.run = (lambda ph=ph, k=k: self.pbatch.run(ph, k, dt, ls=self.ls_state))
        n_sq = self._sq_slots + (1 if self.learn_lw and self.layer_trainable[loss_weights.LAYER] else 0)       # + the loss weights' slot (_plan_optimizer)
        self.sqpart = torch.zeros(max(n_sq, 1), dtype=torch.float32, device=self.device) if self.fused_sqnorm else None

    def _plan_optimizer(self):
        cfg, dev = self.config, self.device
        n = self.n_flat
        self.adam = str(getattr(cfg, "OPTIMIZER", "SGD")).upper() != "SGD"          # net.py:979-983: anything else is Adam(amsgrad)
        clip = float(cfg.GRADIENT_CLIP_NORM or 0.0)
        # hyper-parameters live in device memory so that one captured graph serves a changing learning rate; they are created ONCE:
        # a later set_trainable() (which rebuilds the plan) must not undo compile(lr) / set_lr() (net.py:1073-1075 calls them in
        # either order)
        if self.adam:
            eps = 1e-4 if getattr(cfg, "F16", False) else 1e-7                      # K.epsilon(); net.py:590-593 sets 1e-4 in F16 mode
            if self.hyper is None or self.hyper.numel() != 8:
                self.hyper = torch.tensor([float(cfg.LEARNING_RATE), 0.9, 0.999, eps, clip, 0.0, 1.0 - 0.9, 1.0 - 0.999],
                                          dtype=torch.float32, device=dev)
            if self.flat_v2 is None or self.flat_v2.numel() != self.flat_w.numel():
                self.flat_v2, self.flat_vhat = torch.zeros_like(self.flat_w), torch.zeros_like(self.flat_w)
        elif self.hyper is None or self.hyper.numel() != 3:
            self.hyper = torch.tensor([float(cfg.LEARNING_RATE), float(cfg.LEARNING_MOMENTUM), clip], dtype=torch.float32, device=dev)
        self.normsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sq_ws = torch.empty(hip.sqnorm_ws_bytes(n) // 4, dtype=torch.float32, device=dev)
        if self.accum_k > 1:
            # Config.GRAD_ACCUM_STEPS: a micro-step that does not close ends in ONE launch behind the backward pass (acc = g | acc += g: the
            # role of the micro-step that runs, which a captured graph freezes); the closing one begins its optimizer with g = (acc + g) * c,
            # whose blocks leave the slots of the fused norm -- over all of flat_g, the loss weights' and BN's slices included
            c = float(grad_accum.inv32(self.accum_k))
            self.sqpart = torch.zeros(hip.grad_accum_parts(n), dtype=torch.float32, device=dev)
            self.accum_ops.append(_Launch(lambda: hip.grad_accum(n, self.flat_g, self.flat_acc, self._accum_role == "first"), "grad_accum"))
            self.opt_ops.append(_Launch(lambda: hip.grad_accum_close(n, self.flat_g, self.flat_acc, c, self.sqpart), "grad_close"))
            self.opt_ops.append(_Launch(lambda: hip.sqnorm_final(self.sqpart, self.normsq), "sqnorm"))
        elif self.fused_sqnorm:
            if self.learn_lw and self.layer_trainable[loss_weights.LAYER]:
                # the two log-variances' gradients are written by the losses, not by a finalisation block: their squares reach the fused norm
                # through one more slot of sqpart, the last one, filled by a squared norm over the layer's 8 floats of flat_g (padding is zero).
                # The slot order is fixed, so a replay adds in the same order every time.
                o, slot = self.slices[(loss_weights.LAYER, "ori_weight")][0], self._sq_slots
                assert self.slices[(loss_weights.LAYER, "loc_weight")][0] == o + 4 and self.sqpart.numel() == slot + 1
                self.opt_ops.append(_Launch(lambda: hip.sqnorm(8, self.flat_g[o:o + 8], self.sq_ws, self.sqpart[slot:slot + 1]), "sqnorm_lw"))
            self.opt_ops.append(_Launch(lambda: hip.sqnorm_final(self.sqpart, self.normsq), "sqnorm"))
        else:
            self.opt_ops.append(_Launch(lambda: hip.sqnorm(n, self.flat_g, self.sq_ws, self.normsq), "sqnorm"))
        self.lars_plan, self.lamb_plan = None, None
        lars_keys = lars.validate(cfg, self.world_size)            # (eta, eps, clip mode) | None; refuses Adam, so the branch below is SGD's
        lamb_keys = lamb.validate(cfg, self.world_size)            # the same; refuses SGD and LARS, so its branch is Adam's
        if lars_keys is not None:
            # Config.LARS: behind the global norm, the per-chunk sums of w^2 and g^2 and the per-tensor trust ratios; where the plain SGD
            # launch stands, the update with each tensor's trust.  One tensor per slice; kernels (>= 2 dimensions) adapt, the rest has trust 1.
            # The block map is uploaded here, once per plan; a frozen layer's gradient is zero, so its trust is 1 and its v stays 0
            eta, eps, clip_mode = lars_keys
            lp = self.lars_plan = hip.LarsPlan([(o, cnt, lars.adapts(shape)) for (o, cnt, shape) in self.slices.values()], dev)
            self.opt_ops.append(_Launch(lambda: lp.norms(self.flat_w, self.flat_g), "lars_norms"))
            self.opt_ops.append(_Launch(lambda: lp.trust_ratios(self.hyper, self.normsq, eta, eps, clip_mode, ls=self.ls_state), "lars_trust"))
            self.opt_ops.append(_Launch(lambda: lp.sgd(self.flat_w, self.flat_g, self.flat_v, self.hyper, self.normsq, ls=self.ls_state),
                                        "lars_sgd"))
        elif lamb_keys is not None:
            # Config.LAMB: where the plain Adam launch stands, the tick and the moments with the per-chunk sums of w^2 and r^2, the per-tensor
            # trust ratios, and the update with each tensor's trust.  Tensors and block map as under LARS; flat_v is m, flat_v2 is v
            eta_l, eps_l, clip_l = lamb_keys
            bp = self.lamb_plan = hip.LambPlan([(o, cnt, lamb.adapts(shape)) for (o, cnt, shape) in self.slices.values()], dev)
            if self.lamb_state is None:                                      # created once, like hyper (a rebuilt plan keeps the tick's state)
                self.lamb_state = bp.state
            bp.state = self.lamb_state
            self.opt_ops.append(_Launch(lambda: bp.moments(self.flat_w, self.flat_g, self.flat_v, self.flat_v2, self.flat_vhat, self.hyper,
                                                           self.normsq, ls=self.ls_state), "lamb_moments"))
            self.opt_ops.append(_Launch(lambda: bp.trust_ratios(self.normsq, eta_l, eps_l, clip_l, ls=self.ls_state), "lamb_trust"))
            self.opt_ops.append(_Launch(lambda: bp.apply(self.flat_w, self.flat_v, self.flat_vhat, self.hyper, self.normsq, ls=self.ls_state),
                                        "lamb_apply"))
        elif self.adam:
            self.opt_ops.append(_Launch(lambda: hip.adam_amsgrad_clip(n, self.flat_w, self.flat_g, self.flat_v, self.flat_v2, self.flat_vhat,
                                                                      self.hyper, self.normsq, ls=self.ls_state), "adam"))
        else:
            self.opt_ops.append(_Launch(lambda: hip.sgd_momentum_clip(n, self.flat_w, self.flat_g, self.flat_v, self.hyper, self.normsq,
                                                                      ls=self.ls_state), "sgd"))
        if self.ls_state is not None:                  # after the optimizer: all of its blocks have read the norm and the state
            self.opt_ops.append(_Launch(lambda: hip.loss_scale_update(self.ls_state, self.normsq), "loss_scale"))
        if self.ema_state is not None:                 # last: behind the optimizer, and behind loss_scale so that LAST_SKIPPED is this step's
            self.opt_ops.append(_Launch(lambda: hip.ema_update(n, self.flat_w, self.flat_ema, self.ema_state, ls=self.ls_state), "ema"))
        if self.swa_state is not None:                 # Config.SWA: the very last, for the same reason; its gate is shut on most steps
            self.opt_ops.append(_Launch(lambda: hip.swa_update(n, self.flat_w, self.flat_swa, self.flat_swa_sq, self.swa_state, ls=self.ls_state),
                                        "swa"))

    def _plan_sam(self):
        """Config.SAM (ursonet_amd/sam.py): the three launches of the doubled chain.  Where `prep, forward, losses + backward` stand, the step
        (each micro-step) runs them at w, then sam_norm (the unfused squared norm of ALL of flat_g into sam_state) and sam_ascend (w0 = w,
        w += s g1), then the same launches again at w + e, then sam_descend (w = w0); the optimizer's launches follow unchanged, on g2.
        What the second pass must not leave behind: its losses go into sam_loss instead of loss_buf (the loss launches take their slot of
        whichever buffer self.loss_buf names when they run: _run_passes), and in batch-statistics BN mode the moving statistics of pass 1 are
        kept aside by a device-to-device copy behind the ascent and put back behind the way back.
        Under LOSS_SCALE one thread more, behind the optimizer's norm: a step that the optimizer skips takes its ascents out of applied_total."""
        keys = sam.validate(self.config, self.world_size)
        self.sam_ops = []
        if keys is None:
            self.sam_state = self._sam_keys = self.flat_w0 = self.sam_loss = self.sam_stats = None
            return
        dev, n = self.device, self.n_flat
        if self.sam_state is None:                     # created once, like hyper: a re-plan keeps the counts and set_sam_rho()
            self.sam_state = torch.tensor(sam.initial_state(*keys), dtype=torch.float32, device=dev)
        elif keys != self._sam_keys:                   # the keys changed between plans
            self.sam_state[sam.RHO], self.sam_state[sam.EPS] = keys
        self._sam_keys = keys
        if self.flat_w0 is None:
            self.flat_w0 = torch.zeros_like(self.flat_w)
        self.sam_loss = torch.zeros_like(self.loss_buf)                    # L(w + e), slot for slot as loss_buf
        self.sam_stats = torch.zeros_like(self.flat_stats) if self.train_bn else None
        hip.side_lib("train")                          # a missing library is an error here, not at the first step
        nsq = self.sam_state[sam.NORMSQ:sam.NORMSQ + 1]
        sam_ws = torch.empty_like(self.sq_ws)          # (a workspace of its own: nothing of the optimizer's norm is shared)

        def ascend():
            hip.sam_ascend(n, self.flat_w, self.flat_g, self.flat_w0, self.sam_state)
            if self.sam_stats is not None:
                self.sam_stats.copy_(self.flat_stats)

        def descend():
            hip.sam_descend(n, self.flat_w, self.flat_w0)
            if self.sam_stats is not None:
                self.flat_stats.copy_(self.sam_stats)
        self.sam_ops = [_Launch(lambda: hip.sqnorm(n, self.flat_g, sam_ws, nsq), "sam_norm"), _Launch(ascend, "sam_ascend"),
                        _Launch(descend, "sam_descend")]
        if self.ls_state is not None:
            at = [l.kind for l in self.opt_ops].index("sqnorm") + 1
            self.opt_ops.insert(at, _Launch(lambda: hip.sam_settle(self.sam_state, self.normsq, True), "sam_settle"))

    def _fork_weight_gradients(self):
        """Weight-gradient launches are leaves of the backward pass: nothing reads their partials before the bucket's reduction, every tensor
        has a gradient buffer of its own and nothing later overwrites what they read.  So they may run LATER than where they stand in the
        chain, and beside it: on a second stream, captured into the same hipGraph as a branch.
        What pays (tools/probes/overlap_probe.py, profiles/r05_overlap_probe.txt): an HBM-bound chain and an MFMA-bound chain side by side
        finish 9-12 % sooner than one after the other; two chains of the same kind only get in each other's way (every grid is a static
        partition of its tiles over all 256 CUs, and a block that finds its CU held by the other launch runs behind it).  Hence the
        COMPLEMENTARY fork (URSO_WGRAD_STREAM=2; the default until round 5, opt-in since): only the arithmetic-heavy weight gradients (>= 150 FLOP per byte: stages 4-5,
        the 3x3 layers of stage 3, bottleneck_layer, the heads) leave the chain, and those whose dz is final before the data gradients reach
        stage 3 are DEFERRED to that point, where the chain turns HBM-bound (stage-3 / stage-2 data gradients and weight gradients).  Join =
        the bucket's reduction.  cfg2, alternating in one gpurun call: 7.13 -> 6.97 ms (-2.1 %), bit-identical to the single chain (same
        kernels, same operands; tests/test_model_gpu.py).  Any other value of URSO_WGRAD_STREAM keeps the single chain.  Plans whose buckets are finalised inside the backward pass (data-parallel
        runs: ursonet_amd/dp.py) keep the single chain -- a deferred launch would land behind its bucket's finalisation.
        One edge per fork: the side stream waits for the chain only when the chain has moved since the last side launch.  A captured graph in
        which twenty side nodes each carried their own (redundant) edge from the same chain node ran the chain node BEHIND that fan before
        its predecessors (stale operands from the previous replay; ROCm 7.2, profiles/r05_fork.txt) -- eager streams did not."""
        self.wgrad_stream = None
        self._single_chain_always = False
        self._graph_events = []
        # OPT-IN since round 6: hipGraphLaunch of a forked graph segfaulted inside the ROCm 7.2 runtime in a long-lived process (a pytest
        # run, after ~22 engines of various sizes had come and gone; reproducible for that sequence, gone with URSO_WGRAD_STREAM=0, not cured by
        # keeping the capture's events alive) -- a failure no verification can turn into a fallback.  bench.py opts in (a fresh process: the
        # same path has run hundreds of times there without incident, and it checks the fork against the chain first); the tests of the fork
        # run in processes of their own (tests/workers/fork_worker.py).
        if self._env_wgrad_stream != 2 or self.mode != "training" or self.no_wgrad_fork:       # (no_wgrad_fork: set by ursonet_amd/dp.py)
            return
        if self.ls_state is not None:
            return                           # loss scaling: the forked capture is not supported, the step stays on the single chain
        if self.accum_k > 1:
            return                           # gradient accumulation: likewise (one graph per role)
        if self.sam_ops:
            return                           # SAM: likewise (two backward passes in one graph)
        ops = self.bwd_ops
        fin = ("reduce", "finalize_mat", "finalize_vec", "finalize", "unpack")
        if any(c.batch_bn for c in self.convs.values()):
            return                           # batch-statistics BN: the chain is HBM-bound passes end to end; measured 17.05 -> 17.42 ms with the fork
        es = 4 if self.dt == hip.F32 else 2

        def work(name, back=False):          # (FLOP, bytes) of a layer's weight gradient (back: of its data gradient): operands once, result once
            c = self.convs.get(name)
            g = c.gf if c is not None else None
            if g is None:
                return 0.0, 0.0              # heads: small, latency-bound
            m_out, m_in, k = g.B * g.OH * g.OW, g.B * g.H * g.W, g.KH * g.KW * g.C
            return 2.0 * m_out * k * g.N, (m_in * g.C + m_out * g.N) * es + (es if back else 4.0) * k * g.N

        def totals(l, back=False):          # over the layers of the launch: its data gradients, then its weight gradients
            fl = by = 0.0
            for n in l.dgrad + l.wgrad:
                f, b = work(n, back)
                fl += f; by += b
            return fl, by

        def est_ms(l):                       # what the launch takes at the rates launches of its kind reach here (1.0 PFLOP/s, 4.5 TB/s)
            fl, by = totals(l, bool(l.dgrad))
            return max(fl / 1.0e12, by / 4.5e9)

        def intensity(l):
            fl, by = totals(l)
            return fl / by if by else 1e9

        def wg(l):
            return l.kind in ("wgrad", "wgrad_heads")
        # the deferral point: the first data-gradient launch (plain or fused pair) whose first layer belongs to stage 2 or 3
        at = next((i for i, l in enumerate(ops) if l.kind == "dgrad" and l.dgrad[0][:4] in ("res2", "res3")), None)
        if at is None:
            return
        EARLY, LATE = 150.0, 400.0           # FLOP per byte (swept 50 ... 300 / 250 ... none: 6.93 ... 6.98 ms, nothing to choose between them)
        # the HBM-bound stretch of the chain behind the deferral point, and as much arithmetic-heavy weight-gradient work as fits beside it (1.2 x
        # its estimate: cfg4, ResNet-101 at batch 16, has more such work than stretch -- 0.4 / 0.8 / 1.2 / 2.0: 8.48 / 8.37 / 8.33 / 8.33 ms, chain 8.49):
        # the LAST such launches in front of the point (the others stay where they are, on the chain)
        room = 1.2 * sum(est_ms(l) for l in ops[at:] if l.kind in ("dgrad", "wgrad") and not (wg(l) and intensity(l) >= LATE))
        early = []
        for l in reversed(ops[:at]):
            if wg(l) and (l.kind == "wgrad_heads" or intensity(l) >= EARLY):
                room -= est_ms(l)
                if room < 0:
                    break
                early.append(l)
        early.reverse()
        if not early or any(l.kind in fin for l in ops[ops.index(early[0]):at]):
            return                           # nothing to defer, or a bucket is finalised inside the region: the chain stays as it is
        side = early + [l for l in ops[at:] if wg(l) and intensity(l) >= LATE]      # (behind the point: 3x3 layers of >= 128 channels)
        self.bwd_ops = [l for l in ops[:at] if l not in early] + early + ops[at:]
        self.wgrad_stream = _side_stream(self.device)
        self._side_open = False
        self._main_moved = True
        self._single_chain = False

        def on_side(op):
            def run():
                if self._single_chain or self._single_chain_always:
                    return op()
                main = torch.cuda.current_stream(self.device)
                if self._main_moved or not self._side_open:         # one edge per fork (see above)
                    self._stream_edge(main, self.wgrad_stream)
                    self._main_moved = False
                with torch.cuda.stream(self.wgrad_stream):
                    op()
                self._side_open = True
            return run

        def joined(op):
            def run():
                self._join_weight_gradients()
                self._main_moved = True
                return op()
            return run

        def on_main(op):
            def run():
                self._main_moved = True
                return op()
            return run
        for l in self.bwd_ops:
            l.run = (on_side if l in side else joined if l.kind in fin else on_main)(l.run)
        self.opt_ops[0].run = joined(self.opt_ops[0].run)

    def _stream_edge(self, src, dst):
        """dst waits for what src holds now.  Stream.wait_stream() records a temporary event and lets Python destroy it right away; while a
        stream is capturing, that event becomes part of the graph being built, and a hipGraph replay long after its events were destroyed is
        the one place this code base has seen hipGraphLaunch segfault (round 5: after ~20 dropped engines; round 6: after 22 tests of one
        process).  Events recorded during a capture therefore live as long as the engine that owns the graph."""
        ev = torch.cuda.Event()
        ev.record(src)
        dst.wait_event(ev)
        if torch.cuda.is_current_stream_capturing():
            self._graph_events.append(ev)

    def _join_weight_gradients(self):
        if self.wgrad_stream is not None and self._side_open:
            self._stream_edge(self.wgrad_stream, torch.cuda.current_stream(self.device))
            self._side_open = False

    def _plan_relu_bitmasks(self):
        """A post-ReLU tensor gets a bit mask (1/16 of its bytes) for the backward pass when the conv that produces it can
        emit one from its forward epilogue and every data-gradient pass into it can consume one (urso_conv_igemm_bits_ok);
        otherwise the tensor itself serves as the mask, as before."""
        dt = self.dt
        for X in self.acts.values():
            X.bits = None
            if not X.spec.relu or X.numel % 8:
                continue
            prod = [c for c in self.convs.values() if c.dst is X]
            cons = [c for c in self.convs.values() if c.src is X and c.gd is not None]
            if len(prod) != 1 or not cons or not prod[0].node.relu:
                continue
            P = prod[0]
            if P.batch_bn:
                continue                                   # its output is written by urso_bn_apply, which emits no bit mask: the tensor itself is the mask
            pw = lambda n: (not n.dense) and n.kh == 1 and n.kw == 1
            # ... or bottleneck_layer behind the trunk's last block: its parity-class data gradient (conv_bneck.hip) takes the bit mask too
            bn_ = lambda c: (hip.get_option("bneck") and not c.node.dense and c.node.kh == 3 and c.node.kw == 3 and c.node.stride == 2 and
                             c.npad == 32 and c.node.cin % 64 == 0 and not c.batch_bn)
            if not (pw(P.node) and P.node.stride == 1 and P.N % 32 == 0 and all(pw(c.node) or bn_(c) for c in cons)):
                continue
            # block outputs only (a producer WITH a residual): with pointwise consumers all of them run in the HBM-bound DMA kernel, where
            # the emission hides behind memory time (measured: +1 % on the cfg2 step, data gradient -0.17 ms, forward +0.12 ms)
            if P.res is None:
                continue
            if not hip.conv_igemm_bits_ok(P.gf, dt, P.fwd_flags, P.ws_f):
                continue
            if all(hip.conv_igemm_bits_ok(c.gd, dt, 0, c.ws_d) for c in cons):
                X.bits = torch.empty(X.numel // 8, dtype=torch.uint8, device=self.device)

    def _upload_param_table(self):
        self.pbatch = hip.ParamBatch(self._descs, self.device) if self._descs else None
        if self.pbatch is not None:
            self.pbatch.plan(hip.PB_PREP, "all", list(range(len(self._descs))))

    def _build_heads_io(self):
        cfg, B, dev = self.config, self.B, self.device
        self.quat_head = bool(cfg.REGRESS_ORI and cfg.ORIENTATION_PARAM == "quaternion" and not cfg.REGRESS_KEYPOINTS)
        if self.quat_head:
            self.q_out = torch.zeros(B, 4, dtype=torch.float32, device=dev)
            if self.mode == "inference":
                x = self.out_ori
                self.fwd_ops.append(_Launch(lambda: hip.absdot(B, 4, 8, 1, None, x.data, 1.0, self.dt, self.q_out, None, None), "quat"))

    def _build_losses(self):
        cfg, g, B, dt, dev = self.config, self.graph, self.B, self.dt, self.device
        lw = cfg.LOSS_WEIGHTS
        self.loss_buf = torch.zeros(4, dtype=torch.float32, device=dev)       # loc_loss, ori_loss, k2_loss, k3_loss (weighted)
        self.rel_norms = torch.zeros(2, dtype=torch.float32, device=dev)
        loc, ori = self.out_loc, self.out_ori
        nloc = g.outputs["loc"].c
        nori = g.outputs["ori"].c if "ori" in g.outputs else 0
        self.row_ws = torch.empty(B, dtype=torch.float32, device=dev)
        if cfg.REGRESS_KEYPOINTS:
            # experimental keypoint mode (net.py:657-659): three MSE losses on k1 (=loc), k2, k3
            self.gt_loc = torch.zeros(B, 3, dtype=torch.float32, device=dev)
            self.gt_ori = torch.zeros(B, 3, dtype=torch.float32, device=dev)      # input_gt_k2
            self.gt_k3 = torch.zeros(B, 3, dtype=torch.float32, device=dev)
            for key, gt, wname, li in (("k1", self.gt_loc, "loc_loss", 0), ("k2", self.gt_ori, "k2_loss", 2), ("k3", self.gt_k3, "k3_loss", 3)):
                a = self.acts[g.outputs[key].id]
                gzt = torch.empty(a.numel, dtype=self.tdt, device=dev)
                a.grad, a.grad_written = gzt, True
                self.loss_ops.append(_Launch(lambda a=a, gt=gt, w=float(lw.get(wname, 1.)), li=li, gzt=gzt:
                                             hip.mse(B, 3, 8, gt, a.data, w, dt, self.loss_buf[li:li + 1], gzt, ls=self.ls_state), "loss"))
            return
        if (not cfg.REGRESS_LOC and nloc % 8) or (not cfg.REGRESS_ORI and nori % 8):
            raise ValueError("classification heads need a bin count that is a multiple of 8 (got %d / %d)" % (nloc, nori))
        # location head
        gz_loc = torch.empty(loc.numel, dtype=self.tdt, device=dev)
        loc.grad, loc.grad_written = gz_loc, True
        wl = float(lw.get("loc_loss", 1.))
        lw_loc, lw_ori = self._lw_views("loc_weight"), self._lw_views("ori_weight")      # None: LEARNABLE_LOSS_WEIGHTS off, the plain launches
        if cfg.REGRESS_LOC:
            self.gt_loc = torch.zeros(B, 3, dtype=torch.float32, device=dev)
            self.rel_exact = bool(getattr(cfg, "DP_EXACT_REL_LOSS", False))
            if self.rel_exact:
                # exact global batch-Frobenius ratio under data parallelism: norms -> (dp.py sum-all-reduces them) -> loss + gradient;
                # rel_scale = world size (1 on a single GPU, where the two phases reproduce the one-kernel loss)
                if self.rel_scale is None:
                    self.rel_scale = torch.ones(1, dtype=torch.float32, device=dev)
                self.loss_pre_ops.append(_Launch(lambda: hip.rel_l2_norms(B, 3, 8, self.gt_loc, loc.data, self.rel_norms), "loss"))
                self.loss_ops.append(_Launch(lambda: hip.rel_l2_from_norms(B, 3, 8, self.gt_loc, loc.data, wl, self.rel_scale, dt, self.rel_norms,
                                                                           self.loss_buf[0:1], gz_loc), "loss"))
            else:
                self.loss_ops.append(_Launch(lambda: hip.rel_l2(B, 3, 8, self.gt_loc, loc.data, wl, dt, self.loss_buf[0:1], gz_loc, self.rel_norms,
                                                                ls=self.ls_state, lw=lw_loc), "loss"))
        else:
            self.gt_loc = torch.zeros(B, nloc, dtype=torch.float32, device=dev)
            self.loss_ops.append(_Launch(lambda: hip.softmax_xent(B, nloc, loc.data, self.gt_loc, wl, 1, dt, self.loss_buf[0:1], gz_loc, self.row_ws,
                                                                  ls=self.ls_state, lw=lw_loc), "loss"))
        # orientation head
        gz_ori = torch.empty(ori.numel, dtype=self.tdt, device=dev)
        ori.grad, ori.grad_written = gz_ori, True
        wo = float(lw.get("ori_loss", 1.))
        if cfg.REGRESS_ORI:
            d = 4 if self.quat_head else 3
            self.gt_ori = torch.zeros(B, d, dtype=torch.float32, device=dev)
            qo = self.q_out if self.quat_head else None
            self.loss_ops.append(_Launch(lambda: hip.absdot(B, d, 8, 1 if self.quat_head else 0, self.gt_ori, ori.data, wo, dt, qo,
                                                            self.loss_buf[1:2], gz_ori, ls=self.ls_state, lw=lw_ori), "loss"))
        else:
            self.gt_ori = torch.zeros(B, nori, dtype=torch.float32, device=dev)
            self.loss_ops.append(_Launch(lambda: hip.softmax_xent(B, nori, ori.data, self.gt_ori, wo, 1, dt, self.loss_buf[1:2], gz_ori, self.row_ws,
                                                                  ls=self.ls_state, lw=lw_ori), "loss"))

    def _lw_views(self, wn):
        """(s, ds) of one learnable loss weight: one-element views into flat_w / flat_g (ds None while the layer is frozen: the loss is
        re-weighted by exp(-s), s gets no gradient and its slot of flat_g stays zero).  None when the feature is off."""
        if not self.learn_lw:
            return None
        o = self.slices[(loss_weights.LAYER, wn)][0]
        return self.flat_w[o:o + 1], (self.flat_g[o:o + 1] if self.layer_trainable[loss_weights.LAYER] else None)

    def _plan_compact_gradients(self, need):
        """A block output X whose only consumers are the stride-2 pointwise layers of the next stage's first block (net.py:121-126:
        branch2a and the shortcut conv) receives a gradient that is zero at three of every four pixels.  The dense tensor is never
        materialised: X.grad is [B, H/2, W/2, C] (the sampled pixels), and everything that reads it runs on that form --
          * the stride-2 layers' data gradients are plain pointwise GEMMs over the sampled pixels (no scatter, no 4x zero fill),
            masked by the sampled rows of X's ReLU bit mask (urso_rows_subsample2);
          * the weight gradient of X's producer is a stride-2 weight gradient (its forward input sampled at the same pixels);
          * the producer's own data gradient is the compact-scatter form (GEMM over the sampled pixels, zeros elsewhere), and the 3x3
            layer below it takes that tensor as a scattered dz operand: its weight gradient runs over the even pixels only;
          * the residual branch hands the compact tensor to the fused backward pair (urso_conv_pair, add_h / add_w).
        Where the residual side is not a fused pair (stages 4-5, pair option off) the dense form lives in a buffer zeroed once at
        planning; each step writes only its even pixels with urso_rows_scatter2 (_plan_residual_handover).
        URSO_COMPACT_GRAD=0 keeps the dense path everywhere."""
        g, dt, B, dev = self.graph, self.dt, self.B, self.device
        if dt == hip.F32 or not getattr(self.config, "COMPACT_GRADIENTS", True) or not self._env_compact_grad:
            return
        convs = list(self.convs.values())
        for X in self.acts.values():
            if X.bits is None or not X.spec.relu or X.spec.h % 2 or X.spec.w % 2 or not need.get(X.spec.id, False):
                continue
            prod = [c for c in convs if c.dst is X]
            cons = [c for c in convs if c.src is X]
            if len(prod) != 1 or not cons or any(c.res is X for c in convs) or any(n.op == "pool" and n.src.id == X.spec.id for n in g.nodes):
                continue
            A = prod[0]
            n = A.node
            if not (not n.stem and not n.dense and n.kh == 1 and n.kw == 1 and n.stride == 1 and A.res is not None and not A.batch_bn and
                    A.npad == A.N and A.res.spec.relu and need.get(A.src.spec.id, False) and A.src.spec.relu and A.src.bits is None):
                continue
            if not all((not c.node.dense) and c.node.kh == 1 and c.node.kw == 1 and c.node.stride == 2 and not c.batch_bn and
                       c.npad == c.N and tuple(c.node.pad) == (0, 0) for c in cons):
                continue
            # the residual gradient must land in a fused backward pair: the block's branch2a (consumer of A.res) is the second layer of
            # a fused forward pair, and A.res has no other consumer
            R = A.res
            rc = [c for c in convs if c.src is R]
            if len(rc) != 1 or sum(1 for c in convs if c.res is R) != 1:
                continue
            X.residual_needs_dense = self.pair_first.get(rc[0].name) is None or R.bits is None     # stages 4-5: scattered into a dense buffer (urso_rows_scatter2)
            H, W = X.spec.h, X.spec.w
            gd_ok = True
            for c in cons:
                c.gd_compact = hip.geom(B, H // 2, W // 2, c.npad, H // 2, W // 2, c.node.cin, 1, 1)
                gd_ok = gd_ok and hip.conv_igemm_bits_ok(c.gd_compact, dt, 0, 0)
            if not gd_ok:
                continue
            X.compact = (H, W)
            X.grad = torch.empty(X.numel // 4, dtype=self.tdt, device=dev)
            X.bits_compact = torch.empty(X.numel // 32, dtype=torch.uint8, device=dev)
            # producer: stride-2 weight gradient, compact-scatter data gradient
            A.gf_compact = hip.geom(B, H, W, n.cin, H // 2, W // 2, A.npad, 1, 1, 2, 2, 0, 0)
            A.splits = hip.conv_wgrad_splits(A.gf_compact, dt)
            A.desc.splits = max(A.splits, 1)
            A.gd = hip.geom(B, H // 2, W // 2, A.npad, H // 2, W // 2, n.cin, 1, 1, FH=H, FW=W, OSH=2, OSW=2)
            A.gd_scatter = True
            A.gd_scatter_stride = 2
            A.ws_d = 0
            # one layer further down: A's data gradient (dense tensor, zero off the even grid) is the dz of the layer that produced A's
            # input -- its weight gradient is the stride-2 one over the even pixels, reading dz in place (scattered dz operand)
            P = [c for c in convs if c.dst is A.src]
            if len(P) == 1 and not P[0].batch_bn and not P[0].node.stem and not P[0].node.dense and P[0].node.stride == 1:
                pn, Pc = P[0].node, P[0]
                pt, pl = pn.pad
                if pn.src.h == H and pn.src.w == W and (pn.kh > 1 or pn.kw > 1):
                    Pc.gf_compact = hip.geom(B, H, W, pn.cin, H // 2, W // 2, Pc.npad, pn.kh, pn.kw, 2, 2, pt, pl, FH=H, FW=W, OSH=2, OSW=2)
                    Pc.splits = hip.conv_wgrad_splits(Pc.gf_compact, dt)
                    Pc.desc.splits = max(Pc.splits, 1)
            self._sample_block_output(X)

    def _sample_block_output(self, X):
        """A block output that is only ever read through stride-2 pointwise layers (res{2c,3d,4f}_out of ResNet-50: net.py:121-126)
        is COMPUTED only at the pixels they read: its producing c -> 4c layer runs as a 1x1 / stride-2 layer over the even pixels with
        the identity shortcut read on the input grid (URSO_EPI_ADD_SRCGRID), writing the compact tensor the consumers take
        (X.data_compact) and -- training -- the compact ReLU bit mask directly; the dense tensor (335 MB in stage 2 of cfg2) and its bit
        mask are neither written nor read by anything.  Every value that any output, loss or gradient depends on is computed by the same
        arithmetic (bit-identical: tests/test_kernels_gpu.py::test_block_output_computed_at_the_sampled_pixels_only); what is skipped
        is dead.  Needs the compact-gradient plan in training (X.compact) so that the backward pass, too, reads only the compact forms.
        URSO_SAMPLED_OUTPUTS=0 keeps the dense tensor (e.g. to inspect intermediate activations)."""
        dt, B = self.dt, self.B
        if dt == hip.F32 or not self._env_sampled_outputs or X.data_compact is None:
            return
        convs = list(self.convs.values())
        prod = [c for c in convs if c.dst is X]
        cons = [c for c in convs if c.src is X]
        if len(prod) != 1 or not cons or any(c.res is X for c in convs) or any(c.xin is not X.data_compact for c in cons):
            return
        if any(n.op == "pool" and n.src.id == X.spec.id for n in self.graph.nodes) or any(t.id == X.spec.id for t in self.graph.outputs.values()):
            return
        A = prod[0]
        n = A.node
        training = self.mode == "training"
        if (n.stem or n.dense or n.kh != 1 or n.kw != 1 or n.stride != 1 or A.batch_bn or A.fwd is None or not A.fwd.computes_only(A, or_sampled_store=True) or n.cin % 64 or A.npad % 32 or
                A.npad != A.N or X.spec.h % 2 or X.spec.w % 2 or (A.res is not None and A.res.numel != X.numel)):
            return
        if training and (X.compact is None or X.bits is None or X.bits_compact is None):
            return                                    # the backward pass would read the dense tensor / bit mask
        H, W = X.spec.h, X.spec.w
        gs = hip.geom(B, H, W, n.cin, H // 2, W // 2, A.npad, 1, 1, 2, 2, 0, 0)
        flags = A.fwd_flags | (hip.EPI_ADD_SRCGRID if A.res is not None else 0) | (hip.EPI_EMIT_BITS if training else 0)
        A.fwd.run = (lambda A=A, X=X, gs=gs, flags=flags: hip.conv_igemm_ex(
            gs, dt, flags, A.xin, A.wf, A.biasf, A.res.data if A.res is not None else None, None, X.data_compact,
            X.bits_compact if (flags & hip.EPI_EMIT_BITS) else None))
        A.fwd.kind, A.fwd.label = "fwd@sampled", "fwd:%s@sampled" % A.name
        self._sample_layer_below(A, X)
        if X.gather is not None:                     # the gather pass that filled X.data_compact from the dense tensor (plans without the
            self.fwd_ops.remove(X.gather)            # register-filter kernel's second store) has nothing to read any more
            X.gather = None
        X.fwd_sampled = True

    def _sample_layer_below(self, A, X):
        """One layer further down: the 3x3 layer P whose output Y only feeds the sampled layer A (res{2c,3d,4f}_branch2b, net.py:143) is
        needed at the even pixels only as well -- A's forward pass, A's stride-2 weight gradient and the mask of A's compact-scatter data
        gradient all read Y at those pixels.  P runs as a 3x3 / stride-2 layer whose results are SCATTERED to the even pixels of the dense
        Y buffer (destination scatter of urso_conv_igemm): every reader finds its values where it always did, the other three quarters
        of the buffer are never written and never read.  P's own backward pass does not involve Y's values."""
        convs = list(self.convs.values())
        Y = A.src
        prod = [c for c in convs if c.dst is Y]
        if len(prod) != 1 or any(c.src is Y and c is not A for c in convs) or any(c.res is Y for c in convs) or Y.bits is not None:
            return
        if any(n.op == "pool" and n.src.id == Y.spec.id for n in self.graph.nodes) or Y.data_compact is not None:
            return
        P = prod[0]
        n = P.node
        H, W = X.spec.h, X.spec.w
        if (n.stem or n.dense or n.kh != 3 or n.kw != 3 or n.stride != 1 or tuple(n.pad) != (1, 1) or P.batch_bn or P.res is not None or n.cin % 64 or
                P.npad != P.N or n.src.h != H or n.src.w != W or n.dst.h != H or n.dst.w != W or P.xin is not P.src.data or
                not P.fwd.computes_only(P)):
            return
        gs = hip.geom(self.B, H, W, n.cin, H // 2, W // 2, P.npad, 3, 3, 2, 2, 1, 1, FH=H, FW=W, OSH=2, OSW=2)
        P.fwd.run = (lambda P=P, gs=gs: hip.conv_igemm_ex(gs, self.dt, P.fwd_flags, P.xin, P.wf, P.biasf, None, None, P.dst.data, None, None))
        P.fwd.kind, P.fwd.label = "fwd@sampled", "fwd:%s@sampled" % P.name
        Y.fwd_scattered = True

    def _stem_pool_node(self, g, node, c, dt):
        """The pool node the stem's kernel can compute as well (urso_stem_conv_pool), or None: the stem with its ReLU and a folded BN,
        read by nothing but ONE max-pool, in a 16-bit dtype on a geometry the kernel takes."""
        if not node.stem or not node.relu or c.batch_bn or c.res is not None or node.out_f32 or dt == hip.F32:
            return None
        if any(t.id == node.dst.id for t in g.outputs.values()) or (g.feat is not None and getattr(g.feat, "id", None) == node.dst.id):
            return None
        users = [n for n in g.nodes if n is not node and (n.src.id == node.dst.id or (n.op == "conv" and n.residual is not None and n.residual.id == node.dst.id))]
        if len(users) != 1 or users[0].op != "pool" or not hip.stem_conv_pool_ok(c.gf, dt):
            return None
        return users[0]

    def _dense_levels(self):
        """Dense head layers (net.py:288-352) -> depth behind the bottleneck features (1 = reads them)."""
        g, lv = self.graph, OrderedDict()
        prod = {n.dst.id: n for n in g.nodes if n.op != "pool"}
        for n in g.nodes:
            if n.op == "pool" or not n.dense:
                continue
            p = prod.get(n.src.id)
            lv[n.name] = lv[p.name] + 1 if (p is not None and p.name in lv) else 1
        return lv

    def _dense_multi_ok(self, c):
        n = c.node
        return bool(self.dense_multi and n.dense and not c.batch_bn and c.res is None and n.cin % 8 == 0 and c.npad % 8 == 0 and self.B <= 32)

    def _backward_order(self):
        """reversed(graph.nodes), with the Dense head layers taken depth by depth (both final layers, then both dense_0 layers ...) instead
        of branch by branch, so that the data gradients of one depth can share a launch (urso_dense_multi)."""
        nodes = list(reversed(self.graph.nodes))
        if not self.dense_multi:
            return nodes
        lv = self._dense_levels()
        idx = [i for i, n in enumerate(nodes) if n.op != "pool" and n.name in lv]
        if not idx or idx != list(range(idx[0], idx[0] + len(idx))):
            return nodes
        run = sorted(nodes[idx[0]:idx[-1] + 1], key=lambda n: -lv[n.name])        # stable: the branches keep their order inside a depth
        return nodes[:idx[0]] + run + nodes[idx[-1] + 1:]

    def _fuse_dense_heads(self):
        """Forward plan rewrite: the Dense layers of one depth behind the bottleneck features (loc_dense_0 + ori_dense_0, loc_final + ori_final;
        net.py:288-352) run side by side in one launch (urso_dense_multi: the same kernel body per layer, same results).  hip.options(dense=0)
        keeps one launch per layer."""
        self.dense_multi = self.dt != hip.F32 and bool(hip.get_option("dense"))
        if not self.dense_multi:
            return
        lv = self._dense_levels()
        convs = [self.convs[nm] for nm in lv]
        pos = [self.fwd_ops.index(c.fwd) if c.fwd is not None and c.fwd.computes_only(c) else -1 for c in convs]
        if (len(convs) < 2 or min(pos) < 0 or sorted(pos) != list(range(min(pos), min(pos) + len(pos))) or
                not all(self._dense_multi_ok(c) for c in convs)):
            self.dense_multi = False
            return
        ops = []
        for depth in sorted(set(lv.values())):
            cs = [c for c in convs if lv[c.name] == depth]
            for i in range(0, len(cs), hip.DENSE_MULTI_MAX):
                part = cs[i:i + hip.DENSE_MULTI_MAX]
                m = hip.DenseMulti([dict(src0=c.xin, wgt0=c.wf, K0=c.node.cin, N=c.npad, M=self.B, bias=c.biasf, dst=c.dst.data, flags=c.fwd_flags)
                                    for c in part], self.dt)
                ops.append(_Launch(m.run, "fwd", "fwd:" + "+".join(c.name for c in part), fwd=tuple(c.name for c in part)))
                for c in part:
                    c.fwd = ops[-1]
        self.fwd_ops[min(pos):max(pos) + 1] = ops

    def _fuse_pointwise_pairs(self):
        """Forward plan rewrite: a block-closing pointwise layer (c -> 4c, + residual, ReLU; c = 64 or 128: stages 2 and 3) directly
        followed by the next block's opening pointwise layer (4c -> c, ReLU) becomes ONE launch (urso_conv_pair): the block output is written once and
        the second layer reads it from LDS.  self.pair_first maps the second layer's name to the first layer's _Conv; the backward
        plan mirrors the fusion for the two data gradients.  URSO_OPT_PAIR=0 (hip.options(pair=0)) keeps the layers apart."""
        self.pair_first = {}
        self.shortcut_folded = []          # projection shortcuts computed inside a fused forward pair (conv_pairs.hip)
        g, dt = self.graph, self.dt
        if dt == hip.F32 or not hip.get_option("pair"):
            return
        convs = [n for n in g.nodes if n.op != "pool"]
        for a_node, b_node in zip(convs[:-1], convs[1:]):
            A, Bc = self.convs[a_node.name], self.convs[b_node.name]

            def plain(n, c):
                return (not n.stem and not n.dense and n.kh == 1 and n.kw == 1 and n.stride == 1 and n.relu and not n.out_f32 and
                        not c.batch_bn and c.npad == c.N and c.fwd is not None)
            if not (plain(a_node, A) and plain(b_node, Bc)):
                continue
            if a_node.residual is None or b_node.residual is not None or b_node.src.id != a_node.dst.id:
                continue
            M = self.B * a_node.dst.h * a_node.dst.w
            if not (a_node.cin == b_node.cout and hip.conv_pair_ok(M, dt, a_node.cin, a_node.cout)):
                continue
            A.Mpix = M
            # the residual operand of a stage's first block is its projection shortcut (a conv without activation, net.py:121-126): where
            # that is a plain 64 -> 256 pointwise layer with no other reader (stage 2) it becomes 64 more columns of the pair's first
            # GEMM (conv_pairs.hip) -- its own launch and its output tensor disappear; the backward plan never read that tensor
            S = [self.convs[n.name] for n in convs if n.dst.id == a_node.residual.id]
            readers = [n for n in g.nodes if (n.op == "pool" and n.src.id == a_node.residual.id) or
                       (n.op != "pool" and (n.src.id == a_node.residual.id or (n.residual is not None and n.residual.id == a_node.residual.id)))]
            if (len(S) == 1 and hip.get_option("pair") in (1, 2) and a_node.cin == 64 and M % 64 == 0 and len(readers) == 1 and
                    (lambda n, c: not n.stem and not n.dense and n.kh == 1 and n.kw == 1 and n.stride == 1 and not n.relu and not n.out_f32 and
                     n.residual is None and n.cin == 64 and n.cout == a_node.cout and not c.batch_bn and c.npad == c.N and
                     c.fwd is not None)(S[0].node, S[0])):
                Sc = S[0]
                A.fwd.run = (lambda A=A, Bc=Bc, Sc=Sc: hip.conv_pair_shortcut(
                    A.Mpix, dt, A.src.data, A.wf, A.biasf, Sc.src.data, Sc.wf, Sc.biasf, A.dst.bits, A.dst.data, Bc.wf, Bc.biasf, Bc.dst.data))
                self._share_forward(A, Sc, Bc)
                self.shortcut_folded.append(Sc.name)
            else:
                A.fwd.run = (lambda A=A, Bc=Bc: hip.conv_pair(A.Mpix, A.node.cin, dt, 0, A.src.data, A.wf, A.biasf, A.res.data, A.dst.bits,
                                                             A.dst.data, Bc.wf, Bc.biasf, None, Bc.dst.data))
                self._share_forward(A, Bc)
            self.pair_first[b_node.name] = A

    def _share_forward(self, A, *others):
        """A's forward launch now computes the layers `others` too: their own launches leave the plan, all of them share A's record."""
        A.fwd.fwd = (A.name,) + tuple(c.name for c in others)
        A.fwd.label = "fwd:" + "+".join(A.fwd.fwd)
        for c in others:
            self.fwd_ops.remove(c.fwd)
            c.fwd = A.fwd

    def _fuse_entry_shortcuts(self):
        """Forward plan rewrite (round 6): the block-closing pointwise layer of a stage's FIRST block (`res{4,5}a_branch2c` + BatchNorm, then
        Add with the projection shortcut and ReLU, net.py:148-157) and the shortcut itself (`res{4,5}a_branch1` + BatchNorm: a pointwise layer
        on the same pixels, no activation) become ONE launch with two reduction segments (urso_conv_pointwise2): out = ReLU(b . W2c^T +
        x . Wbr1^T + (bias2c + biasbr1)).  The shortcut's launch, its output tensor (84 MB at cfg2's stage 4: written, then read back as the
        residual) and one rounding step disappear; the weight preparation adds the shortcut's folded bias to branch2c's (urso_param_desc::
        bias_from).  Stages whose branch2c already sits in a fused pair (2-3) keep that form.  Nothing in the backward plan reads the
        shortcut's output (its gradient is the block output's)."""
        g, dt, B = self.graph, self.dt, self.B
        self.n_entry_fwd2 = 0
        if dt == hip.F32:
            return
        convs = [n for n in g.nodes if n.op != "pool"]
        alone = lambda c: c.fwd is not None and c.fwd.computes_only(c)
        outs = set(t.id for t in g.outputs.values()) | ({g.feat.id} if getattr(g, "feat", None) is not None and hasattr(g.feat, "id") else set())
        for a_node in convs:
            A = self.convs[a_node.name]
            if (a_node.stem or a_node.dense or a_node.kh != 1 or a_node.kw != 1 or a_node.stride != 1 or not a_node.relu or a_node.out_f32 or
                    a_node.residual is None or A.batch_bn or A.npad != A.N or not alone(A) or A.dst.fwd_sampled):
                continue
            S = [self.convs[n.name] for n in convs if n.dst.id == a_node.residual.id]
            if len(S) != 1:
                continue
            Sc, sn = S[0], S[0].node
            readers = [n for n in g.nodes if (n.op == "pool" and n.src.id == a_node.residual.id) or
                       (n.op != "pool" and (n.src.id == a_node.residual.id or (n.residual is not None and n.residual.id == a_node.residual.id)))]
            M = B * a_node.dst.h * a_node.dst.w
            if (len(readers) != 1 or a_node.residual.id in outs or sn.stem or sn.dense or sn.kh != 1 or sn.kw != 1 or sn.relu or sn.out_f32 or
                    sn.residual is not None or Sc.batch_bn or Sc.npad != Sc.N or Sc.N != A.N or not alone(Sc) or
                    sn.dst.h != a_node.dst.h or sn.dst.w != a_node.dst.w or
                    Sc.xin.numel() != M * sn.cin or A.xin.numel() != M * a_node.cin):       # both read dense [M][C] tensors (a strided shortcut reads the compact input)
                continue
            fl = hip.EPI_RELU
            if not (hip.conv_pointwise2_ok(B, a_node.dst.h, a_node.dst.w, a_node.cin, sn.cin, A.N, dt, fl) and
                    (A.N % 32 == 0 and hip.conv_pointwise2_ok(B, a_node.dst.h, a_node.dst.w, a_node.cin, sn.cin, A.N, dt, fl | hip.EPI_EMIT_BITS))):
                continue
            A.fwd.run = (lambda A=A, Sc=Sc, oh=a_node.dst.h, ow=a_node.dst.w, c0=a_node.cin, c1=sn.cin: hip.conv_pointwise2(
                B, oh, ow, c0, c1, A.N, dt, hip.EPI_RELU | (hip.EPI_EMIT_BITS if A.dst.bits is not None else 0),
                A.xin, A.wf, Sc.xin, Sc.wf, A.biasf, None, A.dst.data, A.dst.bits))
            self._share_forward(A, Sc)
            A.desc.bias_from = Sc.desc_id + 1
            self.shortcut_folded.append(Sc.name)
            Sc.dst.data = torch.empty(0, dtype=self.tdt, device=self.device)      # never written any more: a read fails instead of finding stale bytes
            self.n_entry_fwd2 += 1

    # ------------------------------------------------------------------ execution
    def run_prep(self):
        for op in self.prep_ops:
            op()

    def run_forward(self):
        for op in self.fwd_ops:
            op()

    def run_backward(self):
        for op in self.loss_pre_ops + self.loss_ops:
            op()
        for op in self.bwd_ops:
            op()

    def run_optimizer(self):
        for op in self.opt_ops:
            op()

    def _run_passes(self):
        """prep, forward, losses + backward: what a step runs in front of its optimizer (or its accumulation launch).  Under Config.SAM
        twice, around the ascent: at w, then at w + e with the losses going into sam_loss, and w is back behind it (_plan_sam)."""
        self.run_prep(); self.run_forward(); self.run_backward()
        if not self.sam_ops:
            return
        norm, ascend, descend = self.sam_ops
        norm(); ascend()
        at_w, self.loss_buf = self.loss_buf, self.sam_loss
        try:
            self.run_prep(); self.run_forward(); self.run_backward()
        finally:
            self.loss_buf = at_w
        descend()

    PLAN_OPTIONS = ("cus", "wgrad_blocks", "wgrad_narrow", "wgrad_big", "hwgrad", "grid_cap", "pair", "stem", "stem_pool", "c3", "bneck", "dense",
                    "pwx")

    def check_cleared_once(self):
        """Debug check of the plan-time clearing invariant (the `once` branch of _build_plan): every pixel OFF the sampled grid of a
        gradient buffer that is cleared once must still be zero.  Returns the offending layers (empty = invariant holds).  Step() calls it
        after every replay when URSO_CHECK_CLEARED=1."""
        bad = []
        for name, buf, h, w, c, sy, sx in self._cleared_once:
            t = buf[:self.B * h * w * c].view(self.B, h, w, c)
            off = t.clone()
            off[:, ::sy, ::sx, :] = 0
            if bool(off.any()):
                bad.append(name)
        return bad

    def _planning_options(self):
        return tuple(hip.get_option(o) for o in self.PLAN_OPTIONS)

    def _check_plan_options(self):
        now = self._planning_options()
        if now != self._plan_options:
            diff = ", ".join("%s %d -> %d" % (o, a, b) for o, a, b in zip(self.PLAN_OPTIONS, self._plan_options, now) if a != b)
            raise RuntimeError("kernel-policy options changed since this engine planned its step (%s): the split counts and partial workspaces of the "
                               "weight-gradient launches are sized at plan time -- build the Engine under the options it runs with" % diff)

    def step_eager(self):
        """One training step, launched kernel by kernel (used for capture, profiling and debugging).  Under Config.GRAD_ACCUM_STEPS > 1: one
        micro-step, the one step() would replay now, and the index advances as it does there."""
        self._check_plan_options()
        if self.accum_k > 1:
            self._run_micro(self._accum_roles[self.accum_micro])
            self.accum_micro = (self.accum_micro + 1) % self.accum_k
            return
        self._run_passes(); self.run_optimizer()

    def _run_micro(self, role):
        """The launches of a micro-step of the given role (Config.GRAD_ACCUM_STEPS > 1), without touching the index: "first" and "add" end
        behind the backward pass in accum_ops, "close" runs the optimizer."""
        assert role in grad_accum.ROLES and self.accum_k > 1
        self._accum_role = role
        self._run_passes()
        for op in (self.opt_ops if role == "close" else self.accum_ops):
            op()

    def param_pass_bytes(self, launch):
        """Algorithmic bytes of a batched parameter-sized launch, from the descriptor table (the library's launch profiler reports none for
        them: a launch covers many layers).  prep: fp32 filter in, compute-type forward + flipped layouts out; reduce: the split partials of
        the layers with more than FUSE_MAX partials in, their fp32 sum out; finalize_mat: fp32 filter + the partials the launch sums itself
        (2 ... FUSE_MAX) or the reduced sum in, fp32 gradient out.  None for other launches."""
        FUSE_MAX = 16                           # the most partials a finalisation sums itself: the library's fused-reduction limit (csrc/common.h)
        es = 4 if self.dt == hip.F32 else 2
        kind = launch.kind
        if launch.bucket is None or kind not in ("prep", "reduce", "finalize_mat"):
            return None
        ds = self._descs if kind == "prep" else [self.convs[nm].desc for nm in self._bucket_groups[launch.bucket]]
        total = 0.0
        for d in ds:
            K, N, npad, sp = int(d.K), int(d.N), int(d.npad), max(int(d.splits), 1)
            if kind == "prep":
                total += K * N * 4 + K * npad * es * (2 if d.wd else 1)
            elif kind == "reduce":
                if sp > FUSE_MAX:
                    total += (sp + 1) * K * npad * 4
            else:
                total += 2 * K * N * 4 + (sp if 1 < sp <= FUSE_MAX else 1) * K * npad * 4
        return total

    def profile_step(self, role=None):
        """One eager training step with the library's HIP-event launch profiler on.
        Returns [(label, kernel_id, ms, flops, bytes, n_kernels, device_symbol)] in launch order.  Under Config.GRAD_ACCUM_STEPS > 1 it is
        the micro-step of the given role ("first" | "add" | "close", default the one step() would run now; the index advances with it)."""
        if self.accum_k > 1:
            if role is not None:
                self.accum_micro = self._accum_roles.index(role)
            role = self._accum_roles[self.accum_micro]
        passes = self.prep_ops + self.fwd_ops + self.loss_pre_ops + self.loss_ops + self.bwd_ops
        if self.sam_ops:                        # Config.SAM: the doubled chain (_run_passes)
            passes = passes + self.sam_ops[:2] + passes + self.sam_ops[2:]
        launches = passes + (self.accum_ops if self.accum_k > 1 and role != "close" else self.opt_ops)
        torch.cuda.synchronize(self.device)
        hip.prof_collect()
        hip.prof_enable(True)
        self._single_chain = True               # every launch timed alone: the weight gradients stay on the chain (_fork_weight_gradients)
        try:
            self.step_eager()
            torch.cuda.synchronize(self.device)
            recs = hip.prof_collect_ex()
        finally:
            self._single_chain = False
            hip.prof_enable(False)
        assert len(recs) == len(launches), (len(recs), len(launches))
        out = []
        for l, r in zip(launches, recs):
            if not r[3]:                            # no bytes from the library: the batched parameter-sized passes are priced from the descriptor table
                by = self.param_pass_bytes(l)
                if by:
                    r = r[:3] + (by,) + r[4:]
            out.append((l.label,) + r)
        return out

    def capture(self, role=None):
        """Capture the step (training) or prep+forward (inference) into a hipGraph.  Under Config.GRAD_ACCUM_STEPS > 1 it is the micro-step
        of one role (default: the one step() would run now) and _graphs maps each role captured so far to its graph."""
        accum = self.mode == "training" and self.accum_k > 1
        if accum:
            role = role if role is not None else self._accum_roles[self.accum_micro]
            self._check_plan_options()
        run_step = (lambda: self._run_micro(role)) if accum else self.step_eager
        torch.cuda.synchronize(self.device)
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):                     # warm-up launch outside capture (module load etc.)
            if self.mode == "training":
                saved = self.save_train_state()
                run_step()
                self.restore_train_state(saved)
            else:
                self.run_prep(); self.run_forward()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        gr = torch.cuda.CUDAGraph()
        # hip.capture_lock: feeder threads (pinned allocations, augmentation kernels) stay out of HIP while the stream is capturing
        with hip.capture_lock, _no_gc():               # see _no_gc: nothing may be destroyed while the stream is capturing
            with torch.cuda.graph(gr):
                if self.mode == "training":
                    run_step()
                else:
                    self.run_prep(); self.run_forward()
        if accum:                                      # (never forked: _fork_weight_gradients)
            self._graphs = dict(self._graphs or {})
            self._graphs[role] = gr
            return gr
        self._graphs = gr
        if self.mode == "training" and self.wgrad_stream is not None and not self._single_chain_always:
            self._verify_forked_graph(gr)
        return self._graphs

    def _verification_batch(self):
        """Context manager: the verification of a forked graph must not run on an all-zero batch (nothing would distinguish a node that
        read stale operands; zero targets make rel_loss 0/0 and NaN never equals NaN).  When the engine's input or target buffers are still
        all zero -- capture before the first load_batch -- they hold a fixed pseudo-random batch for the check and get their bytes back after."""
        eng = self

        class _Ctx(object):
            def __enter__(self):
                self.saved = []
                g = torch.Generator(device=eng.device)
                g.manual_seed(20240607)
                img = eng.in_images_u8 if eng.input_u8 else eng.in_images
                if img is not None and not bool(img.any()):
                    self.saved.append((img, img.clone()))
                    if img.dtype == torch.uint8:
                        img.copy_(torch.randint(0, 256, img.shape, generator=g, device=eng.device, dtype=torch.uint8))
                    else:
                        img.copy_((torch.rand(img.shape, generator=g, device=eng.device) * 255.0 - 110.0).to(img.dtype))
                for name in ("gt_loc", "gt_ori", "gt_k3"):
                    t = getattr(eng, name, None)
                    if t is not None and t.numel() and not bool(t.any()):
                        self.saved.append((t, t.clone()))
                        r = torch.rand(t.shape, generator=g, device=eng.device) + 0.1
                        t.copy_((r / r.sum(-1, keepdim=True)).to(t.dtype))     # rows that are valid soft labels and non-zero regression targets alike
                return self

            def __exit__(self, *exc):
                for t, old in self.saved:
                    t.copy_(old)
        return _Ctx()

    def _verify_forked_graph(self, gr, replays=None):
        """The captured graph with its second branch against the same launches issued eagerly on one chain: `replays` steps each from the same
        state (URSO_FORK_VERIFY_REPLAYS, default 4; the second replay is the first that shows a node run early: the first reads what the
        warm-up step left), compared bit for bit on flat_g and the FORK_COMPARED part of train_state(): weights, gradients, momentum, BN
        statistics, the averages and their states.  NOT compared: Adam's flat_v2 / flat_vhat and hyper (its step counter), lamb_state; a
        forked Adam step is checked through the weights and first moments alone.  (ls_state, sam_state and flat_acc never meet a fork:
        _fork_weight_gradients.)  A graph executor that fails this (see _fork_weight_gradients) costs the engine its side branch, not its results.
        Cost: 2 x replays training steps and two clones of the training state per capture (and per re-capture: set_input_u8 toggles,
        set_trainable).  It runs again wherever verify_fork() is called (UrsoNet.train: once per epoch; tests/test_model_gpu.py holds a
        200-replay stress test); bench.py repeats the comparison with two fresh engines before it times anything."""
        n = int(replays if replays is not None else os.environ.get("URSO_FORK_VERIFY_REPLAYS", "4"))
        with self._verification_batch():
            saved = self.save_train_state()
            for _ in range(n):
                gr.replay()
            torch.cuda.synchronize(self.device)
            written = [self.flat_g] + [t for name, t in self.train_state() if name in self.FORK_COMPARED]
            got = [t.clone() for t in written]
            self.restore_train_state(saved)
            self._single_chain = True
            try:
                for _ in range(n):
                    self.step_eager()
            finally:
                self._single_chain = False
            torch.cuda.synchronize(self.device)
            ok = all(torch.equal(a, b) for a, b in zip(got, written))
            ok = ok and bool(torch.isfinite(self.flat_g).all())       # (NaN never equals NaN: a non-finite check batch proves nothing either way)
            self.restore_train_state(saved)
        self.fork_checks += 1
        if not ok:
            import warnings
            warnings.warn("ursonet_amd: the captured training graph with the weight gradients on a second branch does not reproduce the single chain "
                          "on this device / runtime -- captured again on one chain")
            self._single_chain_always = True
            self._graphs = None
            self.capture()
        return ok

    def verify_fork(self, replays=None):
        """Re-run the forked graph's check against the single chain on the batch that is loaded NOW (training state is restored afterwards).
        True = the step runs forked and is verified; False = it runs (or from now on runs) on one chain."""
        if self.mode != "training" or not self.forked:
            return False
        if self._graphs is None:
            self.capture()                         # (verifies)
            return self.forked
        self._verify_forked_graph(self._graphs, replays)
        return self.forked

    @property
    def forked(self):
        """True when the captured step runs weight gradients on a second graph branch (_fork_weight_gradients) and that graph has been verified."""
        return self.wgrad_stream is not None and not self._single_chain_always

    def step(self):
        """Replay the captured training step (captures on first use)."""
        assert self._stand_in != "ema", "step() while the average is swapped in: leave ema_weights() / call swap_ema() again first"
        assert self._stand_in not in ("swa", "swag"), \
            "step() while the SWA average or a SWAG sample stands in for the weights: leave swa_weights() / swag_weights() / call swap_swa() again first"
        if self.accum_k > 1:                           # Config.GRAD_ACCUM_STEPS: the graph of this micro-step's role, captured on first use
            role = self._accum_roles[self.accum_micro]
            if self._graphs is None or role not in self._graphs:
                self.capture(role)
            self._graphs[role].replay()
            self.accum_micro = (self.accum_micro + 1) % self.accum_k
        else:
            if self._graphs is None:
                self.capture()
            self._graphs.replay()
        if self._cleared_once and os.environ.get("URSO_CHECK_CLEARED", "0") == "1":
            bad = self.check_cleared_once()
            assert not bad, "gradient buffers cleared at plan time hold values off their sampled grid: %s" % bad

    def forward(self):
        if self.mode == "training":
            self.run_prep(); self.run_forward()
        else:
            if self._graphs is None:
                self.capture()
            self._graphs.replay()

    # ------------------------------------------------------------------ I/O helpers
    def load_batch(self, images, gt_loc=None, gt_ori=None, gt_k3=None):
        """images: float32 [B,H,W,3] already molded (mold_image, net.py:1337-1348) -- numpy or torch."""
        self.in_images.copy_(torch.as_tensor(images, dtype=torch.float32).reshape(self.in_images.shape), non_blocking=True)
        if gt_loc is not None:
            self.gt_loc.copy_(torch.as_tensor(gt_loc, dtype=torch.float32).reshape(self.gt_loc.shape), non_blocking=True)
        if gt_ori is not None:
            self.gt_ori.copy_(torch.as_tensor(gt_ori, dtype=torch.float32).reshape(self.gt_ori.shape), non_blocking=True)
        if gt_k3 is not None:
            self.gt_k3.copy_(torch.as_tensor(gt_k3, dtype=torch.float32).reshape(self.gt_k3.shape), non_blocking=True)

    def set_input_u8(self, on=True):
        """Switch the first kernel between molded float32 input (load_batch) and raw uint8 input (load_batch_u8)."""
        on = bool(on)
        if on and self.in_images_u8 is None:
            self.in_images_u8 = torch.zeros(self.B, self.H, self.W, 3, dtype=torch.uint8, device=self.device)
        if on != self.input_u8:
            self.input_u8 = on
            self._graphs = None                    # the captured graph holds the other buffer's address

    def load_batch_u8(self, images_u8, gt_loc=None, gt_ori=None, gt_k3=None):
        """Raw uint8 frames [B,H,W,3] (host array or device tensor, already resized / padded to the model size) + targets;
        device tensors are copied device-to-device on the current stream."""
        self.set_input_u8(True)
        self.in_images_u8.copy_(torch.as_tensor(images_u8).reshape(self.in_images_u8.shape), non_blocking=True)
        for buf, src in ((getattr(self, "gt_loc", None), gt_loc), (getattr(self, "gt_ori", None), gt_ori), (getattr(self, "gt_k3", None), gt_k3)):
            if src is not None and buf is not None:
                buf.copy_(torch.as_tensor(src).reshape(buf.shape), non_blocking=True)

    def outputs(self):
        """(loc [B, n_loc], ori [B, n_ori]) as fp32 device tensors (raw network outputs, net.py:1254-1258)."""
        g = self.graph
        nl = g.outputs["loc"].c
        loc = self.out_loc.data.view(self.B, -1)[:, :nl]
        if self.out_ori is None:             # keypoint mode: (k1, [k2, k3]) -- net.py:678
            return loc, [self.acts[g.outputs[k].id].data.view(self.B, -1)[:, :3] for k in ("k2", "k3")]
        no = g.outputs["ori"].c
        ori = self.q_out if self.quat_head else self.out_ori.data.view(self.B, -1)[:, :no]
        return loc, ori

    def features(self):
        """The bottleneck_layer output (Graph.feat), the tensor both head trunks read, as a [B, h, w, C] view in the engine's dtype: the
        activations of the last forward pass (ursonet_amd/domain.py pools them).  A view of the plan's own buffer; nothing is launched."""
        f = self.graph.feat
        a = self.acts[f.id]
        assert a.numel == self.B * f.h * f.w * f.c, "the bottleneck features are kept dense"
        return a.data.view(self.B, f.h, f.w, f.c)

    def losses(self):
        """{'loc_loss','ori_loss'} (keypoint mode: {'loc_loss','k2_loss','k3_loss'}) weighted by LOSS_WEIGHTS, as in the
        Keras metrics (net.py:989-992, 1019-1028)."""
        l = self.loss_buf.detach().cpu().numpy()
        if self.config.REGRESS_KEYPOINTS:
            return {"loc_loss": float(l[0]), "k2_loss": float(l[2]), "k3_loss": float(l[3])}
        return {"loc_loss": float(l[0]), "ori_loss": float(l[1])}

    def evaluate(self, read=True):
        """Forward + losses on the loaded batch WITHOUT touching any training state: what Keras' validation pass does
        (learning_phase 0, net.py:1155-1157).  In batch-statistics BN mode the moving statistics are restored afterwards (the
        forward kernels of the training plan update them) -- the normalisation itself still uses batch statistics there, which
        is the one deviation from Keras' moving-statistics evaluation (documented in DESIGN.md section 11)."""
        stats = self.flat_stats.clone() if self.train_bn else None
        self.run_prep(); self.run_forward()
        for op in self.loss_pre_ops + self.loss_ops:
            op()
        if stats is not None:
            self.flat_stats.copy_(stats)
        return self.losses() if read else None     # read=False: the scalars stay in loss_buf (UrsoNet.train copies them on the device, no sync)

    # ------------------------------------------------------------------ BN recalibration (ursonet_amd/bn_recal.py)
    def bn_recal_begin(self):
        """Start pooling BN statistics: the table of every batch-statistics layer in plan order (built once per plan), zeroed float64
        accumulators, and a clone of flat_stats for bn_recal_abort().  Eager launches, no graph: no buffer of the captured step moves."""
        if not self.train_bn:
            raise ValueError("bn_recal_begin needs a training engine with batch-statistics BatchNorm (TRAIN_BN = None): no other plan leaves "
                             "the batch mean and variance of every BN layer on the device")
        rp = self._recal_plan
        if rp is None or rp[0] != self.plan_version:
            layers = [(c.bmean, c.bvar, c.Mpix, self.stat_slices[(c.node.bn, "moving_mean")][0], self.stat_slices[(c.node.bn, "moving_variance")][0])
                      for c in self.convs.values() if c.batch_bn]
            assert {c.node.bn for c in self.convs.values() if c.batch_bn} == {ln for ln, _ in self.stat_slices}, "a BN layer without batch statistics"
            rp = self._recal_plan = (self.plan_version, hip.BnRecalPlan(layers, self.flat_stats.numel(), self.device))
        rp[1].reset()
        self._recal_stats = self.flat_stats.clone()

    def bn_recal_add(self):
        """The loaded batch's statistics into the pool: what evaluate() runs in front of the losses, then the one add launch."""
        assert self._recal_stats is not None, "bn_recal_add without bn_recal_begin"
        self.run_prep(); self.run_forward()
        self._recal_plan[1].add()

    def bn_recal_end(self):
        """flat_stats = the pooled statistics of the batches added (at least one).  The momentum updates the forward kernels made on the
        way are overwritten: every BN layer is a batch-statistics layer in this mode, so every slice is settled."""
        assert self._recal_stats is not None, "bn_recal_end without bn_recal_begin"
        self._recal_plan[1].settle(self.flat_stats)

    def bn_recal_abort(self):
        """flat_stats as bn_recal_begin() found it, bit for bit (in mid-pass, or after bn_recal_end); without a begin: nothing."""
        if self._recal_stats is not None:
            self.flat_stats.copy_(self._recal_stats)
            self._recal_stats = None

    def set_lr(self, lr):
        self.hyper[0] = float(lr)

    FORK_COMPARED = ("flat_w", "flat_v", "flat_stats", "flat_ema", "ema_state", "flat_swa", "swa_state", "flat_swa_sq")      # _verify_forked_graph

    def train_state(self):
        """[(name, tensor)] of the persistent device state of training under the current plan, in the order save_train_state() keeps
        (DESIGN.md section 30): everything a step writes and the next step reads.  Scratch (flat_g, flat_w0, _swag_hold) is not in it."""
        names = ["flat_w", "flat_v", "flat_stats"]
        if self.adam:                                  # the moments and hyper, which holds Adam's device-side step counter
            names += ["flat_v2", "flat_vhat", "hyper"]
        names += [n for n in ("lamb_state", "sam_state") if getattr(self, n) is not None]
        if self.ema_state is not None:
            names += ["flat_ema", "ema_state"]
        if self.swa_state is not None:
            names += ["flat_swa", "swa_state"] + (["flat_swa_sq"] if self.flat_swa_sq is not None else [])
        if self.accum_k > 1:
            names.append("flat_acc")
        if self.ls_state is not None:
            names.append("ls_state")
        return [(n, getattr(self, n)) for n in names]

    def save_train_state(self):
        """Clones of train_state(), for the warm-up step before graph capture.  Under Config.GRAD_ACCUM_STEPS the host-side index of the next
        micro-step rides behind flat_acc."""
        st = []
        for name, t in self.train_state():
            st.append(t.clone())
            if name == "flat_acc":
                st.append(self.accum_micro)
        return st

    def restore_train_state(self, st):
        it = iter(st)
        for name, t in self.train_state():
            t.copy_(next(it))
            if name == "flat_acc":
                self.accum_micro = int(next(it))

    def reset_optimizer(self):
        """Zero the optimizer's moments (and restart the loss scale).  The weights' averages (Config.WEIGHT_EMA, Config.SWA) and their schedules
        are no optimizer state: they stay, so staged training keeps one average (reset_swa() restarts SWA's by hand).
        Under Config.GRAD_ACCUM_STEPS > 1 a begun optimizer step is dropped: the next micro-step is a first one (a bit copy into flat_acc)."""
        self.flat_v.zero_()
        self.accum_micro = 0
        if self.adam:
            self.flat_v2.zero_(); self.flat_vhat.zero_(); self.hyper[5] = 0.0
        if self.lamb_plan is not None:                 # Config.LAMB: {p1, p2, kt} = {1, 1, 0}, with t = 0 above
            self.lamb_plan.reset()
        if self.ls_state is not None:
            self.ls_state.copy_(torch.tensor(self._state_init["ls_state"], dtype=torch.float32))
        if self.sam_state is not None:                 # Config.SAM: the last step's record and the counts; rho and eps stay
            self.sam_state[sam.NORMSQ:].zero_()

    def loss_weight_values(self):
        """[ori_weight, loc_weight] as a strided two-element view of flat_w (Config.LEARNABLE_LOSS_WEIGHTS; no copy, no synchronisation)."""
        o = self.slices[(loss_weights.LAYER, "ori_weight")][0]
        return self.flat_w[o:o + 8:4]

    def loss_scale(self):
        """{scale, skipped_total, last_step_skipped, good_steps} of the device-side loss-scale state, read once (one synchronising copy);
        None when Config.LOSS_SCALE is off."""
        if self.ls_state is None:
            return None
        return loss_scale.as_dict(self.ls_state.detach().cpu().tolist())

    def grad_accum(self):
        """{"steps": k, "micro": i}: Config.GRAD_ACCUM_STEPS and the index of the micro-step that step() runs next (0 = the next one begins
        an optimizer step); None when accumulation is off."""
        if self.mode != "training" or self.accum_k == 1:
            return None
        return {"steps": self.accum_k, "micro": self.accum_micro}

    def lars_report(self, adapting_only=False):
        """{(layer, weight): (|w|, |g|, trust)} of the last optimizer step under Config.LARS, one synchronising read of the device-side
        table: the float64 norms the trust ratios were computed from (of the weights BEFORE the step and of the finalised gradient) and
        the float32 trust the update used.  adapting_only: the kernels alone, without the tensors whose trust is 1 by rule.  None when
        Config.LARS is off; zeros and trust 1 before the first step."""
        return self._trust_report(self.lars_plan, adapting_only)

    def lamb_report(self, adapting_only=False):
        """The same under Config.LAMB, {(layer, weight): (|w|, |r|, trust)}: the second norm is that of the Adam direction r.  None when
        Config.LAMB is off."""
        return self._trust_report(self.lamb_plan, adapting_only)

    def _trust_report(self, plan, adapting_only):
        if plan is None:
            return None
        stat, trust = plan.stat.detach().cpu().numpy(), plan.trust.detach().cpu().numpy()
        return OrderedDict((key, (float(stat[t, 0]), float(stat[t, 1]), float(trust[t])))
                           for t, key in enumerate(self.slices) if plan.tensors[t][2] or not adapting_only)

    def set_sam_rho(self, rho):
        """Config.SAM's radius from the next step on: the device field, so a captured graph needs no re-capture."""
        assert self.sam_state is not None, "Config.SAM is off"
        if isinstance(rho, bool) or not isinstance(rho, (float, np.floating)) or not np.isfinite(rho) or rho <= 0:
            raise ValueError("%s must be a finite float > 0, got %r" % (sam.KEY, rho))
        self.sam_state[sam.RHO] = float(rho)

    def sam_report(self):
        """{rho, grad_norm, scale, applied, applied_total, loss, loss_perturbed} of the last step under Config.SAM, one synchronising read:
        grad_norm = |g1|, the norm at w that the ascent divided by; loss = L(w) and loss_perturbed = L(w + e), keyed as losses().  Under
        GRAD_ACCUM_STEPS the last micro-step's.  None when Config.SAM is off; zeros before the first step."""
        if self.sam_state is None:
            return None
        v = torch.cat([self.sam_state, self.loss_buf, self.sam_loss]).detach().cpu().numpy()
        st, l0, l1 = v[:sam.STATE_LEN], v[sam.STATE_LEN:sam.STATE_LEN + 4], v[sam.STATE_LEN + 4:]
        names = ((0, "loc_loss"), (2, "k2_loss"), (3, "k3_loss")) if self.config.REGRESS_KEYPOINTS else ((0, "loc_loss"), (1, "ori_loss"))
        return {"rho": float(st[sam.RHO]), "grad_norm": float(np.sqrt(st[sam.NORMSQ])), "scale": float(st[sam.SCALE]),
                "applied": bool(st[sam.APPLIED] != 0), "applied_total": int(st[sam.APPLIED_TOTAL]),
                "loss": {k: float(l0[i]) for i, k in names}, "loss_perturbed": {k: float(l1[i]) for i, k in names}}

    def weight_ema(self):
        """{decay, warmup, updates, next_decay} of the device-side state of the weights' average, read once (one synchronising copy); None
        when Config.WEIGHT_EMA is off."""
        if self.ema_state is None:
            return None
        return weight_ema.as_dict(self.ema_state.detach().cpu().tolist())

    def swap_ema(self):
        """Exchange flat_w and flat_ema in place (urso_ema_swap) and flip ema_swapped.  Every forward pass reads flat_w only through the prep
        pass, which evaluate() and the captured step both begin with, so nothing else has to move; the BN statistics are shared."""
        assert self.flat_ema is not None, "Config.WEIGHT_EMA is off"
        assert self._stand_in not in ("swa", "swag"), "swap_ema while the SWA average or a SWAG sample stands in for the weights"
        hip.ema_swap(self.n_flat, self.flat_w, self.flat_ema)
        self._stand_in = None if self._stand_in == "ema" else "ema"

    def ema_weights(self):
        """Context manager: the averaged weights are the model's inside (evaluate() and every forward pass), the raw ones are back after it."""
        return _StandIn(self, self.swap_ema, self.swap_ema)

    # ------------------------------------------------------------------ Config.SWA
    def swa(self):
        """{period, start, ticks, models, collected, variance} of the device-side SWA state, read once (one synchronising copy); None when
        Config.SWA is off."""
        if self.swa_state is None:
            return None
        return swa.as_dict(self.swa_state.detach().cpu().tolist())

    def reset_swa(self):
        """Restart the collection: ticks = models = 0.  The first model collected afterwards is copied in, so the buffers need no clearing."""
        assert self.swa_state is not None, "Config.SWA is off"
        assert self._stand_in not in ("swa", "swag"), "reset_swa while the SWA average or a SWAG sample stands in for the weights"
        self.swa_state.copy_(torch.tensor(self._state_init["swa_state"], dtype=torch.int32))

    def set_swa_weights(self, params, sq_params=None, models=None, strict=True):
        """Load params (as set_weights takes them) into the SWA mean and, with SWA_VARIANCE, sq_params into the mean of squares; `models`
        (>= 1) is the number of models they average.  The collection goes on from there: ticks = start + models * period.  The BN statistics,
        which all sets share, are not touched."""
        assert self.swa_state is not None, "Config.SWA is off"
        assert self._stand_in not in ("swa", "swag"), "set_swa_weights while the SWA average or a SWAG sample stands in for the weights"
        if isinstance(models, (bool, np.bool_)) or not isinstance(models, (int, np.integer)) or not 1 <= models <= swa.MAX_MODELS:
            raise ValueError("set_swa_weights: models must be an int in [1, 2^24], got %r" % (models,))
        if (sq_params is not None) != (self.flat_swa_sq is not None):
            raise ValueError("set_swa_weights: sq_params goes with Config.SWA_VARIANCE = True and only with it")
        self._load_trainable(params, self.flat_swa, strict)
        if sq_params is not None:
            self._load_trainable(sq_params, self.flat_swa_sq, strict)
        st = list(self._state_init["swa_state"])
        st[swa.MODELS] = int(models)
        st[swa.TICKS] = min(st[swa.START] + int(models) * st[swa.PERIOD], swa.MAX_TICKS)
        self.swa_state.copy_(torch.tensor(st, dtype=torch.int32))

    def swap_swa(self):
        """Exchange flat_w and flat_swa in place (urso_ema_swap: there is one exchange kernel) and flip swa_swapped; as swap_ema."""
        assert self.flat_swa is not None, "Config.SWA is off"
        assert self._stand_in not in ("ema", "swag"), "swap_swa while the EMA average or a SWAG sample stands in for the weights"
        hip.ema_swap(self.n_flat, self.flat_w, self.flat_swa)
        self._stand_in = None if self._stand_in == "swa" else "swa"

    def swa_weights(self):
        """Context manager: the SWA mean is the model's inside (evaluate() and every forward pass), the raw weights are back after it."""
        def enter():
            assert self._stand_in != "swa", "swa_weights() inside swa_weights() / swap_swa()"
            self.swap_swa()
        return _StandIn(self, enter, self.swap_swa)

    def swag_weights(self, sample, seed=0, var_scale=0.5):
        """Context manager (SWAG-diagonal; needs SWA_VARIANCE and at least two collected models): inside, flat_w holds sample number `sample`
        of N(mean, var_scale * diag(sq - mean^2)) under `seed` (urso_swag_sample; ursonet_amd.swa.sample32 of swa.normals); the raw weights
        wait in a hold buffer allocated on first use and come back bit for bit on exit, also after an exception."""
        assert self.swa_state is not None and self.flat_swa_sq is not None, "swag_weights needs Config.SWA with SWA_VARIANCE = True"
        for name, v, top in (("sample", sample, 2 ** 31), ("seed", seed, 2 ** 64)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
                raise ValueError("swag_weights: %s must be an int in [0, 2^%d), got %r" % (name, 31 if name == "sample" else 64, v))
        s = swa.scale32(var_scale)                     # ValueError: not a finite float >= 0

        def enter():
            assert self._stand_in is None, "swag_weights() while an average or another sample stands in for the weights"
            models = int(self.swa_state[swa.MODELS].item())
            if models < 2:
                raise ValueError("swag_weights needs at least 2 collected models (a variance), the average holds %d" % models)
            if self._swag_hold is None:
                self._swag_hold = torch.empty_like(self.flat_w)
            self._swag_hold.copy_(self.flat_w)
            self._stand_in = "swag"
            hip.swag_sample(self.n_flat, self.flat_swa, self.flat_swa_sq, self.flat_w, s, int(seed), int(sample))

        def leave():
            self.flat_w.copy_(self._swag_hold)         # a copy of the same dtype: the bits
            self._stand_in = None
        return _StandIn(self, enter, leave)

    def flops(self):
        return conv_flops(self.graph, self.B)


def initial_weights(graph, seed=1234, randomize_bn=False):
    """Keras default initialisers (glorot_uniform kernels, zero biases, BN gamma=1 beta=0 mean=0 var=1;
    used by `--weights none`, pose_estimator.py:897).  `randomize_bn` perturbs BN tensors and biases."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for ln, ws in graph.params.items():
        if graph.kinds.get(ln) == loss_weights.KIND:
            out[ln] = loss_weights.initial_values()
            continue
        p = OrderedDict()
        for wn, shape in ws.items():
            if wn == "kernel":
                if len(shape) == 4:
                    rf = shape[0] * shape[1]
                    fi, fo = rf * shape[2], rf * shape[3]
                else:
                    fi, fo = shape
                lim = math.sqrt(6.0 / (fi + fo))
                p[wn] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            elif wn == "bias":
                p[wn] = (rng.normal(0, 0.05, size=shape) if randomize_bn else np.zeros(shape)).astype(np.float32)
            elif wn == "gamma":
                p[wn] = (rng.uniform(0.5, 1.5, size=shape) if randomize_bn else np.ones(shape)).astype(np.float32)
            elif wn in ("beta", "moving_mean"):
                p[wn] = (rng.normal(0, 0.1, size=shape) if randomize_bn else np.zeros(shape)).astype(np.float32)
            else:
                p[wn] = (rng.uniform(0.5, 1.5, size=shape) if randomize_bn else np.ones(shape)).astype(np.float32)
        out[ln] = p
    return out
