"""Drop-in for the reference's `net.py` model API (class UrsoNet, net.py:566-1308) on MI355X.

`pose_estimator.py` programs against: UrsoNet(mode, config, model_dir), .train(), .detect(),
.load_weights(), .find_last(), .get_last_checkpoint(), .get_imagenet_weights(), .get_urso_weights(),
.compile(), .set_trainable(), attributes .config .epoch .log_dir .checkpoint_path .keras_model, and
the module functions load_image_gt / data_generator / mold_image / compose_image_meta.  All of that
is provided here with the same names, argument meaning and error behaviour; the numeric work is
done by ursonet_amd.engine.Engine (HIP kernels through the C ABI) -- there is no Keras/TF and no
CPU fallback: building a model without an MI355X raises.

Weights files: Keras HDF5 (`.h5`, by-name, nested `model_weights` groups handled) through h5py or, where this interpreter has none,
through the HDF5 C library itself (ursonet_amd/h5lite.py: ctypes on libhdf5.so, checked against files written by the real h5py);
always also a `.npz` twin with the same layer/weight names and layouts ("<layer>/<weight>" keys).
"""
import datetime
import logging
import os
import re
from collections import OrderedDict

import numpy as np

from . import utils
from .graph import build_graph, layer_regex as _layer_regex


def log(text, array=None):
    """net.py:46-57."""
    if array is not None:
        text = text.ljust(25)
        text += ("shape: {:20}  min: {:10.5f}  max: {:10.5f}  {}".format(
            str(array.shape), array.min() if array.size else "", array.max() if array.size else "", array.dtype))
    print(text)


############################################################
#  Keras-model shim: layer names / weights / trainable flags
############################################################
class _Layer(object):
    def __init__(self, model, name, kind, weight_names):
        self._model, self.name, self.kind = model, name, kind
        self.weight_names = list(weight_names)
        self.trainable = True

    @property
    def weights(self):
        return ["%s/%s:0" % (self.name, w) for w in self.weight_names]

    def get_weights(self):
        eng = self._model._engine
        return [eng.wview(self.name, w).detach().cpu().numpy().copy() for w in self.weight_names]

    def set_weights(self, arrays):
        self._model._engine.set_weights({self.name: dict(zip(self.weight_names, arrays))}, strict=False)


class KerasModelShim(object):
    """What net.py touches on `keras_model`: .layers, .get_layer(name), .predict(), weight access."""

    def __init__(self, owner, graph):
        self._owner = owner
        self.name = "urso_net"
        self.layers = [_Layer(self, n, graph.kinds[n], ws.keys()) for n, ws in graph.params.items()]
        self._by_name = {l.name: l for l in self.layers}
        self.metrics_names = ["loss", "loc_loss", "ori_loss"]

    @property
    def _engine(self):
        return self._owner._engine

    def get_layer(self, name):
        return self._by_name[name]

    def predict(self, molded_images, verbose=0):
        return self._owner._predict(np.asarray(molded_images))


############################################################
#  Data formatting (net.py:1314-1355)
############################################################
def compose_image_meta(image_id, original_image_shape, image_shape, window, scale):
    return np.array([image_id] + list(original_image_shape) + list(image_shape) + list(window) + [scale])


def mold_image(image, config):
    dt = np.float16 if config.F16 else np.float32
    if image.shape[-1] == 3:
        return image.astype(dt) - config.MEAN_PIXEL
    return image.astype(dt) - np.mean(config.MEAN_PIXEL)


def unmold_image(normalized_images, config):
    return (normalized_images + config.MEAN_PIXEL).astype(np.uint8)


############################################################
#  Data generator (net.py:358-559)
############################################################
def load_image_gt(dataset, config, image_id):
    """Image + pose targets for one sample (net.py:363-461): raw sample -> augmentation (sim2real stages and the camera /
    in-plane rotation warps run on the GPU, same NumPy global-RNG draws as the reference) -> resize / pad -> image_meta.
    Returns (image, image_meta, loc, ori), or (image, image_meta, loc, k1, k2) in keypoint mode."""
    from . import feeder
    s = feeder.augment_samples([feeder.load_sample(dataset, config, image_id)], dataset, config)[0]
    image, image_meta = feeder.finish_sample(s, config)
    if config.REGRESS_KEYPOINTS:
        return image, image_meta, s.loc, np.asarray(s.k1).T, np.asarray(s.k2).T
    return image, image_meta, s.loc, s.ori


def data_generator(dataset, config, shuffle=True, batch_size=1):
    """net.py:463-559: yields ([molded images, image_meta, gt_loc, gt_ori], []) forever (keypoint mode: gt_loc, gt_k1, gt_k2);
    tolerates up to 5 failing samples.  Built on ursonet_amd.feeder (pre-allocated per-field batch arrays, batched augmentation)."""
    from . import feeder
    for asm in feeder.batches(dataset, config, shuffle, batch_size, molded=True):
        yield asm.inputs(), []


############################################################
#  Weight files
############################################################
def read_weights_file(path):
    """-> {layer: {weight: array}} from a Keras HDF5 file (h5py needed) or an .npz twin."""
    if path.endswith(".npz"):
        out = OrderedDict()
        with np.load(path) as z:
            for k in z.files:
                ln, wn = k.rsplit("/", 1)
                out.setdefault(ln, OrderedDict())[wn] = z[k]
        return out
    try:
        import h5py
    except ImportError:
        # no h5py for this interpreter: the HDF5 C library itself through ctypes (ursonet_amd/h5lite.py: same files, same library h5py binds)
        from . import h5lite
        if not h5lite.available():
            raise ImportError("`load_weights` of a Keras .h5 file needs h5py or an HDF5 library (libhdf5.so; $URSO_HDF5_LIB): neither found -- "
                              "use the .npz twin (tools/h5_to_npz.py converts on any machine that has one)")
        return h5lite.read_keras_weights(path)
    out = OrderedDict()
    with h5py.File(path, mode='r') as f:
        if 'layer_names' not in f.attrs and 'model_weights' in f:          # net.py:831-832
            f = f['model_weights']
        for ln in [n.decode('utf8') if isinstance(n, bytes) else n for n in f.attrs['layer_names']]:
            grp = f[ln]
            names = [n.decode('utf8') if isinstance(n, bytes) else n for n in grp.attrs['weight_names']]
            for wn in names:
                short = wn.split("/")[-1].split(":")[0]
                out.setdefault(ln, OrderedDict())[short] = np.asarray(grp[wn])
    return out


def write_weights_file(path, params):
    """Always writes `<path without ext>.npz`; additionally a Keras-layout .h5 when h5py exists."""
    base = path[:-3] if path.endswith(".h5") else (path[:-4] if path.endswith(".npz") else path)
    flat = {"%s/%s" % (ln, wn): a for ln, ws in params.items() for wn, a in ws.items()}
    np.savez(base + ".npz", **flat)
    written = [base + ".npz"]
    if path.endswith(".h5"):
        try:
            import h5py
        except ImportError:
            from . import h5lite
            if h5lite.available():                      # the HDF5 library without h5py: the same Keras layout (keras save_weights_to_hdf5_group)
                h5lite.write_keras_weights(path, params)
                written.append(path)
            return written
        with h5py.File(path, "w") as f:
            f.attrs['layer_names'] = [ln.encode('utf8') for ln in params]
            f.attrs['backend'] = b'tensorflow'
            f.attrs['keras_version'] = b'2.2.4'
            for ln, ws in params.items():
                g = f.create_group(ln)
                names = ["%s/%s:0" % (ln, wn) for wn in ws]
                g.attrs['weight_names'] = [n.encode('utf8') for n in names]
                for n, a in zip(names, ws.values()):
                    g.create_dataset(n, data=a)
        written.append(path)
    return written


def ema_checkpoint_path(path):
    """The averaged twin of a checkpoint (Config.WEIGHT_EMA): `ema_` in front of the file name, in the same directory.  find_last and
    get_last_checkpoint pick files that start with `weights`, so they never see it."""
    return os.path.join(os.path.dirname(path), "ema_" + os.path.basename(path))


def swa_checkpoint_path(path, sqmean=False):
    """The SWA twins of a checkpoint (Config.SWA): `swa_` in front of the file name for the mean, and for the mean of squares
    (SWA_VARIANCE) `swa_sqmean` where the name says `weights`; in the same directory, never seen by find_last either."""
    base = os.path.basename(path)
    if sqmean:
        base = "sqmean" + base[len("weights"):] if base.startswith("weights") else "sqmean_" + base
    return os.path.join(os.path.dirname(path), "swa_" + base)


class BatchLogger(object):
    """net.py:1106-1115 -- per-batch loss history returned by train()."""

    def __init__(self, loss_weights=False, weight_ema=False):
        self.ori_loss_acc, self.loc_loss_acc = [], []
        # (Config.LOSS_SCALE and Config.SAM: train() adds loss_scale_acc / skipped_acc and sam_grad_norm_acc / sam_applied_acc /
        # sam_sharpness_acc, one entry per step -- per micro-step for SAM -- when the feature is on)
        if weight_ema:                                 # Config.WEIGHT_EMA: the decay that every step's update of the average used
            self.ema_decay_acc = []
        if loss_weights:                               # Config.LEARNABLE_LOSS_WEIGHTS: the two log-variances after every step
            self.ori_weight_acc, self.loc_weight_acc = [], []


############################################################
#  UrsoNet
############################################################
class UrsoNet(object):
    def __init__(self, mode, config, model_dir, build_engine=True):
        assert mode in ['training', 'inference']
        self.mode, self.config, self.model_dir = mode, config, model_dir
        self.set_log_dir()
        self._engine = None
        self._layer_regex = ".*"
        self.keras_model = self.build(mode=mode, config=config, build_engine=build_engine)

    def build(self, mode, config, build_engine=True):
        """net.py:581-699.  Validates the config exactly like the reference (image divisibility
        exception, FC-layer count assert) and lowers the graph onto the GPU engine."""
        assert mode in ['training', 'inference']
        graph = build_graph(config)                   # raises the 'dividable by 2 at least 6 times' Exception
        self._graph = graph
        self._dp, self._rank, self._world = None, 0, 1
        from . import loss_weights
        if loss_weights.enabled(config, mode):          # the layer the training engine adds to its own graph (ursonet_amd/loss_weights.py)
            loss_weights.validate(config)              # ValueError: REGRESS_KEYPOINTS / DP_EXACT_REL_LOSS
            loss_weights.add_layer(graph)
        if build_engine:
            from .engine import Engine
            from . import dp, loss_scale
            world = dp.launcher_world()[2]
            if mode == "training":
                loss_weights.validate(config, world)   # ValueError: set under a data-parallel launcher
            if mode == "training":
                from . import grad_accum
                grad_accum.validate(config, world)          # ValueError: a bad GRAD_ACCUM_STEPS, or k > 1 under a data-parallel launcher
                from . import lars
                lars.validate(config, world)                # ValueError: bad LARS keys, LARS with Adam, or LARS under a data-parallel launcher
                from . import lamb
                lamb.validate(config, world)                # ValueError: bad LAMB keys, LAMB with SGD or LARS, or LAMB under a data-parallel launcher
                from . import sam
                sam.validate(config, world)                 # ValueError: bad SAM keys, or SAM under a data-parallel launcher
                loss_scale.initial_state(config, world)     # ValueError: a bad LOSS_SCALE, or one set under a data-parallel launcher
                from . import weight_ema
                weight_ema.initial_state(config, world)     # ValueError: a bad WEIGHT_EMA, or one set under a data-parallel launcher
                from . import bn_recal
                bn_recal.validate(config, world)            # ValueError: a bad BN_RECAL_BATCHES, one without WEIGHT_EMA / with a frozen BN, or under a launcher
                from . import swa
                swa.validate(config, world)                 # ValueError: bad SWA keys, SWA_RECAL_BATCHES without SWA / with a frozen BN, or SWA under a launcher
            if mode == "training" and world > 1:
                # under a launcher (`python -m torch.distributed.run --nproc-per-node N pose_estimator.py train ...`): one process per GPU, this
                # rank's engine takes IMAGES_PER_GPU samples of every global batch of IMAGES_PER_GPU x WORLD_SIZE, the gradient exchange is
                # ursonet_amd.dp.DataParallelEngine (RCCL).  The reference's own knob for this is GPU_COUNT (config.py:20,154) feeding a
                # ParallelModel it left commented out (net.py:694-697); the launcher's world size takes its place
                self._rank, _, self._world = dp.init_from_launcher()
                gc = int(getattr(config, "GPU_COUNT", 1))
                assert gc in (1, self._world), "GPU_COUNT = %d but the launcher started %d ranks" % (gc, self._world)
                self._engine = Engine(config, mode, batch=int(config.IMAGES_PER_GPU))
                self._dp = dp.DataParallelEngine(self._engine, bucket_bytes=int(getattr(config, "DP_BUCKET_BYTES", 32 << 20)),
                                                 compress=getattr(config, "DP_COMPRESS", None))
            else:
                if world > 1:                           # inference under a launcher: N independent replicas, each on its own GPU, no exchange
                    import torch
                    self._rank, local, self._world = dp.launcher_world()
                    torch.cuda.set_device(int(os.environ.get("URSO_DP_DEVICE", local % max(torch.cuda.device_count(), 1))))
                self._engine = Engine(config, mode)
        return KerasModelShim(self, graph)

    # ---------------------------------------------------------------- checkpoints / log dirs
    def get_last_checkpoint(self, model_name):
        """net.py:768-788."""
        dir_names = next(os.walk(self.model_dir))[1]
        assert model_name in dir_names
        model_path = os.path.join(self.model_dir, model_name)
        checkpoints = sorted(f for f in next(os.walk(model_path))[2] if f.startswith("weights"))
        if not checkpoints:
            return model_path, None
        return model_path, os.path.join(model_path, checkpoints[-1])

    def find_last(self):
        """net.py:791-814."""
        dir_names = next(os.walk(self.model_dir))[1]
        key = self.config.NAME.lower()
        dir_names = sorted(f for f in dir_names if f.startswith(key))
        if not dir_names:
            return None, None
        dir_name = os.path.join(self.model_dir, dir_names[-1])
        checkpoints = sorted(f for f in next(os.walk(dir_name))[2] if f.startswith("weights"))
        if not checkpoints:
            return dir_name, None
        return dir_name, os.path.join(dir_name, checkpoints[-1])

    def load_weights(self, weights_in_path, weights_out_path, by_name=False, exclude=None):
        """net.py:816-852: load by name (layers absent from the file keep their values), optional
        exclude list; then point the log dir at weights_out_path."""
        if exclude:
            by_name = True
        params = read_weights_file(weights_in_path)
        if exclude:
            params = OrderedDict((k, v) for k, v in params.items() if k not in exclude)
        if not by_name:
            missing = [ln for ln in self._graph.params if ln not in params]
            if missing:
                raise ValueError("weights file lacks layers %s (use by_name=True)" % missing[:5])
        known = OrderedDict((ln, ws) for ln, ws in params.items() if ln in self._graph.params)
        self._engine.set_weights(known, strict=False)
        # Config.WEIGHT_EMA, training mode: set_weights started the average at the loaded weights; a checkpoint's averaged sibling
        # (ema_weights_... beside weights_..., written by train()) takes their place where there is one
        sibling = ema_checkpoint_path(weights_in_path)
        if getattr(self._engine, "flat_ema", None) is not None and os.path.exists(sibling):
            ema = read_weights_file(sibling)
            self._engine.set_ema_weights(OrderedDict((ln, ws) for ln, ws in ema.items() if ln in self._graph.params and ln not in (exclude or ())),
                                         strict=False)
        self.set_log_dir(weights_out_path)

    def save_weights(self, path, ema=False, swa=False):
        """ema=True (Config.WEIGHT_EMA): the averaged weights, as an ordinary weights file (the BN statistics are the ones both sets share).
        swa=True (Config.SWA): the SWA mean likewise; swa="sq": the running mean of squares (SWA_VARIANCE) under the same names."""
        if swa:
            return write_weights_file(path, self._engine.get_weights(swa=swa))
        return write_weights_file(path, self._engine.get_weights(ema=True) if ema else self._engine.get_weights())

    def swa_weights(self):
        """Context manager (Config.SWA, training mode): inside it the engine runs on the SWA mean; as ema_weights()."""
        return self._engine.swa_weights()

    def swag_weights(self, sample, seed=0, var_scale=0.5):
        """Context manager (Config.SWA with SWA_VARIANCE, at least two collected models): inside it the engine runs on sample number
        `sample` of the SWAG-diagonal Gaussian (Engine.swag_weights), so that save_weights() writes a sampled model for predict() /
        evaluate() -- followed where wanted by recalibrate_bn: the BN statistics are the raw weights'.  No training step may run inside."""
        return self._engine.swag_weights(sample, seed=seed, var_scale=var_scale)

    def load_swa(self, mean_path, sqmean_path=None, models=None):
        """Restore an average that train() wrote: swa_weights_*.h5, with SWA_VARIANCE also swa_sqmean_*.h5, and the number of models they
        hold (the `swa models N` of the log).  The collection goes on from there."""
        keep = lambda params: OrderedDict((ln, ws) for ln, ws in params.items() if ln in self._graph.params)
        self._engine.set_swa_weights(keep(read_weights_file(mean_path)),
                                     keep(read_weights_file(sqmean_path)) if sqmean_path is not None else None, models=models, strict=False)

    def ema_weights(self):
        """Context manager (Config.WEIGHT_EMA, training mode): inside it the engine runs on the averaged weights -- for a custom evaluation
        through the engine (evaluate(), forward()); the raw weights are back after it.  No training step may run inside."""
        return self._engine.ema_weights()

    def get_imagenet_weights(self, architecture):
        """net.py:854-884 downloads from GitHub; there is no network here."""
        raise IOError("get_imagenet_weights(%r): pre-trained weights must be provided locally (no network access); "
                      "pass the path of a .h5/.npz file to --weights" % (architecture,))

    def get_urso_weights(self, dataset_name):
        """net.py:886-940."""
        assert dataset_name in ['soyuz_hard', 'dragon_hard', 'speed']
        raise IOError("get_urso_weights(%r): released weights must be provided locally (no network access)" % (dataset_name,))

    def set_log_dir(self, model_path=None):
        """net.py:944-967."""
        if model_path:
            self.log_dir = os.path.dirname(model_path)
            m = re.search(r"(\d{3,4})\.(h5|npz)$", model_path)
            self.epoch = int(m.group(1)[-3:]) if m else int(model_path[-6:-3])
        else:
            self.epoch = 0
            now = datetime.datetime.now()
            self.log_dir = os.path.join(self.model_dir, "{}{:%Y%m%dT%H%M}".format(self.config.NAME.lower(), now))
        self.checkpoint_path = os.path.join(self.log_dir, "weights_{}_*epoch*.h5".format(self.config.NAME.lower()))
        self.checkpoint_path = self.checkpoint_path.replace("*epoch*", "{epoch:04d}")

    # ---------------------------------------------------------------- training
    def compile(self, learning_rate, momentum):
        """net.py:973-1028: (re)creates the optimizer state (momentum buffers reset, as a new Keras
        optimizer would), sets lr/momentum/clipnorm.  Loss assembly and the L2 term live in the engine."""
        eng = self._engine
        eng.hyper[0] = float(learning_rate)
        if eng.adam:                                   # OPTIMIZER != 'SGD': Adam(learning_rate, amsgrad=True, clipnorm), net.py:982-983
            eng.hyper[4] = float(self.config.GRADIENT_CLIP_NORM or 0.0)
        else:
            eng.hyper[1] = float(momentum)
            eng.hyper[2] = float(self.config.GRADIENT_CLIP_NORM or 0.0)
        eng.reset_optimizer()

    def set_trainable(self, layer_regex, keras_model=None, indent=0, verbose=1):
        """net.py:1030-1066."""
        if verbose > 0 and keras_model is None:
            log("Selecting layers to train")
        self._layer_regex = layer_regex
        for layer in self.keras_model.layers:
            layer.trainable = bool(re.fullmatch(layer_regex, layer.name))
            if layer.trainable and verbose > 0:
                log("{}{:20}   ({})".format(" " * indent, layer.name, layer.kind))
        self._engine.set_trainable(layer_regex)

    def train(self, train_dataset, val_dataset, learning_rate, epochs, layers):
        """net.py:1068-1167: STEPS_PER_EPOCH steps per epoch, VALIDATION_STEPS forward-only validation
        batches, a weights checkpoint per epoch, optional CyclicLR; returns the per-batch loss logger."""
        assert self.mode == "training", "Create model in training mode."
        layers = _layer_regex(layers)
        cfg, eng = self.config, self._engine
        # the reference hands Keras two Python generators and `workers = cpu_count` processes (net.py:1100-1163); here a producer
        # thread + loader threads assemble uint8 batches in pinned memory and a side stream uploads batch k+1 while step k runs
        from .feeder import DeviceFeeder
        from .infer import loader_workers
        import torch
        workers = loader_workers(cfg)
        rank, world, runner = self._rank, self._world, (self._dp or eng)
        # data-parallel run: every rank walks the SAME shuffled order and takes samples [rank * B, (rank + 1) * B) of each global batch (feeder.batches)
        train_feed = DeviceFeeder(eng, train_dataset, cfg, shuffle=True, workers=workers, rank=rank, world=world)
        val_feed = (DeviceFeeder(eng, val_dataset, cfg, shuffle=True, workers=workers, rank=rank, world=world)
                    if int(cfg.VALIDATION_STEPS) > 0 else None)
        use_ema = eng.ema_state is not None            # Config.WEIGHT_EMA: validate and save the average beside the raw weights
        from . import bn_recal
        recal_k = bn_recal.validate(cfg, world)        # Config.BN_RECAL_BATCHES: > 0 = the saved average gets BN statistics of its own
        # Config.SWA: once the average holds a model, validate and save it beside the raw weights (SWA_RECAL_BATCHES: with statistics of its own)
        use_swa = getattr(eng, "swa_state", None) is not None
        swa_recal_k = 0
        if use_swa:
            from . import swa as SWA
            swa_recal_k = SWA.validate(cfg, world)[3]
        history_full = BatchLogger(loss_weights=eng.learn_lw, weight_ema=use_ema)
        chief = rank == 0
        if chief:
            log("\nStarting at epoch {}. LR={}\n".format(self.epoch, learning_rate))
            log("Checkpoint Path: {}".format(self.checkpoint_path))
            if world > 1:
                log("Data parallel: {} ranks x {} images (global batch {})".format(world, eng.B, world * eng.B))
            if eng.accum_k > 1:
                log("Gradient accumulation: {} micro-batches x {} images per optimizer step (effective batch {})".format(
                    eng.accum_k, eng.B, eng.accum_k * eng.B))
        self.set_trainable(layers, verbose=1 if chief else 0)
        self.compile(learning_rate, cfg.LEARNING_MOMENTUM)
        if chief:
            os.makedirs(self.log_dir, exist_ok=True)
        steps, vsteps = int(cfg.STEPS_PER_EPOCH), int(cfg.VALIDATION_STEPS)
        # Keras' BatchLogger reads the batch's losses after every step (net.py:1106-1115): a device -> host round trip per 7 ms step.  Here each
        # step's loss scalars are copied into a device-side history row (same stream, no synchronisation) and read ONCE per epoch -- the same
        # per-batch lists, no bubble; under data parallelism the rows are averaged over the ranks first (the loss of the global batch)
        # Config.GRAD_ACCUM_STEPS = k > 1: STEPS_PER_EPOCH counts optimizer steps, each draws k batches; the history gets a row per micro-batch
        # and is folded on the host into one entry per optimizer step, the mean of its k rows (grad_accum.fold_history)
        n_loss = int(eng.loss_buf.numel())
        acc_k = int(eng.accum_k)
        hist = torch.zeros(max(steps * acc_k, 1), n_loss, dtype=torch.float32, device=eng.device)
        vhist = torch.zeros(max(vsteps, 1), n_loss, dtype=torch.float32, device=eng.device)
        kp = bool(cfg.REGRESS_KEYPOINTS)
        # Config.LOSS_SCALE: the loss-scale state of every step beside its losses (device-side, read once per epoch)
        ls_hist = (torch.zeros(max(steps, 1), int(eng.ls_state.numel()), dtype=torch.float32, device=eng.device)
                   if eng.ls_state is not None else None)
        if ls_hist is not None:
            history_full.loss_scale_acc, history_full.skipped_acc = [], []
        # Config.SAM: the ascent's record and the losses at w + e of every (micro-)step, likewise; L(w) is the loss history's row
        sam_hist = (torch.zeros(max(steps * acc_k, 1), int(eng.sam_state.numel()) + n_loss, dtype=torch.float32, device=eng.device)
                    if getattr(eng, "sam_state", None) is not None else None)
        if sam_hist is not None:
            history_full.sam_grad_norm_acc, history_full.sam_applied_acc, history_full.sam_sharpness_acc = [], [], []
        # Config.LEARNABLE_LOSS_WEIGHTS: the two log-variances after every step, likewise (a strided view of flat_w: ori_weight, loc_weight)
        lw_view = eng.loss_weight_values() if eng.learn_lw else None
        lw_hist = torch.zeros(max(steps, 1), 2, dtype=torch.float32, device=eng.device) if lw_view is not None else None
        # Config.WEIGHT_EMA: the schedule state in front of every step (its NEXT_DECAY is the decay that step's update uses) and a second
        # validation history for the averaged weights, both device-side and read once per epoch
        ema_hist = torch.zeros(max(steps, 1), int(eng.ema_state.numel()), dtype=torch.float32, device=eng.device) if use_ema else None
        vhist_ema = torch.zeros(max(vsteps, 1), n_loss, dtype=torch.float32, device=eng.device) if use_ema else None
        vhist_swa = torch.zeros(max(vsteps, 1), n_loss, dtype=torch.float32, device=eng.device) if use_swa else None
        clr_it = 0
        for epoch in range(self.epoch, epochs):
            for i in range(steps):
                if cfg.CLR:
                    eng.set_lr(utils.clr_triangular(clr_it, cfg.BASE_LEARNING_RATE, cfg.MAX_LEARNING_RATE, cfg.CLR_STEP_SIZE))
                    clr_it += 1
                if ema_hist is not None:               # (the state moves only behind the optimizer: the closing micro-step's update uses this decay)
                    ema_hist[i].copy_(eng.ema_state, non_blocking=True)
                for j in range(acc_k):
                    train_feed.next_into()
                    runner.step()
                    hist[i * acc_k + j].copy_(eng.loss_buf.view(-1), non_blocking=True)
                    if sam_hist is not None:
                        ns = int(eng.sam_state.numel())
                        sam_hist[i * acc_k + j, :ns].copy_(eng.sam_state, non_blocking=True)
                        sam_hist[i * acc_k + j, ns:].copy_(eng.sam_loss.view(-1), non_blocking=True)
                if ls_hist is not None:
                    ls_hist[i].copy_(eng.ls_state, non_blocking=True)
                if lw_hist is not None:
                    lw_hist[i].copy_(lw_view, non_blocking=True)
            swa_now = eng.swa() if use_swa else None    # read once per epoch (one synchronising copy)
            swa_models = swa_now["models"] if swa_now else 0
            for i in range(vsteps):
                val_feed.next_into()
                eng.evaluate(read=False)
                vhist[i].copy_(eng.loss_buf.view(-1), non_blocking=True)
                if use_ema:                             # the same loaded batch under the averaged weights: two in-place exchanges around it
                    with eng.ema_weights():
                        eng.evaluate(read=False)
                        vhist_ema[i].copy_(eng.loss_buf.view(-1), non_blocking=True)
                if swa_models >= 1:                     # and under the SWA mean, likewise
                    with eng.swa_weights():
                        eng.evaluate(read=False)
                        vhist_swa[i].copy_(eng.loss_buf.view(-1), non_blocking=True)
            if world == 1 and eng.forked:
                eng.verify_fork()                       # the forked backward pass against the single chain on this epoch's last batch (engine.py)
            if world > 1:
                from . import dp
                dp.average_over_ranks(hist)
                dp.average_over_ranks(vhist)
            h = hist[:steps * acc_k].cpu().numpy()
            sam_text = None
            if sam_hist is not None and steps:         # (read in front of the fold: one row per micro-step, as the ascents were)
                from . import sam as SAM
                sh = sam_hist[:steps * acc_k].cpu().numpy()
                ns = SAM.STATE_LEN
                rise = sh[:, ns:] - h                  # L(w + e) - L(w), per loss
                cols = ((0, "loc_loss"), (2, "k2_loss"), (3, "k3_loss")) if kp else ((0, "loc_loss"), (1, "ori_loss"))
                history_full.sam_grad_norm_acc += [float(x) for x in np.sqrt(sh[:, SAM.NORMSQ])]
                history_full.sam_applied_acc += [bool(x) for x in sh[:, SAM.APPLIED]]
                history_full.sam_sharpness_acc += [{k: float(r[c]) for c, k in cols} for r in rise]
                sam_text = "epoch %d  sam rho %g  median |g| %.4e  %s  (%d of %d ascents applied)" % (
                    epoch + 1, float(sh[-1, SAM.RHO]), float(np.median(np.sqrt(sh[:, SAM.NORMSQ]))),
                    "  ".join("d_%s %+.3e" % (k, float(np.mean(rise[:, c]))) for c, k in cols), int(sh[:, SAM.APPLIED].sum()), len(sh))
            if acc_k > 1:
                from . import grad_accum
                h = grad_accum.fold_history(h, acc_k)
            for row in h:
                history_full.ori_loss_acc.append(None if kp else float(row[1]))   # None in keypoint mode, as logs.get('ori_loss') is (net.py:1112)
                history_full.loc_loss_acc.append(float(row[0]))
            val = {}
            if vsteps:
                v = vhist[:vsteps].cpu().numpy().mean(0)
                val = ({"loc_loss": v[0], "k2_loss": v[2], "k3_loss": v[3]} if kp else {"loc_loss": v[0], "ori_loss": v[1]})
                if use_ema:
                    v = vhist_ema[:vsteps].cpu().numpy().mean(0)
                    val.update({"ema_loc_loss": v[0], "ema_k2_loss": v[2], "ema_k3_loss": v[3]} if kp else {"ema_loc_loss": v[0], "ema_ori_loss": v[1]})
                if swa_models >= 1:
                    v = vhist_swa[:vsteps].cpu().numpy().mean(0)
                    val.update({"swa_loc_loss": v[0], "swa_k2_loss": v[2], "swa_k3_loss": v[3]} if kp else {"swa_loc_loss": v[0], "swa_ori_loss": v[1]})
            ls_text = ""
            if ls_hist is not None and steps:
                from . import loss_scale as LS
                lh = ls_hist[:steps].cpu().numpy()
                history_full.loss_scale_acc += [float(x) for x in lh[:, LS.SCALE]]
                history_full.skipped_acc += [bool(x) for x in lh[:, LS.LAST_SKIPPED]]
                ls_text = "  loss_scale %g  skipped %d" % (float(lh[-1, LS.SCALE]), int(lh[:, LS.LAST_SKIPPED].sum()))
            lw_text = ""
            if lw_hist is not None and steps:
                wh = lw_hist[:steps].cpu().numpy()
                history_full.ori_weight_acc += [float(x) for x in wh[:, 0]]
                history_full.loc_weight_acc += [float(x) for x in wh[:, 1]]
                lw_text = "  ori var %.5f  loc var %.5f" % (float(np.exp(wh[-1, 0])), float(np.exp(wh[-1, 1])))      # exp(s), as net.py:1141-1142 would print
            ema_text = ""
            if ema_hist is not None and steps:
                from . import weight_ema as WE
                eh = ema_hist[:steps].cpu().numpy()
                history_full.ema_decay_acc += [float(x) for x in eh[:, WE.NEXT_DECAY]]
                ema_text = "  ema_decay %g" % float(eh[-1, WE.NEXT_DECAY])
            if swa_models >= 1:
                ema_text += "  swa models %d" % swa_models
            if chief:
                log("epoch %d  loc_loss %.5f  %s%s%s%s" % (
                    epoch + 1, float(np.mean(h[:, 0])) if steps else float("nan"),
                    "  ".join("val_%s %.5f" % (k, float(x)) for k, x in sorted(val.items())), ls_text, lw_text, ema_text))
                if sam_text is not None:                # Config.SAM: rho, the median gradient norm at w, the mean rise of every loss along the ascent
                    log(sam_text)
                if eng.lars_plan is not None:           # Config.LARS: the trust ratios of the epoch's last step, one read of the device table
                    from . import lars
                    ts = lars.summary(eng.lars_report(adapting_only=True))
                    if ts is not None:
                        log("epoch %d  lars trust  min %.3e  median %.3e  max %.3e  (%d kernels)" % (
                            epoch + 1, ts["min"], ts["median"], ts["max"], ts["tensors"]))
                if getattr(eng, "lamb_plan", None) is not None:       # Config.LAMB: the same line for Adam's trust ratios
                    from . import lamb
                    ts = lamb.summary(eng.lamb_report(adapting_only=True))
                    if ts is not None:
                        log("epoch %d  lamb trust  min %.3e  median %.3e  max %.3e  (%d kernels)" % (
                            epoch + 1, ts["min"], ts["median"], ts["max"], ts["tensors"]))
                self.save_weights(self.checkpoint_path.format(epoch=epoch + 1))     # replicas are identical: one writer
                if use_ema and recal_k:                 # Config.BN_RECAL_BATCHES: the averaged weights with statistics of their own
                    log(self._save_average_recalibrated(ema_checkpoint_path(self.checkpoint_path.format(epoch=epoch + 1)), recal_k, train_feed,
                                                        epoch + 1, "ema"))
                elif use_ema:                           # "ema_" in front: find_last / get_last_checkpoint keep finding the raw file
                    self.save_weights(ema_checkpoint_path(self.checkpoint_path.format(epoch=epoch + 1)), ema=True)
                if swa_models >= 1:                     # "swa_" in front, for the same reason
                    raw_path = self.checkpoint_path.format(epoch=epoch + 1)
                    if swa_recal_k:                     # Config.SWA_RECAL_BATCHES: the SWA mean with statistics of its own
                        log(self._save_average_recalibrated(swa_checkpoint_path(raw_path), swa_recal_k, train_feed, epoch + 1, "swa"))
                    else:
                        self.save_weights(swa_checkpoint_path(raw_path), swa=True)
                    if eng.flat_swa_sq is not None:
                        self.save_weights(swa_checkpoint_path(raw_path, sqmean=True), swa="sq")
            if world > 1:
                import torch.distributed as dist
                dist.barrier()                          # nobody runs ahead of the checkpoint (find_last on another rank sees it)
        train_feed.close()
        if val_feed is not None:
            val_feed.close()
        self.epoch = max(self.epoch, epochs)
        return history_full

    def _save_average_recalibrated(self, path, k, feed, epoch, which):
        """Config.BN_RECAL_BATCHES (which = "ema") / Config.SWA_RECAL_BATCHES (which = "swa"): the next k batches of the training feeder
        through the engine under that average, their pooled BN statistics (ursonet_amd/bn_recal.py) into the averaged checkpoint `path`,
        and the raw statistics back bit for bit.  Statistics that are not finite are not written: the file then holds the shared ones, as
        without the key.  Returns the line to log."""
        from . import bn_recal
        from .graph import BN_EPS
        eng = self._engine
        raw = eng.flat_stats.detach().cpu().numpy().copy()
        try:
            with (eng.ema_weights() if which == "ema" else eng.swa_weights()):
                eng.bn_recal_begin()                    # (keeps the clone of flat_stats that bn_recal_abort puts back)
                for _ in range(k):
                    feed.next_into()
                    eng.bn_recal_add()
                eng.bn_recal_end()
            after = eng.flat_stats.detach().cpu().numpy().copy()
            finite = all(np.all(np.isfinite(after[o:o + n])) for o, n, _s in eng.stat_slices.values())
            if not finite:
                eng.bn_recal_abort()
            self.save_weights(path, ema=which == "ema", swa=which == "swa")
        finally:
            eng.bn_recal_abort()                        # the raw statistics, bit for bit, whatever happened
        if not finite:
            return "epoch %d  bn recal  %d batches x %d images: statistics not finite, the averaged file keeps the shared ones" % (epoch, k, eng.B)
        rep = bn_recal.shift_report(eng.stat_slices, raw, after, BN_EPS)
        return "epoch %d  bn recal  %d batches x %d images under the averaged weights  max mean shift / sigma %.3e  max var ratio %.3e  (%d BN layers)" % (
            epoch, k, eng.B, max(v[0] for v in rep.values()), max(v[1] for v in rep.values()), len(rep))

    # ---------------------------------------------------------------- inference
    def _resized(self, images):
        """resize / pad every frame to the model's input geometry (utils.resize_image) -> [(uint8 frame, window, scale)]."""
        cfg = self.config
        out = []
        for image in images:
            frame, window, scale, _pad, _crop = utils.resize_image(image, min_dim=cfg.IMAGE_MIN_DIM, min_scale=cfg.IMAGE_MIN_SCALE,
                                                                   max_dim=cfg.IMAGE_MAX_DIM, mode=cfg.IMAGE_RESIZE_MODE)
            out.append((frame, window, scale))
        return out

    def mold_inputs(self, images):
        """net.py:1169-1205: (molded images [N,h,w,3], image metas [N,12], windows [N,4])."""
        frames = self._resized(images)
        molded = np.stack([mold_image(f, self.config) for f, _, _ in frames])
        metas = np.stack([compose_image_meta(0, im.shape, f.shape, w, s) for im, (f, w, s) in zip(images, frames)])
        return molded, metas, np.stack([w for _, w, _ in frames])

    def _predict(self, molded_images):
        """keras_model.predict on molded float images -> list of raw output arrays."""
        eng = self._engine
        assert molded_images.shape[0] == eng.B, "batch %d != engine batch %d" % (molded_images.shape[0], eng.B)
        eng.set_input_u8(False)
        eng.load_batch(molded_images.astype(np.float32))
        return self._outputs_after_forward()

    def _outputs_after_forward(self):
        import torch
        eng = self._engine
        eng.forward()
        loc, rest = eng.outputs()
        torch.cuda.synchronize()
        if self.config.REGRESS_KEYPOINTS:
            return [loc.cpu().numpy()] + [k.cpu().numpy() for k in rest]
        return [loc.cpu().numpy(), rest.cpu().numpy()]

    def detect(self, images, verbose=0):
        """net.py:1207-1259: one dict of RAW network outputs per image -- {'loc', 'ori'}, or {'loc', 'k1', 'k2'} in keypoint mode
        (the reference's key names for the three keypoint heads).  uint8 frames take the device path: they are resized / padded on the host
        (Config.DEVICE_RESIZE and frames of one size: uploaded raw and resized there, same bytes), uploaded as uint8 and mean-subtracted by
        the first kernel; anything else goes through mold_inputs / predict."""
        assert self.mode == "inference", "Create model in inference mode."
        assert len(images) == self.config.BATCH_SIZE, "len(images) must be equal to BATCH_SIZE"
        if verbose:
            log("Processing {} images".format(len(images)))
            for image in images:
                log("image", image)
        from .feeder import device_resize_applies
        if device_resize_applies(images, self.config):        # DEVICE_RESIZE: the raw frames go up once and are resized / padded there
            from . import augment
            frames = augment.resize_images(np.stack(images), min_dim=self.config.IMAGE_MIN_DIM, max_dim=self.config.IMAGE_MAX_DIM,
                                           min_scale=self.config.IMAGE_MIN_SCALE, mode=self.config.IMAGE_RESIZE_MODE)[0]
            self._engine.load_batch_u8(frames)
            outs = self._outputs_after_forward()
        elif all(getattr(im, "dtype", None) == np.uint8 and im.ndim == 3 and im.shape[-1] == 3 for im in images):
            frames = [f for f, _, _ in self._resized(images)]
            assert all(f.shape == frames[0].shape for f in frames), \
                "After resizing, all images must have the same size. Check IMAGE_RESIZE_MODE and image sizes."
            self._engine.load_batch_u8(np.stack(frames))
            outs = self._outputs_after_forward()
        else:
            molded, metas, _ = self.mold_inputs(images)
            assert all(m.shape == molded[0].shape for m in molded), \
                "After resizing, all images must have the same size. Check IMAGE_RESIZE_MODE and image sizes."
            if verbose:
                log("molded_images", molded)
                log("image_metas", metas)
            outs = self.keras_model.predict(molded, verbose=0)
        keys = ("loc", "k1", "k2") if self.config.REGRESS_KEYPOINTS else ("loc", "ori")
        return [dict((k, o[i]) for k, o in zip(keys, outs)) for i in range(len(images))]
