"""Input side of the training loop (reference: net.py:358-559 load_image_gt / data_generator and the
fit_generator(workers=cpu_count, max_queue_size=100) call of net.py:1147-1163).

The reference loads, augments, resizes and molds one sample at a time in `cpu_count` worker processes and ships float
images through a queue.  At ~2,800 images/s per GPU that design cannot keep up (32 x 512 x 640 x 3 float32 = 126 MB per step over
PCIe alone is 2.3 ms of an 11.4 ms step).  Here:
  * workers (threads: image decode / synthesis and NumPy release the GIL) only produce the RAW sample -- uint8 frame + pose;
  * everything per-pixel runs batched on the GPU: sim2real stages, camera / in-plane rotation warps (one urso_warp_perspective for
    the minibatch) and target re-encoding (urso_encode_ori); mean subtraction + cast are the engine's first kernel (urso_mold_images
    reads uint8);
  * resize / zero padding (utils.resize_image) run where Config.DEVICE_RESIZE says.  False (default): on the host, frame by frame in the
    producer thread (finish_sample) -- float64 NumPy over the native frame, ~0.3 s per 960 x 1280 frame, by far the slowest stage as soon
    as a frame is really rescaled.  True: a batch of uint8 RGB frames of one size (modes square / pad64) goes up RAW from pinned memory, is
    augmented where it lies and finished by urso_resize_images_u8 (augment.resize_images: the host function's bytes); the augmented frames
    are no longer copied back.  Mixed sizes, other dtypes, 'crop' / 'none' and the molded generator format keep the host path;
  * uint8 frames go host -> device from PINNED memory on a side stream into a double buffer while the previous step computes:
    31 MB instead of 126 MB per step, off the critical path (DEVICE_RESIZE: the raw frames, 118 MB for 32 URSO frames, on the
    producer's own stream; the finished batch reaches the double buffer by a device-to-device copy).
`data_generator` keeps the reference's signature and yield format on top of the same pieces.
"""
import logging
import queue
import threading

import numpy as np

from . import utils


def compose_image_meta(image_id, original_image_shape, image_shape, window, scale):
    return np.array([image_id] + list(original_image_shape) + list(image_shape) + list(window) + [scale])


class Sample(object):
    """One raw training sample: uint8 frame + the pose targets the configured heads need."""
    __slots__ = ("image_id", "image", "loc", "ori", "k1", "k2")

    def __init__(self, image_id, image, loc, ori, k1=None, k2=None):
        self.image_id, self.image, self.loc, self.ori, self.k1, self.k2 = image_id, image, loc, ori, k1, k2


def load_sample(dataset, config, image_id, with_image=True):
    """The host-only first third of load_image_gt (net.py:367-388): frame and targets, no augmentation, no resize.
    with_image=False (Config.DEVICE_CACHE_GB: the frame is resident on the device) skips dataset.load_image; `image` is then None."""
    image = dataset.load_image(image_id) if with_image else None
    loc = dataset.load_location(image_id) if config.REGRESS_LOC else dataset.load_location_encoded(image_id)
    k1 = k2 = None
    if config.REGRESS_KEYPOINTS:
        k1, k2 = dataset.load_keypoints(image_id)[:2]
    if config.REGRESS_KEYPOINTS or config.REGRESS_ORI:
        getter = {"quaternion": dataset.load_quaternion, "euler_angles": dataset.load_euler_angles,
                  "angle_axis": dataset.load_angle_axis}[config.ORIENTATION_PARAM]
        ori = getter(image_id)
    else:
        ori = dataset.load_orientation_encoded(image_id)
    return Sample(image_id, image, loc, ori, k1, k2)


def _hip_section():
    """The lock that keeps this thread out of HIP while another thread captures a hipGraph (hip.capture_lock; Engine.capture holds it).  Taken
    around the batched augmentation launches with their device-to-host copies and around pin_memory only: disk loads, the CPU draws and the
    host resize / padding of a batch run unlocked, so a capture waits for a kernel's worth of work, not for a batch's preparation.  With
    Config.DEVICE_RESIZE (RawUploader) the host copy of the raw frames into the reused pinned buffer runs unlocked as well; the lock is held
    while the batch's upload, augmentation and resize kernels are ENQUEUED (asynchronous launches plus the host algebra of the warps), not
    while they run."""
    from . import hip
    return hip.capture_lock


def augment_samples(samples, dataset, config, frames=None):
    """The augmentation third (net.py:390-438) for a LIST of samples, in place.  NumPy's GLOBAL generator is consumed exactly as the
    reference consumes it, sample by sample: the sim2real dice (net.py:395), then that sample's rotation dice (net.py:415) and angles
    (utils.py:33 / :62) -- the imgaug stage parameters come from a separate generator, as imgaug's do, and only for the samples the dice
    select.  The samples themselves are loaded ahead of the draws and the pixel work is batched (one sim2real pass set and one warp
    launch for all samples of the list that need it), which changes no draw.  Images come back as uint8 arrays.

    frames (DEVICE_RESIZE): a uint8 device tensor [n,H,W,3] that holds the samples' frames, all of one size.  The pixel work then reads and
    writes device memory only -- same draws, same kernels, no copy back -- the samples' `image` fields are left alone, and the tensor of
    the augmented frames is RETURNED instead of the list.  The frame size is the tensor's: the samples need not carry an image
    (Config.DEVICE_CACHE_GB: frames served from the device cache were never loaded)."""
    if not samples:
        return samples if frames is None else frames
    from . import augment
    rot = bool(config.ROT_AUG or config.ROT_IMAGE_AUG)
    if rot:
        assert config.REGRESS_LOC
        assert config.ORIENTATION_PARAM == 'quaternion'
    n = len(samples)
    if frames is not None:
        shapes, same_size = [tuple(frames.shape[1:])] * n, True
    else:
        shapes = [s.image.shape for s in samples]
        same_size = all(sh == shapes[0] for sh in shapes)
    draws, pyr, warp_ids = None, np.zeros((n, 3)), []
    if config.SIM2REAL_AUG:
        draws = []
    for i, s in enumerate(samples):
        if config.SIM2REAL_AUG:
            draws.append(augment.sim2real_draw(1, shapes[i][0], shapes[i][1], prng=augment._PIPELINE_RNG))
        if rot:
            dice = np.random.rand(1)
            if config.ROT_AUG and dice > 0.5:
                pyr[i] = (np.random.rand(3) - 0.5) * 20                           # utils.rotate_cam(..., magnitude 20), utils.py:33
                warp_ids.append(i)
            elif config.ROT_IMAGE_AUG and dice <= 0.5:
                pyr[i, 2] = ((np.random.rand(1) - 0.5) * 170)[0]                   # utils.rotate_image, utils.py:62
                warp_ids.append(i)
    groups = [list(range(n))] if same_size else [[i] for i in range(n)]
    for g in groups:
        if config.SIM2REAL_AUG:
            merged = {"apply": np.concatenate([draws[i]["apply"] for i in g]), "order": np.concatenate([draws[i]["order"] for i in g]),
                      "par": np.concatenate([draws[i]["par"] for i in g]), "seeds": np.concatenate([draws[i]["seeds"] for i in g]),
                      "masks": [draws[i]["masks"][0] for i in g]}
            with _hip_section():
                if frames is not None:
                    frames = augment.sim2real_batch(frames, draw=merged)
                else:
                    out = augment.sim2real_batch(np.stack([samples[i].image for i in g]), draw=merged).cpu().numpy()
            if frames is None:
                for k, i in enumerate(g):
                    samples[i].image = out[k]
        ids = [i for i in g if i in warp_ids]
        if ids:
            quats = []
            for i in ids:
                if not (config.REGRESS_ORI or config.REGRESS_KEYPOINTS):
                    samples[i].ori = dataset.load_quaternion(samples[i].image_id)   # classification targets are re-encoded from the rotated pose
                quats.append(samples[i].ori)
            with _hip_section():
                if frames is not None:
                    import torch
                    sel = torch.as_tensor(ids, dtype=torch.int64, device=frames.device)
                    src = frames.index_select(0, sel)
                else:
                    src = np.stack([samples[i].image for i in ids])
                warped, t_new, q_new = augment.rotate_cam_batch(src, np.stack([samples[i].loc for i in ids]),
                                                                np.stack(quats), dataset.camera.K, pyr[ids])
                if frames is not None:
                    frames.index_copy_(0, sel, warped)
                else:
                    warped = warped.cpu().numpy()
                enc = None
                if not (config.REGRESS_ORI or config.REGRESS_KEYPOINTS):
                    enc = augment.encode_orientations(q_new, dataset.ori_histogram_map, dataset.ori_output_mask, config.BETA).cpu().numpy()
            for k, i in enumerate(ids):
                s = samples[i]
                s.loc, s.ori = t_new[k], q_new[k]
                if frames is None:
                    s.image = warped[k]
                if config.REGRESS_KEYPOINTS:
                    s.k1, s.k2 = augment.encode_as_keypoints(s.ori, s.loc)      # net.py:424, 433
                elif enc is not None:
                    s.ori = enc[k]
    return samples if frames is None else frames


def device_resize_applies(images, config):
    """Config.DEVICE_RESIZE and a batch augment.resize_images takes: uint8 RGB frames of one size, mode square / pad64."""
    if not getattr(config, "DEVICE_RESIZE", False) or config.IMAGE_RESIZE_MODE not in ("square", "pad64") or len(images) == 0:
        return False
    shape = getattr(images[0], "shape", None)
    return all(getattr(im, "dtype", None) == np.uint8 and im.ndim == 3 and im.shape[-1] == 3 and im.shape == shape for im in images)


def _device_resize_mode(config):
    return bool(getattr(config, "DEVICE_RESIZE", False)) and config.IMAGE_RESIZE_MODE in ("square", "pad64")


def check_cache_config(config):
    """Config.DEVICE_CACHE_GB caches the RAW frames Config.DEVICE_RESIZE uploads: without that path there is nothing to cache."""
    if float(getattr(config, "DEVICE_CACHE_GB", 0) or 0) > 0 and not getattr(config, "DEVICE_RESIZE", False):
        raise ValueError("Config.DEVICE_CACHE_GB = %r needs Config.DEVICE_RESIZE = True: the device cache holds the raw frames that "
                         "DEVICE_RESIZE uploads and resizes on the GPU" % (config.DEVICE_CACHE_GB,))


def cache_split(chosen, dataset, config, cache):
    """Config.DEVICE_CACHE_GB, one batch of samples of which those the cache holds carry no image: the samples whose frames have to go
    up (the misses) when the batch can be assembled on the device -- the misses are uint8 RGB frames of the cache's size, modes
    square / pad64 -- else None: the batch keeps the host path, and batches() first loads the images that were skipped."""
    missed = [s for s in chosen if s.image is not None]
    images = [s.image for s in missed]
    if _device_resize_mode(config) and (not missed or (device_resize_applies(images, config) and cache.accepts(images[0].shape))):
        return missed
    return None


class RawUploader(object):
    """DEVICE_RESIZE: a list of same-size uint8 frames [H,W,3] -> one host copy into a REUSED pinned buffer (two of them, alternating: a
    buffer is refilled only after the upload that last read it has run) -> `device` on this object's own stream -> `augment_fn` on the device
    tensor -> augment.resize_images.  Returns (uint8 CUDA tensor [B,OH,OW,3], window, scale, an event recorded behind that work, bytes of
    one pinned buffer).  The host copy runs outside hip.capture_lock; the lock is held where HIP is entered (no call while another thread
    captures a hipGraph): allocation, waiting for a buffer, and enqueueing the batch's copies and kernels.

    cache (Config.DEVICE_CACHE_GB, frame_cache.FrameCache): `frames` are then only the frames of `staged_ids`, the images of the batch
    `ids` that the cache does not hold.  Only they are pinned and uploaded (none: no pinned buffer is touched); the batch tensor is
    FrameCache.assemble's -- resident frames and the fresh upload gathered by one kernel, the new frames stored on the way -- and the
    augmentation and the resize run on it as on an uploaded batch.  The pinned buffers keep the capacity of a whole batch; the byte
    count returned is that of the frames this batch really put into pinned memory."""

    def __init__(self, device=None):
        self.device, self.stream, self.k = device, None, 0
        self.slots = [None, None]                              # [pinned tensor, event behind its last upload]

    def __call__(self, frames, config, augment_fn=None, cache=None, ids=None, staged_ids=None):
        import torch
        from . import augment
        if cache is not None:
            return self._cached(frames, config, augment_fn, cache, ids, staged_ids)
        shape = (len(frames),) + tuple(frames[0].shape)
        i = self.k & 1
        self.k += 1
        slot = self.slots[i]
        with _hip_section():
            if self.stream is None:
                self.stream = torch.cuda.Stream(device=self.device)
            if slot is None or tuple(slot[0].shape) != shape:
                slot = self.slots[i] = [torch.empty(shape, dtype=torch.uint8).pin_memory(), None]
            elif slot[1] is not None:
                slot[1].synchronize()
        host = slot[0].numpy()
        for b, f in enumerate(frames):
            host[b] = f
        with _hip_section(), torch.cuda.stream(self.stream):
            dev = slot[0].to(self.stream.device, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
            if augment_fn is not None:
                dev = augment_fn(dev)
            out, window, scale, _padding = augment.resize_images(dev, min_dim=config.IMAGE_MIN_DIM, max_dim=config.IMAGE_MAX_DIM,
                                                                 min_scale=config.IMAGE_MIN_SCALE, mode=config.IMAGE_RESIZE_MODE)
            ready = torch.cuda.Event()
            ready.record()
        return out, window, scale, ready, slot[0].numel()

    def _cached(self, frames, config, augment_fn, cache, ids, staged_ids):
        import torch
        from . import augment
        M = len(frames)
        assert M == len(staged_ids)
        slot = None
        if M:
            cap = (len(ids),) + tuple(frames[0].shape)         # a whole batch: the number of misses changes from batch to batch
            i = self.k & 1
            self.k += 1
            slot = self.slots[i]
        with _hip_section():
            if self.stream is None:
                self.stream = torch.cuda.Stream(device=self.device)
            if M:
                if slot is None or tuple(slot[0].shape[1:]) != cap[1:] or slot[0].shape[0] < M:
                    slot = self.slots[i] = [torch.empty(cap, dtype=torch.uint8).pin_memory(), None]
                elif slot[1] is not None:
                    slot[1].synchronize()
        if M:
            host = slot[0].numpy()
            for b, f in enumerate(frames):
                host[b] = f
        with _hip_section(), torch.cuda.stream(self.stream):
            staged, nbytes = None, 0
            if M:
                staged = slot[0][:M].to(self.stream.device, non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record()
                nbytes = staged.numel()
            dev = cache.assemble(ids, staged, staged_ids)
            if augment_fn is not None:
                dev = augment_fn(dev)
            out, window, scale, _padding = augment.resize_images(dev, min_dim=config.IMAGE_MIN_DIM, max_dim=config.IMAGE_MAX_DIM,
                                                                 min_scale=config.IMAGE_MIN_SCALE, mode=config.IMAGE_RESIZE_MODE)
            ready = torch.cuda.Event()
            ready.record()
        return out, window, scale, ready, nbytes


def finish_sample(sample, config):
    """The last third of load_image_gt (net.py:440-456): resize / pad and the image_meta vector."""
    original_shape = sample.image.shape
    image, window, scale, padding, crop = utils.resize_image(
        sample.image, min_dim=config.IMAGE_MIN_DIM, min_scale=config.IMAGE_MIN_SCALE, max_dim=config.IMAGE_MAX_DIM,
        mode=config.IMAGE_RESIZE_MODE)
    meta = compose_image_meta(sample.image_id, original_shape, image.shape, window, scale)
    return image, meta


class BatchAssembler(object):
    """Pre-allocated per-field arrays of one minibatch; `images` is uint8 (device path) or the molded float type (reference format)."""

    def __init__(self, config, batch_size, image_shape, meta_len, image_dtype, host_images=True):
        ft = np.float16 if config.F16 else np.float32
        self.config, self.n = config, batch_size
        # DEVICE_RESIZE (host_images=False): the finished frames never visit the host -- `device_images` is the uint8 CUDA tensor, `ready` the
        # event recorded behind the kernels that write it, `raw_pinned_bytes` the pinned memory the raw frames went up from
        self.images = np.zeros((batch_size,) + tuple(image_shape), dtype=image_dtype) if host_images else None
        self.device_images, self.ready, self.raw_pinned_bytes = None, None, 0
        self.meta = np.zeros((batch_size, meta_len), dtype=np.float64)
        self.loc = np.zeros((batch_size, 3 if config.REGRESS_LOC else config.LOC_BINS_PER_DIM ** 3), dtype=ft)
        if config.REGRESS_KEYPOINTS:
            self.k1, self.k2 = np.zeros((batch_size, 3), dtype=ft), np.zeros((batch_size, 3), dtype=ft)
            self.ori = None
        else:
            width = (4 if config.ORIENTATION_PARAM == 'quaternion' else 3) if config.REGRESS_ORI else config.ORI_BINS_PER_DIM ** 3
            self.ori = np.zeros((batch_size, width), dtype=ft)

    def put(self, b, image, meta, sample):
        if self.images is not None:
            self.images[b] = image
        self.meta[b] = meta
        self.loc[b] = sample.loc
        if self.ori is None:
            self.k1[b], self.k2[b] = np.asarray(sample.k1).T, np.asarray(sample.k2).T
        else:
            self.ori[b] = sample.ori

    def inputs(self):
        """[images, image_meta, gt_loc, gt_ori] (keypoints: [.., gt_loc, gt_k1, gt_k2]) -- the model input list of net.py:671-674."""
        if self.ori is None:
            return [self.images, self.meta, self.loc, self.k1, self.k2]
        return [self.images, self.meta, self.loc, self.ori]


DP_SHUFFLE_SEED = 1234


def batches(dataset, config, shuffle, batch_size, molded, workers=0, rank=0, world=1, device=None, cache=None):
    """Endless iterator of BatchAssembler objects.  molded=True: images are mean-subtracted floats (the reference's generator
    format); False: uint8 frames for the device path.  Up to 5 failing samples are logged and skipped, the 6th re-raises
    (net.py:553-559).  workers > 0 loads the raw samples of a batch with that many threads.

    world > 1 (data parallel, one process per GPU): every rank walks the SAME order over the dataset -- the shuffles come from a private
    RandomState(DP_SHUFFLE_SEED), identical on all ranks, instead of NumPy's global one -- and keeps samples [rank * batch_size,
    (rank + 1) * batch_size) of every global batch of world * batch_size: the ranks' shards are disjoint and together they are the batch a
    single process with GPU_COUNT = world would have drawn.  The global RNG (augmentation draws) is seeded with DP_SHUFFLE_SEED + rank so
    that the ranks do not apply identical warps to their different samples.  world == 1 is the reference's generator, draw for draw.

    device: the card Config.DEVICE_RESIZE uploads the raw frames to and resizes them on (None: the calling thread's current device).

    cache (frame_cache.FrameCache, molded=False only; DeviceFeeder makes one when Config.DEVICE_CACHE_GB > 0): the order, the draws and the
    label lookups are unchanged, but dataset.load_image is called only for the images the cache does not hold, only those are pinned and
    uploaded, and the batch is assembled on the device (RawUploader).  Batches DEVICE_RESIZE does not take keep the host path, uncached."""
    from .net import mold_image
    check_cache_config(config)
    if molded:
        cache = None
    ids = np.copy(dataset.image_ids)
    cursor, errors = -1, 0
    order_rng = None
    if world > 1:
        order_rng = np.random.RandomState(DP_SHUFFLE_SEED)
        np.random.seed(DP_SHUFFLE_SEED + int(rank))
    pool = None
    if workers > 0:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=workers)
    ft = np.float16 if config.F16 else np.float32
    uploader = RawUploader(device)                              # DEVICE_RESIZE: pinned buffers + the producer's own stream (upload, augmentation, resize)

    def safe_load(image_id, whole=False):
        try:
            return load_sample(dataset, config, image_id, with_image=whole or cache is None or not cache.has(image_id))
        except (GeneratorExit, KeyboardInterrupt):
            raise
        except Exception:
            logging.exception("Error processing image {}".format(dataset.image_info[image_id]))
            return None
    def advance():
        nonlocal cursor
        cursor = (cursor + 1) % len(ids)
        if shuffle and cursor == 0:
            (order_rng or np.random).shuffle(ids)
        return ids[cursor]
    while True:
        chosen = []
        for _ in range(rank * batch_size if world > 1 else 0):      # the samples of this global batch that belong to the ranks before this one
            advance()
        missed = None
        while True:
            while len(chosen) < batch_size:
                want = batch_size - len(chosen)
                todo = [advance() for _ in range(want)]
                loaded = list(pool.map(safe_load, todo)) if pool is not None else [safe_load(i) for i in todo]
                for s in loaded:
                    if s is None:
                        errors += 1
                        if errors > 5:
                            raise RuntimeError("more than 5 samples failed to load (net.py:553-559)")
                    else:
                        chosen.append(s)
            if cache is None:
                break
            missed = cache_split(chosen, dataset, config, cache)
            skipped = [k for k, s in enumerate(chosen) if s.image is None]
            if missed is not None or not skipped:
                break
            # the host path for this batch (mixed sizes ...): the frames the cache made us skip are loaded after all, by the same loader --
            # in the pool, a failure logged, counted and the sample replaced by the next one, like any other
            todo = [chosen[k].image_id for k in skipped]
            whole = lambda i: safe_load(i, True)
            loaded = list(pool.map(whole, todo)) if pool is not None else [whole(i) for i in todo]
            for k, s in zip(skipped, loaded):
                chosen[k] = s
                if s is None:
                    errors += 1
                    if errors > 5:
                        raise RuntimeError("more than 5 samples failed to load (net.py:553-559)")
            chosen = [s for s in chosen if s is not None]
        for _ in range((world - 1 - rank) * batch_size if world > 1 else 0):     # ... and to the ranks behind it
            advance()
        if missed is not None or (not molded and device_resize_applies([s.image for s in chosen], config)):
            if missed is not None:
                out, window, scale, ready, nbytes = uploader([s.image for s in missed], config,
                                                             lambda dev: augment_samples(chosen, dataset, config, frames=dev), cache=cache,
                                                             ids=[s.image_id for s in chosen], staged_ids=[s.image_id for s in missed])
                shape = cache.frame_shape
            else:
                shape = chosen[0].image.shape
                out, window, scale, ready, nbytes = uploader([s.image for s in chosen], config,
                                                             lambda dev: augment_samples(chosen, dataset, config, frames=dev))
            metas = [compose_image_meta(s.image_id, shape, tuple(out.shape[1:]), window, scale) for s in chosen]
            asm = BatchAssembler(config, batch_size, tuple(out.shape[1:]), len(metas[0]), np.uint8, host_images=False)
            asm.device_images, asm.ready, asm.raw_pinned_bytes = out, ready, nbytes
            for b, s in enumerate(chosen):
                asm.put(b, None, metas[b], s)
            yield asm
            continue
        augment_samples(chosen, dataset, config)
        asm = None
        for b, s in enumerate(chosen):
            image, meta = finish_sample(s, config)
            if asm is None:
                asm = BatchAssembler(config, batch_size, image.shape, len(meta), ft if molded else np.uint8)
            asm.put(b, mold_image(image.astype(ft), config) if molded else image, meta, s)
        yield asm


class DeviceFeeder(object):
    """Keeps the engine fed: a producer thread assembles uint8 batches into pinned host buffers (ring of `depth`), the consumer
    side copies batch k+1 to a device staging buffer on a SIDE stream while step k runs, and `next_into(engine)` makes the
    engine's input buffers hold the next batch (device-to-device copy ordered after the upload by an event)."""

    def __init__(self, engine, dataset, config, shuffle=True, workers=4, depth=3, rank=0, world=1):
        check_cache_config(config)
        import torch
        from .frame_cache import FrameCache
        self.eng, self.torch = engine, torch
        self.q = queue.Queue(maxsize=depth)
        self.stop = False
        self.err = None
        self.side = torch.cuda.Stream(device=engine.device)
        self.stage = [None, None]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [None, None]                           # recorded on the compute stream once a slot's batch has been copied out of it
        self.k = 0
        self.pinned_bytes = 0
        self.cache = FrameCache.from_config(config, engine.device)      # Config.DEVICE_CACHE_GB: this feeder's own, in this rank's HBM
        gen = batches(dataset, config, shuffle, engine.B, molded=False, workers=workers, rank=rank, world=world, device=engine.device,
                      cache=self.cache)

        def produce():
            from . import hip
            try:
                while not self.stop:
                    # the generator takes hip.capture_lock itself around its HIP sections (augment_samples: the batched augmentation kernels and
                    # their device-to-host copies); here only hipHostMalloc in pin_memory needs it -- not while the consumer thread captures a hipGraph
                    asm = next(gen)
                    on_device = asm.device_images is not None  # DEVICE_RESIZE: the frames are finished and stay where they are
                    arrays = [np.ascontiguousarray(a) for a in (([] if on_device else [asm.images]) + [asm.loc] +
                                                                ([asm.k1, asm.k2] if asm.ori is None else [asm.ori]))]
                    with hip.capture_lock:
                        host = [torch.from_numpy(a).pin_memory() for a in arrays]
                    self.q.put((([asm.device_images] if on_device else []) + host, asm.ready, asm.raw_pinned_bytes))
            except BaseException as e:                         # surfaced by next_into
                self.err = e
                self.q.put(None)
        self.thread = threading.Thread(target=produce, daemon=True)
        self.thread.start()
        self._upload()

    def _upload(self):
        torch = self.torch
        item = self.q.get()
        if item is None:
            raise self.err
        host, ready, raw_pinned = item
        slot = self.k & 1
        with torch.cuda.stream(self.side):
            if self.consumed[slot] is not None:
                self.side.wait_event(self.consumed[slot])      # the engine's copy out of this slot (two batches ago) must have run first
            if ready is not None:
                self.side.wait_event(ready)                    # DEVICE_RESIZE: the producer's resize kernel writes host[0] on its own stream
            if self.stage[slot] is None:
                self.stage[slot] = [torch.empty(h.shape, dtype=h.dtype, device=self.eng.device) for h in host]
            for d, h in zip(self.stage[slot], host):
                d.copy_(h, non_blocking=True)
                if h.is_cuda:
                    h.record_stream(self.side)                 # allocated on the producer's stream, read here
            self.events[slot].record(self.side)
        self._pending = (slot, host)                           # keep the pinned tensors alive until the copy has been consumed
        # pinned memory of one ring entry: the targets, and the frames as they went up (finished, or RAW with DEVICE_RESIZE)
        self.pinned_bytes = sum(h.numel() * h.element_size() for h in host if not h.is_cuda) + int(raw_pinned)

    def next_into(self):
        """Engine inputs <- the uploaded batch; immediately starts uploading the following one."""
        torch, eng = self.torch, self.eng
        slot, _ = self._pending
        torch.cuda.current_stream(eng.device).wait_event(self.events[slot])
        st = self.stage[slot]
        eng.load_batch_u8(st[0], st[1], st[2], st[3] if len(st) > 3 else None)
        if self.consumed[slot] is None:
            self.consumed[slot] = torch.cuda.Event()
        self.consumed[slot].record(torch.cuda.current_stream(eng.device))
        self.k += 1
        self._upload()

    def close(self):
        self.stop = True
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass


def eval_batch_plan(image_ids, batch_size):
    """The batches of one evaluation pass over `image_ids`, in order: [(row0, n, slot_ids)], where table rows row0 .. row0 + n - 1
    receive the n valid images and slot_ids lists the image of every one of the batch_size slots -- the tail batch repeats its last
    valid image in the padding slots (n < batch_size), which are computed and not scored.  No images: no batches."""
    ids = list(image_ids)
    out = []
    for row0 in range(0, len(ids), batch_size):
        chunk = ids[row0:row0 + batch_size]
        out.append((row0, len(chunk), chunk + [chunk[-1]] * (batch_size - len(chunk))))
    return out


class EvalBatch(object):
    """One uploaded evaluation batch: table rows [row0, row0 + n), device tensors `images` (uint8 frames, or molded float32 where the
    dataset's frames are not uint8 RGB), `loc_gt` fp64 [B,3], `q_gt` fp64 [B,4] (None from a label-free feeder) and, where a classification head needs them, the
    stored encoded targets `enc_loc` / `enc_ori` fp32 [B,K] (else None)."""
    __slots__ = ("row0", "n", "images", "loc_gt", "q_gt", "enc_loc", "enc_ori")

    def __init__(self, row0, n, tensors):
        self.row0, self.n = row0, n
        self.images, self.loc_gt, self.q_gt, self.enc_loc, self.enc_ori = tensors


class EvalFeeder(object):
    """Finite, ordered, augmentation-free input of evaluate(): walks dataset.image_ids once in order (eval_batch_plan).  Loader
    threads load every image with load_sample / finish_sample (host resize / pad -- with Config.DEVICE_RESIZE the producer instead uploads
    each batch of same-size uint8 RGB frames raw and finishes it with augment.resize_images; no augmentation: ROT_AUG, ROT_IMAGE_AUG and
    SIM2REAL_AUG are ignored, and the encoded targets are the dataset's stored ones); a producer thread assembles each batch in
    pinned memory (under hip.capture_lock, as DeviceFeeder does); iterating uploads batch k+1 on a side stream into the other half
    of a double buffer while batch k is used.  A batch's staging slot is reused only after the work the consumer put on the current
    stream while holding it (the forward pass and the scoring kernels) has run.  `loc_dtype` is the dtype of the dataset's locations.
    With labels=False (predict(): datasets without ground truth) no label loader of the dataset is called, only load_image, and the
    batches' `loc_gt` / `q_gt` are None; everything else is the same code.
    cache (frame_cache.FrameCache, the caller's: it outlives this feeder): images it holds are not loaded again -- load_image is called for
    the others only, they alone are pinned and uploaded, and the cache keeps them -- so a caller that evaluates one dataset repeatedly
    (once per checkpoint) with the same cache pays the decode once.  Needs Config.DEVICE_RESIZE; batches that path does not take (other
    dtypes, mixed sizes, 'crop') stay on the host path, uncached."""

    def __init__(self, model, dataset, config, enc_loc=False, enc_ori=False, workers=4, depth=3, labels=True, cache=None):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        assert labels or not (enc_loc or enc_ori), "the encoded targets are labels"
        check_cache_config(config)
        if cache is not None and not getattr(config, "DEVICE_RESIZE", False):
            raise ValueError("a frame cache (Config.DEVICE_CACHE_GB) needs Config.DEVICE_RESIZE = True")
        self.torch, self.eng = torch, model._engine
        self.plan = eval_batch_plan(dataset.image_ids, self.eng.B)
        self.q = queue.Queue(maxsize=depth)
        self.stop, self.err, self.loc_dtype = False, None, None
        self.side = torch.cuda.Stream(device=self.eng.device)
        self.stage = [None, None]
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [None, None]
        self.k = 0
        uploader = RawUploader(self.eng.device)                # DEVICE_RESIZE: pinned buffers + the producer's own stream (raw upload, resize)
        pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))

        def load(image_id, use_cache=True):
            held = use_cache and cache is not None and cache.has(image_id)
            image = None if held else dataset.load_image(image_id)
            loc = np.asarray(dataset.load_location(image_id)) if labels else None
            q = np.asarray(dataset.load_quaternion(image_id), dtype=np.float64) if labels else None
            el = np.asarray(dataset.load_location_encoded(image_id), dtype=np.float32) if enc_loc else None
            eo = np.asarray(dataset.load_orientation_encoded(image_id), dtype=np.float32) if enc_ori else None
            kind = "float"                                      # not uint8 RGB: molded on the host, as detect does for such frames
            if held:
                kind = "cached"                                 # resident on the device: gathered per batch by the producer
            elif getattr(image, "dtype", None) == np.uint8 and image.ndim == 3 and image.shape[-1] == 3:
                kind = "raw"                                    # DEVICE_RESIZE: finished per batch by the producer
                if not device_resize_applies([image], config):
                    kind, image = "u8", finish_sample(Sample(image_id, image, None, None), config)[0]
            return kind, image, loc, q, el, eo

        def produce():
            from . import hip
            try:
                for row0, n, slots in self.plan:
                    if self.stop:
                        return
                    got = dict(zip(slots[:n], pool.map(load, slots[:n])))
                    cached_ok = False
                    if cache is not None:
                        raw_ids = [i for i in got if got[i][0] == "raw"]
                        raws = [got[i][1] for i in raw_ids]
                        cached_ok = (all(r[0] in ("raw", "cached") for r in got.values()) and _device_resize_mode(config) and
                                     (not raws or (device_resize_applies(raws, config) and cache.accepts(raws[0].shape))))
                        if not cached_ok:                       # the host path for this batch: its resident frames are loaded after all
                            again = [i for i, r in got.items() if r[0] == "cached"]
                            got.update(zip(again, pool.map(lambda i: load(i, False), again)))
                    rows = [got[i] for i in slots]
                    if self.loc_dtype is None and labels:
                        self.loc_dtype = rows[0][2].dtype
                    frames, ready = {i: r[1] for i, r in got.items()}, None
                    if cached_ok:                               # only the misses go up; one gather builds the batch, tail repeats included
                        images, _w, _s, ready, _n = uploader(raws, config, cache=cache, ids=list(slots), staged_ids=raw_ids)
                    elif all(r[0] == "raw" for r in rows) and device_resize_applies([r[1] for r in rows], config):
                        images, _w, _s, ready, _n = uploader([r[1] for r in rows], config)      # uint8 CUDA tensor, finished
                    else:
                        for i, r in got.items():                # DEVICE_RESIZE with mixed frame sizes: the host path for this batch
                            if r[0] == "raw":
                                frames[i] = finish_sample(Sample(i, r[1], None, None), config)[0]
                        if any(r[0] == "float" for r in rows):
                            images = model.mold_inputs([frames[i] for i in slots])[0].astype(np.float32)
                        else:
                            images = np.stack([frames[i] for i in slots])
                    targets = [np.stack([r[2] for r in rows]).astype(np.float64), np.stack([r[3] for r in rows])] if labels else [None, None]
                    targets += [np.stack([r[k] for r in rows]) if rows[0][k] is not None else None for k in (4, 5)]
                    with hip.capture_lock:
                        pin = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
                        host = [images if ready is not None else pin(images)] + [pin(t) for t in targets]
                    self.q.put((row0, n, host, ready))
                self.q.put(None)
            except BaseException as e:                         # surfaced by the consumer
                self.err = e
                self.q.put(None)
            finally:
                pool.shutdown(wait=False)
        self.thread = threading.Thread(target=produce, daemon=True)
        self.thread.start()

    def _upload(self):
        """Starts the upload of the next batch on the side stream; returns False at the end of the plan."""
        torch = self.torch
        item = self.q.get()
        if item is None:
            if self.err is not None:
                raise self.err
            self._pending = None
            return False
        row0, n, host, ready = item
        slot = self.k & 1
        with torch.cuda.stream(self.side):
            if self.consumed[slot] is not None:
                self.side.wait_event(self.consumed[slot])      # the work that read this slot two batches ago must have run first
            if ready is not None:
                self.side.wait_event(ready)                    # DEVICE_RESIZE: host[0] is written by the producer's resize kernel
            st = self.stage[slot]
            if st is None or any((d is None) != (h is None) or (h is not None and (d.shape != h.shape or d.dtype != h.dtype))
                                 for d, h in zip(st, host)):
                st = self.stage[slot] = [None if h is None else torch.empty(h.shape, dtype=h.dtype, device=self.eng.device) for h in host]
            for d, h in zip(st, host):
                if h is not None:
                    d.copy_(h, non_blocking=True)
                    if h.is_cuda:
                        h.record_stream(self.side)
            self.events[slot].record(self.side)
        self._pending = (slot, row0, n, host)                  # the pinned tensors stay alive until their copy has been waited for
        self.k += 1
        return True

    def __iter__(self):
        torch = self.torch
        cur = torch.cuda.current_stream(self.eng.device)
        more = self._upload()
        while more:
            slot, row0, n, _host = self._pending
            cur.wait_event(self.events[slot])
            more = self._upload()                               # batch k+1 goes up while batch k is used
            yield EvalBatch(row0, n, self.stage[slot])
            if self.consumed[slot] is None:
                self.consumed[slot] = torch.cuda.Event()
            self.consumed[slot].record(cur)

    def close(self):
        self.stop = True
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass
