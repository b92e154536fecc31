"""Config.DEVICE_CACHE_GB on the GPU: the three byte-movement kernels of ursonet_amd/csrc/frame_cache.hip through the C ABI, the
FrameCache object, and the feeders / evaluate() / predict() that use it.  Nothing here is arithmetic: every comparison is torch.equal."""
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
HWS = [5 * 7, 16, 130 * 200]                                   # neither HW nor 3 HW a multiple of 16 | one unit | more than one chunk
GUARD = 96


def _arena(nbytes, seed):
    """A device buffer of noise to carve misaligned sources / destinations out of, and its host copy."""
    import torch
    host = np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)
    return torch.as_tensor(host).cuda(), host


def _table(values, dtype):
    import torch
    return torch.tensor(list(values), dtype=dtype).cuda()


def _frames(B, HW, seed):
    """uint8 noise [B,HW,3]; every second frame grey."""
    f = np.random.default_rng(seed).integers(0, 256, size=(B, HW, 3), dtype=np.uint8)
    f[1::2] = f[1::2, :, :1]
    return f


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("HW", HWS)
def test_grey_flags_equal_numpy(HW):
    """Noise, grey, grey but for the LAST pixel, grey but for the FIRST pixel, grey but for one channel of a middle pixel, grey again --
    as one batch of 6 at every source / flag alignment 0..3 (+ 13), and frame by frame with B = 1.  The bytes around the flags stay."""
    import torch
    from ursonet_amd import hip
    rng = np.random.default_rng(HW)
    f = rng.integers(0, 256, size=(6, HW, 3), dtype=np.uint8)
    f[1:] = f[1:, :, :1]
    f[2, HW - 1, 2] ^= 1
    f[3, 0, 1] ^= 0x80
    f[4, HW // 2, 0] ^= 4
    want = np.array([int(np.all(x[:, 0] == x[:, 1]) and np.all(x[:, 1] == x[:, 2])) for x in f], dtype=np.uint8)
    assert want.tolist() == [0, 1, 0, 0, 0, 1]
    for shift in (0, 1, 2, 3, 13):
        src, _ = _arena(f.size + 64, 1)
        src[shift:shift + f.size] = torch.as_tensor(f.reshape(-1)).cuda()
        flags, flags_host = _arena(64, 2)
        hip.frames_grey_flags_u8(6, HW, src[shift:shift + f.size], flags[shift + 1:shift + 7])
        torch.cuda.synchronize()
        flags_host[shift + 1:shift + 7] = want
        assert torch.equal(flags.cpu(), torch.as_tensor(flags_host)), (shift, flags.cpu()[shift + 1:shift + 7].tolist())
    for b in range(6):                                           # B = 1
        flags = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
        hip.frames_grey_flags_u8(1, HW, torch.as_tensor(f[b]).cuda(), flags[1:2])
        assert flags.cpu().tolist() == [7, int(want[b]), 7], b


def _slot_offsets(B, HW, first):
    """B destination offsets with 3 HW + GUARD bytes each, every one at a different alignment mod 16 (first, first + 5, ...)."""
    span = (3 * HW + GUARD + 15) & ~15
    return [GUARD + b * span + ((first + 5 * b) & 15) for b in range(B)], GUARD + B * span + GUARD


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("HW", HWS)
def test_put_then_gather_round_trips_a_mixed_batch(HW, B):
    """put: a mixed batch of kinds (RGB, grey plane, skip) into slots at odd, mutually different alignments; the whole arena is compared,
    so the guard bytes on both sides of every written range and the slots of kind 2 are untouched.  gather: from those slots, from a
    frame of the uploaded batch itself and twice from the same source, into a destination at an odd address with guards around it."""
    import torch
    from ursonet_amd import hip
    f = _frames(B, HW, 10 * HW + B)
    kinds = [1, 0, 2, 0, 1][:B] if B > 1 else [1]
    for first in (0, 1) if B > 1 else (0, 7):
        for flip in (False, True):
            if flip:
                kinds = [{0: 1, 1: 0, 2: 2}[k] for k in kinds]   # every slot position sees both kinds
            src, _ = _arena(f.size + 32, 3)
            s0 = 16 if first == 0 else 3                        # the uploaded batch aligned, and not
            src[s0:s0 + f.size] = torch.as_tensor(f.reshape(-1)).cuda()
            offs, size = _slot_offsets(B, HW, first)
            arena, want = _arena(size, 4)
            base = arena.data_ptr()
            hip.frames_put_u8(B, HW, src[s0:s0 + f.size], _table([base + o for o in offs], torch.int64), _table(kinds, torch.uint8))
            torch.cuda.synchronize()
            for b, (o, k) in enumerate(zip(offs, kinds)):
                if k == 0:
                    want[o:o + HW] = f[b, :, 0]
                elif k == 1:
                    want[o:o + 3 * HW] = f[b].reshape(-1)
            nbad = int((arena.cpu() != torch.as_tensor(want)).sum())
            assert torch.equal(arena.cpu(), torch.as_tensor(want)), "put HW %d B %d first %d kinds %s: %d bytes differ" % (HW, B, first, kinds, nbad)
            # gather B + 3 slots: the B cache slots in reverse order, then slot 0 again (a duplicate), a frame of the staged batch, a skip
            g_src = [base + offs[b] for b in reversed(range(B))] + [base + offs[0], src.data_ptr() + s0 + (B - 1) * 3 * HW, base + offs[0]]
            g_kind = [kinds[b] for b in reversed(range(B))] + [kinds[0], 1, 2]
            n = len(g_src)
            d0 = 5 if first else 32
            dst, dwant = _arena(d0 + n * 3 * HW + GUARD, 5)
            hip.frames_gather_u8(n, HW, _table(g_src, torch.int64), _table(g_kind, torch.uint8), dst[d0:d0 + n * 3 * HW])
            torch.cuda.synchronize()
            stored = {b: (f[b] if kinds[b] == 1 else np.repeat(f[b, :, :1], 3, axis=1)) for b in range(B) if kinds[b] != 2}
            rows = [stored.get(b) for b in reversed(range(B))] + [stored.get(0), f[B - 1], None]
            for j, r in enumerate(rows):
                if r is not None:
                    dwant[d0 + j * 3 * HW:d0 + (j + 1) * 3 * HW] = r.reshape(-1)
            nbad = int((dst.cpu() != torch.as_tensor(dwant)).sum())
            assert torch.equal(dst.cpu(), torch.as_tensor(dwant)), "gather HW %d B %d first %d kinds %s: %d bytes differ" % (HW, B, first, g_kind, nbad)
            assert torch.equal(arena.cpu(), torch.as_tensor(want)) and torch.equal(src[s0:s0 + f.size].cpu(), torch.as_tensor(f.reshape(-1)))


def test_invalid_arguments_return_einval_and_launch_nothing():
    import torch
    from ursonet_amd import hip
    L, HW, B = hip._lib, 35, 2
    src = torch.as_tensor(_frames(B, HW, 0)).cuda()
    dst = torch.full((B, HW, 3), 9, dtype=torch.uint8, device="cuda")
    flags = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
    addr, kind = _table([dst.data_ptr(), dst.data_ptr() + 3 * HW], torch.int64), _table([1, 1], torch.uint8)
    st = hip.stream_ptr()
    p = lambda t: t.data_ptr()
    bad = [L.urso_frames_grey_flags_u8(-1, HW, p(src), p(flags), st), L.urso_frames_grey_flags_u8(B, -5, p(src), p(flags), st),
           L.urso_frames_grey_flags_u8(B, HW, None, p(flags), st), L.urso_frames_grey_flags_u8(B, HW, p(src), None, st),
           L.urso_frames_put_u8(-1, HW, p(src), p(addr), p(kind), st), L.urso_frames_put_u8(B, -1, p(src), p(addr), p(kind), st),
           L.urso_frames_put_u8(B, HW, None, p(addr), p(kind), st), L.urso_frames_put_u8(B, HW, p(src), None, p(kind), st),
           L.urso_frames_put_u8(B, HW, p(src), p(addr), None, st), L.urso_frames_put_u8(70000, HW, p(src), p(addr), p(kind), st),
           L.urso_frames_gather_u8(-1, HW, p(addr), p(kind), p(dst), st), L.urso_frames_gather_u8(B, -1, p(addr), p(kind), p(dst), st),
           L.urso_frames_gather_u8(B, HW, None, p(kind), p(dst), st), L.urso_frames_gather_u8(B, HW, p(addr), None, p(dst), st),
           L.urso_frames_gather_u8(B, HW, p(addr), p(kind), None, st), L.urso_frames_gather_u8(B, 1 << 30, p(addr), p(kind), p(dst), st)]
    assert bad == [EINVAL] * len(bad), bad
    assert "urso_frames_gather_u8" in hip.last_error()
    assert L.urso_frames_put_u8(0, HW, p(src), p(addr), p(kind), st) == 0 and L.urso_frames_gather_u8(B, 0, p(addr), p(kind), p(dst), st) == 0
    torch.cuda.synchronize()
    assert int((dst != 9).sum()) == 0 and flags.cpu().tolist() == [9, 9]
    with pytest.raises(hip.UrsoHipError):
        hip.frames_grey_flags_u8(-1, HW, src, flags)
    hip.frames_put_u8(B, HW, src, addr, kind)                     # and the valid call does run
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


# ------------------------------------------------------------------ FrameCache
def _assemble(cache, frames, ids):
    import torch
    hits, misses = cache.lookup(ids)
    staged = torch.as_tensor(np.stack([frames[i] for i in misses])).cuda() if misses else None
    out = cache.assemble(ids, staged, misses)
    torch.cuda.synchronize()
    want = torch.as_tensor(np.stack([frames[i] for i in ids]))
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(want.shape)
    assert torch.equal(out.cpu(), want), (ids, hits, misses)
    return out, hits, misses


def test_frame_cache_serves_hits_misses_and_mixtures_across_slab_boundaries():
    """9 frames of 13 x 17 (HW = 221: nothing is a multiple of 16), slabs of two RGB frames, a budget of three slabs.  Frame 2 is grey.
    Fed in order, 5 of the 9 fit: slab 0 = {0, 1}, slab 1 (grey) = {2}, slab 2 = {3, 4}; 5 .. 8 are refused and stay misses."""
    import torch
    from ursonet_amd.frame_cache import FrameCache, GREY, RGB, round16
    H, W = 13, 17
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(9)]
    frames[2] = np.repeat(frames[2][:, :, :1], 3, axis=2)
    slab = 2 * round16(3 * H * W)
    cache = FrameCache("cuda", budget_bytes=3 * slab + 100, slab_bytes=slab)
    assert cache.lookup([0, 1, 1]) == ([], [0, 1]) and cache.stats()["slabs"] == 0
    for ids in ([0, 1, 2], [3, 4, 5], [6, 7, 8]):
        _, hits, misses = _assemble(cache, frames, ids)
        assert hits == [] and misses == ids
    st = cache.stats()
    assert sorted(cache.planner.entries) == [0, 1, 2, 3, 4] and st["slabs"] == 3 and st["slab_bytes"] == 3 * slab <= cache.budget_bytes
    assert (st["grey_frames"], st["rgb_frames"], st["frozen"]) == (1, 4, True) and (st["hits"], st["misses"]) == (0, 9)
    assert cache.planner.entries[2] == (GREY, 1, 0) and cache.planner.entries[4] == (RGB, 2, 1) and len(cache.slabs) == 3
    out, hits, misses = _assemble(cache, frames, [4, 3, 2, 1, 0])                  # all hits, both pools, all three slabs
    assert misses == [] and out.data_ptr() not in [s.data_ptr() for s in cache.slabs]
    _, hits, misses = _assemble(cache, frames, [8, 2, 5, 0, 5])                    # a mixture with a repeated miss
    assert hits == [2, 0] and misses == [8, 5]
    _assemble(cache, frames, [2, 2, 2, 4])                                         # a padded tail: one source three times
    assert sorted(cache.planner.entries) == [0, 1, 2, 3, 4] and cache.stats()["slabs"] == 3         # the refused stay refused
    # the returned batch is the caller's: writing into it never reaches a slab
    out, _, _ = _assemble(cache, frames, [0, 2, 4, 6])
    out.fill_(0xAB)
    torch.cuda.synchronize()
    again, _, _ = _assemble(cache, frames, [0, 2, 4, 6])                           # compared with the ORIGINAL frames in _assemble
    assert again.data_ptr() != out.data_ptr() and int((out != 0xAB).sum()) == 0
    _assemble(cache, frames, [4, 2, 0])
    # per batch slot: 0 + 5 + 2 + 4 + 3 + 3 + 3 served from slabs, 9 + 0 + 3 + 0 + 1 + 1 + 0 from the upload
    assert cache.stats()["hits"] == 20 and cache.stats()["misses"] == 14


# ------------------------------------------------------------------ feeders
def _dataset(cfg, n, sizes, seed=11, grey_every=3):
    """An in-memory dataset of native-size uint8 RGB frames whose load_image counts its calls per id; every grey_every-th frame is grey
    (one plane three times), the others are tinted."""
    from ursonet_amd.dataset import SyntheticPoses

    class Counting(SyntheticPoses):
        def load_image(self, image_id):
            with self.lock:
                self.calls[int(image_id)] = self.calls.get(int(image_id), 0) + 1
            return self.frames[int(image_id)]
    ds = Counting(n, sizes[0][0], sizes[0][1], cfg, seed=seed)
    ds.lock, ds.calls = threading.Lock(), {}
    rng = np.random.default_rng(seed)
    ds.frames = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:h, 0:w]
        f = rng.integers(0, 40, size=(h, w, 3)) + (((yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2) < (0.2 * h) ** 2)[:, :, None] * rng.integers(60, 200, size=(1, 1, 3))
        f = f.astype(np.uint8)
        if grey_every and i % grey_every == 0:
            f = np.repeat(f[:, :, :1], 3, axis=2)
        ds.frames.append(f)
    return ds


def _run(eng, ds, cfg, cache_gb, n=9, device_resize=True):
    """DeviceFeeder from a fixed seed of every generator the input side draws from -> ([(in_images_u8, gt_loc, gt_ori)] of n batches,
    pinned_bytes behind each batch, load_image calls per id, the feeder's cache)."""
    import random
    import torch
    from ursonet_amd import augment
    from ursonet_amd.feeder import DeviceFeeder
    cfg.DEVICE_RESIZE, cfg.DEVICE_CACHE_GB = device_resize, cache_gb
    ds.calls = {}
    np.random.seed(5); random.seed(5); augment._PIPELINE_RNG.seed(7)
    out, pinned = [], []
    feed = None
    try:
        feed = DeviceFeeder(eng, ds, cfg, shuffle=True, workers=2)
        for _ in range(n):
            pinned.append(feed.pinned_bytes)                                   # of the batch next_into is about to hand over
            feed.next_into()
            torch.cuda.synchronize()
            out.append((eng.in_images_u8.cpu().clone(), eng.gt_loc.cpu().clone(), eng.gt_ori.cpu().clone()))
    finally:
        if feed is not None:
            feed.close()
            feed.thread.join(60)                                               # it draws from the global generators: it must be gone before the next seed
            assert not feed.thread.is_alive()
        cfg.DEVICE_RESIZE, cfg.DEVICE_CACHE_GB = False, 0
    return out, pinned, dict(ds.calls), feed.cache


def _same(a, b):
    import torch
    assert len(a) == len(b) and len(a) >= 3
    for k, (x, y) in enumerate(zip(a, b)):
        nbad = int((x[0] != y[0]).sum())
        assert torch.equal(x[0], y[0]), "batch %d: %d differing image bytes of %d" % (k, nbad, x[0].numel())
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), "batch %d: targets differ" % k
    assert not torch.equal(a[0][0], a[1][0]) and int(a[0][0].max()) > 0           # really different, non-empty batches


def _engine(h=64, w=128, aug=False):
    from util import make_config
    from ursonet_amd.engine import Engine
    cfg = make_config("resnet18", h, w, batch=4, regress_ori=True, dtype="float32")
    cfg.ROT_AUG = cfg.SIM2REAL_AUG = aug
    return cfg, Engine(cfg, "training", seed=1)


@pytest.mark.parametrize("aug", [False, True])
def test_device_feeder_serves_three_epochs_from_one_load_per_image(aug, monkeypatch):
    """12 in-memory frames (130 x 200 -> 64 x 128, pad64; ids 0, 3, 6, 9 grey), batch 4, 9 batches = three epochs, ResNet-18.  With
    DEVICE_CACHE_GB set the engine receives the in_images_u8 bytes and the targets of the DEVICE_RESIZE-only run from the same seeds --
    plain, and with ROT_AUG + SIM2REAL_AUG working in place on the assembled batches -- while every image is loaded exactly once
    (uncached: once per epoch at least) and a late batch pins no raw frame."""
    from ursonet_amd import frame_cache
    monkeypatch.setattr(frame_cache, "SLAB_BYTES", 1 << 20)                     # 1 MiB slabs (13 RGB frames): the budget of 1 GiB is never the limit
    cfg, eng = _engine(aug=aug)
    ds = _dataset(cfg, 12, [(130, 200)])
    ref, pinned_ref, calls_ref, none = _run(eng, ds, cfg, 0)
    got, pinned, calls, cache = _run(eng, ds, cfg, 1)
    assert none is None and cache is not None
    _same(ref, got)
    assert sorted(calls) == list(range(12)) and set(calls.values()) == {1}, calls
    assert sorted(calls_ref) == list(range(12)) and min(calls_ref.values()) >= 3, calls_ref
    st = cache.stats()
    assert (st["grey_frames"], st["rgb_frames"]) == (4, 8) and st["frame_shape"] == (130, 200, 3)
    assert st["frame_bytes"] == 4 * 130 * 200 + 8 * 3 * 130 * 200
    raw = 4 * 130 * 200 * 3
    assert pinned_ref[0] == pinned_ref[8] == pinned[0] and pinned_ref[8] - pinned[8] == raw       # epoch 1 pins what the parent pins; epoch 3 no frame
    assert all(p == pinned[8] for p in pinned[3:])
    if aug:
        cfg2, eng2 = _engine(aug=False)
        plain, _, _, _ = _run(eng2, ds, cfg2, 0)
        assert any(not np.array_equal(p[0].numpy(), o[0].numpy()) for p, o in zip(plain, ref))        # the augmentation did something


def test_a_budget_of_five_frames_keeps_the_batches_and_reloads_exactly_the_uncached(monkeypatch):
    """Slabs of one RGB frame (or three grey planes), a budget of five slabs: the batches stay those of the uncached run, the images that
    found a slot are loaded once, and exactly the others are loaded again in every epoch."""
    from ursonet_amd import frame_cache
    cfg, eng = _engine()
    ds = _dataset(cfg, 12, [(130, 200)])
    slab = frame_cache.round16(3 * 130 * 200)
    monkeypatch.setattr(frame_cache, "SLAB_BYTES", slab)
    ref, _, _, _ = _run(eng, ds, cfg, 0)
    got, pinned, calls, cache = _run(eng, ds, cfg, (5 * slab + 1000) / float(1 << 30))
    _same(ref, got)
    st = cache.stats()
    held = set(cache.planner.entries)
    assert cache.budget_bytes == 5 * slab + 1000 and st["slabs"] == 5 and st["slab_bytes"] == 5 * slab and st["frozen"]
    assert 5 <= len(held) < 12 and st["rgb_frames"] + (st["grey_frames"] + 2) // 3 <= 5
    # the exact set: without augmentation only the shuffles draw from the seeded global generator, so the order in which the images
    # meet the cache is known, and the planner (tests/test_frame_cache_cpu.py) says which of them find a slot
    order, ids = np.random.RandomState(5), np.arange(12)
    sim = frame_cache.FramePlanner(130 * 200, 5 * slab + 1000, slab)
    for _ in range(3):
        order.shuffle(ids)
        for i in ids:
            sim.assign(int(i), frame_cache.GREY if i % 3 == 0 else frame_cache.RGB)
    assert held == set(sim.entries) and {i: cache.planner.entries[i] for i in held} == sim.entries, (sorted(held), sorted(sim.entries))
    assert {i for i, c in calls.items() if c > 1} == set(range(12)) - held, (calls, held)
    assert all(calls[i] == 1 for i in held) and all(calls[i] >= 3 for i in set(range(12)) - held)
    assert st["refused"] > 0


def test_mixed_sizes_and_crop_keep_the_host_path_with_identical_batches(monkeypatch):
    from ursonet_amd import frame_cache
    monkeypatch.setattr(frame_cache, "SLAB_BYTES", 1 << 20)
    cfg, eng = _engine()
    ds = _dataset(cfg, 14, [(130, 200), (128, 256), (130, 200)])                 # batches with both sizes
    ref, _, _, _ = _run(eng, ds, cfg, 0, n=6, device_resize=False)
    got, _, calls, cache = _run(eng, ds, cfg, 1, n=6)
    _same(ref, got)
    assert cache.frame_shape in (None, (130, 200, 3), (128, 256, 3))
    from util import make_config
    from ursonet_amd.engine import Engine
    crop = make_config("resnet18", 64, 64, batch=4, regress_ori=True, dtype="float32")
    crop.IMAGE_RESIZE_MODE = "crop"
    crop.update()
    ds = _dataset(crop, 14, [(130, 200)])
    eng = Engine(crop, "training", seed=1)
    ref, _, calls_ref, _ = _run(eng, ds, crop, 0, n=6, device_resize=False)
    got, _, calls, cache = _run(eng, ds, crop, 1, n=6)
    _same(ref, got)
    assert cache.stats()["slabs"] == 0 and cache.stats()["hits"] == 0 and cache.frame_shape is None      # 'crop': untouched and uncached
    assert sum(calls.values()) >= 24 and sum(calls_ref.values()) >= 24                             # every sample of every batch was loaded


# ------------------------------------------------------------------ evaluate(), predict()
def test_evaluate_and_predict_load_every_image_once_with_a_shared_cache(tmp_path):
    """10 images at batch 4 (the padded tail batch repeats image 9): evaluate() twice and predict() once with one FrameCache give the
    tables of the uncached calls; the first pass loads each image once, the later ones load nothing."""
    from util import make_config
    from ursonet_amd import evaluate as ev, net, predict as pr
    from ursonet_amd.frame_cache import FrameCache, round16
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=True, dtype="float32")
    cfg.NAME = "syn"
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    path = str(tmp_path / "weights_cache_0001.npz")
    tr.save_weights(path)
    del tr
    model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    model.load_weights(path, path, by_name=True)
    ds = _dataset(cfg, 10, [(130, 200)])
    with pytest.raises(ValueError):
        ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0, cache=FrameCache(model._engine.device, 1 << 24))      # DEVICE_RESIZE is off
    cfg.DEVICE_RESIZE = True
    try:
        ref = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0)
        pref = pr.predict(model, ds)
        cache = FrameCache(model._engine.device, budget_bytes=1 << 24, slab_bytes=4 * round16(3 * 130 * 200))
        ds.calls = {}
        first = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0, cache=cache)
        assert ds.calls == {i: 1 for i in range(10)}, ds.calls
        ds.calls = {}
        second = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0, cache=cache)
        pred = pr.predict(model, ds, cache=cache)
        assert ds.calls == {}, ds.calls
    finally:
        cfg.DEVICE_RESIZE = False
    for res in (first, second):
        for k in ("loc_est", "q_est", "loc_err", "ori_err", "esa", "dist"):
            assert np.array_equal(getattr(ref, k), getattr(res, k)), k
        assert list(res.image_ids) == list(ds.image_ids) and np.all(np.isfinite(res.esa))
    assert np.array_equal(pref.loc_est, pred.loc_est) and np.array_equal(pref.q_est, pred.q_est)
    st = cache.stats()
    assert (st["grey_frames"], st["rgb_frames"]) == (4, 6) and st["misses"] == 12 and st["hits"] == 24        # 3 batches of 4 slots per pass
