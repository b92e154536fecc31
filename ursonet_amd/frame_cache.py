"""Config.DEVICE_CACHE_GB: decoded frames stay resident in HBM across epochs.

The reference reloads (decodes) every frame in every epoch.  Here a frame is decoded ONCE: the first time a feeder meets an image it goes
up raw, as before (Config.DEVICE_RESIZE), and is also stored in a slab of device memory; from then on a batch that needs it is assembled
on the device from the resident bytes -- no dataset.load_image, no pinned copy, no upload.

Layout.  Storage is a list of fixed-size uint8 slab tensors (SLAB_BYTES, 1 GiB by default), allocated lazily, never freed, never moved.
Every slab belongs to one of two pools: GREY holds frames whose three channels are equal everywhere (urso_frames_grey_flags_u8 decides,
on the uploaded bytes) as ONE plane of H W bytes, RGB holds every other frame as its 3 H W bytes.  A slab is an array of slots of the pool's
stride (the frame's byte count rounded up to 16, so that every slot starts 16-byte aligned and the kernels take their all-vector path).
`image_id -> (pool, slab, slot)` is a dict.  A byte budget caps the sum of the slab sizes: when the next slab would exceed it -- or its
allocation runs out of device memory -- the cache stops growing for good and the frames that found no slot simply stay misses.  There is no
eviction: every frame is needed once per epoch, so LRU would evict exactly what is needed next.

FramePlanner is that bookkeeping alone (pure Python, no torch: tests/test_frame_cache_cpu.py); FrameCache owns the slabs and issues the
kernels (ursonet_amd/csrc/frame_cache.hip).

Two rules.  (1) The batch FrameCache.assemble returns is a FRESH tensor: augmentation works on it in place and never sees a slab.
(2) Frames are assumed IMMUTABLE per image_id: the cache never looks at the dataset again for an id it holds, so a dataset whose
load_image(i) changes between calls (on-the-fly synthesis with new noise, files rewritten during training) must not be cached.  One cache
serves one (dataset, device, frame shape).
"""
import logging

GREY, RGB, SKIP = 0, 1, 2                       # pools; also the `kind` bytes of urso_frames_put_u8 / urso_frames_gather_u8
SLAB_BYTES = 1 << 30                            # default slab size (FrameCache.from_config reads it at call time)


def round16(n):
    return (int(n) + 15) & ~15


class FramePlanner(object):
    """Slot allocator and budget arithmetic of FrameCache.  frame_pixels = H W; budget_bytes caps the sum of the slab sizes; slab_bytes is
    the size of every slab.  `alloc(pool, slab_index) -> bool` is asked for every new slab once the budget has admitted it (FrameCache:
    the device allocation); False freezes the planner exactly as the budget does."""

    def __init__(self, frame_pixels, budget_bytes, slab_bytes=None, alloc=None):
        if frame_pixels <= 0:
            raise ValueError("frame_pixels must be positive")
        self.frame_pixels = int(frame_pixels)
        self.budget_bytes = max(0, int(budget_bytes))
        self.slab_bytes = int(SLAB_BYTES if slab_bytes is None else slab_bytes)
        self.frame_bytes = {GREY: self.frame_pixels, RGB: 3 * self.frame_pixels}
        self.stride = {GREY: round16(self.frame_pixels), RGB: round16(3 * self.frame_pixels)}
        self.slots_per_slab = {p: self.slab_bytes // s for p, s in self.stride.items()}
        self.slab_pool = []                     # pool of slab k
        self.used = []                          # slots taken in slab k
        self.open = {GREY: None, RGB: None}     # the slab of each pool that still has free slots
        self.entries = {}                       # image_id -> (pool, slab, slot)
        self.frozen = False                     # no further slab: over budget, or an allocation failed
        self.refused = 0
        self._alloc = alloc

    @property
    def max_slabs(self):
        return self.budget_bytes // self.slab_bytes if self.slab_bytes > 0 else 0

    @property
    def slab_total_bytes(self):
        return len(self.slab_pool) * self.slab_bytes

    def __contains__(self, image_id):
        return image_id in self.entries

    def full(self):
        """Nothing can be added any more: no further slab and no free slot in either pool's open slab."""
        return self.frozen and all(self._free(p) == 0 for p in (GREY, RGB))

    def _free(self, pool):
        k = self.open[pool]
        return 0 if k is None else self.slots_per_slab[pool] - self.used[k]

    def assign(self, image_id, pool):
        """The slot of `image_id` in `pool` -> (pool, slab, slot); None when the cache cannot take it (it stays a miss).  An id that is
        already held keeps its entry."""
        if image_id in self.entries:
            return self.entries[image_id]
        if self._free(pool) == 0:
            k = len(self.slab_pool)
            if self.frozen or self.slots_per_slab[pool] == 0 or k + 1 > self.max_slabs:
                self.frozen = self.frozen or k + 1 > self.max_slabs
                self.refused += 1
                return None
            if self._alloc is not None and not self._alloc(pool, k):
                self.frozen = True
                self.refused += 1
                return None
            self.slab_pool.append(pool)
            self.used.append(0)
            self.open[pool] = k
        k = self.open[pool]
        entry = (pool, k, self.used[k])
        self.used[k] += 1
        self.entries[image_id] = entry
        return entry

    def byte_range(self, entry):
        """(slab, first byte, byte count) of an entry inside its slab."""
        pool, slab, slot = entry
        return slab, slot * self.stride[pool], self.frame_bytes[pool]

    def lookup(self, ids):
        """(hits, misses): the ids held, and the ids not held -- each id once, in order of first appearance."""
        hits, misses, seen = [], [], set()
        for i in ids:
            if i in seen:
                continue
            seen.add(i)
            (hits if i in self.entries else misses).append(i)
        return hits, misses

    def plan(self, ids, staged_ids, staged_grey):
        """One batch.  ids: the image of every batch slot (repeats allowed: the padded tail batch of evaluate()); staged_ids: the
        images uploaded for it, frame j of the staging tensor being staged_ids[j]; staged_grey[j]: truthy = that frame is grey (may be
        None when nothing can be added).  Assigns slots to the staged images that are not held yet and returns
            puts     [(j, entry)]                      staged frame j is stored at entry
            sources  [("slab", entry) | ("staged", j)] where each batch slot is gathered from
        An id that is neither held nor staged is an error."""
        where = {}
        for j, i in enumerate(staged_ids):
            where.setdefault(i, j)
        puts = []
        for i, j in where.items():
            if i not in self.entries and staged_grey is not None:
                entry = self.assign(i, GREY if staged_grey[j] else RGB)
                if entry is not None:
                    puts.append((j, entry))
        sources = []
        for i in ids:
            if i in where:
                sources.append(("staged", where[i]))       # the uploaded bytes, whether or not they were stored as well
            elif i in self.entries:
                sources.append(("slab", self.entries[i]))
            else:
                raise KeyError("image %r is neither cached nor staged" % (i,))
        return puts, sources

    def stats(self):
        held = {GREY: 0, RGB: 0}
        for pool, _slab, _slot in self.entries.values():
            held[pool] += 1
        return {"grey_frames": held[GREY], "rgb_frames": held[RGB], "slabs": len(self.slab_pool), "slab_bytes": self.slab_total_bytes,
                "frame_bytes": held[GREY] * self.frame_bytes[GREY] + held[RGB] * self.frame_bytes[RGB], "budget_bytes": self.budget_bytes,
                "frozen": self.frozen, "refused": self.refused}


class FrameCache(object):
    """The device side.  budget_bytes / slab_bytes as in FramePlanner; the frame shape (H, W) is fixed by the first batch assembled.
    Not thread-safe: one producer thread uses it at a time (lookups from loader threads happen while that thread waits for them)."""

    def __init__(self, device=None, budget_bytes=0, slab_bytes=None):
        self.device = device
        self.budget_bytes = int(budget_bytes)
        self.slab_bytes = int(SLAB_BYTES if slab_bytes is None else slab_bytes)
        self.frame_shape = None                 # (H, W, 3)
        self.planner = None
        self.slabs = []
        self.hits = self.misses = 0
        self._last = None                       # (stream, event behind the last kernels that touched the slabs)

    @classmethod
    def from_config(cls, config, device=None):
        """The cache Config.DEVICE_CACHE_GB asks for (None when it is 0)."""
        gb = float(getattr(config, "DEVICE_CACHE_GB", 0) or 0)
        if gb <= 0:
            return None
        return cls(device, int(round(gb * (1 << 30))), SLAB_BYTES)

    # ------------------------------------------------------------------ host-side queries
    def has(self, image_id):
        return self.planner is not None and image_id in self.planner.entries

    def accepts(self, shape):
        """Frames of this shape ([H,W,3] uint8) can go through this cache."""
        shape = tuple(int(x) for x in shape)
        return len(shape) == 3 and shape[2] == 3 and shape[0] * shape[1] > 0 and (self.frame_shape is None or self.frame_shape == shape)

    def lookup(self, ids):
        if self.planner is None:
            hits, misses = FramePlanner(1, 0, 1).lookup(ids)
            return hits, misses
        return self.planner.lookup(ids)

    def stats(self):
        st = self.planner.stats() if self.planner is not None else FramePlanner(1, self.budget_bytes, self.slab_bytes).stats()
        st.update(hits=self.hits, misses=self.misses, frame_shape=self.frame_shape)
        return st

    # ------------------------------------------------------------------ device side
    def _alloc_slab(self, pool, k):
        import torch
        assert k == len(self.slabs)
        try:
            self.slabs.append(torch.empty(self.slab_bytes, dtype=torch.uint8, device=self.device))
        except RuntimeError as e:               # torch.cuda.OutOfMemoryError is one
            if "out of memory" not in str(e).lower():
                raise
            logging.warning("FrameCache: slab %d (%d bytes) does not fit into device memory; the cache stops growing at %d bytes",
                            k, self.slab_bytes, k * self.slab_bytes)
            return False
        return True

    def _address(self, entry):
        slab, first, count = self.planner.byte_range(entry)
        assert 0 <= first and first + count <= self.slab_bytes
        return self.slabs[slab].data_ptr() + first

    def assemble(self, ids, staged=None, staged_ids=(), stream=None):
        """The uint8 batch [B,H,W,3] of the images `ids`, a fresh tensor.  staged: uint8 device tensor [M,H,W,3] with the frames of
        staged_ids (the misses of lookup(ids), already uploaded on `stream`), or None when every id is held.  The new frames are
        classified (one read-back of M flag bytes), given slots and stored (urso_frames_put_u8); then one urso_frames_gather_u8 builds
        the batch from slab slots and staged frames alike.  stream: a torch stream (None: the current one)."""
        import torch
        from . import hip
        ids, staged_ids = list(ids), list(staged_ids)
        M = len(staged_ids)
        if M:
            assert staged is not None and staged.is_cuda and staged.dtype == torch.uint8 and staged.is_contiguous()
            assert staged.dim() == 4 and staged.shape[0] == M and staged.shape[3] == 3
            shape = tuple(int(x) for x in staged.shape[1:])
            if self.frame_shape is None:
                self.frame_shape = shape
                self.planner = FramePlanner(shape[0] * shape[1], self.budget_bytes, self.slab_bytes, alloc=self._alloc_slab)
                if self.device is None:
                    self.device = staged.device
            assert shape == self.frame_shape, "one FrameCache serves one frame shape"
        assert self.planner is not None, "nothing cached and nothing staged"
        H, W = self.frame_shape[:2]
        HW, B = H * W, len(ids)
        dev = staged.device if M else self.slabs[0].device
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            cur = torch.cuda.current_stream(dev)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])   # another stream stored the frames this one is about to read
            grey = None
            fresh = [i for i in staged_ids if i not in self.planner.entries]
            if fresh and not self.planner.full():
                flags = torch.empty(M, dtype=torch.uint8, device=dev)
                hip.frames_grey_flags_u8(M, HW, staged, flags, cur)
                grey = flags.cpu().tolist()     # waits for the upload and the flags kernel on this stream
            puts, sources = self.planner.plan(ids, staged_ids, grey)
            staged_base = staged.data_ptr() if M else 0
            addr, kind = [0] * M, [SKIP] * M
            for j, entry in puts:
                addr[j], kind[j] = self._address(entry), entry[0]
            for src in sources:
                if src[0] == "staged":
                    addr.append(staged_base + src[1] * 3 * HW)
                    kind.append(RGB)
                    self.misses += 1
                else:
                    addr.append(self._address(src[1]))
                    kind.append(src[1][0])
                    self.hits += 1
            addr_d = torch.tensor(addr, dtype=torch.int64).to(dev)
            kind_d = torch.tensor(kind, dtype=torch.uint8).to(dev)
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
            if puts:
                hip.frames_put_u8(M, HW, staged, addr_d[:M], kind_d[:M], cur)
            hip.frames_gather_u8(B, HW, addr_d[M:], kind_d[M:], out, cur)
            ev = torch.cuda.Event()
            ev.record(cur)
            self._last = (cur, ev)
        return out
