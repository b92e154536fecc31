"""Config.DEVICE_CACHE_GB without a GPU: the slot allocator and budget arithmetic of ursonet_amd/frame_cache.py (FramePlanner: pure
Python), the batch plan of a padded evaluation tail, the configuration key and its check, and the C ABI's new symbols."""
import numpy as np
import pytest

from ursonet_amd.frame_cache import GREY, RGB, FramePlanner, round16


def _ranges(p):
    """[(slab, first, last + 1)] of every entry."""
    out = []
    for e in p.entries.values():
        slab, first, count = p.byte_range(e)
        out.append((slab, first, first + count))
    return out


@pytest.mark.parametrize("hw", [5 * 7, 16, 130 * 200, 960 * 1280, 1200 * 1920 + 1])
def test_slot_strides_are_multiples_of_16_and_hold_a_frame(hw):
    p = FramePlanner(hw, 1 << 40, 1 << 30)
    assert p.stride[GREY] % 16 == 0 and p.stride[RGB] % 16 == 0
    assert hw <= p.stride[GREY] < hw + 16 and 3 * hw <= p.stride[RGB] < 3 * hw + 16
    assert p.frame_bytes == {GREY: hw, RGB: 3 * hw}
    assert p.slots_per_slab[GREY] == (1 << 30) // p.stride[GREY] and p.slots_per_slab[RGB] == (1 << 30) // p.stride[RGB]
    assert round16(0) == 0 and round16(1) == 16 and round16(16) == 16 and round16(17) == 32


def test_slab_count_follows_the_budget_and_a_refused_frame_stays_refused():
    hw = 130 * 200
    slab = 2 * round16(3 * hw)                                  # two RGB frames per slab
    p = FramePlanner(hw, 3 * slab + slab // 2, slab)            # 3.5 slabs of budget: three slabs
    assert p.max_slabs == 3 and p.slots_per_slab[RGB] == 2
    asked = []
    p._alloc = lambda pool, k: asked.append((pool, k)) or True
    got = [p.assign(i, RGB) for i in range(6)]
    assert got == [(RGB, 0, 0), (RGB, 0, 1), (RGB, 1, 0), (RGB, 1, 1), (RGB, 2, 0), (RGB, 2, 1)]
    assert asked == [(RGB, 0), (RGB, 1), (RGB, 2)] and p.slab_total_bytes == 3 * slab <= p.budget_bytes and not p.frozen
    assert p.assign(6, RGB) is None and p.frozen and 6 not in p                 # the 7th: a fourth slab would exceed the budget
    assert p.assign(6, RGB) is None and p.assign(7, RGB) is None and p.assign(6, RGB) is None
    assert p.assign(8, GREY) is None                             # no slab for the other pool either: the cache has stopped growing
    assert len(asked) == 3 and len(p.slab_pool) == 3 and p.full()
    assert p.assign(2, RGB) == (RGB, 1, 0)                       # a held id keeps its slot
    st = p.stats()
    assert st["rgb_frames"] == 6 and st["grey_frames"] == 0 and st["slabs"] == 3 and st["slab_bytes"] == 3 * slab
    assert st["frame_bytes"] == 6 * 3 * hw and st["refused"] == 5 and st["frozen"]
    assert p.lookup([7, 0, 6, 0, 5, 7]) == ([0, 5], [7, 6])


def test_a_budget_below_one_slab_and_a_budget_of_zero_cache_nothing():
    for budget in (0, 999):
        p = FramePlanner(16, budget, 1000)
        assert p.max_slabs == 0 and p.assign(0, GREY) is None and p.assign(0, RGB) is None and p.frozen and p.stats()["slabs"] == 0
    p = FramePlanner(1000, 1 << 20, 2000)                        # a slab smaller than an RGB frame: only grey frames find room
    assert p.slots_per_slab[RGB] == 0 and p.assign(0, RGB) is None and p.assign(1, GREY) == (GREY, 0, 0)


def test_a_failed_allocation_freezes_the_cache_like_the_budget():
    p = FramePlanner(64, 1 << 20, 64 * 3 * 2, alloc=lambda pool, k: k < 1)
    assert p.assign(0, RGB) == (RGB, 0, 0) and p.assign(1, RGB) == (RGB, 0, 1)
    assert p.assign(2, RGB) is None and p.frozen and len(p.slab_pool) == 1 and p.assign(3, GREY) is None


def test_grey_and_rgb_pools_fill_independently():
    hw = 100                                                    # strides 112 and 304; a slab of 640 bytes holds 5 grey or 2 RGB frames
    p = FramePlanner(hw, 3 * 640, 640)
    assert p.stride == {GREY: 112, RGB: 304} and p.slots_per_slab == {GREY: 5, RGB: 2}
    assert p.assign("a", RGB) == (RGB, 0, 0)
    assert p.assign("b", GREY) == (GREY, 1, 0)
    assert p.assign("c", RGB) == (RGB, 0, 1)
    assert p.assign("d", RGB) == (RGB, 2, 0)                     # the RGB pool opens the third slab, the grey slab keeps filling
    assert [p.assign(k, GREY) for k in "efgh"] == [(GREY, 1, 1), (GREY, 1, 2), (GREY, 1, 3), (GREY, 1, 4)]
    assert p.assign("i", GREY) is None and p.frozen              # a fourth slab is over budget ...
    assert not p.full()
    assert p.assign("j", RGB) == (RGB, 2, 1)                     # ... but the open RGB slab still takes a frame
    assert p.assign("k", RGB) is None and p.full()
    assert p.slab_pool == [RGB, GREY, RGB] and p.used == [2, 5, 2]
    st = p.stats()
    assert (st["grey_frames"], st["rgb_frames"], st["frame_bytes"]) == (5, 4, 5 * 100 + 4 * 300)


@pytest.mark.parametrize("hw", [35, 16, 26000])
def test_ids_map_to_distinct_non_overlapping_byte_ranges_inside_their_slabs(hw):
    slab = 3 * round16(3 * hw) + 7                              # not a multiple of any stride
    p = FramePlanner(hw, 50 * slab, slab)
    rng = np.random.default_rng(hw)
    for i in range(60):
        p.assign(i, GREY if rng.random() < 0.5 else RGB)
    assert len(p.entries) == 60 and len(set(p.entries.values())) == 60
    ranges = sorted(_ranges(p))
    for slab_k, first, end in ranges:
        assert first % 16 == 0 and 0 <= first < end <= slab and 0 <= slab_k < len(p.slab_pool)
    for a, b in zip(ranges, ranges[1:]):
        assert a[0] != b[0] or a[2] <= b[1], (a, b)              # same slab: the earlier range ends before the later one starts
    for i, (pool, k, slot) in p.entries.items():
        assert p.slab_pool[k] == pool and slot < p.slots_per_slab[pool]


def test_the_padded_tail_of_eval_batch_plan_yields_duplicate_sources():
    from ursonet_amd.feeder import eval_batch_plan
    plan = eval_batch_plan(list(range(10)), 4)
    p = FramePlanner(64, 1 << 20, 1 << 12)
    held_before = set()
    for row0, n, slots in plan:
        hits, misses = p.lookup(slots)
        assert set(hits) == held_before & set(slots) and misses == slots[:n]
        puts, sources = p.plan(slots, misses, [i % 2 == 0 for i in misses])
        assert [j for j, _ in puts] == list(range(n)) and len(sources) == 4
        assert sources[:n] == [("staged", j) for j in range(n)]
        assert all(src == sources[n - 1] for src in sources[n:])                  # the tail repeats its last image: the same source
        held_before |= set(slots)
    assert plan[-1][1] == 2 and plan[-1][2] == [8, 9, 9, 9]
    # second pass: everything is resident, nothing is staged, the tail's three slots read one slab range
    for row0, n, slots in plan:
        assert p.lookup(slots) == (slots[:n], [])
        puts, sources = p.plan(slots, [], None)
        assert puts == [] and all(s[0] == "slab" for s in sources)
        assert [s[1] for s in sources] == [p.entries[i] for i in slots]
    tail = [s[1] for s in p.plan([8, 9, 9, 9], [], None)[1]]
    assert tail[1] == tail[2] == tail[3] != tail[0]
    assert p.entries[8][0] == GREY and p.entries[9][0] == RGB
    with pytest.raises(KeyError):
        p.plan([99], [], None)


def test_config_key_defaults_to_off_and_needs_device_resize():
    from ursonet_amd.config import Config
    from ursonet_amd import feeder
    from ursonet_amd.frame_cache import FrameCache
    cfg = Config()
    assert cfg.DEVICE_CACHE_GB == 0 and Config.DEVICE_CACHE_GB == 0
    assert FrameCache.from_config(cfg) is None
    feeder.check_cache_config(cfg)
    cfg.DEVICE_CACHE_GB = 2
    for make in (lambda: feeder.DeviceFeeder(None, None, cfg), lambda: feeder.EvalFeeder(None, None, cfg),
                 lambda: next(feeder.batches(None, cfg, True, 4, molded=False))):
        with pytest.raises(ValueError) as e:
            make()
        assert "DEVICE_CACHE_GB" in str(e.value) and "DEVICE_RESIZE" in str(e.value)
    cfg.DEVICE_RESIZE = True
    feeder.check_cache_config(cfg)
    c = FrameCache.from_config(cfg)
    assert c.budget_bytes == 2 << 30 and c.slab_bytes == 1 << 30 and c.stats()["slabs"] == 0 and c.lookup([3, 3, 4]) == ([], [3, 4])


def test_the_abi_declares_and_exports_the_three_entry_points():
    import ursonet_amd.hip as hip
    for name in ("urso_frames_grey_flags_u8", "urso_frames_put_u8", "urso_frames_gather_u8"):
        assert name in hip.EXPORTED_SYMBOLS and hasattr(hip._lib, name)
