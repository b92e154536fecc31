#!/usr/bin/env python3
"""What Config.DEVICE_CACHE_GB buys, on one GPU (ResNet-50, 512 x 640, bf16, B = 32).

  python tools/cache_bench.py [--runs 5] [--out profiles/frame_cache_bench.json]

  kernels   urso_frames_grey_flags_u8 / urso_frames_put_u8 / urso_frames_gather_u8 on 32 URSO-size (960 x 1280) and 32 SPEED-size
            (1200 x 1920) frames, grey and RGB kinds: --kernel-iters warm launches each (torch events; min / median / max) and the
            bytes each moves per second.
  memory    DeviceFeeder images/s and DeviceFeeder + engine.step() images/s over PRE-GENERATED 960 x 1280 frames held in host memory, three
            cases alternated in one process, --runs runs each: `parent` (DEVICE_RESIZE alone: what the feeder did before the cache),
            `epoch1` (cache on, the first pass: every batch is uploaded, classified and stored) and `steady` (cache on, timed after a
            whole warm pass: every batch is gathered from HBM).  `parent_spread` = (max - min) / median of the parent's runs; the
            acceptance condition is steady median >= parent median * (1 - parent_spread).
  synthetic the same with SyntheticPoses at 960 x 1280, whose generator (~NumPy noise + a blob per frame) stands in for a slow decoder.
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def mmm(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3), "runs": len(v)}


def in_memory_dataset(cfg, n, h, w, seed=1):
    """Grey frames replicated to RGB (what the datasets' loaders return) with every fourth one tinted, so that both pools are used."""
    from ursonet_amd.dataset import SyntheticPoses

    class InMemory(SyntheticPoses):
        def load_image(self, image_id):
            return self.frames[int(image_id)]
    ds = InMemory(n, h, w, cfg, seed=seed)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ds.frames = []
    for i in range(n):
        blob = ((yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2) < (rng.uniform(0.12, 0.3) * h) ** 2
        grey = (rng.integers(0, 12, size=(h, w)) + blob * rng.integers(80, 220)).astype(np.uint8)
        f = np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))
        if i % 4 == 3:
            f[:, :, 2] //= 2
        ds.frames.append(f)
    return ds


def kernel_times(iters):
    import torch
    from ursonet_amd import hip
    out = {}
    for name, (h, w) in (("urso_960x1280", (960, 1280)), ("speed_1200x1920", (1200, 1920))):
        B, HW = 32, h * w
        rgb = torch.randint(0, 256, (B, HW, 3), dtype=torch.uint8, device="cuda")
        grey = rgb[:, :, :1].expand(B, HW, 3).contiguous()
        slab = torch.empty(B * 3 * HW, dtype=torch.uint8, device="cuda")
        dst = torch.empty((B, HW, 3), dtype=torch.uint8, device="cuda")
        flags = torch.empty(B, dtype=torch.uint8, device="cuda")
        a_rgb = torch.tensor([slab.data_ptr() + b * 3 * HW for b in range(B)], dtype=torch.int64).cuda()
        a_grey = torch.tensor([slab.data_ptr() + b * HW for b in range(B)], dtype=torch.int64).cuda()
        k0, k1 = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.ones(B, dtype=torch.uint8, device="cuda")
        cases = {
            "grey_flags_grey": (lambda: hip.frames_grey_flags_u8(B, HW, grey, flags), B * 3 * HW),
            "grey_flags_rgb": (lambda: hip.frames_grey_flags_u8(B, HW, rgb, flags), B * 3 * HW),
            "put_rgb": (lambda: hip.frames_put_u8(B, HW, rgb, a_rgb, k1), 2 * B * 3 * HW),
            "gather_rgb": (lambda: hip.frames_gather_u8(B, HW, a_rgb, k1, dst), 2 * B * 3 * HW),
            "put_grey": (lambda: hip.frames_put_u8(B, HW, grey, a_grey, k0), B * 4 * HW),
            "gather_grey": (lambda: hip.frames_gather_u8(B, HW, a_grey, k0, dst), B * 4 * HW),
        }
        res = {}
        for cname, (fn, nbytes) in cases.items():
            for _ in range(3):
                fn()
            ms = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            res[cname] = {"ms": mmm(ms), "bytes": nbytes, "TBps_at_median": round(nbytes / (statistics.median(ms) * 1e-3) / 1e12, 3)}
        out[name] = res
        del rgb, grey, slab, dst
        torch.cuda.empty_cache()
    return out


def feeder_run(eng, ds, cfg, cache_gb, warm, k, step, workers):
    import torch
    from ursonet_amd.feeder import DeviceFeeder
    cfg.DEVICE_RESIZE, cfg.DEVICE_CACHE_GB, cfg.ROT_AUG, cfg.SIM2REAL_AUG = True, cache_gb, False, False
    feed = DeviceFeeder(eng, ds, cfg, shuffle=True, workers=workers)
    try:
        for _ in range(warm):
            feed.next_into()
            if step:
                eng.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            feed.next_into()
            if step:
                eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        pinned = feed.pinned_bytes
        stats = feed.cache.stats() if feed.cache is not None else None
    finally:
        feed.close()
        feed.thread.join(120)
        cfg.DEVICE_RESIZE, cfg.DEVICE_CACHE_GB = False, 0
    return k * eng.B / dt, pinned, stats


def three_cases(eng, ds, cfg, runs, frames, batches, workers, gb, parent_batches=None):
    """parent / epoch1 / steady, alternated; -> {"feeder": {...}, "train_loop": {...}}."""
    per_epoch = frames // eng.B
    out = {}
    for step in (False, True):
        res = {"parent": [], "epoch1": [], "steady": []}
        extra = {}
        for _ in range(runs):
            r = feeder_run(eng, ds, cfg, 0, 2, parent_batches or batches, step, workers)
            res["parent"].append(r[0]); extra["parent_pinned_bytes"] = r[1]
            # the first pass of a fresh cache: the constructor has batch 0 under way, the window is the rest of the epoch
            r = feeder_run(eng, ds, cfg, gb, 0, max(1, per_epoch - 1), step, workers)
            res["epoch1"].append(r[0]); extra["epoch1_pinned_bytes"] = r[1]
            r = feeder_run(eng, ds, cfg, gb, per_epoch + 4, batches, step, workers)
            res["steady"].append(r[0]); extra["steady_pinned_bytes"] = r[1]; extra["steady_cache"] = r[2]
        p = mmm(res["parent"])
        spread = (p["max"] - p["min"]) / p["median"]
        s = mmm(res["steady"])
        out["train_loop" if step else "feeder"] = dict(
            parent_img_s=p, epoch1_img_s=mmm(res["epoch1"]), steady_img_s=s, parent_spread=round(spread, 4),
            steady_over_parent=round(s["median"] / p["median"], 3), accepted=bool(s["median"] >= p["median"] * (1 - spread)), **extra)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--synthetic-frames", type=int, default=64)
    ap.add_argument("--synthetic-runs", type=int, default=3)
    ap.add_argument("--synthetic-parent-batches", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--cache-gb", type=float, default=8)
    ap.add_argument("--skip", default="", help="comma list of sections to skip: kernels, memory, synthetic")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "frame_cache_bench.json"))
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    import torch
    from util import make_config
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.engine import Engine
    H, W, h, w, B = 960, 1280, 512, 640, 32
    out = {"gpu": torch.cuda.get_device_name(0), "backbone": a.backbone, "native": [H, W], "model": [h, w], "batch": B, "dtype": "bfloat16",
           "cache_gb": a.cache_gb, "workers": a.workers}
    if "kernels" not in skip:
        out["kernels"] = kernel_times(a.kernel_iters)
    cfg = make_config(a.backbone, h, w, batch=B, regress_ori=False, ori_bins=24, dtype="bfloat16")
    eng = Engine(cfg, "training", seed=1)
    if "memory" not in skip:
        ds = in_memory_dataset(cfg, a.frames, H, W)
        feeder_run(eng, ds, cfg, a.cache_gb, 1, 2, True, a.workers)         # warm-up: graph capture, code objects, pinned pools
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50):
            eng.step()
        torch.cuda.synchronize()
        out["bare_step_ms"] = round((time.perf_counter() - t0) / 50 * 1e3, 3)
        out["memory"] = dict(frames=a.frames, runs=a.runs, timed_batches=a.batches,
                             **three_cases(eng, ds, cfg, a.runs, a.frames, a.batches, a.workers, a.cache_gb))
        del ds
    if "synthetic" not in skip:
        syn = SyntheticPoses(a.synthetic_frames, H, W, cfg, seed=3)
        t0 = time.perf_counter()
        syn.load_image(0)
        out["synthetic"] = dict(frames=a.synthetic_frames, runs=a.synthetic_runs, timed_batches=a.batches,
                                parent_timed_batches=a.synthetic_parent_batches, load_image_ms=round((time.perf_counter() - t0) * 1e3, 1),
                                **three_cases(eng, syn, cfg, a.synthetic_runs, a.synthetic_frames, a.batches, a.workers, a.cache_gb,
                                              parent_batches=a.synthetic_parent_batches))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
