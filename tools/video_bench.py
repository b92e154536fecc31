#!/usr/bin/env python3
"""Throughput of track() (ursonet_amd/video.py) against the reference's per-frame video loop, on one GPU.

  python tools/video_bench.py [--backbone resnet50] [--h 512] [--w 576] [--n 256] [--n-loop 8] [--reps 5] [--out profiles/video_bench.json]
                              [--prep-stats DIR] [--bench-json FILE]

Synthetic 960 x 1280 uint8 frames held in memory, the reference's VideoPrep (crop 1 / 150 columns, pad 400, weights 0.21 / 0.72 / 0.07:
1760 x 1929 x 3 per prepared frame), soft classification with n = 24, bf16, initial weights.  Resize mode pad64 turns the prepared frame
into 512 x 561 inside 512 x 576, so that is the engine's input size here (a 512 x 640 engine does not take this frame: track() says so).
For IMAGES_PER_GPU 32 and 1: a warm-up pass of each variant, then `reps` timed passes of track() and of track(render=True), alternated
(at batch 1 the reference's loop joins the alternation: VideoPrep.host + model.detect([frame]) + decode_orientations + pose_unreal per
frame, over --n-loop frames; it has no drawing, OpenCV being no dependency).  Every pass ends in a device synchronise.  Reported: min /
median / max frames per second.  No threshold: nothing of this path had been measured before.

The prep kernel's own time comes from a run of its own under the profiler, which this script only feeds and reads:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/video_bench.py --role prep-kernel
  python tools/video_bench.py ... --prep-stats DIR

--role prep-kernel launches urso_video_prep_u8 alone (32 frames, 20 launches after 3 warm-up launches); --prep-stats DIR reads the
profiler's kernel statistics from DIR and records the kernel's average time, the bytes it moves (the cropped source once + the whole
output) and their rate as a fraction of 8.0 TB/s (HBM3E peak) and of 6.29 TB/s (what a float4 copy reaches on this part).  Prints one
JSON line."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAME_H, FRAME_W = 960, 1280
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
PREP_KERNEL = "video_prep_kernel"


def make_frames(n, cfg, distinct=16):
    """n frames in memory, each its own array; `distinct` different pictures, repeated."""
    from ursonet_amd.dataset import SyntheticPoses
    ds = SyntheticPoses(distinct, FRAME_H, FRAME_W, cfg, seed=1)
    base = [ds.load_image(i) for i in ds.image_ids]
    return ds, [base[i % distinct].copy() for i in range(n)]


def prep_bytes(prep, B):
    oh, ow = prep.out_shape(FRAME_H, FRAME_W)
    ch, cw = oh - 2 * prep.pad, ow - 2 * prep.pad
    return B * 3 * (ch * cw + oh * ow)


def role_prep_kernel():
    import torch
    from ursonet_amd import augment
    from ursonet_amd.video import VideoPrep
    prep, B = VideoPrep(), 32
    rng = np.random.default_rng(0)
    raw = torch.as_tensor(rng.integers(0, 256, size=(B, FRAME_H, FRAME_W, 3), dtype=np.uint8)).cuda()
    out = None
    for _ in range(23):
        out = augment.video_prep(raw, prep, out=out)
    torch.cuda.synchronize()
    print(json.dumps({"role": "prep-kernel", "B": B, "launches": 23, "bytes_per_launch": prep_bytes(prep, B)}))


def read_prep_stats(d):
    """Average nanoseconds and calls of the prep kernel from the profiler's *kernel_stats.csv under d."""
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if PREP_KERNEL in (row.get("Name") or ""):
                    return {"calls": int(float(row["Calls"])), "avg_ns": float(row["AverageNs"]), "min_ns": float(row.get("MinNs") or "nan"),
                            "max_ns": float(row.get("MaxNs") or "nan"), "file": os.path.basename(path)}
    raise SystemExit("no %s row in a *kernel_stats.csv under %s" % (PREP_KERNEL, d))


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=576)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-loop", type=int, default=8)
    ap.add_argument("--ori-bins", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--prep-stats", default=None)
    ap.add_argument("--role", default=None, help="prep-kernel: only launch urso_video_prep_u8 (for a profiler run)")
    ap.add_argument("--bench-json", default=None, help="reuse the timings of an earlier run of this script; only --prep-stats is (re)read")
    a = ap.parse_args()
    if a.role == "prep-kernel":
        role_prep_kernel()
        return
    from ursonet_amd import video
    prep = video.VideoPrep()
    if a.bench_json:
        with open(a.bench_json) as f:
            out = json.load(f)
        finish(a, out, prep)
        return
    import torch
    from util import make_config
    from ursonet_amd import net, utils
    from ursonet_amd.infer import loader_workers
    stat = lambda v: {"min": float(min(v)), "median": float(np.median(v)), "max": float(max(v)), "runs": [float(x) for x in v]}   # noqa: E731
    out = {"backbone": a.backbone, "h": a.h, "w": a.w, "dtype": "bfloat16", "ori_bins": a.ori_bins, "frame": [FRAME_H, FRAME_W], "n": a.n,
           "n_loop": a.n_loop, "reps": a.reps, "prepared_frame": list(prep.out_shape(FRAME_H, FRAME_W)) + [3], "unit": "frames/s"}
    td = tempfile.mkdtemp()
    for B in [int(b) for b in a.batches.split(",")]:
        cfg = make_config(a.backbone, a.h, a.w, batch=B, regress_ori=False, ori_bins=a.ori_bins, dtype="bfloat16")
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=td)
        ds, frames = make_frames(a.n, cfg)
        sunk = [0]

        def sink(i, f):
            sunk[0] += f.shape[0]

        def loop():
            for f in frames[:a.n_loop]:
                r = model.detect([prep.host(f)])[0]
                q = utils.decode_orientations(r["ori"][None], ds.ori_histogram_map)[0]
                video.pose_unreal(r["loc"], q)
        variants = [("track", lambda: video.track(model, frames, ds, prep=prep), a.n),
                    ("track_render", lambda: video.track(model, frames, ds, prep=prep, render=True, sink=sink), a.n)]
        if B == 1:
            variants.append(("reference_loop", loop, a.n_loop))
        for _name, fn, _n in variants:                                     # warm-up: capture, code objects, pinned buffers
            fn()
        rates = {name: [] for name, _, _ in variants}
        for _ in range(a.reps):
            for name, fn, n in variants:
                rates[name].append(timed(fn, n))
        for name in rates:
            out["%s_B%d" % (name, B)] = stat(rates[name])
        del model
        torch.cuda.empty_cache()
    out["box"] = "one %s, LOADER_WORKERS %d" % (torch.cuda.get_device_name(0), loader_workers(cfg))
    finish(a, out, prep)


def finish(a, out, prep):
    if a.prep_stats:
        s = read_prep_stats(a.prep_stats)
        by = prep_bytes(prep, 32)
        rate = by / (s["avg_ns"] * 1e-9)
        out["prep_kernel"] = dict(s, B=32, bytes_per_launch=by, bytes_per_s=rate, fraction_of_hbm_peak_8_0_TBs=rate / HBM_PEAK,
                                  fraction_of_float4_copy_6_29_TBs=rate / HBM_COPY, source="rocprofv3 --kernel-trace --stats, a run of its own")
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
