#!/usr/bin/env python3
"""What Config.DEVICE_RESIZE buys, on one GPU, from native-size frames held in memory.

  python tools/resize_bench.py [--runs 5] [--out profiles/resize_bench.json]

  kernel    urso_resize_images_u8 for B = 32 at 960 x 1280 -> 512 x 640 (URSO) and 1200 x 1920 -> 640 x 960 (SPEED), pad64, both
            URSO_RESIZE_COMPAT modes: median of --kernel-iters warm launches (torch events), next to the time the same bytes (frames
            read once + result written) take at the rate tools/hbm_probe.py's read-heavy 4:1 stream reaches on this box (restated here).
  feeder    DeviceFeeder images/s with DEVICE_RESIZE off and on, alternated in one process, --runs runs each (min / median / max), from
            a dataset that returns PRE-GENERATED 960 x 1280 frames (SyntheticPoses.load_image would dominate both sides), without
            augmentation and with ROT_AUG + SIM2REAL_AUG.  The host path makes ~4 frames/s, so its timed window is --host-batches
            batch(es) (the batch the producer works on while the first is uploaded: if anything in the host path's favour); the device
            path is timed over --device-batches after --device-warm.
  train     the same loop with engine.step() consuming every batch (what UrsoNet.train sees), and the bare step time of that engine.
  evaluate  evaluate() images/s off and on over --eval-n frames (tools/eval_bench.py's setup: bf16, soft-classification head).
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def mmm(v):
    return {"min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2), "runs": len(v)}


def in_memory_dataset(cfg, n, h, w, seed=1):
    from ursonet_amd.dataset import SyntheticPoses

    class InMemory(SyntheticPoses):
        def load_image(self, image_id):
            return self.frames[int(image_id)]
    ds = InMemory(n, h, w, cfg, seed=seed)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ds.frames = []
    for _ in range(n):
        blob = ((yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2) < (rng.uniform(0.12, 0.3) * h) ** 2
        grey = (rng.integers(0, 12, size=(h, w)) + blob * rng.integers(80, 220)).astype(np.uint8)
        ds.frames.append(np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2)))
    return ds


def hbm_rate():
    """tools/hbm_probe.py's read4_write1 stream at 335 MB [bytes/s]."""
    import torch
    n = 335 * 1000 * 1000 // 2
    x4 = torch.randn(n, device="cuda", dtype=torch.bfloat16).view(-1, 4)
    y1 = torch.empty(x4.shape[0], device="cuda", dtype=torch.bfloat16)
    for _ in range(3):
        torch.sum(x4, dim=1, out=y1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        torch.sum(x4, dim=1, out=y1)
    e1.record()
    torch.cuda.synchronize()
    return 1.25 * 335e6 / (e0.elapsed_time(e1) / 20 * 1e-3)


def kernel_times(iters, rate):
    import torch
    from ursonet_amd import augment
    out = {}
    for name, (h, w, mn, mx) in (("urso_960x1280_to_512x640", (960, 1280, 512, 640)), ("speed_1200x1920_to_640x960", (1200, 1920, 640, 960))):
        x = torch.randint(0, 256, (32, h, w, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty((32, mn, mx, 3), dtype=torch.uint8, device="cuda")
        nbytes = x.numel() + dst.numel()
        for compat in ("0.18", "0.19"):
            os.environ["URSO_RESIZE_COMPAT"] = compat
            for _ in range(3):
                augment.resize_images(x, min_dim=mn, max_dim=mx, mode="pad64", out=dst)
            ms = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                augment.resize_images(x, min_dim=mn, max_dim=mx, mode="pad64", out=dst)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            out["%s_compat%s" % (name, compat)] = {"ms": mmm(ms), "bytes": nbytes, "ms_at_hbm_rate": round(nbytes / rate * 1e3, 4),
                                                   "images_per_s": round(32 / (statistics.median(ms) * 1e-3))}
        os.environ.pop("URSO_RESIZE_COMPAT", None)
        del x, dst
    return out


def feeder_run(eng, ds, cfg, on, aug, warm, k, step):
    import torch
    from ursonet_amd.feeder import DeviceFeeder
    cfg.DEVICE_RESIZE, cfg.ROT_AUG, cfg.SIM2REAL_AUG = on, aug, aug
    feed = DeviceFeeder(eng, ds, cfg, shuffle=True, workers=4)
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
    finally:
        feed.close()
        feed.thread.join(120)
        cfg.DEVICE_RESIZE = False
    return k * eng.B / dt, dt / k * 1e3, pinned


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--host-batches", type=int, default=1)
    ap.add_argument("--device-warm", type=int, default=4)
    ap.add_argument("--device-batches", type=int, default=20)
    ap.add_argument("--eval-n", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from util import make_config
    from ursonet_amd import net
    from ursonet_amd.engine import Engine
    from ursonet_amd.evaluate import evaluate
    H, W, h, w, B = 960, 1280, 512, 640, 32
    out = {"gpu": torch.cuda.get_device_name(0), "backbone": a.backbone, "native": [H, W], "model": [h, w], "batch": B, "runs": a.runs}
    rate = hbm_rate()
    out["hbm_read4_write1_TBps"] = round(rate / 1e12, 2)
    out["kernel"] = kernel_times(a.kernel_iters, rate)

    cfg = make_config(a.backbone, h, w, batch=B, regress_ori=False, ori_bins=24, dtype="bfloat16")
    ds = in_memory_dataset(cfg, a.frames, H, W)
    eng = Engine(cfg, "training", seed=1)
    feeder_run(eng, ds, cfg, True, False, 1, 2, True)                       # warm-up: graph capture, code objects, pinned pools
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        eng.step()
    torch.cuda.synchronize()
    out["bare_step_ms"] = round((time.perf_counter() - t0) / 50 * 1e3, 3)
    for step in (False, True):
        for aug in (False, True):
            res = {False: [], True: []}
            for _ in range(a.runs):
                for on in (False, True):                                    # alternated in one process
                    res[on].append(feeder_run(eng, ds, cfg, on, aug, a.device_warm if on else 0, a.device_batches if on else a.host_batches, step))
            key = ("train_loop" if step else "feeder") + ("_rot_sim2real" if aug else "_plain")
            out[key] = {"off_img_s": mmm([r[0] for r in res[False]]), "on_img_s": mmm([r[0] for r in res[True]]),
                        "off_ms_per_batch": mmm([r[1] for r in res[False]]), "on_ms_per_batch": mmm([r[1] for r in res[True]]),
                        "off_pinned_bytes": res[False][0][2], "on_pinned_bytes": res[True][0][2]}
    del eng
    torch.cuda.empty_cache()

    td = tempfile.mkdtemp()
    ecfg = make_config(a.backbone, h, w, batch=B, regress_ori=False, ori_bins=24, dtype="bfloat16")
    model = net.UrsoNet(mode="inference", config=ecfg, model_dir=td)
    eds = in_memory_dataset(ecfg, a.eval_n, H, W, seed=2)
    ecfg.DEVICE_RESIZE = True
    evaluate(model, eds, out_dir=td, verbose=0)                             # warm-up
    res = {False: [], True: []}
    for _ in range(a.runs):
        for on in (False, True):
            ecfg.DEVICE_RESIZE = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate(model, eds, out_dir=td, verbose=0)
            res[on].append(a.eval_n / (time.perf_counter() - t0))
    out["evaluate"] = {"n": a.eval_n, "off_img_s": mmm(res[False]), "on_img_s": mmm(res[True])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
