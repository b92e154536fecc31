#!/usr/bin/env python3
"""Throughput of evaluate() (ursonet_amd/evaluate.py) against the reference-style per-image loop, on one GPU.

  python tools/eval_bench.py [--backbone resnet50] [--h 512] [--w 640] [--n 256] [--ori-bins 24]

For IMAGES_PER_GPU 32 and 1: evaluate() images/s (after one warm-up pass), and the time of the same number of bare
engine.forward() replays, whose complement is the share of evaluate() spent outside forward().  Then the reference's loop at
batch 1: detect + ursonet_amd.utils.decode_orientations + pose_errors per image.  Synthetic dataset, initial weights, bf16,
soft-classification orientation head.  Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-loop", type=int, default=64)
    ap.add_argument("--ori-bins", type=int, default=24)
    a = ap.parse_args()
    import torch
    from util import make_config
    from ursonet_amd import net, utils
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.evaluate import evaluate
    out = {"backbone": a.backbone, "h": a.h, "w": a.w, "ori_bins": a.ori_bins, "n": a.n}
    td = tempfile.mkdtemp()
    for B in (32, 1):
        cfg = make_config(a.backbone, a.h, a.w, batch=B, regress_ori=False, ori_bins=a.ori_bins, dtype="bfloat16")
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=td)
        n = a.n if B > 1 else a.n_loop
        ds = SyntheticPoses(n, a.h, a.w, cfg, seed=1)
        evaluate(model, ds, out_dir=td, verbose=0)                          # warm-up: capture, code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate(model, ds, out_dir=td, verbose=0)
        t_eval = time.perf_counter() - t0
        eng = model._engine
        steps = -(-n // B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.forward()
        torch.cuda.synchronize()
        t_fwd = time.perf_counter() - t0
        out["evaluate_B%d_img_s" % B] = n / t_eval
        out["forward_only_B%d_img_s" % B] = steps * B / t_fwd
        out["share_outside_forward_B%d" % B] = 1 - t_fwd / t_eval
        if B == 1:                                                          # the reference's loop, on this model
            for rep in range(2):
                t0 = time.perf_counter()
                for i in ds.image_ids:
                    r = model.detect([ds.load_image(i)])[0]
                    q = utils.decode_orientations(r["ori"][None], ds.ori_histogram_map)[0]
                    utils.pose_errors(r["loc"], q, ds.load_location(i), ds.load_quaternion(i))
                t_loop = time.perf_counter() - t0
            out["reference_loop_B1_img_s"] = n / t_loop
        del model, eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
