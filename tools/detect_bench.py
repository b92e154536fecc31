#!/usr/bin/env python3
"""Throughput of detect_dataset(render=True) (ursonet_amd/detect.py) against the reference-style per-image loop, on one GPU.

  python tools/detect_bench.py [--backbone resnet50] [--h 512] [--w 640] [--n 64] [--ori-bins 24] [--out profiles/detect_bench.json]

IMAGES_PER_GPU 32: detect_dataset over n drawn images with the four pictures per image (render=True) and without (render=False),
images/s after one warm-up pass, and the launch profiler's time per urso_pmf_sheet_u8 call (32 sheets of n^3 bins, cell 4, gap 2).
IMAGES_PER_GPU 1: the reference's loop -- detect at batch 1 + ursonet_amd.utils.decode_orientations + pose_errors per image, no figure
at all (matplotlib's would only add to it).  Synthetic dataset, initial weights, bf16, soft-classification orientation head.  Prints one
JSON line and writes it to --out.  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--n-loop", type=int, default=32)
    ap.add_argument("--ori-bins", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    a = ap.parse_args()
    import torch
    from util import make_config
    from ursonet_amd import hip, net, utils
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.detect import detect_dataset
    out = {"backbone": a.backbone, "h": a.h, "w": a.w, "ori_bins": a.ori_bins, "n": a.n, "n_loop": a.n_loop,
           "device": torch.cuda.get_device_name(0)}
    td = tempfile.mkdtemp()
    ids = list(range(a.n))
    for B in (32, 1):
        cfg = make_config(a.backbone, a.h, a.w, batch=B, regress_ori=False, ori_bins=a.ori_bins, dtype="bfloat16")
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=td)
        if B > 1:
            ds = SyntheticPoses(a.n, a.h, a.w, cfg, seed=1)
            for render in (True, False):
                detect_dataset(model, ds, a.n, image_ids=ids, render=render, verbose=0, sink=lambda i, name, p: None)      # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                detect_dataset(model, ds, a.n, image_ids=ids, render=render, verbose=0, sink=lambda i, name, p: None)
                torch.cuda.synchronize()
                out["detect_dataset_render%d_B%d_img_s" % (render, B)] = a.n / (time.perf_counter() - t0)
            hip.prof_enable(True)
            detect_dataset(model, ds, a.n, image_ids=ids, render=True, verbose=0, sink=lambda i, name, p: None)
            recs = [r for r in hip.prof_collect_ex() if "pmf_" in r[5]]
            hip.prof_enable(False)
            if recs:
                out["pmf_sheet_calls"] = len(recs)
                out["pmf_sheet_ms_per_call"] = sum(r[1] for r in recs) / len(recs)
                out["pmf_sheet_gb_s"] = sum(r[3] for r in recs) / sum(r[1] for r in recs) / 1e6
        else:
            ds = SyntheticPoses(a.n_loop, a.h, a.w, cfg, seed=1)
            for _rep in range(2):
                t0 = time.perf_counter()
                for i in ds.image_ids:
                    r = model.detect([ds.load_image(i)])[0]
                    q = utils.decode_orientations(r["ori"][None], ds.ori_histogram_map)[0]
                    utils.pose_errors(r["loc"], q, ds.load_location(i), ds.load_quaternion(i))
                t_loop = time.perf_counter() - t0
            out["reference_loop_B1_img_s"] = a.n_loop / t_loop
        del model
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
