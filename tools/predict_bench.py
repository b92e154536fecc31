#!/usr/bin/env python3
"""Throughput of predict() (ursonet_amd/predict.py) against the reference-style per-image loop and against evaluate(), on one GPU.

  python tools/predict_bench.py [--backbone resnet50] [--h 512] [--w 640] [--n 256] [--ori-bins 24] [--reps 5]
                                [--yardstick-tree DIR] [--out profiles/predict_bench.json]

For IMAGES_PER_GPU 32 and 1, on one synthetic dataset and one engine, in this order: one warm-up pass each, then `reps` timed passes
of evaluate() and `reps` of predict().  --yardstick-tree names a built checkout of the commit to measure evaluate() of (the parent
of the change under test); the script re-runs itself there with --role evaluate in a child process of its own, so the two code
bases never share a process.  Without it, evaluate() is this tree's.  Then, at batch 1, the reference's loop: detect + host decode
per image.  ResNet-50, 512 x 640, bf16, soft classification with n = 24 unless told otherwise; synthetic frames, initial weights.
The margin predict() gets is the spread (max - min) / median of the yardstick's own timings.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(a, tree, role):
    """Timed passes of `role` (evaluate / predict / loop) with the code of `tree`, in this process."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    from util import make_config
    from ursonet_amd import net, utils
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.infer import loader_workers
    td = tempfile.mkdtemp()
    out = {}
    for B in (32, 1):
        cfg = make_config(a.backbone, a.h, a.w, batch=B, regress_ori=False, ori_bins=a.ori_bins, dtype="bfloat16")
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=td)
        n = a.n if B > 1 else a.n_loop
        ds = SyntheticPoses(n, a.h, a.w, cfg, seed=1)
        if role == "evaluate":
            from ursonet_amd.evaluate import evaluate
            once = lambda: evaluate(model, ds, out_dir=td, verbose=0)            # noqa: E731
        elif role == "predict":
            from ursonet_amd.predict import predict
            once = lambda: predict(model, ds)                                    # noqa: E731
        else:
            if B != 1:
                continue

            def once():
                for i in ds.image_ids:
                    r = model.detect([ds.load_image(i)])[0]
                    utils.decode_orientations(r["ori"][None], ds.ori_histogram_map)
        once()                                                                   # warm-up: capture, code objects
        rates = []
        for _ in range(a.reps if role != "loop" else 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
        out["B%d_img_s" % B] = rates
        del model
        torch.cuda.empty_cache()
    out["box"] = "one %s, LOADER_WORKERS %d" % (torch.cuda.get_device_name(0), loader_workers(cfg))
    return out


def child(a, tree, role):
    cmd = [sys.executable, os.path.join(tree, "tools", "predict_bench.py") if os.path.exists(os.path.join(tree, "tools", "predict_bench.py"))
           else os.path.abspath(__file__), "--role", role, "--tree", tree]
    for k in ("backbone", "h", "w", "n", "n_loop", "ori_bins", "reps"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    env = dict(os.environ, PYTHONPATH="")
    res = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree)
    if res.returncode != 0:
        raise RuntimeError("%s pass failed (%d):\n%s" % (role, res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-loop", type=int, default=64)
    ap.add_argument("--ori-bins", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yardstick-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        print(json.dumps(run(a, a.tree, a.role)))
        return
    yard = os.path.abspath(a.yardstick_tree) if a.yardstick_tree else ROOT
    ev, pr, loop = child(a, yard, "evaluate"), child(a, ROOT, "predict"), child(a, ROOT, "loop")
    med = lambda v: float(np.median(v))                                          # noqa: E731
    out = {"backbone": a.backbone, "h": a.h, "w": a.w, "ori_bins": a.ori_bins, "n": a.n, "n_loop": a.n_loop, "reps": a.reps,
           "yardstick": "evaluate() of the parent commit" if a.yardstick_tree else "evaluate() of this tree",
           "reference_loop_B1_img_s": med(loop["B1_img_s"])}
    for B in (32, 1):
        e, p = ev["B%d_img_s" % B], pr["B%d_img_s" % B]
        spread = (max(e) - min(e)) / med(e)
        out["evaluate_B%d_img_s" % B], out["predict_B%d_img_s" % B] = med(e), med(p)
        out["evaluate_B%d_runs" % B], out["predict_B%d_runs" % B] = e, p
        out["evaluate_B%d_spread" % B] = spread
        out["predict_B%d_not_slower" % B] = bool(med(p) >= med(e) * (1 - spread))
    out["box"] = pr["box"]
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
