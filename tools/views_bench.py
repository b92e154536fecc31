#!/usr/bin/env python3
"""What test-time view fusion (predict(views=...), ursonet_amd/views.py) costs in throughput, on one GPU.

  python tools/views_bench.py [--backbone resnet50] [--h 512] [--w 640] [--n 256] [--n-b1 64] [--ori-bins 24] [--reps 5]
                              [--yardstick-tree DIR] [--out profiles/views_bench.json]

For IMAGES_PER_GPU 32 and 1, on one synthetic dataset and one engine per batch size: a warm-up pass and `reps` timed passes of predict()
with views=None, ROLL_VIEWS(1, 0), ROLL_VIEWS(3, 30) and ROLL_VIEWS(7, 60), one configuration after the other in one child process.
--yardstick-tree names a built checkout of the parent commit; the script runs its predict() (no views argument) on the same dataset in
a child process of its own, before and apart from this tree's, so the two code bases never share a process.  ResNet-50, 512 x 640,
bf16, soft classification with n = 24 unless told otherwise (the configuration of tools/predict_bench.py); synthetic frames, initial
weights.  Reported per configuration: the median rate in images per second and the run-to-run spread (max - min) / median.  The one
gate: views=None is not slower than the parent beyond the larger of the two spreads -- it runs the same code.  The cost of V > 1 is
reported, not gated.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (("none", None), ("roll1", (1, 0)), ("roll3", (3, 30)), ("roll7", (7, 60)))


def run(a, tree, role):
    """Timed passes with the code of `tree`, in this process: role "parent" = predict() as the tree has it, "views" = every configuration."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    from util import make_config
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.infer import loader_workers
    from ursonet_amd.predict import predict
    td = tempfile.mkdtemp()
    out = {}
    for B in (32, 1):
        cfg = make_config(a.backbone, a.h, a.w, batch=B, regress_ori=False, ori_bins=a.ori_bins, dtype="bfloat16")
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=td)
        n = a.n if B > 1 else a.n_b1
        ds = SyntheticPoses(n, a.h, a.w, cfg, seed=1)
        if role == "parent":
            calls = [("parent", lambda: predict(model, ds))]
        else:
            from ursonet_amd.views import ROLL_VIEWS
            calls = [(name, (lambda: predict(model, ds)) if roll is None else (lambda v=ROLL_VIEWS(*roll): predict(model, ds, views=v)))
                     for name, roll in CONFIGS]
        for name, once in calls:
            once()                                                               # warm-up: capture, code objects, the extension library
            rates = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                once()
                torch.cuda.synchronize()
                rates.append(n / (time.perf_counter() - t0))
            out["%s_B%d_img_s" % (name, B)] = rates
        del model
        torch.cuda.empty_cache()
    out["box"] = "one %s, LOADER_WORKERS %d" % (torch.cuda.get_device_name(0), loader_workers(cfg))
    return out


def child(a, tree, role):
    cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--tree", tree]
    for k in ("backbone", "h", "w", "n", "n_b1", "ori_bins", "reps"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
    res = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=""), cwd=tree)
    if res.returncode != 0:
        raise RuntimeError("%s pass failed (%d):\n%s" % (role, res.returncode, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n-b1", type=int, default=64)
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
    parent = child(a, os.path.abspath(a.yardstick_tree), "parent") if a.yardstick_tree else None
    this = child(a, ROOT, "views")
    med = lambda v: float(np.median(v))                                          # noqa: E731
    spread = lambda v: float((max(v) - min(v)) / np.median(v))                   # noqa: E731
    out = {"backbone": a.backbone, "h": a.h, "w": a.w, "ori_bins": a.ori_bins, "n": a.n, "n_b1": a.n_b1, "reps": a.reps,
           "yardstick": "predict() of the parent commit, a process of its own" if parent else None}
    for B in (32, 1):
        rows = ([("parent", parent["parent_B%d_img_s" % B])] if parent else []) + [(name, this["%s_B%d_img_s" % (name, B)]) for name, _ in CONFIGS]
        for name, runs in rows:
            out["%s_B%d_img_s" % (name, B)], out["%s_B%d_spread" % (name, B)], out["%s_B%d_runs" % (name, B)] = med(runs), spread(runs), runs
        base = out["none_B%d_img_s" % B]
        for name, roll in CONFIGS[1:]:
            out["%s_B%d_cost" % (name, B)] = base / out["%s_B%d_img_s" % (name, B)]      # wall time per image relative to views=None
        if parent:
            margin = max(out["parent_B%d_spread" % B], out["none_B%d_spread" % B])
            out["none_B%d_not_slower" % B] = bool(base >= out["parent_B%d_img_s" % B] * (1 - margin))
    out["box"] = this["box"]
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
