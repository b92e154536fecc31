#!/usr/bin/env python3
"""What the conformal bounds cost (conformal(), predict / evaluate with conformal=...): the bf16 ResNet-50 at
512 x 640, engine batch 32, soft orientation head with 32^3 bins and regressed location, on one GPU.

  python tools/conformal_bench.py [--images 128] [--windows 5] [--out profiles/conformal_bench.json]

A fresh process per configuration, all in one run of this tool, each reporting the median over its windows after one untimed call:
  launches           urso_conf_score and urso_conf_bound (q = 0.9) under either metric back to back on a batch of 32 rows of 32^3 logits,
                     200 calls each between two events, beside urso_ens_add (first = 0) and urso_temp_stats (J = 1) in the same process.
                     Bytes are the algorithm's: per row and sweep K * 4 of logits and K * 16 (angle) or K * 24 (Euclid) of map, two sweeps
                     for the score and seven for the bound.  bound_over_ens_add is the angle bound's time over urso_ens_add's;
  conformal          a window is one conformal() of the dataset: the pass over the images, the scoring and the score kernel;
  evaluate           a window is one evaluate() of the same images (the pass that conformal() shares);
  predict            a window is one predict() of the same images;
  predict_conformal  a window is one predict(conformal=...) of the same images: what the bounds add to that.
The dataset is synthetic (frames drawn on the host per call, as every call loads its images), so the windows hold the loader as a
user's would.  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=32, bottleneck=32, branch=1024,
           dtype="bfloat16")
CHILDREN = ("launches", "conformal", "evaluate", "predict", "predict_conformal")


def launches(a, out):
    import torch
    sys.path.insert(0, ROOT)
    from ursonet_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("tools/conformal_bench.py needs the GPU: nothing here can be measured without one")
    out["device"] = torch.cuda.get_device_name(0)
    B, K = CFG["batch"], CFG["ori_bins"] ** 3
    z = torch.randn(B, K, device="cuda") * 4
    y = torch.softmax(torch.randn(B, K, device="cuda") * 4, dim=1)
    hq = torch.nn.functional.normalize(torch.randn(K, 4, device="cuda"), dim=1).contiguous()
    pts = (torch.rand(K, 3, dtype=torch.float64, device="cuda") * 4 - 2).contiguous()
    q_est = torch.nn.functional.normalize(torch.randn(B, 4, dtype=torch.float64, device="cuda"), dim=1).contiguous()
    q_ref = torch.nn.functional.normalize(torch.randn(B, 4, dtype=torch.float64, device="cuda"), dim=1).contiguous()
    l_est, l_ref = torch.rand(B, 3, dtype=torch.float64, device="cuda"), torch.rand(B, 3, dtype=torch.float64, device="cuda")
    rows = torch.empty(B, hip.CONF_COLS, dtype=torch.float64, device="cuda")
    trows = torch.empty(B, hip.TEMP_COLS, dtype=torch.float64, device="cuda")
    acc = torch.empty(B, K, dtype=torch.float64, device="cuda")
    stat = torch.empty(B, hip.ENS_STAT, dtype=torch.float64, device="cuda")
    hip.ens_add(B, B, 0, z, acc, stat, True)
    sweeps = 1 + hip.CONF_PASSES
    calls = {"conf_score_angle": (lambda: hip.conf_score(B, B, 0, hip.CONF_ANGLE, z, hq, q_est, q_ref, rows), B * K * 2 * 20.0),
             "conf_score_euclid": (lambda: hip.conf_score(B, B, 0, hip.CONF_EUCLID, z, pts, l_est, l_ref, rows), B * K * 2 * 28.0),
             "conf_bound_angle": (lambda: hip.conf_bound(B, B, 0, hip.CONF_ANGLE, 0.9, z, hq, q_est, rows), B * K * (4.0 + (sweeps - 1) * 20.0)),
             "conf_bound_euclid": (lambda: hip.conf_bound(B, B, 0, hip.CONF_EUCLID, 0.9, z, pts, l_est, rows), B * K * (4.0 + (sweeps - 1) * 28.0)),
             "ens_add": (lambda: hip.ens_add(B, B, 0, z, acc, stat, False), B * K * 20.0),
             "temp_stats_j1": (lambda: hip.temp_stats(B, B, 0, [0.7], z, y, trows), B * K * 8.0)}
    for name, (call, nbytes) in calls.items():
        ms = []
        for _ in range(a.windows):
            for _ in range(10):
                call()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(200):
                call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / 200)
        med = statistics.median(ms)
        out[name] = {"bytes": nbytes, "ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5),
                     "GBps": round(nbytes / (med * 1e-3) / 1e9, 1)}
    out["rows"], out["bins"], out["sweeps_of_the_bound"] = B, K, sweeps
    out["bound_over_ens_add"] = round(out["conf_bound_angle"]["ms_median"] / out["ens_add"]["ms_median"], 3)
    out["score_over_ens_add"] = round(out["conf_score_angle"]["ms_median"] / out["ens_add"]["ms_median"], 3)


def child(a):
    out = {}
    if a.child == "launches":
        launches(a, out)
        print("RESULT " + json.dumps(out))
        return
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config
    from ursonet_amd import conformal as cf, evaluate as ev, net, predict as pr
    from ursonet_amd.dataset import SyntheticPoses
    if not torch.cuda.is_available():
        raise SystemExit("tools/conformal_bench.py needs the GPU: nothing here can be measured without one")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = make_config(**CFG)
        cfg.NAME = "bench"
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=tmp)
        out["device"] = torch.cuda.get_device_name(0)
        ds = SyntheticPoses(a.images, CFG["h"], CFG["w"], cfg, seed=5)
        if a.child == "conformal":
            run = lambda: cf.conformal(model, ds)                                               # noqa: E731
        elif a.child == "evaluate":
            run = lambda: ev.evaluate(model, ds, out_dir=tmp, verbose=0)                        # noqa: E731
        elif a.child == "predict":
            run = lambda: pr.predict(model, ds)                                                 # noqa: E731
        else:
            levels = cf.Conformal(0.1, "pmf", "error", np.linspace(0.0, 0.99, 100), np.linspace(0.0, 2.0, 100), k_ori=CFG["ori_bins"] ** 3)
            run = lambda: pr.predict(model, ds, conformal=levels)                               # noqa: E731
        r = run()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            r = run()                                                                           # (ends in a read from the device)
            ws.append(time.perf_counter() - t0)
        out.update({"seconds_median": round(statistics.median(ws), 4), "seconds_min": round(min(ws), 4), "seconds_max": round(max(ws), 4),
                    "windows": [round(x, 4) for x in ws]})
        if a.child == "conformal":
            out.update({"ori_q": r.ori_q, "loc_q": r.loc_q, "ori_kind": r.ori_kind, "loc_kind": r.loc_kind})
        if a.child == "predict_conformal":
            out.update({"ori_level": levels.ori_q, "ori_bound_mean_deg": float(np.mean(r.ori_bound)), "ori_region_bins_mean": float(np.mean(r.ori_region_bins))})
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conformal_bench.json"))
    ap.add_argument("--child", choices=CHILDREN)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    for name in CHILDREN:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--images", str(a.images), "--windows", str(a.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            raise SystemExit("configuration %s failed (exit %d)" % (name, p.returncode))
        res[name] = json.loads(lines[-1][len("RESULT "):])
        print(name, res[name], file=sys.stderr, flush=True)
    device = res["launches"].pop("device")
    for k in CHILDREN[1:]:
        res[k].pop("device", None)
    out = {"config": CFG, "images": a.images, "windows": a.windows, "device": device, "launches": res["launches"],
           "conformal": res["conformal"], "evaluate": res["evaluate"], "predict": res["predict"], "predict_with_conformal": res["predict_conformal"],
           "conformal_over_evaluate": round(res["conformal"]["seconds_median"] / res["evaluate"]["seconds_median"], 4),
           "predict_with_conformal_over_predict": round(res["predict_conformal"]["seconds_median"] / res["predict"]["seconds_median"], 4)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
