#!/usr/bin/env python3
"""What temperature scaling costs (calibrate(), predict / evaluate with calibration=...): the bf16 ResNet-50 at
512 x 640, engine batch 32, soft orientation head with 32^3 bins and regressed location, on one GPU.

  python tools/calibrate_bench.py [--images 128] [--windows 5] [--out profiles/calibrate_bench.json]

A fresh process per configuration, all in one run of this tool, each reporting the median over its windows after one untimed call:
  launches   urso_temp_stats at J = 1 and at J = 8 and urso_temp_scale back to back on a batch of 32 rows of 32^3 logits, 200 calls each
             between two events, beside urso_ens_add (first = 0) and urso_ens_settle in the same process.  Bytes are the algorithm's:
             per row K * 8 for the stats (logits and targets once: the logits' second read comes from L2), K * 8 for the scale.
             eight_j1_over_j8 is 8 x the J = 1 time over the J = 8 time: above 1, one launch for eight temperatures is the faster way;
  calibrate  a window is one calibrate() of the dataset: the pass over the images, the copies and the fit of the head;
  evaluate   a window is one evaluate() of the same images (the pass that calibrate() shares, with the decode and the scoring);
  applied    a window is one evaluate(calibration=...) of the same images: what applying a calibration adds to that.
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
CHILDREN = ("launches", "calibrate", "evaluate", "applied")


def launches(a, out):
    import torch
    sys.path.insert(0, ROOT)
    from ursonet_amd import calibrate as cal, hip
    if not torch.cuda.is_available():
        raise SystemExit("tools/calibrate_bench.py needs the GPU: nothing here can be measured without one")
    out["device"] = torch.cuda.get_device_name(0)
    B, K = CFG["batch"], CFG["ori_bins"] ** 3
    z = torch.randn(B, K, device="cuda") * 4
    y = torch.softmax(torch.randn(B, K, device="cuda") * 4, dim=1)
    rows = torch.empty(B, hip.TEMP_COLS, dtype=torch.float64, device="cuda")
    scaled = torch.empty(B, K, device="cuda")
    acc = torch.empty(B, K, dtype=torch.float64, device="cuda")
    stat = torch.empty(B, hip.ENS_STAT, dtype=torch.float64, device="cuda")
    logp = torch.empty(B, K, dtype=torch.float32, device="cuda")
    table = torch.empty(B, hip.ENS_COLS, dtype=torch.float64, device="cuda")
    hip.ens_add(B, B, 0, z, acc, stat, True)
    calls = {"temp_stats_j1": (lambda: hip.temp_stats(B, B, 0, [0.7], z, y, rows), B * K * 8.0),
             "temp_stats_j8": (lambda: hip.temp_stats(B, B, 0, cal.GRID, z, y, rows), B * K * 8.0),
             "temp_scale": (lambda: hip.temp_scale(B, B, 0.7, z, scaled), B * K * 8.0),
             "ens_add": (lambda: hip.ens_add(B, B, 0, z, acc, stat, False), B * K * 20.0),
             "ens_settle": (lambda: hip.ens_settle(B, 0, 64, acc, stat, logp, table), B * K * 12.0)}
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
    out["rows"], out["bins"] = B, K
    out["eight_j1_over_j8"] = round(8 * out["temp_stats_j1"]["ms_median"] / out["temp_stats_j8"]["ms_median"], 3)


def child(a):
    out = {}
    if a.child == "launches":
        launches(a, out)
        print("RESULT " + json.dumps(out))
        return
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from util import make_config
    from ursonet_amd import calibrate as cal, evaluate as ev, net
    from ursonet_amd.dataset import SyntheticPoses
    if not torch.cuda.is_available():
        raise SystemExit("tools/calibrate_bench.py needs the GPU: nothing here can be measured without one")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = make_config(**CFG)
        cfg.NAME = "bench"
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=tmp)
        out["device"] = torch.cuda.get_device_name(0)
        ds = SyntheticPoses(a.images, CFG["h"], CFG["w"], cfg, seed=5)
        if a.child == "calibrate":
            run = lambda: cal.calibrate(model, ds)                                              # noqa: E731
        elif a.child == "applied":
            c = cal.Calibration(ori_beta=0.7)
            run = lambda: ev.evaluate(model, ds, out_dir=tmp, verbose=0, calibration=c)         # noqa: E731
        else:
            run = lambda: ev.evaluate(model, ds, out_dir=tmp, verbose=0)                        # noqa: E731
        run()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            r = run()                                                                           # (ends in a read from the device)
            ws.append(time.perf_counter() - t0)
        out.update({"seconds_median": round(statistics.median(ws), 4), "seconds_min": round(min(ws), 4), "seconds_max": round(max(ws), 4),
                    "windows": [round(x, 4) for x in ws]})
        if a.child == "calibrate":
            out.update({"ori_beta": r.ori_beta, "passes": r.ori_passes, "clamped": r.ori_clamped, "nll_before": r.ori_nll_before,
                        "nll_after": r.ori_nll_after})
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_bench.json"))
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
           "calibrate": res["calibrate"], "evaluate": res["evaluate"], "evaluate_with_calibration": res["applied"],
           "calibrate_over_evaluate": round(res["calibrate"]["seconds_median"] / res["evaluate"]["seconds_median"], 4)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
