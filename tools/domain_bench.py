#!/usr/bin/env python3
"""What the domain-shift scores cost (fit_domain(), predict / evaluate with domain=...): the bf16 ResNet-50 at
512 x 640, engine batch 32, bottleneck width 128 (features of 8 x 10 cells), soft orientation head with 32^3 bins and regressed
location, on one GPU.

  python tools/domain_bench.py [--images 128] [--windows 5] [--out profiles/domain_bench.json]

A fresh process per configuration, all in one run of this tool, each reporting the median over its windows after one untimed call:
  launches        urso_feat_pool, urso_feat_gram_add and urso_feat_maha back to back for 32 rows at D = 128 (grid (1, 1)) and D = 512
                  (grid (2, 2)), 200 calls each between two events, beside urso_ens_add (32 rows of 32^3 logits, first = 0) and
                  urso_ema_update (25.6 M weights) in the same process.  Bytes are the algorithm's: the pool reads the activations once
                  and writes 8 n D; the Gram pass reads and writes the upper triangle, 8 D (D + 1), beside 8 n D of rows; the score reads
                  the lower triangle of W once per group of 8 rows, 4 D (D + 1) ceil(n / 8), beside 8 n D.  gram_accumulator_GBps is the
                  accumulator bytes alone over the Gram pass's time, gram_over_ema_rate that rate over urso_ema_update's;
  fit_domain      a window is one fit_domain(grid=(2, 2)) of the dataset: the pass over the images, pool and Gram per batch, the read and
                  the host's settlement (a Cholesky factor and a triangular solve of 512 x 512);
  predict         a window is one predict() of the same images: the parent's code path (domain=None launches nothing);
  predict_domain  a window is one predict(domain=...) of the same images at D = 512: what pool and score add to that.
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
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=32, bottleneck=128, branch=1024,
           dtype="bfloat16")
GEOMETRY = (8, 10, 128)
GRIDS = {128: (1, 1), 512: (2, 2)}
CHILDREN = ("launches", "fit_domain", "predict", "predict_domain")
EMA_WEIGHTS = 25600000


def launches(a, out):
    import torch
    sys.path.insert(0, ROOT)
    from ursonet_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("tools/domain_bench.py needs the GPU: nothing here can be measured without one")
    out["device"] = torch.cuda.get_device_name(0)
    B, K = CFG["batch"], CFG["ori_bins"] ** 3
    h, w, Cc = GEOMETRY
    f64 = dict(dtype=torch.float64, device="cuda")
    act = torch.randn(B, h, w, Cc, device="cuda").to(torch.bfloat16)
    z = torch.randn(B, K, device="cuda") * 4
    acc, stat = torch.empty(B, K, **f64), torch.empty(B, hip.ENS_STAT, **f64)
    hip.ens_add(B, B, 0, z, acc, stat, True)
    wts, ema = torch.randn(EMA_WEIGHTS, device="cuda"), torch.randn(EMA_WEIGHTS, device="cuda")
    st = torch.tensor([0.999, 0, 0, 0.999, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
    groups = -(-B // hip.FEAT_MAHA_ROWS)
    calls = {"ens_add": (lambda: hip.ens_add(B, B, 0, z, acc, stat, False), B * K * 20.0),
             "ema_update": (lambda: hip.ema_update(EMA_WEIGHTS, wts, ema, st), EMA_WEIGHTS * 12.0)}
    keep = []
    for D, grid in sorted(GRIDS.items()):
        x, centre, s, G = torch.randn(B, D, **f64), torch.randn(D, **f64), torch.zeros(D, **f64), torch.zeros(D, D, **f64)
        mean, wt, rows = torch.randn(D, **f64), (torch.randn(D, D, **f64) / D ** 0.5).contiguous(), torch.empty(B, hip.FEAT_COLS, **f64)
        xp = torch.empty(B, D, **f64)
        keep.append((x, centre, s, G, mean, wt, rows, xp))
        calls["feat_pool_d%d" % D] = (lambda grid=grid, xp=xp: hip.feat_pool(B, B, 0, grid, act, xp), act.numel() * 2.0 + 8.0 * B * D)
        calls["feat_gram_add_d%d" % D] = (lambda x=x, centre=centre, s=s, G=G: hip.feat_gram_add(B, B, 0, x, centre, s, G), 8.0 * D * (D + 1) + 8.0 * B * D)
        calls["feat_maha_d%d" % D] = (lambda x=x, mean=mean, wt=wt, rows=rows: hip.feat_maha(B, B, 0, x, mean, wt, rows), 4.0 * D * (D + 1) * groups + 8.0 * B * D)
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
    out["rows"], out["geometry"], out["ema_weights"] = B, list(GEOMETRY), EMA_WEIGHTS
    for D in sorted(GRIDS):
        g = out["feat_gram_add_d%d" % D]
        g["accumulator_bytes"] = 8.0 * D * (D + 1)
        g["gram_accumulator_GBps"] = round(g["accumulator_bytes"] / (g["ms_median"] * 1e-3) / 1e9, 2)
        g["gram_over_ema_rate"] = round(g["gram_accumulator_GBps"] / out["ema_update"]["GBps"], 5)


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
    from ursonet_amd import domain as dm, net, predict as pr
    from ursonet_amd.dataset import SyntheticPoses
    if not torch.cuda.is_available():
        raise SystemExit("tools/domain_bench.py needs the GPU: nothing here can be measured without one")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = make_config(**CFG)
        cfg.NAME = "bench"
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=tmp)
        out["device"] = torch.cuda.get_device_name(0)
        ds = SyntheticPoses(a.images, CFG["h"], CFG["w"], cfg, seed=5)
        grid = GRIDS[512]
        if a.child == "fit_domain":
            run = lambda: dm.fit_domain(model, ds, grid=grid)                                   # noqa: E731
        elif a.child == "predict":
            run = lambda: pr.predict(model, ds)                                                 # noqa: E731
        else:
            dom = dm.fit_domain(model, ds, grid=grid)
            run = lambda: pr.predict(model, ds, domain=dom)                                     # noqa: E731
        r = run()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            r = run()                                                                           # (ends in a read from the device)
            ws.append(time.perf_counter() - t0)
        out.update({"seconds_median": round(statistics.median(ws), 4), "seconds_min": round(min(ws), 4), "seconds_max": round(max(ws), 4),
                    "windows": [round(x, 4) for x in ws]})
        if a.child == "fit_domain":
            out.update({"D": r.D, "n": r.n, "shrink": r.shrink})
        if a.child == "predict_domain":
            out.update({"D": dom.D, "score_median": float(np.median(r.domain_score)), "score_over_D": float(np.median(r.domain_score)) / dom.D})
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domain_bench.json"))
    ap.add_argument("--child", choices=CHILDREN)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    for name in CHILDREN:                                                                      # a fresh child per configuration; this process never opens the GPU
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
           "fit_domain": res["fit_domain"], "predict": res["predict"], "predict_with_domain": res["predict_domain"],
           "fit_domain_over_predict": round(res["fit_domain"]["seconds_median"] / res["predict"]["seconds_median"], 4),
           "predict_with_domain_over_predict": round(res["predict_domain"]["seconds_median"] / res["predict"]["seconds_median"], 4)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
