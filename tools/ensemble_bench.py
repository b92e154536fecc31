#!/usr/bin/env python3
"""What the ensemble pass costs (predict(members=...)): the bf16 ResNet-50 at 512 x 640, engine batch 32, soft
orientation head with 32^3 bins and regressed location, on one GPU.

  python tools/ensemble_bench.py [--images 128] [--members 4] [--windows 5] [--out profiles/ensemble_bench.json]

A fresh process per configuration, all in one run of this tool, each reporting the median over its windows after one untimed call:
  plain     a window is `members` calls of the plain predict() of the model (what a user did before: one call per weight set, the
            poses combined on the host afterwards -- which this figure leaves out, as it leaves out loading each weight set);
  loaded    the same with what that user also paid: each of the `members` calls behind read_weights_file + set_weights of its file;
  members   a window is one predict(members=[...]) over `members` weight files (.npz, written beforehand): the weight loads, the
            accumulation, the closing pass and the restoring of the model's weights included;
  launches  urso_ens_add (first = 0) and urso_ens_settle back to back on a batch of 32 rows of 32^3 logits, 200 calls each between two
            events, beside urso_ema_update over the network's parameters in the same process.  Bytes are the algorithm's: per row
            K * (4 + 16) for the add (the logits once: their re-reads come from L2; the accumulator read and written) and K * (8 + 4)
            for the settle; 12 per parameter for the EMA pass.
The dataset is synthetic (frames drawn on the host per call, as every call of predict() loads its images), so the windows hold the
loader as a user's would.  There is no threshold: the numbers are recorded, not judged."""
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


def _model(tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from util import make_config
    from ursonet_amd import net
    if not torch.cuda.is_available():
        raise SystemExit("tools/ensemble_bench.py needs the GPU: nothing here can be measured without one")
    cfg = make_config(**CFG)
    cfg.NAME = "bench"
    return cfg, net.UrsoNet(mode="inference", config=cfg, model_dir=tmp)


def child(a):
    import numpy as np
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        cfg, model = _model(tmp)
        eng = model._engine
        out = {"device": torch.cuda.get_device_name(0)}
        if a.child == "launches":
            from ursonet_amd import hip
            B, K = CFG["batch"], CFG["ori_bins"] ** 3
            z = torch.randn(B, K, device="cuda") * 4
            acc = torch.empty(B, K, dtype=torch.float64, device="cuda")
            stat = torch.empty(B, hip.ENS_STAT, dtype=torch.float64, device="cuda")
            logp = torch.empty(B, K, dtype=torch.float32, device="cuda")
            table = torch.empty(B, hip.ENS_COLS, dtype=torch.float64, device="cuda")
            hip.ens_add(B, B, 0, z, acc, stat, True)
            n = int(eng.flat_w.numel())
            w, e = eng.flat_w.clone(), eng.flat_w.clone()
            st = torch.tensor([0.999, 0, 0, 0.999, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
            calls = {"ens_add": (lambda: hip.ens_add(B, B, 0, z, acc, stat, False), B * K * 20.0),
                     "ens_settle": (lambda: hip.ens_settle(B, 0, 64, acc, stat, logp, table), B * K * 12.0),
                     "ema_update": (lambda: hip.ema_update(n, w, e, st), n * 12.0)}
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
            out["rows"], out["bins"], out["parameters"] = B, K, n
            print("RESULT " + json.dumps(out))
            return
        from ursonet_amd import predict as pr
        from ursonet_amd.dataset import SyntheticPoses
        ds = SyntheticPoses(a.images, CFG["h"], CFG["w"], cfg, seed=5)
        paths = []
        if a.child in ("members", "loaded"):
            base = eng.get_weights()
            rng = np.random.default_rng(3)
            for j in range(a.members):
                moved = {ln: {wn: (v + 0.01 * v.std() * rng.normal(size=v.shape).astype(np.float32) if wn == "kernel" else v)
                              for wn, v in ws.items()} for ln, ws in base.items()}
                eng.set_weights(moved, strict=True)
                paths.append(os.path.join(tmp, "weights_m%d_0001.npz" % j))
                model.save_weights(paths[-1])
            eng.set_weights(base, strict=True)
        if a.child == "members":
            run = lambda: pr.predict(model, ds, members=paths)                                  # noqa: E731
        elif a.child == "loaded":
            from ursonet_amd.net import read_weights_file

            def run():
                out = []
                for p in paths:
                    eng.set_weights(read_weights_file(p), strict=True)
                    out.append(pr.predict(model, ds))
                return out
        else:
            run = lambda: [pr.predict(model, ds) for _ in range(a.members)]                     # noqa: E731
        run()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            r = run()                                                                           # (ends in the read of the tables)
            ws.append(time.perf_counter() - t0)
        out.update({"seconds_median": round(statistics.median(ws), 4), "seconds_min": round(min(ws), 4), "seconds_max": round(max(ws), 4),
                    "windows": [round(x, 4) for x in ws]})
        if a.child == "members":
            out["mean_ori_mi_nats"], out["mean_member_ori_spread_deg"] = float(np.mean(r.ori_mi)), float(np.mean(r.member_ori_spread))
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    ap.add_argument("--child", choices=("plain", "loaded", "members", "launches"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    for name in ("plain", "loaded", "members", "launches"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--images", str(a.images), "--members", str(a.members),
               "--windows", str(a.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            raise SystemExit("configuration %s failed (exit %d)" % (name, p.returncode))
        res[name] = json.loads(lines[-1][len("RESULT "):])
        print(name, res[name], file=sys.stderr, flush=True)
    out = {"config": CFG, "images": a.images, "members": a.members, "windows": a.windows, "device": res["plain"].pop("device"),
           "plain_predict_x_members": res["plain"], "load_and_plain_predict_x_members": res["loaded"], "predict_members": res["members"],
           "launches": res["launches"], "members_over_plain": round(res["members"]["seconds_median"] / res["plain"]["seconds_median"], 4),
           "members_over_loaded": round(res["members"]["seconds_median"] / res["loaded"]["seconds_median"], 4)}
    for k in ("loaded", "members", "launches"):
        res[k].pop("device", None)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
