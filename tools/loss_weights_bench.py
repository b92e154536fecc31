#!/usr/bin/env python3
"""What learnable loss weights cost a step: the bf16 ResNet-50 step of bench.py's configuration (512 x 640, batch 32, regressed location,
16^3 orientation bins, uint8 input) with Config.LEARNABLE_LOSS_WEIGHTS off and on, on one GPU.

  python tools/loss_weights_bench.py [--steps 20] [--passes 5] [--warmup 10] [--repeats 3] [--out profiles/loss_weights_bench.json]

Every measurement is a fresh child process with its own time limit; a child replays the captured step `warmup` times, then times
`passes` passes of `steps` replays; the parent process takes the median pass.  The modes are taken in turn (off, on, off_again, off, ...):
"off" is measured TWICE per round, under two names, so that the run-to-run spread of one and the same plan stands beside the difference
between the plans.  The on-plan replaces the two loss launches one for one and adds one small launch in front of the norm's final
reduction.  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=16, bottleneck=32, branch=1024,
           dtype="bfloat16")
MODES = {"off": False, "on": True, "off_again": False}


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd.engine import Engine
    cfg = make_config(**CFG)
    cfg.LEARNABLE_LOSS_WEIGHTS = MODES[a.child]
    img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
    u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
    eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
    eng.set_input_u8(True)
    eng.load_batch_u8(u8, loc, ori)
    for _ in range(max(a.warmup, 1)):
        eng.step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"mode": a.child, "ms_per_step_passes": [round(x, 4) for x in ms], "launches": sum(
        len(x) for x in (eng.prep_ops, eng.fwd_ops, eng.loss_pre_ops, eng.loss_ops, eng.bwd_ops, eng.opt_ops)),
        "opt_launches": eng.labels["opt"], "device": torch.cuda.get_device_name(0), "finite_weights": bool(torch.isfinite(eng.flat_w).all())}
    if eng.learn_lw:
        out["loss_weights"] = dict(zip(("ori_weight", "loc_weight"), eng.loss_weight_values().tolist()))
    print("RESULT " + json.dumps(out), flush=True)


def run_child(mode, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps), "--passes", str(a.passes), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout, cwd=ROOT)
    text = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        raise SystemExit("child %s ended with %d:\n%s" % (mode, p.returncode, text[-3000:]))
    line = [l for l in text.splitlines() if l.startswith("RESULT ")][-1]
    r = json.loads(line[len("RESULT "):])
    r["ms_per_step_median"] = round(statistics.median(r["ms_per_step_passes"]), 4)
    r["spread_ms"] = round(max(r["ms_per_step_passes"]) - min(r["ms_per_step_passes"]), 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(MODES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_weights_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"config": CFG, "steps": a.steps, "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "runs": []}
    names = ("off", "on", "off_again")
    procs = {name: [] for name in names}
    for _ in range(max(a.repeats, 1)):
        for name in names:
            r = run_child(name, a)                    # a fault or a time limit in a child ends the whole run (SystemExit / TimeoutExpired)
            procs[name].append(r)
            print("%-10s %.4f ms/step (passes spread %.4f)" % (name, r["ms_per_step_median"], r["spread_ms"]), file=sys.stderr, flush=True)
    for name in names:
        rs = procs[name]
        r = {k: v for k, v in rs[-1].items() if k not in ("ms_per_step_passes", "ms_per_step_median", "spread_ms")}
        r["processes"] = [{"ms_per_step_passes": x["ms_per_step_passes"], "ms_per_step_median": x["ms_per_step_median"], "spread_ms": x["spread_ms"]} for x in rs]
        meds = [x["ms_per_step_median"] for x in rs]
        r["ms_per_step_median"] = round(statistics.median(meds), 4)                 # median over the processes of their median pass
        r["spread_between_processes_ms"] = round(max(meds) - min(meds), 4)
        out["runs"].append(r)
    by = {r["mode"]: r for r in out["runs"]}
    out["delta_ms_vs_off"] = {m: round(by[m]["ms_per_step_median"] - by["off"]["ms_per_step_median"], 4) for m in ("on", "off_again")}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
