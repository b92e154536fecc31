#!/usr/bin/env python3
"""What loss scaling costs a step: the fp16 ResNet-50 step of BASELINE.md's f16 configuration (classification heads, 640 x 960, batch 32;
tools/config_sweep.py cfg5) with Config.LOSS_SCALE off, static 1, static 1024 and "dynamic", on one GPU.

  python tools/loss_scale_bench.py [--parent-tree DIR] [--steps 20] [--passes 5] [--warmup 10] [--repeats 3] [--out profiles/loss_scale_bench.json]

Every measurement is a fresh child process with its own time limit (a process that has run one engine does not time the next); a child
replays the captured step `warmup` times, then times `passes` passes of `steps` replays; the parent process takes the median pass.
--repeats: that many processes per mode, the modes taken in turn (parent, off, static 1, static 1024, dynamic, parent, ...), so that the spread between
processes of ONE mode -- which the passes inside a process do not show -- stands beside the differences between modes.
--parent-tree: a checkout of the commit before this feature with its library built (`python -m ursonet_amd.build` there): its step is
measured the same way in the same session, and "off" is set against it.  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=640, w=960, batch=32, regress_ori=False, regress_loc=False, ori_bins=16, loc_bins=16, f16=True)
# static_1: the launches of a scaled step with the VALUES of the unscaled one -- apart from static_1024 only by what the fp16 backward pass multiplies
MODES = {"off": None, "static_1": 1.0, "static_1024": 1024.0, "dynamic": "dynamic"}


def child(a):
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd.engine import Engine
    cfg = make_config(**CFG)
    if MODES[a.child] is not None:
        cfg.LOSS_SCALE = MODES[a.child]
    img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
    eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
    eng.load_batch(img, loc, ori)
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
    out = {"mode": a.child, "tree": tree, "ms_per_step_passes": [round(x, 4) for x in ms], "launches": sum(
        len(x) for x in (eng.prep_ops, eng.fwd_ops, eng.loss_pre_ops, eng.loss_ops, eng.bwd_ops, eng.opt_ops)),
        "device": torch.cuda.get_device_name(0), "finite_weights": bool(torch.isfinite(eng.flat_w).all())}
    if getattr(eng, "loss_scale", None) is not None and eng.loss_scale() is not None:
        out["loss_scale"] = eng.loss_scale()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(mode, tree, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--steps", str(a.steps), "--passes", str(a.passes),
           "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout, cwd=tree)
    text = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        raise SystemExit("child %s (%s) ended with %d:\n%s" % (mode, tree, p.returncode, text[-3000:]))
    line = [l for l in text.splitlines() if l.startswith("RESULT ")][-1]
    r = json.loads(line[len("RESULT "):])
    r["ms_per_step_median"] = round(statistics.median(r["ms_per_step_passes"]), 4)
    r["spread_ms"] = round(max(r["ms_per_step_passes"]) - min(r["ms_per_step_passes"]), 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(MODES))
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent-tree")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_scale_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    out = {"config": CFG, "steps": a.steps, "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "runs": []}
    modes = ([("parent_commit", "off", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [(m, m, ROOT) for m in ("off", "static_1", "static_1024", "dynamic")]
    procs = {name: [] for name, _, _ in modes}
    for _ in range(max(a.repeats, 1)):
        for name, mode, tree in modes:
            r = run_child(mode, tree, a)              # a fault or a time limit in a child ends the whole run (SystemExit / TimeoutExpired)
            r.pop("tree")
            procs[name].append(r)
            print("%-14s %.4f ms/step (passes spread %.4f)" % (name, r["ms_per_step_median"], r["spread_ms"]), file=sys.stderr, flush=True)
    for name, _, _ in modes:
        rs = procs[name]
        r = {k: v for k, v in rs[-1].items() if k not in ("ms_per_step_passes", "ms_per_step_median", "spread_ms")}
        r["mode"] = name
        r["processes"] = [{"ms_per_step_passes": x["ms_per_step_passes"], "ms_per_step_median": x["ms_per_step_median"], "spread_ms": x["spread_ms"]} for x in rs]
        meds = [x["ms_per_step_median"] for x in rs]
        r["ms_per_step_median"] = round(statistics.median(meds), 4)                 # median over the processes of their median pass
        r["spread_between_processes_ms"] = round(max(meds) - min(meds), 4)
        r["spread_within_process_ms"] = round(max(x["spread_ms"] for x in rs), 4)
        out["runs"].append(r)
    by = {r["mode"]: r for r in out["runs"]}
    base = by.get("parent_commit", by["off"])
    out["delta_ms_vs_%s" % base["mode"]] = {m: round(r["ms_per_step_median"] - base["ms_per_step_median"], 4) for m, r in by.items() if r is not base}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
