#!/usr/bin/env python3
"""What a BN recalibration pass costs (recalibrate_bn, Config.BN_RECAL_BATCHES): the bf16 ResNet-50 of bench.py's
geometry (512 x 640, batch 32, regressed location, 16^3 orientation bins, uint8 input) with batch-statistics BatchNorm (TRAIN_BN = None),
on one GPU: ms per Engine.bn_recal_add() against ms per Engine.evaluate(read=False) on the same engine and the same loaded batch, and the
add and settle launches alone.

  python tools/bn_recal_bench.py [--processes 3] [--steps 10] [--rounds 5] [--warmup 5] [--out profiles/bn_recal_bench.json]

Fresh processes, one engine each, in turn.  A process warms both calls up, then times `rounds` windows of `steps` calls of each, the two
taking turns (a host clock around eager launches that end in a device synchronise).  Per call the median over all windows of all
processes is reported, with the range of the per-process medians (the run-to-run spread).  evaluate() runs prep, forward and the losses
and copies flat_stats twice; bn_recal_add() runs prep, forward and the one add launch: the expected shape is a ratio just under 1.  The
launches alone: 100 calls between two device events, five repeats, medians; bytes are the algorithm's (per channel the add reads two
floats and reads and writes two doubles, 40 bytes; the settlement reads two doubles and writes two floats, 24).  The feeder, which bounds
the real pass, is not part of this.  There is no threshold: the numbers are recorded, not judged."""
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


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/bn_recal_bench.py needs the GPU: nothing here can be measured without one")
    cfg = make_config(**CFG)
    cfg.TRAIN_BN = None
    img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
    u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
    eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
    eng.set_input_u8(True)
    eng.load_batch_u8(u8, loc, ori)
    eng.bn_recal_begin()
    calls = {"bn_recal_add": eng.bn_recal_add, "evaluate": lambda: eng.evaluate(read=False)}
    for _ in range(max(a.warmup, 1)):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    windows = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, call in calls.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            torch.cuda.synchronize()
            windows[k].append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    plan = eng._recal_plan[1]
    launches = {"add": plan.add, "settle": lambda: plan.settle(eng.flat_stats)}
    alone = {}
    for k, call in launches.items():
        for _ in range(10):
            call()
        reps = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(100):
                call()
            t1.record()
            torch.cuda.synchronize()
            reps.append(t0.elapsed_time(t1) / 100)
        alone[k] = round(statistics.median(reps), 5)
    batches = plan.t
    eng.bn_recal_end()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(eng.flat_stats).all())
    eng.bn_recal_abort()
    channels = sum(int(row[0].numel()) for row in plan.layers)
    out = {"windows_ms": windows, "launch_alone_ms": alone, "bn_layers": plan.L, "channels": channels, "batches_pooled": batches,
           "fwd_launches": len(eng.labels["fwd"]), "finite_statistics": finite, "device": torch.cuda.get_device_name(0)}
    print("BN_RECAL_BENCH " + json.dumps(out), flush=True)


def _run_child(a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("BN_RECAL_BENCH ")]
    if r.returncode != 0 or not lines:                 # nothing more is started on the GPU behind a process that failed
        raise SystemExit("tools/bn_recal_bench.py: a process failed (exit %d):\n%s" % (r.returncode, r.stdout[-4000:]))
    rec = json.loads(lines[-1][len("BN_RECAL_BENCH "):])
    print(rec["windows_ms"], file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_recal_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    recs = [_run_child(a) for _ in range(a.processes)]
    calls = {}
    for k in ("bn_recal_add", "evaluate"):
        ws = [x for r in recs for x in r["windows_ms"][k]]
        meds = [statistics.median(r["windows_ms"][k]) for r in recs]
        calls[k] = {"ms_per_call_median": round(statistics.median(ws), 4), "ms_per_call_min": min(ws), "ms_per_call_max": max(ws),
                    "per_process_medians_ms": [round(m, 4) for m in meds], "spread_between_processes_ms": round(max(meds) - min(meds), 4)}
    ch = recs[0]["channels"]
    alone = {k: {"ms_median": round(statistics.median(r["launch_alone_ms"][k] for r in recs), 5),
                 "ms_per_process": [r["launch_alone_ms"][k] for r in recs], "bytes": b * ch}
             for k, b in (("add", 40), ("settle", 24))}
    add, ev = calls["bn_recal_add"]["ms_per_call_median"], calls["evaluate"]["ms_per_call_median"]
    out = {"config": dict(CFG, TRAIN_BN=None), "device": recs[0]["device"], "processes": a.processes, "steps": a.steps, "rounds": a.rounds,
           "warmup": a.warmup, "bn_layers": recs[0]["bn_layers"], "channels": ch, "fwd_launches": recs[0]["fwd_launches"], "calls": calls,
           "bn_recal_add_as_a_multiple_of_evaluate": round(add / ev, 4), "bn_recal_add_minus_evaluate_ms": round(add - ev, 4),
           "launch_alone": alone, "windows": [r["windows_ms"] for r in recs],
           "finite_statistics": all(r["finite_statistics"] for r in recs)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
