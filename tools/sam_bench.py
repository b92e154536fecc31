#!/usr/bin/env python3
"""What SAM costs a step (Config.SAM): the bf16 ResNet-50 step of bench.py's geometry (512 x 640, batch 32, regressed
location, 16^3 orientation bins, uint8 input, SGD) with the key off -- the plan of the commit before the feature, launch for launch --
and on, on one GPU; and the rates of the two new streams beside urso_ema_update's.

  python tools/sam_bench.py [--processes 3] [--steps 20] [--rounds 5] [--warmup 10] [--profile-steps 5] [--out profiles/sam_bench.json]

Fresh processes, one engine each, in turn: off, on, off, on, ...  (`processes` of each plan).  A process replays its step `warmup` times,
then times `rounds` windows of `steps` replays (a host clock around replays that end in a device synchronise).  Per plan the median over
all windows of all its processes is reported, with the range of the per-process medians (the run-to-run spread) and the range over the
windows.  The SAM step is given as a multiple of the plain one, and its excess over twice the plain step beside that spread: the expected
shape is two passes plus the three launches.  The `on` processes also time every launch of `profile-steps` eager steps with the library's
HIP-event launch profiler (median per label), where the three launches run in the step's own cache state.

One more process times `urso_sam_ascend`, `urso_sam_descend` and `urso_ema_update` back to back on buffers of the model's size (100 calls
between two device events, five repeats, three passes over the three kernels in turn).  Bytes are the algorithm's: 16 per parameter for the
ascent (read w and g, write w0 and w), 8 for the way back, 12 for the average (read w and ema, write ema).  `spread` of a rate is the range
over the passes' medians.  There is no threshold: the numbers are recorded, not judged."""
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
RHO = 0.05
SAM_LABELS = ["sam_norm", "sam_ascend", "sam_descend"]


def _engine(rho):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/sam_bench.py needs the GPU: nothing here can be measured without one")
    cfg = make_config(**CFG)
    cfg.SAM = rho
    img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
    u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
    eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
    eng.set_input_u8(True)
    eng.load_batch_u8(u8, loc, ori)
    return eng, torch


def child_step(a):
    """One plan in this process: the windows, and for the SAM plan the launches inside eager steps."""
    eng, torch = _engine(RHO if a.child == "on" else None)
    for _ in range(max(a.warmup, 1)):
        eng.step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step()
        torch.cuda.synchronize()
        windows.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    out = {"plan": a.child, "windows_ms": windows, "launches": sum(len(v) for v in eng.labels.values()), "labels_sam": eng.labels.get("sam"),
           "opt_launches": eng.labels["opt"], "parameters": int(eng.n_flat), "device": torch.cuda.get_device_name(0)}
    if a.child == "on":
        per, sums = {k: [] for k in SAM_LABELS}, []
        for _ in range(max(a.profile_steps, 1)):
            recs = eng.profile_step()
            sums.append(sum(float(r[2]) for r in recs))
            for r in recs:
                if r[0] in per:
                    per[r[0]].append(float(r[2]))
        out["in_step_ms"] = {k: round(statistics.median(v), 5) for k, v in per.items()}
        out["eager_sum_ms"] = round(statistics.median(sums), 4)
        out["eager_launches"] = len(recs)
        out["sam_report"] = eng.sam_report()
    out["finite_weights"] = bool(torch.isfinite(eng.flat_w).all())
    print("SAM_BENCH " + json.dumps(out), flush=True)


def child_kernels(a):
    """The two streams and the yardstick back to back, on buffers of the model's size."""
    eng, torch = _engine(RHO)
    from ursonet_amd import hip, sam
    n, dev = int(eng.n_flat), eng.device
    w, w0, ema = eng.flat_w.clone(), torch.zeros_like(eng.flat_w), eng.flat_w.clone()
    g = torch.zeros_like(w)                            # s g = 0: the weights stay where they are however often the ascent runs
    del eng
    torch.cuda.empty_cache()
    st = torch.tensor(sam.initial_state(RHO, 1e-12), dtype=torch.float32, device=dev)
    st[sam.NORMSQ] = 1.0
    ema_state = torch.tensor([0.999, 0.0, 0.0, 0.999, 0.0, 0.0, 0.0, 0.0][:hip.EMA_FIELDS], dtype=torch.float32, device=dev)
    by = {"sam_ascend": 16.0 * n, "sam_descend": 8.0 * n, "ema_update": 12.0 * n}
    calls = {"sam_ascend": lambda: hip.sam_ascend(n, w, g, w0, st), "sam_descend": lambda: hip.sam_descend(n, w, w0),
             "ema_update": lambda: hip.ema_update(n, w, ema, ema_state)}
    passes = {k: [] for k in calls}
    for _ in range(3):
        for k, call in calls.items():
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
            passes[k].append(statistics.median(reps))
    out = {"plan": "kernels", "parameters": n, "kernels": {}}
    for k, ms in passes.items():
        rates = [by[k] / (x * 1e-3) / 1e9 for x in ms]
        out["kernels"][k] = {"bytes": by[k], "bytes_per_parameter": by[k] / n, "ms_per_pass": [round(x, 5) for x in ms],
                             "ms_median": round(statistics.median(ms), 5), "GBps_median": round(statistics.median(rates), 1),
                             "GBps_range": [round(min(rates), 1), round(max(rates), 1)], "GBps_spread": round(max(rates) - min(rates), 1)}
    assert float(st[sam.APPLIED]) == 1 and bool(torch.equal(w, w0))
    print("SAM_BENCH " + json.dumps(out), flush=True)


def _run_child(a, plan):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", plan, "--steps", str(a.steps), "--rounds", str(a.rounds),
           "--warmup", str(a.warmup), "--profile-steps", str(a.profile_steps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("SAM_BENCH ")]
    if r.returncode != 0 or not lines:                 # nothing more is started on the GPU behind a process that failed
        raise SystemExit("tools/sam_bench.py: the %r process failed (exit %d):\n%s" % (plan, r.returncode, r.stdout[-4000:]))
    rec = json.loads(lines[-1][len("SAM_BENCH "):])
    print("%-7s %s" % (plan, rec.get("windows_ms", "")), file=sys.stderr, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", choices=["off", "on", "kernels"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bench.json"))
    a = ap.parse_args()
    if a.child in ("off", "on"):
        return child_step(a)
    if a.child == "kernels":
        return child_kernels(a)
    recs = {"off": [], "on": []}
    for _ in range(a.processes):
        for plan in ("off", "on"):
            recs[plan].append(_run_child(a, plan))
    kern = _run_child(a, "kernels")
    step = {}
    for plan in ("off", "on"):
        ws = [x for r in recs[plan] for x in r["windows_ms"]]
        meds = [statistics.median(r["windows_ms"]) for r in recs[plan]]
        step[plan] = {"ms_per_step_median": round(statistics.median(ws), 4), "ms_per_step_min": min(ws), "ms_per_step_max": max(ws),
                      "per_process_medians_ms": [round(m, 4) for m in meds], "spread_between_processes_ms": round(max(meds) - min(meds), 4),
                      "launches": recs[plan][0]["launches"], "opt_launches": recs[plan][0]["opt_launches"]}
    off, on = step["off"]["ms_per_step_median"], step["on"]["ms_per_step_median"]
    in_step = {k: round(statistics.median(r["in_step_ms"][k] for r in recs["on"]), 5) for k in SAM_LABELS}
    n = kern["parameters"]
    in_step_rate = {k: round(b * n / (in_step[k] * 1e-3) / 1e9, 1) for k, b in (("sam_norm", 4.0), ("sam_ascend", 16.0), ("sam_descend", 8.0))}
    ks = kern["kernels"]
    yard = ks["ema_update"]
    spread = max(v["GBps_spread"] for v in ks.values())
    out = {"config": CFG, "optimizer": "SGD", "rho": RHO, "device": recs["on"][0]["device"], "parameters": n, "processes_per_plan": a.processes,
           "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup, "step": step,
           "sam_step_as_a_multiple_of_the_plain_step": round(on / off, 4),
           "excess_over_twice_the_plain_step_ms": round(on - 2 * off, 4),
           "spread_between_processes_ms": {p: step[p]["spread_between_processes_ms"] for p in step},
           "labels_sam": recs["on"][0]["labels_sam"], "in_step_ms_median": in_step, "in_step_GBps": in_step_rate,
           "in_step_sum_of_the_three_ms": round(sum(in_step.values()), 5),
           "eager_sum_ms": [r["eager_sum_ms"] for r in recs["on"]], "eager_launches": recs["on"][0]["eager_launches"],
           "kernels_back_to_back": ks, "yardstick": "ema_update",
           "short_of_the_yardstick_by_more_than_the_spread": {k: bool(ks[k]["GBps_median"] + spread < yard["GBps_median"])
                                                              for k in ("sam_ascend", "sam_descend")},
           "sam_report_last_step": recs["on"][-1]["sam_report"], "windows": {p: [r["windows_ms"] for r in recs[p]] for p in recs},
           "finite_weights": all(r["finite_weights"] for p in recs for r in recs[p])}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
