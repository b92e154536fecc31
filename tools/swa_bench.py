#!/usr/bin/env python3
"""What stochastic weight averaging costs a step (Config.SWA): the bf16 ResNet-50 step of bench.py's configuration
(512 x 640, batch 32, regressed location, 16^3 orientation bins, uint8 input) on one GPU under four plans:

  off      SWA = None: the plan of the commit before the feature, launch for launch
  shut     SWA = 2^30: the `swa` launch is in the plan and its gate never opens (what every step between two collections pays)
  on       SWA = 1: every step collects (the 12-byte pass)
  on_var   SWA = 1 with SWA_VARIANCE (the 20-byte pass)

  python tools/swa_bench.py [--steps 20] [--windows 5] [--turns 2] [--warmup 10] [--out profiles/swa_bench.json]

Fresh processes in turn: every plan runs in a process of its own, `turns` times, in the order off, shut, on, on_var, off, ...; a process
builds its engine, replays the captured step `warmup` times and then times `windows` windows of `steps` replays.  Per plan the median over
all its windows is reported with their range, and the largest difference between the medians of two processes of one plan (the
run-to-run spread that a difference between two plans has to exceed to mean anything).

One more process times the passes back to back (100 calls each between two events, on copies of the buffers, in this order in the same
process): urso_ema_update (12 bytes per parameter), urso_swa_update with an open gate without and with sq (12 and 20), with a shut gate
(two near-empty launches), and urso_swag_sample.  There is no threshold: the numbers are recorded, not judged."""
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
PLANS = {"off": dict(SWA=None), "shut": dict(SWA=2 ** 30), "on": dict(SWA=1), "on_var": dict(SWA=1, SWA_VARIANCE=True)}


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/swa_bench.py needs the GPU: nothing here can be measured without one")
    return torch


def _engine(keys):
    import numpy as np
    from util import make_config, synthetic_batch
    from ursonet_amd.engine import Engine
    cfg = make_config(**CFG)
    for k, v in keys.items():
        setattr(cfg, k, v)
    img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
    u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
    eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
    eng.set_input_u8(True)
    eng.load_batch_u8(u8, loc, ori)
    return eng


def child_plan(name, a):
    torch = _setup()
    eng = _engine(PLANS[name])
    for _ in range(max(a.warmup, 1)):
        eng.step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step()
        torch.cuda.synchronize()
        windows.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
    print(json.dumps({"plan": name, "windows_ms": windows, "opt_launches": eng.labels["opt"], "launches": sum(len(v) for v in eng.labels.values()),
                      "swa": eng.swa(), "parameters": int(eng.n_flat), "finite_weights": bool(torch.isfinite(eng.flat_w).all()),
                      "device": torch.cuda.get_device_name(0)}))


def child_rates(a):
    torch = _setup()
    from ursonet_amd import hip, swa, weight_ema
    from ursonet_amd.config import Config
    n = a.parameters
    w = torch.randn(n, device="cuda")
    e, mean, sq, out = w.clone(), w.clone(), (w * w), torch.empty_like(w)
    cfg = Config()
    cfg.WEIGHT_EMA = 0.9999
    est = torch.tensor(weight_ema.initial_state(cfg), dtype=torch.float32, device="cuda")
    state = lambda period, models, var: torch.tensor([period, 0, 0, models, 0, int(var), 0, 0], dtype=torch.int32, device="cuda")
    st12, st20, shut = state(1, 5, False), state(1, 5, True), state(2 ** 30, 5, False)
    s = swa.scale32(0.5)
    calls = [("ema_update", 12.0 * n, lambda: hip.ema_update(n, w, e, est)),
             ("swa_update_12", 12.0 * n, lambda: hip.swa_update(n, w, mean, None, st12)),
             ("swa_update_20", 20.0 * n, lambda: hip.swa_update(n, w, mean, sq, st20)),
             ("swa_update_shut", None, lambda: hip.swa_update(n, w, mean, None, shut)),
             ("ema_update_again", 12.0 * n, lambda: hip.ema_update(n, w, e, est)),
             ("swag_sample", 12.0 * n, lambda: hip.swag_sample(n, mean, sq, out, s, 1, 0))]
    res = {}
    for name, nbytes, call in calls:
        for _ in range(10):
            call()
        reps = []
        for _ in range(a.windows):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(100):
                call()
            t1.record()
            torch.cuda.synchronize()
            reps.append(t0.elapsed_time(t1) / 100)
        ms = statistics.median(reps)
        res[name] = {"ms_median": round(ms, 5), "ms_min": round(min(reps), 5), "ms_max": round(max(reps), 5)}
        if nbytes:
            res[name].update(bytes=nbytes, GBps_median=round(nbytes / (ms * 1e-3) / 1e9, 1), GBps_min=round(nbytes / (max(reps) * 1e-3) / 1e9, 1),
                             GBps_max=round(nbytes / (min(reps) * 1e-3) / 1e9, 1))
    assert int(st12[swa.MODELS]) > 5 and int(shut[swa.MODELS]) == 5         # the open gate collected, the shut one did not
    print(json.dumps({"parameters": n, "calls_per_window": 100, "windows": a.windows, "passes": res}))


def _run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d): nothing more is started" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--turns", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swa_bench.json"))
    ap.add_argument("--child-plan", default=None)
    ap.add_argument("--child-rates", action="store_true")
    ap.add_argument("--parameters", type=int, default=0)
    a = ap.parse_args()
    if a.child_plan:
        return child_plan(a.child_plan, a)
    if a.child_rates:
        return child_rates(a)
    common = ["--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)]
    runs = {name: [] for name in PLANS}
    for turn in range(a.turns):
        for name in PLANS:
            runs[name].append(_run_child(common + ["--child-plan", name]))
            print("turn %d  %-6s %s" % (turn + 1, name, runs[name][-1]["windows_ms"]), file=sys.stderr, flush=True)
    n = runs["off"][0]["parameters"]
    assert runs["shut"][0]["opt_launches"] == runs["off"][0]["opt_launches"] + ["swa"] == runs["on"][0]["opt_launches"]
    step = {}
    for name, rs in runs.items():
        ws = [x for r in rs for x in r["windows_ms"]]
        meds = [statistics.median(r["windows_ms"]) for r in rs]
        step[name] = {"ms_per_step_median": round(statistics.median(ws), 4), "ms_per_step_min": min(ws), "ms_per_step_max": max(ws),
                      "spread_between_processes_ms": round(max(meds) - min(meds), 4), "windows_ms": [r["windows_ms"] for r in rs],
                      "launches": rs[0]["launches"], "opt_launches": rs[0]["opt_launches"], "swa_state_at_end": rs[-1]["swa"],
                      "finite_weights": all(r["finite_weights"] for r in rs)}
    off = step["off"]["ms_per_step_median"]
    delta = {name: round(step[name]["ms_per_step_median"] - off, 4) for name in PLANS if name != "off"}
    rates = _run_child(["--child-rates", "--parameters", str(n), "--windows", str(a.windows)])
    p = rates["passes"]
    out = {"config": CFG, "device": runs["off"][0]["device"], "parameters": n, "steps": a.steps, "windows": a.windows, "turns": a.turns,
           "warmup": a.warmup, "step": step, "delta_vs_off_ms": delta,
           "run_to_run_spread_ms": max(s["spread_between_processes_ms"] for s in step.values()), "back_to_back": rates,
           "swa_12_over_ema_rate": round(p["swa_update_12"]["GBps_median"] / p["ema_update"]["GBps_median"], 3)}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
