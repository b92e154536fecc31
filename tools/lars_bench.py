#!/usr/bin/env python3
"""What layer-wise adaptive rate scaling costs a step (Config.LARS): the bf16 ResNet-50 step of bench.py's
configuration (512 x 640, batch 32, regressed location, 16^3 orientation bins, uint8 input) with the key off -- the plan of the commit
before the feature, launch for launch -- and on, on one GPU.

  python tools/lars_bench.py [--steps 20] [--rounds 7] [--warmup 10] [--profile-steps 7] [--out profiles/lars_bench.json]

One process, two engines from the same seed.  After `warmup` replays of each, `rounds` rounds are timed; a round times `steps` replays
of off, on, off again and on again, so that two windows of one and the same plan stand beside the difference between the plans.  Per plan
the median over all its windows is reported, with the largest difference between two windows of one plan in one round (the run-to-run
spread) and the range over the rounds.

The three launches (`lars_norms`, `lars_trust`, `lars_sgd`) and the off-engine's `sgd` are timed by the library's HIP-event launch
profiler in `profile-steps` eager steps (median), where they run in the step's own cache state, and once more back to back (100 calls
each between two events, on copies of the buffers).  Bytes are the algorithm's: 8 per parameter for `lars_norms` (read w, g), 20 for
`lars_sgd` and `sgd` (read g, v, w; write v, w), and the slot pairs plus the per-tensor tables for `lars_trust`, whose time is not a
stream's: it is set by the tensor with the most slots, added in index order by one wave.  The rates stand beside those recorded for
`urso_ema_update` (profiles/ema_bench.json) and `urso_grad_accum_close` (profiles/accum_bench.json).  There is no threshold: the
numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=16, bottleneck=32, branch=1024,
           dtype="bfloat16")
ETA = 0.001


def _recorded(path, *keys):
    """A figure of an earlier bench's JSON file (None when the file or the key is not there)."""
    try:
        with open(os.path.join(ROOT, "profiles", path)) as fh:
            x = json.load(fh)
        for k in keys:
            x = x[k]
        return x
    except (OSError, KeyError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lars_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd import hip, lars
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/lars_bench.py needs the GPU: nothing here can be measured without one")

    engines = {}
    for name, eta in (("off", None), ("on", ETA)):
        cfg = make_config(**CFG)
        cfg.LARS = eta
        img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
        u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
        eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
        eng.set_input_u8(True)
        eng.load_batch_u8(u8, loc, ori)
        for _ in range(max(a.warmup, 1)):
            eng.step()
        torch.cuda.synchronize()
        engines[name] = eng
    off, on = engines["off"], engines["on"]
    NEW = ["lars_norms", "lars_trust", "lars_sgd"]
    assert off.labels["opt"][-1] == "sgd" and on.labels["opt"] == off.labels["opt"][:-1] + NEW
    assert all(on.labels[k] == off.labels[k] for k in ("prep", "fwd", "loss", "bwd"))

    def window(eng):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    rounds = []
    for _ in range(a.rounds):
        rounds.append({"off": [], "on": []})
        for name in ("off", "on", "off", "on"):
            rounds[-1][name].append(round(window(engines[name]), 4))
        print("round %d  off %s  on %s" % (len(rounds), rounds[-1]["off"], rounds[-1]["on"]), file=sys.stderr, flush=True)
    step = {}
    for name in ("off", "on"):
        ws = [x for r in rounds for x in r[name]]
        step[name] = {"ms_per_step_median": round(statistics.median(ws), 4), "ms_per_step_min": min(ws), "ms_per_step_max": max(ws),
                      "spread_within_round_ms": round(max(abs(r[name][0] - r[name][1]) for r in rounds), 4),
                      "launches": sum(len(v) for v in engines[name].labels.values()), "opt_launches": engines[name].labels["opt"]}
    delta = round(step["on"]["ms_per_step_median"] - step["off"]["ms_per_step_median"], 4)

    # the launches inside the step (eager, one HIP-event pair per launch)
    lp = on.lars_plan
    n = int(sum(cnt for _o, cnt, _a in lp.tensors))
    slots_max = int(max(int(lp.first_h[t + 1]) - int(lp.first_h[t]) for t in range(lp.T)))
    by = {"lars_norms": 8.0 * n, "lars_trust": 8.0 * lp.nblocks + 36.0 * lp.T, "lars_sgd": 20.0 * n, "sgd": 20.0 * int(off.n_flat)}
    per = {k: [] for k in by}
    sums = {"off": [], "on": []}
    for _ in range(max(a.profile_steps, 1)):
        for name in ("off", "on"):
            recs = engines[name].profile_step()
            sums[name].append(sum(float(r[2]) for r in recs))
            for rec in recs:
                if rec[0] in per and (rec[0] == "sgd") == (name == "off"):
                    per[rec[0]].append(float(rec[2]))
    launches = {}
    for k in by:
        ms = statistics.median(per[k])
        launches[k] = {"bytes": by[k], "in_step_ms_median": round(ms, 5), "in_step_ms_min": round(min(per[k]), 5),
                       "in_step_ms_max": round(max(per[k]), 5), "in_step_GBps": round(by[k] / (ms * 1e-3) / 1e9, 1)}
    eager_cmp = {"sum_ms_off": round(statistics.median(sums["off"]), 4), "sum_ms_on": round(statistics.median(sums["on"]), 4),
                 "new_launches_minus_sgd_ms": round(sum(launches[k]["in_step_ms_median"] for k in NEW) - launches["sgd"]["in_step_ms_median"], 5)}

    # back to back on copies of the buffers (lr 0: the values stay where they are)
    w, g, v = on.flat_w.clone(), on.flat_g.clone(), on.flat_v.clone()
    hyper = torch.tensor([0.0, 0.9, 0.0], dtype=torch.float32, device=on.device)
    nsq = torch.ones(1, dtype=torch.float32, device=on.device)
    plan = hip.LarsPlan(lp.tensors, on.device)
    calls = {"lars_norms": lambda: plan.norms(w, g), "lars_trust": lambda: plan.trust_ratios(hyper, nsq, ETA, 1e-8, False),
             "lars_sgd": lambda: plan.sgd(w, g, v, hyper, nsq), "sgd": lambda: hip.sgd_momentum_clip(int(off.n_flat), w, g, v, hyper, nsq)}
    for k, call in calls.items():
        for _ in range(10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(100):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / 100
        launches[k]["back_to_back_ms"] = round(ms, 5)
        launches[k]["back_to_back_GBps"] = round(by[k] / (ms * 1e-3) / 1e9, 1)
    launches["lars_trust"].pop("in_step_GBps")
    launches["lars_trust"].pop("back_to_back_GBps")
    launches["lars_trust"]["note"] = "not a stream: one wave per tensor adds its slots in index order; the time is the largest tensor's"

    recorded = {"urso_ema_update": {"file": "profiles/ema_bench.json", "in_step_ms": _recorded("ema_bench.json", "launches", "ema", "in_step_ms_median"),
                                    "in_step_GBps": _recorded("ema_bench.json", "launches", "ema", "in_step_GBps"),
                                    "back_to_back_GBps": _recorded("ema_bench.json", "launches", "ema", "back_to_back_GBps")},
                "urso_grad_accum_close": {"file": "profiles/accum_bench.json",
                                          "in_step_ms": _recorded("accum_bench.json", "launches", "close", "in_step_ms_median"),
                                          "in_step_GBps": _recorded("accum_bench.json", "launches", "close", "in_step_GBps"),
                                          "back_to_back_GBps": _recorded("accum_bench.json", "launches", "close", "back_to_back_GBps")}}
    ema_rate = recorded["urso_ema_update"]["in_step_GBps"]
    if ema_rate:
        for k in ("lars_norms", "lars_sgd", "sgd"):
            launches[k]["rate_over_ema"] = round(launches[k]["in_step_GBps"] / ema_rate, 3)
    summ = lars.summary(on.lars_report(adapting_only=True))
    out = {"config": CFG, "eta": ETA, "device": torch.cuda.get_device_name(0), "parameters": n, "tensors": lp.T, "blocks": lp.nblocks,
           "slots_of_the_largest_tensor": slots_max, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup, "step": step,
           "delta_on_minus_off_ms": delta, "windows": rounds, "launches": launches, "eager_launch_comparison": eager_cmp,
           "recorded_beside": recorded, "trust_summary_last_step": summ,
           "finite_weights": bool(torch.isfinite(on.flat_w).all() and torch.isfinite(off.flat_w).all())}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
