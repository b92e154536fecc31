#!/usr/bin/env python3
"""What LAMB costs a step (Config.LAMB): the bf16 ResNet-50 step of bench.py's geometry (512 x 640, batch 32,
regressed location, 16^3 orientation bins, uint8 input) under OPTIMIZER = 'Adam' with the key off -- the plan of the commit before the
feature, launch for launch -- and on, on one GPU.

  python tools/lamb_bench.py [--steps 20] [--rounds 7] [--warmup 10] [--profile-steps 7] [--out profiles/lamb_bench.json]

One process, two engines from the same seed.  After `warmup` replays of each, `rounds` rounds are timed; a round times `steps` replays
of off, on, off again and on again, so that two windows of one and the same plan stand beside the difference between the plans.  Per plan
the median over all its windows is reported, with the largest difference between two windows of one plan in one round (the run-to-run
spread) and the range over the rounds.

The three launches (`lamb_moments`, `lamb_trust`, `lamb_apply`) and the off-engine's `adam` are timed by the library's HIP-event launch
profiler in `profile-steps` eager steps (median), where they run in the step's own cache state, and once more back to back (100 calls
each between two events, on copies of the buffers) -- in that same back-to-back run so are `urso_lars_sgd` and `urso_adam_amsgrad_clip`,
the 16-byte stream and the 4-byte stream they stand beside.  Bytes are the algorithm's: 32 per parameter for `lamb_moments` (read w, g, m,
v, vhat; write m, v, vhat), 16 for `lamb_apply` (read w, m, vhat; write w), 36 for `adam`, 20 for `lars_sgd`, and the slot pairs plus the
per-tensor tables for `lamb_trust`, whose time is not a stream's.  `spread` of a back-to-back figure is the range over five repeats of
the 100 calls.  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=16, bottleneck=32, branch=1024,
           dtype="bfloat16")
ETA = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd import hip, lamb
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/lamb_bench.py needs the GPU: nothing here can be measured without one")

    engines = {}
    for name, eta in (("off", None), ("on", ETA)):
        cfg = make_config(**CFG)
        cfg.OPTIMIZER, cfg.LAMB = "Adam", eta
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
    NEW = ["lamb_moments", "lamb_trust", "lamb_apply"]
    assert off.labels["opt"][-1] == "adam" and on.labels["opt"] == off.labels["opt"][:-1] + NEW
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
    bp = on.lamb_plan
    n = int(sum(cnt for _o, cnt, _a in bp.tensors))
    slots_max = int(max(int(bp.first_h[t + 1]) - int(bp.first_h[t]) for t in range(bp.T)))
    by = {"lamb_moments": 32.0 * n, "lamb_trust": 8.0 * bp.nblocks + 36.0 * bp.T, "lamb_apply": 16.0 * n, "adam": 36.0 * int(off.n_flat)}
    per = {k: [] for k in by}
    sums = {"off": [], "on": []}
    for _ in range(max(a.profile_steps, 1)):
        for name in ("off", "on"):
            recs = engines[name].profile_step()
            sums[name].append(sum(float(r[2]) for r in recs))
            for rec in recs:
                if rec[0] in per and (rec[0] == "adam") == (name == "off"):
                    per[rec[0]].append(float(rec[2]))
    launches = {}
    for k in by:
        ms = statistics.median(per[k])
        launches[k] = {"bytes": by[k], "in_step_ms_median": round(ms, 5), "in_step_ms_min": round(min(per[k]), 5),
                       "in_step_ms_max": round(max(per[k]), 5), "in_step_GBps": round(by[k] / (ms * 1e-3) / 1e9, 1)}
    eager_cmp = {"sum_ms_off": round(statistics.median(sums["off"]), 4), "sum_ms_on": round(statistics.median(sums["on"]), 4),
                 "new_launches_minus_adam_ms": round(sum(launches[k]["in_step_ms_median"] for k in NEW) - launches["adam"]["in_step_ms_median"], 5)}

    # back to back on copies of the buffers (lr 0 and zero gradients: the weights stay where they are, the moments decay)
    w, m, v, vhat = on.flat_w.clone(), on.flat_v.clone(), on.flat_v2.clone(), on.flat_vhat.clone()
    g, mom = torch.zeros_like(w), torch.zeros_like(w)
    hyper = torch.tensor([0.0, 0.9, 0.999, 1e-7, 0.0, 0.0, 0.1, 0.001], dtype=torch.float32, device=on.device)
    hyper3 = torch.tensor([0.0, 0.9, 0.0], dtype=torch.float32, device=on.device)
    nsq = torch.ones(1, dtype=torch.float32, device=on.device)
    plan = hip.LambPlan(bp.tensors, on.device)
    by.update(lars_sgd=20.0 * n)
    calls = {"lamb_moments": lambda: plan.moments(w, g, m, v, vhat, hyper, nsq),
             "lamb_trust": lambda: plan.trust_ratios(nsq, ETA, 1e-8, False),
             "lamb_apply": lambda: plan.apply(w, m, vhat, hyper, nsq),
             "lars_sgd": lambda: plan.tables.sgd(w, g, mom, hyper3, nsq),
             "adam": lambda: hip.adam_amsgrad_clip(int(off.n_flat), w, g, m, v, vhat, hyper, nsq)}
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
        ms = statistics.median(reps)
        launches.setdefault(k, {"bytes": by[k]})
        launches[k]["back_to_back_ms"] = round(ms, 5)
        launches[k]["back_to_back_spread_ms"] = round(max(reps) - min(reps), 5)
        launches[k]["back_to_back_GBps"] = round(by[k] / (ms * 1e-3) / 1e9, 1)
        launches[k]["back_to_back_GBps_range"] = [round(by[k] / (x * 1e-3) / 1e9, 1) for x in (max(reps), min(reps))]
    for key in ("in_step_GBps", "back_to_back_GBps", "back_to_back_GBps_range"):
        launches["lamb_trust"].pop(key)
    launches["lamb_trust"]["note"] = "not a stream: one wave per tensor adds its slots in index order; the time is the largest tensor's"
    lo = launches["lars_sgd"]["back_to_back_GBps_range"][0]
    below = {k: bool(launches[k]["back_to_back_GBps_range"][1] < lo) for k in ("lamb_moments", "lamb_apply")}

    summ = lamb.summary(on.lamb_report(adapting_only=True))
    out = {"config": CFG, "optimizer": "Adam", "eta": ETA, "device": torch.cuda.get_device_name(0), "parameters": n, "tensors": bp.T,
           "blocks": bp.nblocks, "slots_of_the_largest_tensor": slots_max, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup,
           "step": step, "delta_on_minus_off_ms": delta, "windows": rounds, "launches": launches, "eager_launch_comparison": eager_cmp,
           "below_lars_sgd_rate_by_more_than_the_spread": below, "trust_summary_last_step": summ,
           "finite_weights": bool(torch.isfinite(on.flat_w).all() and torch.isfinite(off.flat_w).all())}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
