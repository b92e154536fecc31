#!/usr/bin/env python3
"""What the weights' moving average costs a step (Config.WEIGHT_EMA): the bf16 ResNet-50 step of bench.py's
configuration (512 x 640, batch 32, regressed location, 16^3 orientation bins, uint8 input) with the key off -- the plan of the commit
before the feature, launch for launch -- and on, on one GPU.

  python tools/ema_bench.py [--steps 20] [--rounds 7] [--warmup 10] [--profile-steps 7] [--out profiles/ema_bench.json]

One process, two engines from the same seed.  After `warmup` replays of each, `rounds` rounds are timed; a round times `steps` replays
of off, on, off again and on again, so that two windows of one and the same plan stand beside the difference between the plans.  Per plan
the median over all its windows is reported, with the largest difference between two windows of one plan in one round (the run-to-run
spread) and the range over the rounds.

The `ema` launch itself (the streaming pass and the one-thread kernel behind it, in one profiler record) and the `sgd` launch are timed by
the library's HIP-event launch profiler in `profile-steps` eager steps of the on-engine (median), where both run in the step's own cache
state, and once more back to back (100 calls each between two events, on copies of the buffers).  Bytes are the algorithm's: 12 per
parameter for `ema` (read w, read ema, write ema), 20 for `sgd` (read g, v, w; write v, w).  The prediction is 12 n bytes at the best
rate this project measured for a stream that reads and writes HBM (profiles/r05_hbm_rates.txt: 5.18 TB/s).  There is no threshold: the
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
HBM_TBS = 5.18              # profiles/r05_hbm_rates.txt, first row: the fastest read + write stream measured in the step
DECAY = 0.9999


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd import hip
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py needs the GPU: nothing here can be measured without one")

    engines = {}
    for name, decay in (("off", None), ("on", DECAY)):
        cfg = make_config(**CFG)
        cfg.WEIGHT_EMA = decay
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
    assert on.labels["opt"] == off.labels["opt"] + ["ema"] and all(on.labels[k] == off.labels[k] for k in ("prep", "fwd", "loss", "bwd"))
    same_weights = bool(torch.equal(off.flat_w, on.flat_w))                 # the same trajectory so far, bit for bit

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

    # the two launches inside the step (eager, one HIP-event pair per launch), and every other launch of both plans beside them: where
    # a step-time difference beyond the launch's own time would have to come from
    n = int(on.n_flat)
    per = {"ema": [], "sgd": []}
    eager = {"off": [], "on": []}                       # per profiled step: [ms of every launch, in launch order]
    for _ in range(max(a.profile_steps, 1)):
        for name in ("off", "on"):
            recs = engines[name].profile_step()
            eager[name].append([float(r[2]) for r in recs])
            if name == "on":
                for rec in recs:
                    if rec[0] in per:
                        per[rec[0]].append(float(rec[2]))
    order = [l for k in ("prep", "fwd", "loss", "bwd", "opt") for l in off.labels[k]]
    med = {name: [statistics.median(col) for col in zip(*eager[name])] for name in ("off", "on")}
    assert len(med["off"]) == len(order) and len(med["on"]) == len(order) + 1
    diffs = sorted(((med["on"][i] - med["off"][i], i) for i in range(len(order))), reverse=True)
    eager_cmp = {"sum_ms_off": round(sum(med["off"]), 4), "sum_ms_on_without_ema": round(sum(med["on"][:-1]), 4), "ema_ms": round(med["on"][-1], 5),
                 "first_launch": {"label": order[0], "off_ms": round(med["off"][0], 5), "on_ms": round(med["on"][0], 5)},
                 "largest_increases": [{"launch": i, "label": order[i], "off_ms": round(med["off"][i], 5), "on_ms": round(med["on"][i], 5)} for _, i in diffs[:5]]}
    by = {"ema": 12.0 * n, "sgd": 20.0 * n}
    launches = {}
    for k in ("ema", "sgd"):
        ms = statistics.median(per[k])
        launches[k] = {"bytes": by[k], "in_step_ms_median": round(ms, 5), "in_step_ms_min": round(min(per[k]), 5), "in_step_ms_max": round(max(per[k]), 5),
                       "in_step_GBps": round(by[k] / (ms * 1e-3) / 1e9, 1)}

    # back to back on copies (the buffers total 0.3 / 0.5 GB: past the L2, partly inside the 256 MiB last-level cache)
    w, e, g, v = (on.flat_w.clone() for _ in range(4))
    st = on.ema_state.clone()
    hyper = torch.tensor([0.0, 0.9, 0.0], dtype=torch.float32, device=on.device)          # lr 0: the values stay where they are
    nsq = torch.ones(1, dtype=torch.float32, device=on.device)
    # ema_fixed: the same entry point over 4 elements: what its two kernels cost before any byte streams (the profiler's `ema` record
    # holds both kernels, the `sgd` record one)
    calls = {"ema": lambda: hip.ema_update(n, w, e, st), "sgd": lambda: hip.sgd_momentum_clip(n, w, g, v, hyper, nsq),
             "ema_fixed": lambda: hip.ema_update(4, w, e, st)}
    by["ema_fixed"], launches["ema_fixed"] = 48.0, {"bytes": 48.0}
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

    launches["ema_fixed"].pop("back_to_back_GBps")
    stream_ms = launches["ema"]["in_step_ms_median"] - launches["ema_fixed"]["back_to_back_ms"]
    launches["ema"]["in_step_GBps_without_fixed_cost"] = round(by["ema"] / (stream_ms * 1e-3) / 1e9, 1)
    predicted_ms = by["ema"] / (HBM_TBS * 1e12) * 1e3
    out = {"config": CFG, "decay": DECAY, "device": torch.cuda.get_device_name(0), "parameters": n, "steps": a.steps, "rounds": a.rounds,
           "warmup": a.warmup, "same_weights_after_warmup": same_weights, "step": step, "delta_on_minus_off_ms": delta,
           "windows": rounds, "launches": launches, "eager_launch_comparison": eager_cmp,
           "prediction": {"hbm_TBps": HBM_TBS, "source": "profiles/r05_hbm_rates.txt", "ema_bytes": by["ema"], "ema_ms": round(predicted_ms, 5),
                          "measured_in_step_over_predicted": round(launches["ema"]["in_step_ms_median"] / predicted_ms, 3),
                          "measured_back_to_back_over_predicted": round(launches["ema"]["back_to_back_ms"] / predicted_ms, 3)},
           "ema_state": on.weight_ema(), "finite_weights": bool(torch.isfinite(on.flat_w).all() and torch.isfinite(on.flat_ema).all())}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
