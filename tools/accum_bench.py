#!/usr/bin/env python3
"""What gradient accumulation costs and saves (Config.GRAD_ACCUM_STEPS): the bf16 ResNet-50 step of bench.py's
configuration (512 x 640, batch 32, regressed location, 16^3 orientation bins, uint8 input, SGD) at k = 1 -- the plan of the commit before
the feature, launch for launch -- and at k = 2, 4, 8, on one GPU.

  python tools/accum_bench.py [--steps 6] [--rounds 5] [--warmup 3] [--profile-steps 5] [--out profiles/accum_bench.json]

One process, one engine per k from the same seed.  After `warmup` optimizer steps of each, `rounds` rounds are timed; a round times `steps`
optimizer steps (steps x k replays) of every k in turn and of k = 1 a second time, so that two windows of one and the same plan stand
beside the differences between the plans.  Per k: ms per optimizer step, ms per micro-step and images per second.

The three new launches (grad_accum as copy and as add, grad_close) are timed by the library's HIP-event launch profiler in `profile-steps`
eager micro-steps of each role of the k = 4 engine (median), in the step's own cache state, and once more back to back (100 calls each
between two events, on copies of the buffers) beside urso_ema_update, which has the same access shape and whose rate in the step is on
record (profiles/ema_bench.json).  Bytes are the algorithm's: 8 per parameter for the copy, 12 for the add, the close and the average.  A
launch whose back-to-back rate is below 0.9 of urso_ema_update's in the same run is flagged (`below_0.9_of_ema`); nothing else is judged.

The last part is recorded, not gated: on a small soft-classification model (folded BN, so every loss is a mean over the batch) the
gradient of k = 4 micro-batches of 2 images against that of one batch of the same 8 images, as a relative L2 difference -- the two
differ by the order of summation only."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=16, bottleneck=32, branch=1024,
           dtype="bfloat16")
SMALL = dict(backbone="resnet18", h=64, w=64, bottleneck=16, branch=64, regress_ori=False, regress_loc=False, dtype="float32")
KS = (1, 2, 4, 8)
BYTES = {"copy": 8.0, "add": 12.0, "close": 12.0, "ema": 12.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from util import make_config, synthetic_batch
    from ursonet_amd import grad_accum, hip
    from ursonet_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("tools/accum_bench.py needs the GPU: nothing here can be measured without one")

    engines = {}
    for k in KS:
        cfg = make_config(**CFG)
        cfg.GRAD_ACCUM_STEPS = k
        img, loc, ori, _ = synthetic_batch(cfg, CFG["batch"], seed=1234)
        u8 = np.clip(np.rint(img + np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)), 0, 255).astype(np.uint8)
        eng = Engine(cfg, "training", seed=1234, randomize_bn=True)
        eng.set_input_u8(True)
        eng.load_batch_u8(u8, loc, ori)
        for _ in range(max(a.warmup, 1) * k):
            eng.step()
        torch.cuda.synchronize()
        engines[k] = eng
        print("k = %d ready: opt %s" % (k, eng.labels["opt"]), file=sys.stderr, flush=True)
    assert "accum" not in engines[1].labels and engines[1].flat_acc is None
    assert all(engines[k].labels["opt"] == ["grad_close"] + engines[1].labels["opt"] and engines[k].labels["accum"] == ["grad_accum"] for k in KS[1:])

    def window(k):
        eng = engines[k]
        t0 = time.perf_counter()
        for _ in range(a.steps * k):
            eng.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    rounds = []
    for _ in range(a.rounds):
        r = {k: [] for k in KS}
        for k in KS + (1,):
            r[k].append(round(window(k), 4))
        rounds.append({str(k): v for k, v in r.items()})
        print("round %d  %s" % (len(rounds), rounds[-1]), file=sys.stderr, flush=True)
    step = {}
    for k in KS:
        ws = [x for r in rounds for x in r[str(k)]]
        med = statistics.median(ws)
        step[str(k)] = {"ms_per_optimizer_step_median": round(med, 4), "ms_per_optimizer_step_min": min(ws), "ms_per_optimizer_step_max": max(ws),
                        "ms_per_micro_step_median": round(med / k, 4), "images_per_s": round(k * CFG["batch"] / (med * 1e-3), 1),
                        "effective_batch": k * CFG["batch"], "launches_closing": sum(len(v) for p, v in engines[k].labels.items() if p != "accum"),
                        "opt_launches": engines[k].labels["opt"]}
    step["1"]["spread_within_round_ms"] = round(max(abs(r["1"][0] - r["1"][1]) for r in rounds), 4)

    # the three launches inside the step (eager, one HIP-event pair per launch), by role, with the optimizer launches they stand beside
    eng = engines[4]
    n = int(eng.n_flat)
    per = {"copy": [], "add": [], "close": [], "sqnorm": [], "sgd": []}
    eager = {"k1": [], "first": [], "add": [], "close": []}      # per profiled step: [ms of every launch in front of the tail, in launch order]
    order = [l for p in ("prep", "fwd", "loss", "bwd") for l in eng.labels[p]]
    assert len(order) == sum(len(engines[1].labels[p]) for p in ("prep", "fwd", "loss", "bwd"))
    for _ in range(max(a.profile_steps, 1)):
        eager["k1"].append([float(r[2]) for r in engines[1].profile_step()][:len(order)])
        for role, name in (("first", "copy"), ("add", "add")):
            recs = eng.profile_step(role)
            eager[role].append([float(r[2]) for r in recs][:len(order)])
            per[name] += [float(r[2]) for r in recs if r[0] == "grad_accum"]
        recs = eng.profile_step("close")
        eager["close"].append([float(r[2]) for r in recs][:len(order)])
        for r in recs:
            if r[0] in ("grad_close", "sqnorm", "sgd"):
                per["close" if r[0] == "grad_close" else r[0]].append(float(r[2]))
    # where a step-time difference beyond the new launches' own time would have to come from: every other launch, role by role, beside
    # the same launch of the k = 1 engine
    med = {name: [statistics.median(col) for col in zip(*rows)] for name, rows in eager.items()}
    eager_cmp = {"launches_compared": len(order), "sum_ms": {name: round(sum(v), 4) for name, v in med.items()}, "largest_increases": {}}
    for role in ("first", "add", "close"):
        diffs = sorted(((med[role][i] - med["k1"][i], i) for i in range(len(order))), reverse=True)
        eager_cmp["largest_increases"][role] = [{"launch": i, "label": order[i], "k1_ms": round(med["k1"][i], 5), "ms": round(med[role][i], 5)}
                                                for _, i in diffs[:5]]
    launches = {}
    for name, ms in per.items():
        m = statistics.median(ms)
        launches[name] = {"in_step_ms_median": round(m, 5), "in_step_ms_min": round(min(ms), 5), "in_step_ms_max": round(max(ms), 5)}
        if name in BYTES:
            launches[name]["bytes"] = BYTES[name] * n
            launches[name]["in_step_GBps"] = round(BYTES[name] * n / (m * 1e-3) / 1e9, 1)

    # back to back on copies, urso_ema_update beside them
    g, acc, w, e = (eng.flat_w.clone() for _ in range(4))
    g.mul_(1e-3)
    acc.mul_(1e-3)
    sq = torch.zeros(hip.grad_accum_parts(n), dtype=torch.float32, device=eng.device)
    st = torch.tensor([0.9999, 0.0, 0.0, 0.9999, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=eng.device)
    calls = {"copy": lambda: hip.grad_accum(n, g, acc, True), "add": lambda: hip.grad_accum(n, g, acc, False),
             "close": lambda: hip.grad_accum_close(n, g, acc, 0.5, sq), "ema": lambda: hip.ema_update(n, w, e, st)}
    launches["ema"] = {"bytes": BYTES["ema"] * n}
    for name, call in calls.items():
        for _ in range(10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(100):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / 100
        launches[name]["back_to_back_ms"] = round(ms, 5)
        launches[name]["back_to_back_GBps"] = round(BYTES[name] * n / (ms * 1e-3) / 1e9, 1)
    for name in ("copy", "add", "close"):
        ratio = launches[name]["back_to_back_GBps"] / launches["ema"]["back_to_back_GBps"]
        launches[name]["rate_over_ema"] = round(ratio, 3)
        launches[name]["below_0.9_of_ema"] = bool(ratio < 0.9)

    # k x B accumulated against one batch of k B: soft classification, folded BN
    kk, b = 4, 2
    cfg_small = make_config(batch=b, **SMALL)
    cfg_small.GRAD_ACCUM_STEPS = kk
    cfg_big = make_config(batch=kk * b, **SMALL)
    img, loc, ori, _ = synthetic_batch(cfg_big, kk * b, seed=77)
    small = Engine(cfg_small, "training", seed=5, randomize_bn=True)
    big = Engine(cfg_big, "training", seed=5, randomize_bn=True)
    for j in range(kk):
        small.load_batch(img[j * b:(j + 1) * b], loc[j * b:(j + 1) * b], ori[j * b:(j + 1) * b])
        small.step_eager()
    big.load_batch(img, loc, ori)
    big.run_prep(); big.run_forward(); big.run_backward()
    torch.cuda.synchronize()
    ga, gb = small.flat_g.double(), big.flat_g.double()
    rel = float((ga - gb).norm() / gb.norm())

    out = {"config": CFG, "device": torch.cuda.get_device_name(0), "parameters": n, "steps": a.steps, "rounds": a.rounds, "warmup": a.warmup,
           "step": step, "windows": rounds, "launches": launches, "profiled_engine_k": 4, "eager_launch_comparison": eager_cmp,
           "accumulated_vs_one_batch": {"config": SMALL, "micro_batches": kk, "images_per_micro_batch": b, "c": float(grad_accum.inv32(kk)),
                                        "relative_l2_difference": rel, "gradient_norm": float(gb.norm())},
           "finite_weights": {str(k): bool(torch.isfinite(engines[k].flat_w).all()) for k in KS}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
