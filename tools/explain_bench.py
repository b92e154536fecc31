#!/usr/bin/env python3
"""What occlusion-sensitivity maps cost (explain()): the bf16 ResNet-50 at 512 x 640, engine batch 32, soft
orientation head with 32^3 bins and regressed location, on one GPU.

  python tools/explain_bench.py [--images 2] [--windows 5] [--out profiles/explain_bench.json]

A fresh process per configuration, all in one run of this tool, each reporting the median over its windows after one untimed call:
  launches   urso_occl_fill_u8 (32 rows of 512 x 640 x 3, 64 x 64 rects), urso_occl_score (32 rows of 32^3 logits, one head),
             urso_occl_splat (285 patches of 64 x 64 at stride 32 into 5 maps of 512 x 640) and urso_heat_overlay_u8 (512 x 640) back to
             back, 200 calls each between two events, beside urso_frames_gather_u8 (32 frames of 512 x 640 x 3 copied) and urso_ens_add
             (32 rows of 32^3 logits, first = 0) in the same process.  Bytes are the algorithm's: the fill reads and writes a row's bytes
             once (the source frame stays in cache: 2 n H W C is the upper bound the gather's figure uses too); the score reads both
             rows' logits once (4 K per row and the baseline's 4 K, the second and third sweep come out of L2); the splat writes 8 M h w;
             the overlay reads 8 h w and reads and writes 3 h w.  fill_over_gather_rate is the fill's rate over the gather's;
  explain    a window is one explain(patch=64, stride=32) of the images: per image 286 rows in 9 passes, the splat and the read; beside
             it, in the same process, the same number of bare Engine.load_batch_u8 + Engine.forward replays of a resident batch, ended
             by one synchronise.  added_ms_per_pass is the difference per pass: the fill, the heads' decode, urso_pose_decode,
             urso_occl_score and, once per image, the splat, the read and the host's bookkeeping -- and the loading of the frames, which
             happens in front of a call's first pass: load_image_seconds_median is one dataset.load_image() on the host, loads_per_call
             how many a call makes, read_bytes_per_image the size of the one read.
The dataset is synthetic (frames drawn on the host per call).  There is no threshold: the numbers are recorded, not judged."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(backbone="resnet50", h=512, w=640, batch=32, regress_ori=False, regress_loc=True, ori_bins=32, bottleneck=128, branch=1024,
           dtype="bfloat16")
PATCH, STRIDE = 64, 32
CHILDREN = ("launches", "explain")


def launches(a, out):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from ursonet_amd import explain as ex, hip
    if not torch.cuda.is_available():
        raise SystemExit("tools/explain_bench.py needs the GPU: nothing here can be measured without one")
    out["device"] = torch.cuda.get_device_name(0)
    B, K, H, W = CFG["batch"], CFG["ori_bins"] ** 3, CFG["h"], CFG["w"]
    N = H * W * 3
    f64 = dict(dtype=torch.float64, device="cuda")
    frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda")
    batch = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
    grid = ex.occlusion_rects((0, 0, H, W), PATCH, STRIDE)
    rects = torch.as_tensor(grid).cuda()
    P = len(grid)
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
    addr = torch.tensor([frames[b].data_ptr() for b in range(B)], dtype=torch.int64, device="cuda")
    kind = torch.ones(B, dtype=torch.uint8, device="cuda")
    z, z0 = torch.randn(B, K, device="cuda") * 4, torch.randn(K, device="cuda") * 4
    dec = torch.randn(B, hip.DEC_COLS, **f64)
    table = torch.empty(B, hip.OCCL_COLS, **f64)
    acc, stat = torch.empty(B, K, **f64), torch.empty(B, hip.ENS_STAT, **f64)
    hip.ens_add(B, B, 0, z, acc, stat, True)
    scores, cols = torch.randn(P, hip.OCCL_COLS, **f64), [0, 1, 2, 3, 4]
    maps = torch.empty(len(cols), H, W, **f64)
    lut = torch.as_tensor(ex.heat_lut()).cuda()
    pic = frame.clone()
    calls = {"occl_fill_u8": (lambda: hip.occl_fill_u8(frame, rects[100:100 + B], (124, 117, 104, 0), batch, B), 2.0 * B * N),
             "frames_gather_u8": (lambda: hip.frames_gather_u8(B, H * W, addr, kind, batch), 2.0 * B * N),
             "occl_score": (lambda: hip.occl_score(B, B, 0, dec[0], dec, table, ori_z0=z0, ori_z=z), 4.0 * B * K + 4.0 * K),
             "ens_add": (lambda: hip.ens_add(B, B, 0, z, acc, stat, False), B * K * 20.0),
             "occl_splat": (lambda: hip.occl_splat(scores, cols, rects, (0, 0, H, W), maps), 8.0 * len(cols) * H * W),
             "heat_overlay_u8": (lambda: hip.heat_overlay_u8(maps[0], -3.0, 255.0 / 6.0, lut, 128, pic), 14.0 * H * W)}
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
    out["rows"], out["frame"], out["logits"], out["patches"], out["maps"] = B, [H, W, 3], K, P, len(cols)
    out["fill_over_gather_rate"] = round(out["occl_fill_u8"]["GBps"] / out["frames_gather_u8"]["GBps"], 4)
    # the fill against its NumPy statement at this size, once: a benchmark of a wrong kernel is no benchmark
    torch.cuda.synchronize()
    want = ex.occlude_host(frame.cpu().numpy(), grid[100:100 + B], (124, 117, 104))
    hip.occl_fill_u8(frame, rects[100:100 + B], (124, 117, 104, 0), batch, B)
    out["fill_equals_occlude_host"] = bool(np.array_equal(batch.cpu().numpy(), want))


def child(a):
    out = {}
    if a.child == "launches":
        launches(a, out)
        print("RESULT " + json.dumps(out))
        return
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from util import make_config
    from ursonet_amd import explain as ex, net
    from ursonet_amd.dataset import SyntheticPoses
    if not torch.cuda.is_available():
        raise SystemExit("tools/explain_bench.py needs the GPU: nothing here can be measured without one")
    with tempfile.TemporaryDirectory() as tmp:
        cfg = make_config(**CFG)
        cfg.NAME = "bench"
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=tmp)
        out["device"] = torch.cuda.get_device_name(0)
        ds = SyntheticPoses(a.images, CFG["h"], CFG["w"], cfg, seed=5)
        run = lambda: ex.explain(model, ds, patch=PATCH, stride=STRIDE)                         # noqa: E731
        r = run()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            r = run()                                                                           # (ends in a read from the device)
            ws.append((time.perf_counter() - t0) / a.images)
        passes = int(r.passes[0])
        eng = model._engine
        batch = torch.randint(0, 256, (CFG["batch"], CFG["h"], CFG["w"], 3), dtype=torch.uint8, device="cuda")
        fs = []
        for _ in range(a.windows + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                eng.load_batch_u8(batch)
                eng.forward()
            torch.cuda.synchronize()
            fs.append(time.perf_counter() - t0)
        fs = fs[1:]
        ls = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            ds.load_image(ds.image_ids[0])
            ls.append(time.perf_counter() - t0)
        e, f = statistics.median(ws), statistics.median(fs)
        # per call the first frame is loaded once for the refusals and every frame once by the feeder, all in front of the first pass
        out.update({"load_image_seconds_median": round(statistics.median(ls), 4), "loads_per_call": a.images + 1,
                    "read_bytes_per_image": 8 * ((int(r.patches[0]) + 1) * ex.COLS + len(r.maps[0]) * CFG["h"] * CFG["w"] + ex.DEC_COLS)})
        out.update({"patch": PATCH, "stride": STRIDE, "patches": int(r.patches[0]), "passes_per_image": passes,
                    "explain_seconds_per_image_median": round(e, 4), "explain_seconds_per_image_min": round(min(ws), 4),
                    "explain_seconds_per_image_max": round(max(ws), 4), "forward_seconds_same_passes_median": round(f, 4),
                    "forward_seconds_same_passes_min": round(min(fs), 4), "forward_seconds_same_passes_max": round(max(fs), 4),
                    "forward_ms_per_pass": round(1e3 * f / passes, 3), "added_ms_per_pass": round(1e3 * (e - f) / passes, 3),
                    "explain_over_forward": round(e / f, 4)})
        print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_bench.json"))
    ap.add_argument("--child", choices=CHILDREN)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    for name in CHILDREN:                                                                      # a fresh child per configuration; this process never opens the GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--images", str(a.images), "--windows", str(a.windows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            raise SystemExit("configuration %s failed (exit %d)" % (name, p.returncode))
        res[name] = json.loads(lines[-1][len("RESULT "):])
        print(name, res[name], file=sys.stderr, flush=True)
    device = res["launches"].pop("device")
    res["explain"].pop("device", None)
    out = {"config": CFG, "images": a.images, "windows": a.windows, "device": device, "launches": res["launches"], "explain": res["explain"]}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
