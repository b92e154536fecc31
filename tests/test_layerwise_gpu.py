"""Teacher-forced per-layer parity of the benchmarked dtype (VERDICT r04 "next round" item 5a).

The whole-step comparisons of tests/test_model_gpu.py compound rounding residue through 50 layers, so their bf16 gates are wide
(1.2e-1 of a tensor's max on the small image).  Here nothing compounds: after ONE device training step every conv / dense layer of
the plan is checked on its own -- the DEVICE's stored input activation (and residual operand) goes through the oracle's single layer
(oracle.graph_ref.conv_bn / _qdense with StorageRounding: net.py:60-76, 101-158, 288-352), the DEVICE's stored output gradient dz goes
back through that layer by autograd, and the layer's output, its parameter gradients (kernel, bias, BN gamma / beta, incl. the L2 term
of net.py:1008-1012) and every activation gradient (sum over the tensor's consumers, ReLU-masked, as the device accumulates it) are
compared with what the device stored.  What is left between the two is ONE layer's fp32 summation order and one or two 16-bit
roundings, so the gates sit at a few rounding units on every seed.

Batch-statistics BN (Config.TRAIN_BN = None) leaves the conv unfolded and stores its raw output z and the gradient dz that reaches it
(Engine._plan_conv_forward: conv -> bn_stats -> bn_apply; bn_bwd on the way back).  Such a layer is checked in two halves that meet at
those stored tensors: the conv from the device's input to z and from the device's dz back, and the normalisation (float64: statistics,
moving statistics, output, dz, gamma / beta gradients) from the device's z and the device's output gradient.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from layerref import DeviceTensors, _l2_rel, _max_rel, _pad_for, forward_layer_errors      # noqa: F401  (re-exported)
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu


BN_MOMENTUM = 0.99           # Keras BatchNormalization default (net.py:60-76 passes none)


def _bn_layer_errors(eng, dev, c, P, w0, w1, grads_dev, z4c, xt, rnd, wd, out, skipped, add_contrib):
    """The checks of one batch-statistics layer (module docstring).  z4c: the oracle's conv + bias of the device's input (autograd graph
    to xt and the layer's kernel / bias).  Every other operand is the device's own stored tensor."""
    import exactprobe as X
    from oracle import graph_ref as G
    n, B, N = c.node, eng.B, c.N
    M = c.Mpix
    nchw = lambda flat: flat.float().cpu().view(B, n.dst.h, n.dst.w, N).permute(0, 3, 1, 2).contiguous()
    z_dev, dz_dev = nchw(c.z), nchw(c.dz)
    Pc = P[n.name]
    # ---- z: the raw conv output, rounded once
    zo = rnd(z4c.detach())
    out["z"][n.name] = (_max_rel(zo, z_dev), _l2_rel(zo, z_dev))
    # ---- stats: batch mean / biased variance of the device's z, and the moving statistics the step left (include/ursonet_hip.h:
    #      mvar' = mvar mom + var M / (M - (1 + eps)) (1 - mom)); reference and bound are exactprobe.bn_stats64's, as for the kernel alone
    st = X.bn_stats64(c.z.float().cpu().view(M, N), torch.tensor(w0[n.bn]["moving_mean"]), torch.tensor(w0[n.bn]["moving_variance"]),
                      BN_MOMENTUM, G.BN_EPS)
    for key, got in (("mean", c.bmean.cpu()), ("var", c.bvar.cpu()), ("mmean", torch.tensor(w1[n.bn]["moving_mean"])),
                     ("mvar", torch.tensor(w1[n.bn]["moving_variance"]))):
        ref, bound = st[key]
        err = (got.double() - ref).abs()
        ratio = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
        out["stats"][n.bn + "/" + key] = (ratio, float(err.max() / (ref.abs().max() + 1e-30)))
    # ---- fwd: float64 batch-statistics BN of the DEVICE's z (+ residual, ReLU), one rounding
    res = None
    if c.res is not None:
        rv = dev.values(c.res)
        if rv is None:
            skipped["fwd"].append(n.name); return
        res = rv[0]
    Pb = {k: torch.tensor(np.asarray(w0[n.bn][k]), dtype=torch.float64) for k in ("gamma", "beta", "moving_mean", "moving_variance")}
    Pb["gamma"].requires_grad_(True); Pb["beta"].requires_grad_(True)
    zt = z_dev.double().requires_grad_(True)
    y4 = G.batchnorm(zt, Pb, None)
    if res is not None:
        y4 = y4 + res.double()
    y = rnd((torch.relu(y4) if n.relu else y4).detach().float())
    dv = dev.values(c.dst)
    if dv is None:
        skipped["fwd"].append(n.name)
    else:
        out["fwd"][n.name] = (_max_rel(y, dv[0], dv[1]), _l2_rel(y, dv[0], dv[1]))
    # ---- dz, gamma / beta gradients: the device's output gradient back through the float64 BN
    gy = dev.grad(c.dst)
    if gy is None:
        skipped["bwd"].append(n.name)
        if not n.stem:
            add_contrib(c.src, None, False)
        if c.res is not None:
            add_contrib(c.res, None, False)
        return
    if c.res is not None:
        add_contrib(c.res, gy, True)
    gz, ggam, gbet = torch.autograd.grad((y4 * gy.double()).sum(), [zt, Pb["gamma"], Pb["beta"]])
    dzo = rnd(gz.float())
    out["dz"][n.name] = (_max_rel(dz_dev, dzo), _l2_rel(dz_dev, dzo))
    out["dz_absmax"][n.name] = float(dz_dev.abs().max())       # (a gradient that is zero on both sides compares equal: the tests assert it is not)
    for wn, g in (("gamma", ggam), ("beta", gbet)):
        gd = torch.tensor(grads_dev[n.bn][wn])
        out["dvec"][n.bn + "/" + wn] = (_max_rel(gd, g), _l2_rel(gd, g))
    # ---- the conv's backward half from the device's dz: input gradient, kernel gradient (+ L2 term)
    obj = (z4c * dz_dev).sum() + wd * (Pc["kernel"] * Pc["kernel"]).sum() / Pc["kernel"].numel()
    gx, gk = torch.autograd.grad(obj, [xt, Pc["kernel"]])
    if not n.stem:
        add_contrib(c.src, gx, True)
    gd = torch.tensor(grads_dev[n.name]["kernel"])
    out["dkernel"][n.name + "/kernel"] = (_max_rel(gd, gk), _l2_rel(gd, gk))
    if "bias" in Pc:
        # the exact gradient of a bias in front of a batch-statistics BN is sum(dz) = 0: what both sides hold is the sum of the 16-bit
        # rounding errors of the device's dz (+ the L2 term 2 wd b / numel), so the comparison is ABSOLUTE: float64 sum of the device's
        # dz against an fp32 sum of M terms in any order (exactprobe.ACC_FACTOR sqrt(M) 2^-24 sum|dz|), + one fp32 rounding of the result
        d64 = dz_dev.double()
        b64 = Pc["bias"].detach().double()
        ref = d64.sum(dim=(0, 2, 3)) + 2.0 * wd * b64 / b64.numel()
        bound = X.ACC_FACTOR * math.sqrt(M) * 2.0 ** -24 * d64.abs().sum(dim=(0, 2, 3)) + 2.0 ** -23 * ref.abs()
        err = (torch.tensor(grads_dev[n.name]["bias"]).double() - ref).abs()
        out["dbias"][n.name + "/bias"] = (float((err / bound.clamp_min(1e-300)).max()), float(err.max()))


def layerwise_errors(eng, w0, img, cfg, dtype, only=None):
    """One pass over the plan of an engine that has just run ONE training step from weights w0 on the loaded batch.
    Returns {check name: {layer or tensor: (max-norm error, Euclidean error)}} and the lists of what could not be read.
    ('stats' and 'dbias' hold (largest |error| / bound, largest |error|) instead: their gates are elementwise bounds.)
    only: a regular expression; layers whose name it does not match (re.search) are left out, and so is every activation gradient
    one of them contributes to.
    The forward half -- the oracle's single layer on the device's operands and the 'fwd' entries -- is layerref.forward_layer_errors,
    the walk the inference plan is checked with as well (tests/test_inference_layerwise_gpu.py); what is added here, layer by layer
    through its hook, is the backward half (and the normalisation half of a batch-statistics layer, which reads the layer's stored z)."""
    from oracle import graph_ref as G
    rnd = lambda t: t.to(dtype).float()
    dev = DeviceTensors(eng)
    grads_dev = eng.get_grads()
    wd = float(cfg.WEIGHT_DECAY)
    out = {"fwd": {}, "dkernel": {}, "dvec": {}, "dx": {}, "z": {}, "dz": {}, "stats": {}, "dbias": {}, "dz_absmax": {}}
    skipped = {"fwd": [], "bwd": [], "dx": []}
    any_bn = any(c.batch_bn for c in eng.convs.values())
    w1 = eng.get_weights() if any_bn else None
    contrib, complete = {}, {}           # activation id -> summed consumer contributions / whether every consumer's dz could be read
    acts_by_id = {X.spec.id: X for X in eng.acts.values()}

    def add_contrib(X, t, ok):
        i = X.spec.id
        if t is not None:
            contrib[i] = t if i not in contrib else contrib[i] + t
        complete[i] = complete.get(i, True) and ok

    def no_gradient_through(c):
        if not c.node.stem:
            add_contrib(c.src, None, False)
        if c.res is not None:
            add_contrib(c.res, None, False)

    def backward_half(event, L):
        c = L.c
        n = c.node
        if event == "unselected":
            no_gradient_through(c)
            return
        if event == "batch_bn":
            _bn_layer_errors(eng, dev, c, L.P, w0, w1, grads_dev, L.z4c, L.xt, rnd, wd, out, skipped, add_contrib)
            return
        Pc, Pb, xt, z4 = L.Pc, L.Pb, L.xt, L.z4
        # ---- backward: the device's dz through the layer
        if L.stored == "pooled":
            pool = dev.pool_of_stem[c.dst.spec.id]
            dzp = dev.grad(acts_by_id[pool.dst.id])
            if dzp is None:
                skipped["bwd"].append(n.name); return
            yr = torch.relu(z4)
            yy = yr + (rnd(yr.detach()) - yr.detach())           # the pool picks its arg-max among the STORED (rounded) values; the gradient is the ReLU's
            obj = (G.maxpool_3x3_s2_same(yy) * dzp).sum()
        else:
            dz = dev.grad(c.dst)                                 # (a folded shortcut: its dz is that of the layer that adds it)
            if dz is None:
                skipped["bwd"].append(n.name)
                if L.stored == "folded":
                    add_contrib(c.src, None, False)
                else:
                    no_gradient_through(c)
                return
            obj = (z4 * dz).sum()
            if c.res is not None:
                add_contrib(c.res, dz, True)                      # Add: the residual operand receives dz itself
        leaves = [("kernel", Pc["kernel"])] + ([("bias", Pc["bias"])] if "bias" in Pc else [])
        for _, w in leaves:                                       # net.py:1008-1012: WEIGHT_DECAY * sum(w^2) / numel(w) per non-BN weight
            obj = obj + wd * (w * w).sum() / w.numel()
        bnl = [("gamma", Pb["gamma"]), ("beta", Pb["beta"])] if Pb is not None else []
        gs = torch.autograd.grad(obj, [xt] + [w for _, w in leaves] + [w for _, w in bnl], allow_unused=True)
        if not n.stem:
            add_contrib(c.src, gs[0], True)
        for (wn, _), g in zip(leaves, gs[1:1 + len(leaves)]):
            gd = torch.tensor(grads_dev[n.name][wn])
            (out["dkernel"] if wn == "kernel" else out["dvec"])[n.name + "/" + wn] = (_max_rel(gd, g), _l2_rel(gd, g))
        for (wn, _), g in zip(bnl, gs[1 + len(leaves):]):
            gd = torch.tensor(grads_dev[n.bn][wn])
            out["dvec"][n.bn + "/" + wn] = (_max_rel(gd, g), _l2_rel(gd, g))

    fwd, skipped_fwd = forward_layer_errors(eng, w0, img, cfg, dtype, only=only, hook=backward_half, dev=dev)
    out["fwd"].update(fwd)
    skipped["fwd"][:0] = skipped_fwd
    # ---- activation gradients: sum over the consumers, ReLU mask of the tensor's own stored values, one rounding
    for i, t in contrib.items():
        X = acts_by_id[i]
        gd = dev.grad(X)
        if gd is None or not complete.get(i, False):
            skipped["dx"].append("T%d" % i); continue
        if X.spec.relu:
            xv = dev.values(X)
            if xv is None:
                skipped["dx"].append("T%d" % i); continue
            t = t * (xv[0] > 0)
        if t.dim() != gd.dim():
            t = t.reshape(gd.shape)
        out["dx"]["T%d[%dx%dx%d]" % (i, X.spec.h, X.spec.w, X.spec.c)] = (_max_rel(gd, rnd(t)), _l2_rel(gd, rnd(t)))
    return out, skipped


def _worst(d):
    if not d:
        return ("-", 0.0, 0.0)
    k1 = max(d, key=lambda k: d[k][0])
    k2 = max(d, key=lambda k: d[k][1])
    return (k1, d[k1][0], d[k2][1])


# gates: a few 16-bit rounding units (bf16: 2^-8 = 3.9e-3 of a value, fp16: 2^-11 = 4.9e-4).  An output element is rounded once (the two
# sides can land on neighbouring 16-bit values where their fp32 sums differ: one unit); an activation gradient that two consumers
# accumulate into is rounded twice on the device; parameter gradients are fp32 sums over the pixels of operands that are IDENTICAL on
# both sides, so they agree to fp32 summation order.
# Measured (profiles/r05_parity.txt; cfg2 width, three seeds x two plans, and fp16 ResNet-101): bf16 outputs <= 6.4e-3 of the tensor's max
# (2.5e-4 Euclidean), activation gradients <= 7.0e-3 (3.0e-3), kernels <= 1.0e-3 (9.2e-4), vectors <= 1.1e-3 (9.0e-4); fp16 8.6e-4 (6.6e-5),
# 8.2e-4 (3.2e-4), 1.0e-4, 4.5e-5.  Gates = ~1.5x those.
GATES = {
    "bfloat16": {"fwd": (1.0e-2, 5e-4), "dx": (1.1e-2, 4.5e-3), "dkernel": (1.6e-3, 1.4e-3), "dvec": (2e-3, 1.4e-3)},
    "float16": {"fwd": (1.3e-3, 1e-4), "dx": (1.3e-3, 5e-4), "dkernel": (2e-4, 1e-4), "dvec": (2e-4, 1e-4)},
}


def _run(dtype_name, kw, seed, opts, train_bn=False, only=None, before_step=None):
    import ursonet_amd.hip as hip
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype_name, **kw)
    cfg.TRAIN_BN = train_bn
    img, loc, ori, _ = synthetic_batch(cfg, cfg.BATCH_SIZE, seed=seed)
    with hip.options(**opts):
        eng = Engine(cfg, "training", seed=3, randomize_bn=True)
        if before_step is not None:
            before_step(eng)
        w0 = eng.get_weights()
        eng.load_batch(img, loc, ori)
        eng.step()
        torch.cuda.synchronize()
    tdt = torch.bfloat16 if dtype_name == "bfloat16" else torch.float16
    return layerwise_errors(eng, w0, img, cfg, tdt, only=only), eng


def _report(tag, errs, skipped):
    lines = ["%s: %d outputs, %d kernels, %d vectors, %d activation gradients checked; not stored on the device: fwd %s bwd %s dx %s"
             % (tag, len(errs["fwd"]), len(errs["dkernel"]), len(errs["dvec"]), len(errs["dx"]), skipped["fwd"], skipped["bwd"], skipped["dx"])]
    for k in ("fwd", "dx", "dkernel", "dvec") + (("z", "dz") if errs.get("z") else ()):
        w = _worst(errs[k])
        lines.append("  %-8s worst max-norm %.3e (%s)   worst Euclidean %.3e" % (k, w[1], w[0], w[2]))
    for k, second in (("stats", "relative to the vector's max"), ("dbias", "absolute")):
        if errs.get(k):
            w = _worst(errs[k])
            lines.append("  %-8s worst |error| / bound %.3f (%s)   worst |error| %.3e (%s), %d checked" % (k, w[1], w[0], w[2], second, len(errs[k])))
    txt = "\n".join(lines)
    print(txt)
    d = os.environ.get("URSO_PARITY_LOG")
    if d:
        with open(d, "a") as f:
            f.write(txt + "\n")


# batch-statistics layers: the raw conv output z and the gradient dz that bn_bwd stores are rounded once like any layer output / activation
# gradient (GATES fwd / dx); statistics and the conv bias gradient are held to elementwise bounds (|error| / bound <= 1: exactprobe.bn_stats64,
# the bounds tests/test_step_tail_exact_gpu.py::test_batch_stat_bn_elementwise uses for the same kernels; the fp32 M-term sum bound for the bias)
# The statistics bound has NO headroom by construction: it is half an fp32 ulp of the float64 result + the float64 summation term, i.e. it
# holds because urso_bn_batch_stats sums in float64 and rounds once (measured |error| / bound up to 1.000: elements that round to the
# neighbouring fp32 value's tie).  A bn_stats that accumulates in fp32 fails here, as it fails test_batch_stat_bn_elementwise.
SAME_GATE = {"z": "fwd", "dz": "dx"}


def _check(dtype_name, errs, own_gates=None):
    bad = []
    for k in ("stats", "dbias"):
        for name, (ratio, e) in errs[k].items():
            if not ratio <= 1.0:
                bad.append("%s %s: |error| / bound %.3f (|error| %.3e)" % (k, name, ratio, e))
    gates = dict(GATES[dtype_name])
    for k, like in SAME_GATE.items():
        gates[k] = gates[like]
    for k, (gm0, g20) in gates.items():
        for name, (em, e2) in errs[k].items():
            gm, g2 = (own_gates or {}).get((k, name), (gm0, g20))
            if not (em <= gm and e2 <= g2):
                bad.append("%s %s: max-norm %.3e (gate %.1e) Euclidean %.3e (gate %.1e)" % (k, name, em, gm, e2, g2))
    assert not bad, "teacher-forced layer parity exceeded:\n" + "\n".join(bad)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("plan", ["policy", "apart"])
def test_teacher_forced_layer_parity_bf16_at_cfg2_width(plan, seed):
    """Every conv / dense layer of the cfg2 plan (ResNet-50, bottleneck 32, ori_resolution 16, 512 x 640; batch 2 shortens the tile
    streams only) on three data seeds.  'policy' = the plan the benchmark runs (fused pairs keep some gradients on chip: those tensors
    are listed, not checked); 'apart' = pair 0, where every activation gradient reaches memory and every layer is checked.
    The default suite runs both plans on seed 1 and the benchmark's plan on seed 2 (each case is 25-45 s of host-side oracle time, and the
    suite has to fit a GPU box's time slot); URSO_ALL_SEEDS=1 runs all six (profiles/r05_parity.txt holds them)."""
    if (plan, seed) not in (("policy", 1), ("apart", 1), ("policy", 2)) and os.environ.get("URSO_ALL_SEEDS", "0") != "1":
        pytest.skip("URSO_ALL_SEEDS=1 runs this seed")
    kw = dict(backbone="resnet50", h=512, w=640, batch=2, regress_ori=False, ori_bins=16)
    (errs, skipped), eng = _run("bfloat16", kw, seed, {} if plan == "policy" else {"pair": 0})
    _report("bf16 cfg2-width %s seed %d" % (plan, seed), errs, skipped)
    nconv = len(eng.convs)
    assert len(errs["fwd"]) == nconv - len(eng.shortcut_folded) and not skipped["fwd"]
    if plan == "apart":
        assert len(errs["dkernel"]) == nconv and not skipped["bwd"], skipped
        assert len(errs["dx"]) >= 40, (len(errs["dx"]), skipped["dx"])
    else:
        assert len(errs["dkernel"]) >= nconv - 4, skipped
    _check("bfloat16", errs)


def test_teacher_forced_layer_parity_fp16_resnet101():
    """The fp16 path (cfg5's arithmetic) on cfg4's trunk: ResNet-101 at 128 x 192."""
    kw = dict(backbone="resnet101", h=128, w=192, batch=2, regress_ori=False, ori_bins=8)
    (errs, skipped), eng = _run("float16", kw, 1, {})
    _report("fp16 r101 128x192", errs, skipped)
    assert len(errs["fwd"]) == len(eng.convs) - len(eng.shortcut_folded)
    _check("float16", errs)


@pytest.mark.parametrize("case", ["cfg4_r101_n24_512x640_bf16", "cfg5_r50_f16_classify_loc_640x960"])
def test_teacher_forced_layer_parity_at_cfg4_cfg5_geometry(case):
    """Every conv / dense layer of BASELINE.json configs[3] and configs[4] at their real image sizes (batch 2): ResNet-101's 105 convs on
    512 x 640 in bf16 with the 13,824-bin head, ResNet-50 in fp16 on 640 x 960 with both heads classifying over 4,096 bins -- each layer fed
    the DEVICE's stored input / output gradient and compared with the oracle's single layer, no compounding (VERDICT r05 missing 4)."""
    if case.startswith("cfg4"):
        dtype_name, kw = "bfloat16", dict(backbone="resnet101", h=512, w=640, batch=2, regress_ori=False, ori_bins=24)
    else:
        dtype_name, kw = "float16", dict(backbone="resnet50", h=640, w=960, batch=2, regress_ori=False, regress_loc=False, ori_bins=16,
                                         loc_bins=16, f16=True)
    (errs, skipped), eng = _run(dtype_name, kw, 1, {})
    _report("%s batch 2" % case, errs, skipped)
    nconv = len(eng.convs)
    assert len(errs["fwd"]) == nconv - len(eng.shortcut_folded) and not skipped["fwd"]
    assert len(errs["dkernel"]) >= nconv - 4, skipped
    # conv1's filter gradient is a sum over 2 x 320 x 480 x 64 pooled-gradient values routed through max-pool arg-max choices: on 614,400-pixel
    # fp16 maps a handful of windows hold two EQUAL maxima, where the device (integer keys, value over tap priority) and torch's max-pool may
    # route the gradient to different taps -- both are subgradients.  Measured here: max-norm 3.0e-4, Euclidean 7.8e-5 (round 6, first run).
    _check(dtype_name, errs, {("dkernel", "conv1/kernel"): (5e-4, 1e-4)} if dtype_name == "float16" else None)



# ---------------------------------------------------------------- batch-statistics BN (Config.TRAIN_BN = None)
def _assert_every_bn_layer_checked(eng, errs, skipped):
    assert eng.train_bn
    assert not eng.shortcut_folded                                 # the fusions are off in this mode: every layer output is a stored tensor
    assert not skipped["fwd"] and not skipped["bwd"], skipped
    bn = [c for c in eng.convs.values() if c.batch_bn]
    assert bn and len(bn) == sum(1 for c in eng.convs.values() if c.node.bn)
    names = {c.name for c in bn}
    for k in ("z", "fwd", "dz"):
        assert names <= set(errs[k]), (k, sorted(names - set(errs[k])))
    dead = sorted(nm for nm, v in errs["dz_absmax"].items() if not v > 0)
    assert not dead, "no gradient reached %s: the comparison of its backward half is 0 against 0" % dead
    assert set(errs["fwd"]) == {c.name for c in eng.convs.values()}
    assert {c.name + "/kernel" for c in eng.convs.values()} == set(errs["dkernel"])
    assert {c.node.bn + "/" + k for c in bn for k in ("mean", "var", "mmean", "mvar")} == set(errs["stats"])
    assert {c.node.bn + "/" + k for c in bn for k in ("gamma", "beta")} <= set(errs["dvec"])
    assert {c.name + "/bias" for c in bn if c.node.bias} == set(errs["dbias"])
    # ... and the gradient of every tensor a batch-statistics layer reads (its input, its residual operand)
    reads = {c.src.spec.id for c in bn if not c.node.stem} | {c.res.spec.id for c in bn if c.res is not None}
    assert reads <= {int(k[1:k.index("[")]) for k in errs["dx"]}, skipped["dx"]


BN_CASES = {
    "r50_64x128_b4_bf16": ("bfloat16", dict(backbone="resnet50", h=64, w=128, batch=4, regress_ori=False, ori_bins=4)),
    "r50_64x128_b4_fp16": ("float16", dict(backbone="resnet50", h=64, w=128, batch=4, regress_ori=False, ori_bins=4)),
    "r18_128x128_b3_bf16": ("bfloat16", dict(backbone="resnet18", h=128, w=128, batch=3, regress_ori=True)),
}


@pytest.mark.parametrize("case", list(BN_CASES))
def test_teacher_forced_layer_parity_batch_statistics_bn(case):
    """TRAIN_BN = None in the 16-bit types: every conv of the plan after ONE step, each batch-statistics layer in both of its halves
    (module docstring) -- z, statistics and moving statistics, normalised output, dz, gamma / beta, kernel and (absolutely) conv bias
    gradients, and every activation gradient.  Stage 5 is 2 x 4 (4 x 4) pixels x batch: statistics over 32 (48) values."""
    dtype_name, kw = BN_CASES[case]
    (errs, skipped), eng = _run(dtype_name, kw, 1, {}, train_bn=None)
    _report("batch-statistics BN %s" % case, errs, skipped)
    _assert_every_bn_layer_checked(eng, errs, skipped)
    _check(dtype_name, errs)


def test_batch_statistics_bn_layers_get_the_halo_workspace():
    """A 3x3 layer the halo-tile kernel takes must be launched with that kernel's dedicated (zeroed) hand-over workspace, in
    batch-statistics mode as in frozen mode -- never with the split-K workspace, which holds other layers' fp32 partials where the
    stream-K schedule expects zero flags (conv_halo.hip).  ResNet-50 at 512 x 640, batch 6, bf16: res5*_branch2b (512 -> 512 on 16 x 20
    pixels, M = 1920) has a split-K size of 9 x 1920 x 512 x 4 = 35.4 MB (urso_conv_igemm_ws_bytes does not exclude halo layers), the
    hand-over workspace is 4096 + 256 x 128 KiB = 33.6 MB, and the layer's 36 halo tiles are fewer than the CUs, so stream-K engages.
    The premise is asserted, the plan property is asserted before stepping, and stage 5 is then checked layer by layer after one step."""
    import ursonet_amd.hip as hip
    kw = dict(backbone="resnet50", h=512, w=640, batch=6, regress_ori=False, ori_bins=16)

    def plan_property(eng):
        dt = eng.dt
        halo_bytes = hip.conv_igemm_halo_ws_bytes()
        assert eng.igemm_ws.numel() * 4 >= halo_bytes, "premise: the split-K workspace is no longer large enough to pass for the hand-over one"
        risky = [c.name for c in eng.convs.values() if c.batch_bn and hip.conv_igemm_halo_ok(c.gf, dt, 0, False) and c.ws_f > 0]
        assert any(re.match("res5", nm) for nm in risky), "premise: no stage-5 halo layer with a split-K size (%s)" % risky
        for c in eng.convs.values():
            flags = 0 if c.batch_bn else c.fwd_flags | (hip.EPI_EMIT_BITS if c.dst.bits is not None else 0)
            if hip.conv_igemm_halo_ok(c.gf, dt, flags, (not c.batch_bn) and c.res is not None):
                assert c.halo_f and eng.forward_workspace(c) is eng.halo_ws, c.name
            else:
                assert eng.forward_workspace(c) is not eng.halo_ws, c.name
        assert int(eng.halo_ws[:1024].view(torch.int32).abs().max()) == 0

    (errs, skipped), eng = _run("bfloat16", kw, 1, {}, train_bn=None, only="^res5", before_step=plan_property)
    _report("batch-statistics BN r50 512x640 b6 bf16, stage 5", errs, skipped)
    assert eng.train_bn and int(eng.halo_ws[:1024].view(torch.int32).abs().max()) == 0, "hand-over flags not left zero"
    stage5 = {c.name for c in eng.convs.values() if c.name.startswith("res5")}
    assert len(stage5) == 10 and all(stage5 == set(errs[k]) for k in ("z", "fwd", "dz")) and not skipped["fwd"] and not skipped["bwd"]
    assert all(v > 0 for v in errs["dz_absmax"].values()), "no gradient reached stage 5: %s" % errs["dz_absmax"]
    _check("bfloat16", errs)
