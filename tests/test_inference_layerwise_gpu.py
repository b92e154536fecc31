"""Teacher-forced per-layer parity of the INFERENCE plan in the 16-bit types, with the library's default options: the plan that detect,
evaluate, predict, track, calibrate, conformal, fit_domain and explain replay (ursonet_amd/infer.py).

The inference plan is not the training forward pass: Engine._build_plan returns early for it, every activation goes through
_sample_block_output, no ReLU bit mask is emitted, the parameter table is uploaded at plan time, the weight preparation sits inside the
captured graph, frames may arrive as uint8, and it runs at batch sizes training never uses.  After forward() every conv / dense layer is
checked on its own (tests/layerref.py): the DEVICE's stored input and residual operand through the oracle's single layer against the
DEVICE's stored output, at the forward gates of tests/test_layerwise_gpu.py -- unchanged: one 16-bit rounding on both sides, so two
results differ by one unit (2^-8 bf16, 2^-11 fp16) where their fp32 sums fall on two sides of a rounding boundary; the max-norm gate is
about 2.5 units.

Image sizes: the graph takes multiples of 64 only (net.py:596-600: ursonet_amd.graph.build_graph raises otherwise), so no stage-4 / stage-5
map of this network is ever odd and _sample_block_output never meets `h % 2`.  The odd case is therefore 192 x 320 at batch 3: the
bottleneck features are 3 x 5, stage 5 is 6 x 10 (60 x 3 = 180 pixel rows: ragged 128-row tiles), the batch is odd.
"""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from layerref import DeviceTensors, forward_layer_errors
from test_layerwise_gpu import GATES, _check, _report
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

TORCH_DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}

CASES = OrderedDict([
    # the benchmark's trunk and head kind
    ("r50_bf16_soft", ("bfloat16", dict(backbone="resnet50", h=128, w=192, batch=2, regress_ori=False, ori_bins=8))),
    # cfg5's arithmetic, padded fp32 classification heads
    ("r50_fp16_classify_both", ("float16", dict(backbone="resnet50", h=128, w=192, batch=2, regress_loc=False, regress_ori=False, loc_bins=4,
                                                ori_bins=4, f16=True))),
    # batch 1 as detect runs it; the long stage 4
    ("r101_fp16", ("float16", dict(backbone="resnet101", h=64, w=128, batch=1))),
    # odd bottleneck map, ragged pixel tiles, odd batch (module docstring)
    ("r50_bf16_odd", ("bfloat16", dict(backbone="resnet50", h=192, w=320, batch=3))),
    # basic blocks, regressed quaternion head
    ("r18_bf16_quat", ("bfloat16", dict(backbone="resnet18", h=128, w=128, batch=3, regress_ori=True))),
    # three regression heads, no orientation head
    ("r18_fp16_keypoints", ("float16", dict(backbone="resnet18", h=64, w=128, batch=2, regress_ori=True, keypoints=True))),
])
# the benchmark's geometry (the kw of test_teacher_forced_layer_parity_bf16_at_cfg2_width)
BENCH = ("bfloat16", dict(backbone="resnet50", h=512, w=640, batch=2, regress_ori=False, ori_bins=16))


def _log(txt):
    print(txt)
    d = os.environ.get("URSO_PARITY_LOG")
    if d:
        with open(d, "a") as f:
            f.write(txt + "\n")


# ---------------------------------------------------------------- the forward kernel kinds of a plan
def _layer_class(c):
    n = c.node
    if n.stem:
        return "stem"
    if n.dense:
        return "dense" + ("/f32" if n.out_f32 else "")
    return "%dx%ds%d%s%s" % (n.kh, n.kw, n.stride, "+add" if c.res is not None else "", "" if n.relu else "/linear")


def layer_kinds(eng):
    """{layer: kind}.  A kind is what the plan knows of the launch that computes the layer: the launch record's kind (fwd | fwd+sampled |
    fwd@sampled | fwd+maxpool), the classes of the layers it computes (one for a launch of its own, several for a fused one), whether it
    reads the compact form of its input, and -- for a launch of urso_conv_igemm_ex on the layer's own geometry -- whether the library
    sends it to the halo-tile kernel (and that kernel's tile shape) or splits K."""
    import ursonet_amd.hip as hip
    out = OrderedDict()
    for c in eng.convs.values():
        k = "%s[%s]" % (c.fwd.kind, "+".join(_layer_class(eng.convs[nm]) for nm in c.fwd.fwd))
        if c.xin is not c.src.data and not c.node.stem:
            k += "/compact-in"
        if c.fwd.kind == "fwd" and len(c.fwd.fwd) == 1 and not c.node.dense:
            if c.halo_f:
                k += "/halo%d" % hip.conv_igemm_halo2_shape(c.gf, eng.dt, c.fwd_flags, c.res is not None, True)
            elif c.ws_f:
                k += "/split-K"
        out[c.name] = k
    return out


def forward_kinds(eng):
    """The set of layer kinds + the shapes of the forward labels (layer and tensor names taken out): the launches that compute no layer
    (mold, maxpool, subsample, quat) and the suffixes (@sampled, +sampled, +maxpool) are in it through them."""
    names = sorted(eng.convs, key=len, reverse=True)
    shape = lambda l: re.sub(r"T\d+", "T", re.sub("|".join(re.escape(nm) for nm in names), "L", l))
    return set(layer_kinds(eng).values()) | {"label " + shape(l) for l in eng.labels["fwd"] if l}


def n_sampled(eng):
    return sum(1 for l in eng.labels["fwd"] if l and l.endswith("@sampled"))


# ---------------------------------------------------------------- one case: build, forward, check
class _Run(object):
    pass


_runs = {}


def _molded_and_u8(cfg, seed=1):
    """The synthetic batch as uint8 frames and as the float32 frames host molding makes of them."""
    img = synthetic_batch(cfg, cfg.BATCH_SIZE, seed=seed)[0]
    mean = np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)
    u8 = np.rint(img + mean).astype(np.uint8)
    return u8.astype(np.float32) - mean, u8


def _as_checks(errs):
    return {"fwd": errs, "dx": {}, "dkernel": {}, "dvec": {}, "z": {}, "dz": {}, "stats": {}, "dbias": {}}


def _beyond(errs, dtype_name):
    gm, g2 = GATES[dtype_name]["fwd"]
    return sorted(k for k, (em, e2) in errs.items() if not (em <= gm and e2 <= g2))


def _run(case):
    """The case's inference engine after one forward pass, with the checker's result (computed once per session)."""
    if case in _runs:
        return _runs[case]
    from ursonet_amd.engine import Engine
    dtype_name, kw = CASES[case] if case in CASES else BENCH
    r = _Run()
    r.dtype_name, r.tdt = dtype_name, TORCH_DT[dtype_name]
    r.cfg = make_config(dtype=dtype_name, **kw)
    r.img, r.u8 = _molded_and_u8(r.cfg)
    r.eng = Engine(r.cfg, "inference", seed=3, randomize_bn=True)
    r.w = r.eng.get_weights()
    r.kinds, r.n_sampled = forward_kinds(r.eng), n_sampled(r.eng)
    r.eng.load_batch(r.img)
    r.eng.forward()
    torch.cuda.synchronize()
    r.refs = {}
    if case in CASES:
        r.errs, r.skipped = forward_layer_errors(r.eng, r.w, r.img, r.cfg, r.tdt, refs=r.refs)
    _runs[case] = r
    return r


@pytest.mark.parametrize("case", list(CASES))
def test_inference_layers_match_the_oracle_layer(case):
    """Every conv / dense layer of the default inference plan, the head outputs as outputs() returns them, and features()."""
    r = _run(case)
    eng, errs = r.eng, r.errs
    _report("inference %s" % case, _as_checks(errs), {"fwd": r.skipped, "bwd": [], "dx": []})
    km, k2 = max(errs, key=lambda k: errs[k][0]), max(errs, key=lambda k: errs[k][1])
    _log("  worst layer per norm: max-norm %s %.3e, Euclidean %s %.3e; %d layers not read" % (km, errs[km][0], k2, errs[k2][1], len(r.skipped)))
    _log("  kinds reached by %s (%d @sampled): %s" % (case, r.n_sampled, sorted(r.kinds)))
    assert len(errs) == len(eng.convs) - len(eng.shortcut_folded) and not r.skipped, r.skipped
    _check(r.dtype_name, _as_checks(errs))
    # ---- outputs(): the fp32 head tensors against the oracle's head layer on the device's stored head input
    g = eng.graph
    loc, ori = eng.outputs()
    got = {"loc": loc}
    if eng.out_ori is None:
        got["k2"], got["k3"] = ori
    elif not eng.quat_head:
        got["ori"] = ori
    producer = {c.dst.spec.id: c.name for c in eng.convs.values()}
    for key, t in got.items():
        ref = r.refs[producer[g.outputs[key].id]].reshape(eng.B, -1).double()
        d = (t.cpu().double() - ref).abs()
        bound = 1e-5 * float(ref.abs().max()) + 1e-6
        _log("  %s %s: %d values, largest |error| %.3e (bound %.3e)" % (case, key, d.numel(), float(d.max()), bound))
        assert t.dtype == torch.float32 and t.shape == ref.shape and float(d.max()) <= bound, (key, float(d.max()), bound)
    if eng.quat_head:
        raw = eng.out_ori.data.view(eng.B, -1)[:, :4].cpu().double()
        ref = raw / raw.pow(2).sum(-1, keepdim=True).clamp_min(1e-12).sqrt()
        d = (ori.cpu().double() - ref).abs()
        _log("  %s quaternion: largest |error| %.3e (bound %.3e)" % (case, float(d.max()), 2.0 ** -23 * float(ref.abs().max())))
        assert float(d.max()) <= 2.0 ** -23 * float(ref.abs().max())
        ref_raw = r.refs[producer[g.outputs["ori"].id]].reshape(eng.B, -1).double()
        assert float((raw - ref_raw).abs().max()) <= 1e-5 * float(ref_raw.abs().max()) + 1e-6
    # ---- features(): the bits the layer check read as bottleneck_layer's stored output
    f = eng.features()
    stored = DeviceTensors(eng).values(eng.acts[g.feat.id])[0]
    assert f.dtype == r.tdt and tuple(f.shape) == (eng.B, g.feat.h, g.feat.w, g.feat.c)
    assert torch.equal(f.float().cpu().permute(0, 3, 1, 2), stored) and float(stored.abs().max()) > 0


def test_small_cases_reach_every_forward_kind_of_the_benchmark_plan():
    """Premise of the cases: between them they run every forward kind of the inference plan at the benchmark's geometry (K).  A kind
    small images cannot reach (the library splits K on small grids where it takes the halo-tile or a register-filter kernel at full
    size) is checked at 512 x 640 itself: the device runs the whole pass, the oracle only one layer of each missing kind."""
    from ursonet_amd.engine import Engine
    dtype_name, kw = BENCH
    big = Engine(make_config(dtype=dtype_name, **kw), "inference", seed=3, randomize_bn=True)      # built, not run
    K = forward_kinds(big)
    reached = set()
    for case in CASES:
        reached |= _run(case).kinds
    missing = K - reached
    _log("forward kinds K of the benchmark plan (ResNet-50, 512 x 640, batch 2, bf16): %s" % sorted(K))
    _log("forward kinds reached by the small cases: %s" % sorted(reached))
    _log("kinds of K the small cases do not reach: %s" % sorted(missing))
    del big
    if missing:
        r = _run("bench")
        lk = layer_kinds(r.eng)
        names = sorted(r.eng.convs, key=len, reverse=True)
        shape = lambda l: "label " + re.sub(r"T\d+", "T", re.sub("|".join(re.escape(nm) for nm in names), "L", l))
        first = OrderedDict()                                    # one layer per missing layer kind: the first in graph order ...
        for nm, k in lk.items():
            if k in missing:
                first.setdefault(k, nm)
        chosen = list(first.values())
        for op in r.eng.fwd_ops:                                 # ... and every layer of the first launch of a missing label shape
            if op.label and shape(op.label) in missing and shape(op.label) not in first:
                first[shape(op.label)] = op.label
                chosen += [nm for nm in op.fwd if nm not in chosen]
        only = "^(%s)$" % "|".join(re.escape(nm) for nm in chosen)
        errs, skipped = forward_layer_errors(r.eng, r.w, r.img, r.cfg, r.tdt, only=only)
        _report("inference 512x640 batch 2 bf16, only=%s" % only, _as_checks(errs), {"fwd": skipped, "bwd": [], "dx": []})
        folded = set(r.eng.shortcut_folded)
        assert not skipped and {nm for nm in chosen if nm not in folded} <= {k.split("+maxpool")[0] for k in errs}
        _check(dtype_name, _as_checks(errs))
        reached |= set(first)
        _log("forward kinds reached with the 512 x 640 case: %s" % sorted(reached))
    assert K <= reached, sorted(K - reached)
    assert any(k.startswith("fwd@sampled") for k in K)
    # ---- the sampled block outputs are reached, and so is the plan in which _sample_block_output declines
    ns = {case: _run(case).n_sampled for case in CASES}
    _log("@sampled layers per case: %s" % ns)
    assert max(ns.values()) > 0
    # res{2c,3d,4f}_out and the 3x3 layer below each: every bottleneck case samples all six, the 192 x 320 one included -- a size at
    # which `h % 2` declines does not exist (module docstring), so that case cannot have fewer than r50_bf16_soft
    assert all(ns[c] == 6 for c in CASES if CASES[c][1]["backbone"] != "resnet18"), ns
    # where the producer is not a block-closing pointwise layer (basic blocks) _sample_block_output declines: the stride-2 layers read
    # a compact input that a gather pass fills, and those layers are among the ones checked above
    declined = [c for c in CASES if ns[c] == 0]
    assert declined and all("label subsample:T" in _run(c).kinds and any("/compact-in" in k for k in _run(c).kinds) for c in declined), ns


def _changed_weights(w):
    rng = np.random.default_rng(11)
    w2 = OrderedDict()
    for ln, ws in w.items():
        w2[ln] = OrderedDict()
        for wn, a in ws.items():
            if wn == "kernel":
                w2[ln][wn] = (a * np.float32(rng.uniform(0.9, 1.1))).astype(np.float32)
            elif wn == "moving_variance":
                w2[ln][wn] = (a * np.float32(1.3)).astype(np.float32)
            elif wn == "moving_mean":
                w2[ln][wn] = (a + np.float32(0.1)).astype(np.float32)
            else:
                w2[ln][wn] = a.copy()
    return w2


def test_set_weights_reaches_every_prepared_filter_of_the_captured_graph():
    """Stale preparation: after set_weights() the ALREADY CAPTURED graph must fold and round the new weights -- every layer within the
    gates against the new weights, and the same stored tensors far from the old ones (the device moved and the checker sees it)."""
    r = _run("r50_bf16_soft")
    eng = r.eng
    assert eng._graphs is not None
    graph = eng._graphs
    w2 = _changed_weights(r.w)
    try:
        eng.set_weights(w2)
        eng.forward()
        torch.cuda.synchronize()
        assert eng._graphs is graph, "the graph was captured again"
        errs, skipped = forward_layer_errors(eng, w2, r.img, r.cfg, r.tdt)
        _report("inference r50_bf16_soft after set_weights, against the new weights", _as_checks(errs), {"fwd": skipped, "bwd": [], "dx": []})
        assert len(errs) == len(eng.convs) - len(eng.shortcut_folded) and not skipped
        _check(r.dtype_name, _as_checks(errs))
        old, _ = forward_layer_errors(eng, r.w, r.img, r.cfg, r.tdt)
        bad = _beyond(old, r.dtype_name)
        _log("  against the old weights: %d of %d layers beyond the gate" % (len(bad), len(old)))
        assert len(bad) > len(old) // 2, (len(bad), len(old))
    finally:
        eng.set_weights(r.w)
        eng.forward()
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["r50_bf16_soft", "r50_fp16_classify_both"])
def test_a_wrong_layer_in_the_reference_is_seen_on_that_layer_alone(case):
    """The checker is not blind, in bf16 and at the fp16 gates a 2 % error has to get past: with one mid-network layer of the REFERENCE
    changed (gamma x 1.02; kernel rolled by one input channel) exactly that layer exceeds the gate."""
    r = _run(case)
    layer = next(nm for nm in r.eng.convs if re.match(r"res3.*_branch2b$", nm))
    bn = r.eng.convs[layer].node.bn
    for change in ("gamma", "roll"):
        w2 = OrderedDict((ln, OrderedDict(ws)) for ln, ws in r.w.items())
        if change == "gamma":
            w2[bn]["gamma"] = r.w[bn]["gamma"] * np.float32(1.02)
        else:
            w2[layer]["kernel"] = np.roll(r.w[layer]["kernel"], 1, axis=2)
        errs, _ = forward_layer_errors(r.eng, w2, r.img, r.cfg, r.tdt)
        _log("  %s, reference %s with %s changed: max-norm %.3e Euclidean %.3e; beyond the gate: %s"
             % (case, layer, change, errs[layer][0], errs[layer][1], _beyond(errs, r.dtype_name)))
        assert _beyond(errs, r.dtype_name) == [layer]


def test_uint8_frames_give_the_same_bits_in_every_stored_activation():
    """Two inference engines from the same weights, one fed through load_batch_u8 and one through load_batch with host molding: the
    molded input and EVERY stored activation hold the same bits (the molding kernel's 16-bit rounding inside the plan)."""
    from ursonet_amd.engine import Engine
    r = _run("r50_bf16_soft")
    e8 = Engine(r.cfg, "inference", seed=3, randomize_bn=True)
    e8.set_weights(r.w)
    e8.load_batch_u8(r.u8)
    e8.forward()
    torch.cuda.synchronize()
    a, b = DeviceTensors(r.eng), DeviceTensors(e8)
    x0 = r.eng.graph.tensors[0].id
    assert torch.equal(r.eng.acts[x0].data, e8.acts[x0].data) and float(e8.acts[x0].data.float().abs().max()) > 0
    compared = 0
    for i, X in r.eng.acts.items():
        if i == x0:
            continue
        va, vb = a.values(X), b.values(e8.acts[i])
        assert (va is None) == (vb is None), i
        if va is None:
            continue
        assert torch.equal(va[0], vb[0]), "T%d differs between the uint8 and the float input path" % i
        compared += 1
    assert compared >= len(r.eng.convs) - len(r.eng.shortcut_folded)
    assert all(torch.equal(s, t) for s, t in zip(r.eng.outputs(), e8.outputs()))
