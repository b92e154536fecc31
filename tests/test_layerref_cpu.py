"""What the teacher-forced forward checker (tests/layerref.py) can and cannot see, shown without a GPU.

OracleEngine is a host stand-in of an engine after forward(): it walks ursonet_amd.graph with oracle.graph_ref under StorageRounding and
keeps every activation the way the checker expects to read a device buffer -- flat NHWC in the 16-bit type, channels padded to a
multiple of 8 (the padding holds garbage), fp32 for the head outputs.  Each layer reads the STORED form of its operands, as a device
layer does.  A mutation makes ONE layer compute something else; every later layer goes on from what that layer stored, so a checker
that isolates layers reports the mutated layer and no other.

The graph refuses image sizes that are no multiple of 64 (net.py:596-600), so the smallest config is 64 x 64 (stage 5 is 2 x 2 pixels).
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from layerref import forward_layer_errors
from test_layerwise_gpu import GATES
from util import make_config, synthetic_batch

GARBAGE = 7.0           # what lies where the stand-in's "device" never writes: channel padding, pixels off the sampled grid


class _Act(object):
    def __init__(self, spec):
        self.spec, self.data, self.data_compact = spec, None, None
        self.fused_pool = self.fwd_sampled = self.fwd_scattered = False


class _Conv(object):
    batch_bn = False

    def __init__(self, node, acts):
        self.node, self.name, self.N, self.npad = node, node.name, node.cout, -(-node.cout // 8) * 8
        self.src = acts[node.src.id]
        self.dst = acts[node.dst.id]
        self.res = acts[node.residual.id] if node.residual is not None else None


MUTATIONS = ("scale", "shift", "swap", "no_residual", "no_relu")


class OracleEngine(object):
    """convs / acts / graph / B / shortcut_folded of an engine whose forward pass is the rounding oracle's.
    mutate = (layer, one of MUTATIONS); sampled = name of a block-closing layer whose output is kept at the even pixels only
    (Engine._sample_block_output: fwd_sampled + data_compact), the 3x3 layer below it scattered to the even pixels of its dense buffer."""

    def __init__(self, cfg, weights, img, dtype, mutate=None, sampled=None):
        from oracle import graph_ref as G
        from ursonet_amd.graph import build_graph
        self.graph, self.B, self.shortcut_folded = build_graph(cfg), int(img.shape[0]), []
        self.acts = {t.id: _Act(t) for t in self.graph.tensors}
        self.convs = OrderedDict((n.name, _Conv(n, self.acts)) for n in self.graph.nodes if n.op != "pool")
        q = G.StorageRounding(dtype)
        P = G.to_torch(weights, requires_grad=False)
        B = self.B
        npad = {c.dst.spec.id: c.npad for c in self.convs.values()}
        for n in self.graph.nodes:
            if n.op == "pool":
                npad[n.dst.id] = n.dst.c

        def store(X, y, elt):
            """NCHW fp32 -> the flat NHWC buffer with padded channels."""
            buf = torch.full((B, y.shape[2], y.shape[3], npad[X.spec.id]), GARBAGE, dtype=elt)
            buf[..., :X.spec.c] = y.permute(0, 2, 3, 1).to(elt)
            return buf.reshape(-1)

        def load(X):
            s = X.spec
            return X.data.float().view(B, s.h, s.w, npad[s.id])[..., :s.c].permute(0, 3, 1, 2).contiguous()

        mut_layer, mut = mutate if mutate is not None else (None, None)
        assert mut in MUTATIONS + (None,)
        scattered = self.convs[sampled].src if sampled is not None else None
        with torch.no_grad():
            for n in self.graph.nodes:
                if n.op == "pool":
                    X = self.acts[n.dst.id]
                    X.data = store(X, G.maxpool_3x3_s2_same(load(self.acts[n.src.id])), dtype)
                    continue
                c = self.convs[n.name]
                m = mut if n.name == mut_layer else None
                x = torch.as_tensor(img, dtype=torch.float32).to(dtype).float().permute(0, 3, 1, 2).contiguous() if n.stem else load(c.src)
                if n.dense:
                    z = G._qdense(x.permute(0, 2, 3, 1).reshape(B, -1), P[n.name], q).view(B, -1, 1, 1)
                else:      # paddings as oracle.graph_ref states them, not as the checker derives them from the node: ZeroPadding2D(3) of the
                    #        stem, TF-SAME of the stride-2 bottleneck_layer, one pixel around every other 3x3 layer
                    pad = 3 if n.stem else ("same" if n.name == "bottleneck_layer" else (1 if n.kh == 3 else "valid"))
                    z = G.conv_bn(x, P[n.name], P[n.bn] if n.bn else None, False, stride=n.stride, padding=pad, q=q)
                if c.res is not None and m != "no_residual":
                    z = z + load(c.res)
                y = torch.relu(z) if (n.relu and m != "no_relu") else z
                if m == "scale":
                    y = y * 1.02
                elif m == "shift":
                    y = torch.roll(y, 1, dims=3)
                elif m == "swap":
                    y = torch.cat([y[:, 1:2], y[:, 0:1], y[:, 2:]], dim=1)
                elt = torch.float32 if n.out_f32 else dtype
                c.dst.data = store(c.dst, y, elt)
                if n.name == sampled or c.dst is scattered:
                    # the buffers hold the even pixels only; c.dst.data stays dense until the walk is over (the stand-in's own later layers
                    # read it, and what they read at the even pixels is what the buffers hold)
                    dense = c.dst.data
                    even = dense.view(B, n.dst.h, n.dst.w, -1)[:, ::2, ::2].clone()
                    if n.name == sampled:
                        c.dst.data_compact, c.dst.fwd_sampled = even.reshape(-1), True
                        c.dst._left = torch.full_like(dense, GARBAGE)
                    else:
                        g = torch.full_like(dense, GARBAGE).view(B, n.dst.h, n.dst.w, -1)
                        g[:, ::2, ::2] = even
                        c.dst._left, c.dst.fwd_scattered = g.reshape(-1), True
        for X in self.acts.values():                             # hand the checker the buffers as the "device" left them
            if hasattr(X, "_left"):
                X.data = X._left


CONFIGS = {
    "resnet18": (dict(backbone="resnet18", h=64, w=64, batch=2, regress_ori=True), "stage2_unit2_conv2"),
    "resnet50": (dict(backbone="resnet50", h=64, w=64, batch=2, regress_ori=False, ori_bins=4), "res3b_branch2c"),
}
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
_cache = {}


def _inputs(backbone):
    """(cfg, weights, molded batch) of a backbone, built once."""
    if backbone not in _cache:
        from oracle import graph_ref as G
        kw, _ = CONFIGS[backbone]
        cfg = make_config(**kw)
        img = synthetic_batch(cfg, cfg.BATCH_SIZE, seed=1)[0]
        _cache[backbone] = (cfg, G.init_params(cfg, seed=3, randomize_bn=True), img)
    return _cache[backbone]


def _beyond(errs, dtype_name):
    gm, g2 = GATES[dtype_name]["fwd"]
    return sorted(k for k, (em, e2) in errs.items() if not (em <= gm and e2 <= g2))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("backbone", list(CONFIGS))
def test_untouched_stand_in_has_zero_error_on_every_layer(backbone, dtype_name):
    cfg, w, img = _inputs(backbone)
    eng = OracleEngine(cfg, w, img, DTYPES[dtype_name])
    errs, skipped = forward_layer_errors(eng, w, img, cfg, DTYPES[dtype_name])
    assert not skipped and set(errs) == set(eng.convs)
    assert all(v == (0.0, 0.0) for v in errs.values()), {k: v for k, v in errs.items() if v != (0.0, 0.0)}
    errs2, _ = forward_layer_errors(eng, w, img, cfg, DTYPES[dtype_name], only="^res3|^stage2")
    assert errs2 and all(k.startswith(("res3", "stage2")) for k in errs2) and all(errs2[k] == errs[k] for k in errs2)


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("backbone", list(CONFIGS))
def test_a_mutated_layer_is_reported_on_that_layer_and_no_other(backbone, dtype_name, mutation):
    cfg, w, img = _inputs(backbone)
    layer = CONFIGS[backbone][1]
    eng = OracleEngine(cfg, w, img, DTYPES[dtype_name], mutate=(layer, mutation))
    assert eng.convs[layer].res is not None and eng.convs[layer].node.relu and eng.convs[layer].node.dst.w > 2
    errs, skipped = forward_layer_errors(eng, w, img, cfg, DTYPES[dtype_name])
    assert not skipped and _beyond(errs, dtype_name) == [layer], (_beyond(errs, dtype_name), errs[layer])
    assert all(v == (0.0, 0.0) for k, v in errs.items() if k != layer)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_wrong_reference_weights_are_reported_on_their_layer_alone(dtype_name):
    """The other direction, as the GPU tests use it: the stand-in is right and the REFERENCE has one layer's gamma scaled by 1.02 or
    its kernel rolled along the input channels."""
    cfg, w, img = _inputs("resnet50")
    layer, bn = "res3a_branch2b", "bn3a_branch2b"
    eng = OracleEngine(cfg, w, img, DTYPES[dtype_name])
    for change in ("gamma", "roll"):
        w2 = OrderedDict((ln, OrderedDict(ws)) for ln, ws in w.items())
        if change == "gamma":
            w2[bn]["gamma"] = w[bn]["gamma"] * np.float32(1.02)
        else:
            w2[layer]["kernel"] = np.roll(w[layer]["kernel"], 1, axis=2)
        errs, _ = forward_layer_errors(eng, w2, img, cfg, DTYPES[dtype_name])
        assert _beyond(errs, dtype_name) == [layer], (change, _beyond(errs, dtype_name), errs[layer])


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_sampled_block_output_is_read_through_the_even_pixel_mask(dtype_name):
    """fwd_sampled / data_compact on res2c's output (its dense buffer is garbage) and fwd_scattered on the 3x3 layer below it (garbage off
    the even pixels): every layer still compares equal, and a mutation of the sampled layer is still seen."""
    cfg, w, img = _inputs("resnet50")
    dt = DTYPES[dtype_name]
    eng = OracleEngine(cfg, w, img, dt, sampled="res2c_branch2c")
    X, Y = eng.convs["res2c_branch2c"].dst, eng.convs["res2c_branch2b"].dst
    assert X.fwd_sampled and X.data_compact.numel() * 4 == X.data.numel() and bool((X.data.float() == GARBAGE).all())
    assert Y.fwd_scattered and float((Y.data.float() == GARBAGE).float().mean()) >= 0.75
    errs, skipped = forward_layer_errors(eng, w, img, cfg, dt)
    assert not skipped and set(errs) == set(eng.convs)
    assert all(v == (0.0, 0.0) for v in errs.values()), {k: v for k, v in errs.items() if v != (0.0, 0.0)}
    eng = OracleEngine(cfg, w, img, dt, sampled="res2c_branch2c", mutate=("res2c_branch2c", "scale"))
    errs, _ = forward_layer_errors(eng, w, img, cfg, dt)
    assert _beyond(errs, dtype_name) == ["res2c_branch2c"]
