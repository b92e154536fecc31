"""The oracle's single layer on the device's own operands: the forward half of the teacher-forced layer checks.

For every conv / dense layer of an engine's plan the DEVICE's stored input activation (and residual operand) goes through the oracle's
single layer (oracle.graph_ref.conv_bn / _qdense with StorageRounding) and the result is compared with the DEVICE's stored output.
Nothing compounds: what is left between the two is one layer's fp32 summation order and one 16-bit rounding.  Both engine modes keep
every activation in a buffer of its own (plan_state._Act), so the same walk serves a training engine that has just stepped
(tests/test_layerwise_gpu.py, which adds the backward half through `hook`) and an inference engine after forward()
(tests/test_inference_layerwise_gpu.py).  Nothing here reads a gradient, a ReLU bit mask or a batch-statistics layer's raw output:
a batch-statistics layer is handed to the hook with the oracle's conv of the device's input and is otherwise listed as skipped.

tests/test_layerref_cpu.py runs this walk against a host stand-in of an engine, so what it can and cannot see is known without a GPU.
"""
import re
import types

import torch
import torch.nn.functional as F


def _max_rel(a, b, valid=None):
    a, b = a.double(), b.double()
    d = (a - b).abs()
    if valid is not None:
        d = d * valid
        b = b * valid
    return float(d.max() / (b.abs().max() + 1e-30))


def _l2_rel(a, b, valid=None):
    a, b = a.double(), b.double()
    if valid is not None:
        a, b = a * valid, b * valid
    return float(torch.linalg.vector_norm(a - b) / (torch.linalg.vector_norm(b) + 1e-30))


class DeviceTensors(object):
    """Reads the engine's activation / gradient buffers back as dense fp32 NCHW tensors (+ the mask of the pixels the device computes)."""

    def __init__(self, eng):
        self.eng, self.B = eng, eng.B
        self.npad = {}
        for c in eng.convs.values():
            self.npad[c.dst.spec.id] = c.npad
        # a projection shortcut computed inside the fused forward pair (conv_pairs.hip) has no output tensor
        self.never_stored = {eng.convs[nm].dst.spec.id for nm in getattr(eng, "shortcut_folded", [])}
        self.producer = {c.dst.spec.id: c for c in eng.convs.values()}
        self.pool_of_stem = {}
        for n in eng.graph.nodes:
            if n.op == "pool":
                self.npad[n.dst.id] = n.dst.c
                self.pool_of_stem[n.src.id] = n

    def _even(self, X):
        m = torch.zeros(1, 1, X.spec.h, X.spec.w)
        m[:, :, ::2, ::2] = 1
        return m

    def _nchw(self, flat, X, h, w):
        C = self.npad[X.spec.id]
        return flat.float().cpu().view(self.B, h, w, C)[..., :X.spec.c].permute(0, 3, 1, 2).contiguous()

    def values(self, X):
        """(values [B, C, H, W] with zeros where the device computes nothing, valid-pixel mask or None = all) -- None when the tensor is never stored."""
        s = X.spec
        if getattr(X, "fused_pool", False) or X.spec.id in self.never_stored:
            return None
        if getattr(X, "fwd_sampled", False):                     # computed at the even pixels only, stored compact
            v = torch.zeros(self.B, s.c, s.h, s.w)
            v[:, :, ::2, ::2] = self._nchw(X.data_compact, X, s.h // 2, s.w // 2)
            return v, self._even(X)
        v = self._nchw(X.data, X, s.h, s.w)
        if getattr(X, "fwd_scattered", False):                   # even pixels written, the rest of the buffer is whatever the allocator left
            m = self._even(X)
            return torch.where(m.bool().expand_as(v), v, torch.zeros_like(v)), m
        return v, None

    def grad(self, X):
        """dL/d(pre-activation of X's producer) as the device stored it, dense; None when it never reaches memory in full."""
        if X.grad is None or not X.grad_written or getattr(X.grad, "_urso_on_chip", False):
            return None
        s = X.spec
        if X.compact is not None:                                # [B, H/2, W/2, C]: zero off the even grid
            g = torch.zeros(self.B, s.c, s.h, s.w)
            g[:, :, ::2, ::2] = self._nchw(X.grad, X, s.h // 2, s.w // 2)
            return g
        return self._nchw(X.grad, X, s.h, s.w)


def _pad_for(n, x):
    """Explicit zero padding of node n (graph.py keeps (top, left); bottom / right follow from the output size): ZeroPadding2D(3) of the
    stem, 'same' of the 3x3 layers, TF-SAME of the stride-2 bottleneck_layer (net.py:170, 106, 639)."""
    pt, pl = n.pad
    pb = (n.dst.h - 1) * n.stride + n.kh - x.shape[2] - pt
    pr = (n.dst.w - 1) * n.stride + n.kw - x.shape[3] - pl
    return F.pad(x, (pl, max(pr, 0), pt, max(pb, 0)))


def forward_layer_errors(eng, weights, img, cfg, dtype, only=None, hook=None, dev=None, refs=None):
    """One pass over the plan of an engine whose buffers hold a forward pass from `weights` on the molded batch `img`.
    Returns ({layer: (max-norm error, Euclidean error)} of every layer's stored output, [layers that could not be read]).
    A stem whose kernel also pools (only the pooled tensor exists) is entered as '<name>+maxpool'; a projection shortcut computed inside
    the launch of the layer that adds it has no entry of its own: it is checked, unrounded, through that layer.
    only: a regular expression; layers whose name it does not match (re.search) are left out.
    refs: a dict that receives the oracle's output of every fp32-stored layer (the heads), {layer: [B, C, 1, 1]}.
    hook(event, L): the caller's second half of a layer (tests/test_layerwise_gpu.py: the gradients), called with L.c the layer and
      'unselected'  the layer is left out by `only`;
      'batch_bn'    a batch-statistics layer: L.xt the device's input (requires grad), L.z4c the oracle's conv + bias of it; no entry is made here;
      'layer'       after the comparison: L.xt, L.z4 (pre-activation, autograd graph to L.xt and the leaves L.Pc / L.Pb), L.y, L.res and
                    L.stored = 'tensor' | 'pooled' (the fused stem) | 'folded' (the shortcut inside another layer's launch).
    With a hook the oracle's layer keeps its autograd graph; without one nothing is recorded."""
    from oracle import graph_ref as G
    q = G.StorageRounding(dtype, unstored=getattr(eng, "shortcut_folded", ()))
    rnd = lambda t: t.to(dtype).float()
    dev = dev if dev is not None else DeviceTensors(eng)
    P = G.to_torch(weights, requires_grad=hook is not None)
    B = eng.B
    errs, skipped = {}, []
    acts_by_id = {X.spec.id: X for X in eng.acts.values()}
    for c in eng.convs.values():
        n = c.node
        L = types.SimpleNamespace(c=c, P=P, q=q, rnd=rnd, dev=dev)
        if only is not None and not re.search(only, n.name):
            if hook is not None:
                hook("unselected", L)
            continue
        Pc = P[n.name]
        Pb = P[n.bn] if n.bn else None
        # ---- the device's stored operands
        if n.stem:
            x = rnd(torch.as_tensor(img, dtype=torch.float32)).permute(0, 3, 1, 2).contiguous()
            xvalid = None
        else:
            xv = dev.values(c.src)
            if xv is None:
                skipped.append(n.name); continue
            x, xvalid = xv
        if getattr(c, "batch_bn", False):
            if hook is None:
                skipped.append(n.name); continue
            assert xvalid is None and not n.dense
            L.xt = x.clone().requires_grad_(True)
            L.z4c = G.conv2d(_pad_for(n, L.xt), {"kernel": q.weight(Pc["kernel"]), **({"bias": Pc["bias"]} if "bias" in Pc else {})}, stride=n.stride)
            hook("batch_bn", L)
            continue
        with torch.set_grad_enabled(hook is not None):
            res = None
            if c.res is not None:
                rv = dev.values(c.res)
                if rv is None and c.res.spec.id in dev.never_stored:
                    # the shortcut lives inside this layer's fused launch as more columns of its GEMM, added in fp32 and never rounded to
                    # storage: the oracle's shortcut layer on ITS device input, unrounded
                    Sc = dev.producer[c.res.spec.id]
                    sx = dev.values(Sc.src)[0]
                    with torch.no_grad():
                        res = G.conv_bn(_pad_for(Sc.node, sx), P[Sc.node.name], P[Sc.node.bn] if Sc.node.bn else None, False,
                                        stride=Sc.node.stride, padding="valid", q=q)
                elif rv is None:
                    skipped.append(n.name); continue
                else:
                    res = rv[0]
            xt = x.clone().requires_grad_(True) if hook is not None else x
            # ---- the oracle's single layer on them
            if n.dense:
                feat = xt.permute(0, 2, 3, 1).reshape(B, -1) if xt.dim() == 4 and xt.shape[2] * xt.shape[3] > 1 else xt.reshape(B, -1)
                z4 = G._qdense(feat, Pc, q).view(B, -1, 1, 1)
            else:
                z4 = G.conv_bn(_pad_for(n, xt), Pc, Pb, False, stride=n.stride, padding="valid", q=q)
            if res is not None:
                z4 = z4 + res
            y = torch.relu(z4) if n.relu else z4
            y = y if n.out_f32 else rnd(y.detach())
        if refs is not None and n.out_f32:
            refs[n.name] = y.detach()
        # ---- the layer's stored output
        dv = dev.values(c.dst)
        if dv is None and c.dst.spec.id in dev.never_stored:     # the folded shortcut: checked through the layer that adds it (above)
            stored = "folded"
        elif dv is None:                                         # conv1 inside urso_stem_conv_pool: only the pooled tensor exists
            stored = "pooled"
            pool = dev.pool_of_stem[c.dst.spec.id]
            pd = dev.values(acts_by_id[pool.dst.id])[0]
            yp = G.maxpool_3x3_s2_same(y.detach())
            errs[n.name + "+maxpool"] = (_max_rel(yp, pd), _l2_rel(yp, pd))
        else:
            stored = "tensor"
            errs[n.name] = (_max_rel(y.detach(), dv[0], dv[1]), _l2_rel(y.detach(), dv[0], dv[1]))
        if hook is not None:
            L.Pc, L.Pb, L.xt, L.res, L.z4, L.y, L.stored = Pc, Pb, xt, res, z4, y, stored
            hook("layer", L)
    return errs, skipped
