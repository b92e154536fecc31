"""Records of Engine._build_plan (ursonet_amd/engine.py): the launches, activation tensors and layers of a plan, and the backward-pass
launches that wait for company until the plan flushes them."""
import torch

from . import hip


def _round_up(v, m):
    return (v + m - 1) // m * m


class _Launch(object):
    """One planned launch: an entry of Engine.prep_ops / fwd_ops / loss_pre_ops / loss_ops / bwd_ops / opt_ops, called like the function it
    wraps.  Everything the planner, the fork (Engine._fork_weight_gradients) and ursonet_amd/dp.py need to know about a launch is a field;
    `label` is what profiles print and nothing reads it back.  A rewrite of the plan mutates the record or removes it from its list (by
    identity: records compare by identity), so whoever holds a reference -- _Conv.fwd, _Act.gather -- keeps the right launch.
      kind    what the launch is: prep | mold | maxpool | fwd | fwd+sampled (and a second store of the sampled pixels) | fwd@sampled (at the
              sampled pixels only) | fwd+maxpool | bn_stats | bn_apply | subsample | quat | loss | bn_bwd | maxpool_bwd | wgrad | unpack |
              finalize | reduce | finalize_mat | finalize_vec | expand | dgrad+wgrad | dgrad (with `wgrad` set: a fused backward pair that
              writes weight-gradient partials too) | dgrad_heads | wgrad_heads | bits_subsample | zero | sqnorm_lw | sqnorm | sgd | adam | loss_scale |
              ema | grad_accum | grad_close | lars_norms | lars_trust | lars_sgd | lamb_moments | lamb_trust | lamb_apply |
              sam_norm | sam_ascend | sam_descend | sam_settle
      fwd, dgrad, wgrad   names of the layers whose forward output / data gradient / weight gradient it computes, in label order
      done    names of the layers whose gradient contribution is complete once it is enqueued (ursonet_amd/dp.py cuts the pass there)
      bucket  key of the batched parameter-sized passes (hip.ParamBatch): a gradient bucket's index or "all", else None"""
    __slots__ = ("run", "kind", "label", "fwd", "dgrad", "wgrad", "done", "bucket")

    def __init__(self, run, kind, label=None, fwd=(), dgrad=(), wgrad=(), done=(), bucket=None):
        self.run, self.kind, self.label = run, kind, label if label is not None else kind
        self.fwd, self.dgrad, self.wgrad, self.done, self.bucket = fwd, dgrad, wgrad, done, bucket

    def __call__(self):
        return self.run()

    def computes_only(self, c, or_sampled_store=False):
        """The launch is layer c's forward pass as first planned: c alone (in no fused launch), at every pixel, with no second store of the
        sampled pixels (unless or_sampled_store)."""
        return self.fwd == (c.name,) and (self.kind == "fwd" or (or_sampled_store and self.kind == "fwd+sampled"))


class _Act(object):
    """An activation tensor in HBM (+ its gradient buffer, allocated on demand)."""

    def __init__(self, eng, spec, numel, dtype):
        self.spec, self.numel = spec, numel
        self.fused_pool = False      # conv1's output when urso_stem_conv_pool computes the max-pool as well: never stored
        self.data = torch.empty(numel, dtype=dtype, device=eng.device)
        self.grad = None
        self.grad_written = False
        self.pending = None          # gradient tensor to be folded into the next dgrad into this tensor
        self.bits = None             # ReLU bit mask (1 byte per 8 elements), written by the producing conv's forward epilogue
        self.compact = None          # (H, W): the gradient buffer holds only the even rows / columns of the pixel grid ([B, H/2, W/2, C])
        self.pending_hw = None       # same, for a pending residual gradient
        self.grad_dense, self.residual_needs_dense = None, False      # dense form of a compact gradient for the residual branch
        self.data_compact = self.bits_compact = None    # the even rows / columns of the tensor and of its bit mask ([B, H/2, W/2, C])
        self.fwd_sampled = False     # only data_compact is computed (_sample_block_output)
        self._compact_first = None   # (launch, conv, dz) of the first compact data gradient into this tensor (_dgrad_compact)
        self.gather = None           # the forward launch that fills data_compact from the dense tensor, if any (_plan_compact_input)
        self.eng = eng

    @property
    def data(self):
        if self.fused_pool:
            raise RuntimeError("T%d is conv1's output inside the fused conv1 + ReLU + max-pool kernel: it is never stored (option stem_pool = 0 keeps it)" % self.spec.id)
        return self._data

    @data.setter
    def data(self, t):
        self._data = t

    def grad_buf(self):
        if self.grad is None:
            self.grad = torch.empty(self.numel, dtype=self.data.dtype, device=self.eng.device)
        return self.grad


class _Conv(object):
    """Planner state of one conv / Dense layer."""

    def __init__(self, node):
        self.node, self.name, self.bn = node, node.name, node.bn
        self.N, self.npad = node.cout, _round_up(node.cout, 8)
        self.src = self.dst = self.res = None      # _Act: input, output, residual operand
        self.xin = None                            # the tensor the forward pass and the weight gradient read (gf describes it)
        self.gf = self.gd = self.gf_compact = self.gd_compact = None      # geometries: forward, data gradient, their compact forms
        self.gd_scatter, self.gd_scatter_stride = False, 0                 # gd writes every stride-th pixel of a pre-zeroed buffer
        self.K_raw, self.fwd_flags, self.fwd, self.winograd = 0, 0, None, False    # fwd: the _Launch that computes dst; None for batch-statistics layers
        self.w = self.b = self.gamma = self.beta = self.mean = self.var = self.wf = self.wd = self.biasf = self.scale = None
        self.batch_bn, self.Mpix = False, None
        self.bn_gamma = self.bn_beta = self.bn_mmean = self.bn_mvar = self.z = self.dz = self.bmean = self.bvar = self.dbeta = self.dgamma = None
        self.splits, self.desc, self.desc_id = 0, None, None       # weight-gradient splits and hip.ParamDesc (the stem has neither)
        self.ws_f = self.ws_d = 0                  # split-K workspace bytes, forward / data gradient
        self.halo_f = self.halo_d = False
        self.pooled_grad = None                    # stem: (pool output, arg-max bytes) its weight gradient reads instead of its own dz
        self.solo = self.wgrad_by_pair = self.dgrad_done_by_pair = False  # gradients written by a fused launch (_plan_wgrad, _dgrad_pair)
        self.wg_ws, self.wg_npart = None, 0        # weight-gradient split partials and their count
        self.dw_raw = self.colsum = self.dotpart = self.dw_unp = None


class _PendingLaunches(object):
    """The launches of a backward plan that wait for company, and the order in which they are flushed:
      wg   weight gradients of the general kernel, grouped into shared launches (urso_wgrad_group_run);
      hw   3x3 weight gradients of the register-resident kernel, two to a launch (urso_conv_wgrad_partial2);
      dd   data gradients of the Dense heads of one depth (urso_dense_multi);
      dwg  weight gradients of the Dense heads (urso_dense_wgrad_multi): leaves of the backward pass, so all of them wait for one
           launch behind the last Dense data gradient (or the end of their gradient bucket).
    wg / hw hold (conv, name, input, dz, weight-gradient geometry); dd / dwg hold the layer dicts of hip.DenseMulti / DenseWgradMulti (+ "names" / "name": the layers of the entry)."""

    WGRAD_GROUP_FILL = 0.7      # a layer that would drop a shared launch's fill of the resident block slots below this starts a new group

    def __init__(self, eng, wg_max):
        self.eng, self.dt = eng, eng.dt
        self.wg_max = wg_max    # most layers in one grouped weight-gradient launch (<= 1: no grouping, no pairing)
        self.wg, self.hw, self.dd, self.dwg = [], [], [], []

    def _emit(self, run, kind, names):
        """The weight gradients of the layers `names` in one launch (kind dgrad_heads: their data gradients, which complete no layer)."""
        dgrad = kind == "dgrad_heads"
        self.eng.bwd_ops.append(_Launch(run, kind, "%s:%s" % (kind, "+".join(names)), dgrad=names if dgrad else (),
                                        wgrad=() if dgrad else names, done=() if dgrad else names))

    def emit_wgrad(self, c, name, xw, G, gf_w):
        dt = self.dt
        self._emit(lambda: hip.conv_wgrad_partial(gf_w, dt, xw, G, c.wg_ws), "wgrad", (name,))

    def at_node(self, level):
        """Before the backward plan of a node of Dense depth `level` (None: not a Dense head layer)."""
        if self.dd and level != self.dd[0]["level"]:
            self.flush_dense_dgrads()
        if self.dwg and level is None:
            self.flush_dense_wgrads()

    def add_wgrad_pair(self, item):
        self.hw.append(item)
        if len(self.hw) == 2:
            self.flush_hw_pair()

    def add_wgrad_group(self, item):
        cand = self.wg + [item]
        wide = lambda g: g.KH * g.KW * g.C >= 256 and g.N >= 256      # (256 x 256 tiles when every layer of the group is this wide)
        if len(cand) > 1 and (wide(cand[-1][4]) != wide(cand[0][4]) or
                              hip.WgradGroup([t[4] for t in cand], self.dt).fill < self.WGRAD_GROUP_FILL):
            self.flush_wgrads()                 # another tile shape, or the newcomer's tile count / pixel count does not divide the slots well
        self.wg.append(item)
        if len(self.wg) >= self.wg_max:
            self.flush_wgrads()

    def add_dense_dgrad(self, L):
        prev = [P for P in self.dd if P["dst"] is L["dst"]]
        if prev and L["add"] is L["dst"] and prev[-1].get("src1") is None:
            prev[-1].update(src1=L["src0"], wgt1=L["wgt0"], K1=L["K0"], names=prev[-1]["names"] + L["names"])
            return
        if prev:
            self.flush_dense_dgrads()           # a third writer of the same tensor: accumulate behind the launch that holds the first two
        self.dd.append(L)

    def add_dense_wgrad(self, L):
        self.dwg.append(L)

    def flush_bucket(self):
        """At the end of a gradient bucket: its reduction reads every partial of the bucket."""
        if self.dwg and any(L["dz"] is P["dst"] for L in self.dwg for P in self.dd):
            self.flush_dense_dgrads()           # (a waiting weight gradient reads what a waiting data gradient writes)
        self.flush_dense_wgrads()
        self.flush_wgrads()
        self.flush_hw_pair()

    def flush(self):
        """At the end of the backward pass."""
        self.flush_dense_dgrads()
        self.flush_bucket()

    def flush_hw_pair(self):
        items, self.hw = self.hw, []
        sp = hip.conv_wgrad_pair_splits(items[0][4], items[1][4], self.dt) if len(items) == 2 else None
        if sp is None:
            for t in items:
                self.emit_wgrad(*t)
            return
        for (c, _, _, _, _), s_ in zip(items, sp):
            assert s_ <= c.splits
            c.splits = c.desc.splits = s_
            c.wg_npart = s_ * (c.K_raw * c.npad + hip.WGRAD_PART_PAD)
            c.desc.part, c.desc.colpart = c.wg_ws.data_ptr(), c.wg_ws.data_ptr() + 4 * c.wg_npart
        (c0, n0, x0, G0, g0), (c1, n1, x1, G1, g1) = items
        dt = self.dt
        self._emit(lambda: hip.conv_wgrad_partial2(g0, g1, dt, x0, G0, c0.wg_ws, x1, G1, c1.wg_ws), "wgrad", (n0, n1))
        self.eng.n_wgrad_groups += 1

    def flush_wgrads(self):
        items, self.wg = self.wg, []
        dev = self.eng.device
        while items:
            take = items
            grp = None
            while len(take) > 1:
                grp = hip.WgradGroup([t[4] for t in take], self.dt)
                if grp.nblocks:
                    break
                take, grp = take[:len(take) - 1], None           # more tiles than resident blocks: a smaller group
            items = items[len(take):]
            if grp is None:
                self.emit_wgrad(*take[0])
                continue
            for (c, _, _, _, _), s in zip(take, grp.splits):
                need_f = s * (c.K_raw * c.npad + hip.WGRAD_PART_PAD) + s * c.npad + 64
                if c.wg_ws.numel() < need_f:           # (the workspace was sized for the layer alone)
                    c.wg_ws = torch.empty(need_f, dtype=torch.float32, device=dev)
                if s > 1 and c.dw_raw is None:
                    c.dw_raw = torch.empty(c.K_raw * c.npad, dtype=torch.float32, device=dev)
                    c.colsum = torch.empty(c.npad, dtype=torch.float32, device=dev)
                    c.desc.dw_raw, c.desc.colsum = hip.ptr(c.dw_raw), hip.ptr(c.colsum)
                c.splits = c.desc.splits = s
                c.wg_npart = s * (c.K_raw * c.npad + hip.WGRAD_PART_PAD)
                c.desc.part, c.desc.colpart = c.wg_ws.data_ptr(), c.wg_ws.data_ptr() + 4 * c.wg_npart
            grp.bind([t[2] for t in take], [t[3] for t in take], [t[0].wg_ws for t in take], dev)
            self._emit(grp.run, "wgrad", tuple(t[1] for t in take))
            self.eng.n_wgrad_groups += 1

    def flush_dense_dgrads(self):
        layers, self.dd = self.dd, []
        for i in range(0, len(layers), hip.DENSE_MULTI_MAX):
            part = layers[i:i + hip.DENSE_MULTI_MAX]
            self._emit(hip.DenseMulti(part, self.dt).run, "dgrad_heads", tuple(n for L in part for n in L["names"]))

    def flush_dense_wgrads(self):
        layers, self.dwg = self.dwg, []
        for i in range(0, len(layers), hip.DENSE_MULTI_MAX):
            part = layers[i:i + hip.DENSE_MULTI_MAX]
            self._emit(hip.DenseWgradMulti(part, self.dt).run, "wgrad_heads", tuple(L["name"] for L in part))
