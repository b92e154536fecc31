"""Elementwise float64 probes of the weight preparation and of the batched parameter passes (helpers: tests/exactprobe.py), in the
conventions of tests/test_step_tail_exact_gpu.py: every kernel is called through the C ABI on outputs that live in NaN-guarded buffers
(no NaN may remain inside the extent, every bit past it must be unchanged) and compared ELEMENT BY ELEMENT, over its whole extent, with
a float64 reference of the operation's definition; each bound is half an ulp of the storage type plus the fp32 roundings counted from
the operation (fold_bounds, reduce_bound, finalize_bounds state their counts; tests/test_exactprobe_cpu.py shows that they accept a plain
fp32 restatement and reject the faults a kernel can have).  ran() asserts which kernel an entry point launched.

  * urso_conv_weight_prep, urso_stem_weight_pack, urso_stem_wgrad_unpack: the fold rounded ONCE to fp32 / bf16 / fp16 at every edge of
    the 32 x 32 tile walk, with and without bias / BN / wd, fp16 subnormals kept.
  * urso_param_batch_run(PB_PREP): a permuted subset of a descriptor table with both tile forms (64 x 64 vector, 32 x 32), two layers
    carrying bias_from, one layer left out.
  * PB_REDUCE + PB_FINALIZE_MAT / _VEC from random partials at every split-lane count and on the fused sums, their _sq and _ls forms,
    urso_param_grad_finalize_ls.
  * the table the engine builds: every conv's prepared tensors against fold64 of its own master tensors.

The largest error / bound per quantity (printed as RATIO lines at the end of the module), MI355X:
  batch finalize gb                      0.371   batch finalize gbeta                   0.495   batch finalize ggamma                  0.051
  batch finalize gw                      0.456   batch finalize sq slots                0.028   batch prep 32 bias_from biasf          0.192
  batch prep 32 bias_from scale          0.291   batch prep 32 bias_from wd bf16        0.999   batch prep 32 bias_from wd fp16        0.998
  batch prep 32 bias_from wd fp32        0.332   batch prep 32 bias_from wf bf16        0.999   batch prep 32 bias_from wf fp16        0.998
  batch prep 32 bias_from wf fp32        0.332   batch prep 32 biasf                    0.163   batch prep 32 scale                    0.339
  batch prep 32 wd bf16                  0.995   batch prep 32 wd fp16                  0.999   batch prep 32 wd fp32                  0.405
  batch prep 32 wf bf16                  0.995   batch prep 32 wf fp16                  0.999   batch prep 32 wf fp32                  0.405
  batch prep 64 bias_from biasf          0.266   batch prep 64 bias_from scale          0.361   batch prep 64 bias_from wd bf16        0.999
  batch prep 64 bias_from wd fp16        0.999   batch prep 64 bias_from wd fp32        0.442   batch prep 64 bias_from wf bf16        1.000
  batch prep 64 bias_from wf fp16        0.999   batch prep 64 bias_from wf fp32        0.442   batch prep 64 biasf                    0.377
  batch prep 64 scale                    0.436   batch prep 64 wd bf16                  1.000   batch prep 64 wd fp16                  0.999
  batch prep 64 wd fp32                  0.504   batch prep 64 wf bf16                  1.000   batch prep 64 wf fp16                  0.999
  batch prep 64 wf fp32                  0.504   engine biasf                           0.510   engine scale                           0.422
  engine wd bf16                         1.000   engine wd fp16                         1.000   engine wd fp32                         0.502
  engine wf bf16                         1.000   engine wf fp16                         1.000   engine wf fp32                         0.502
  finalize_ls gb                         0.325   finalize_ls gbeta                      0.000   finalize_ls ggamma                     0.029
  finalize_ls gw                         0.428   prep biasf                             0.382   prep scale                             0.330
  prep wd bf16                           1.000   prep wd fp16                           1.000   prep wd fp32                           0.414
  prep wf bf16                           1.000   prep wf fp16                           1.000   prep wf fp32                           0.414
  reduce colsum                          0.087   reduce dw_raw                          0.207   stem pack biasf                        0.379
  stem pack scale                        0.348   stem pack wf bf16                      1.000   stem pack wf fp16                      1.000
  stem pack wf fp32                      0.430
(16-bit wf / wd: half an ulp of the storage type, reached.  ggamma and the sq slots sit near 0.05 and below: their bounds are the worst
case of a 20 - 35 deep chain of additions whose errors mostly cancel; there the bit identities with urso_param_grad_finalize and between
the plain, _sq and _ls forms are the sharp checks.  gbeta of the per-layer form is a copy: bound 0, exact.)
"""
import pytest
import torch

import exactprobe as X
from test_step_tail_exact_gpu import NAN, SLACK, assert_guard, guarded       # NaN-guarded buffers: the same helpers

pytestmark = pytest.mark.gpu

EPS, WD = 1e-3, 1e-2
EINVAL = -1


def _hip():
    import ursonet_amd.hip as hip
    return hip


def dev(t, dt=0):
    return None if t is None else t.contiguous().to(X.tdtype(dt)).cuda()


def assert_untouched(buf, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "%s was written" % what


_worst = {}


def note(name, ratio):
    _worst[name] = max(_worst.get(name, 0.0), float(ratio))


def check(name, got, ref, bound, what=None):
    note(name, X.assert_within(got, ref, bound, what or name))


def bits_equal(a, b, what):
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    bad = a.view(it) != b.view(it)
    assert not bool(bad.any()), "%s: %d of %d elements differ in their bits (first at %d: %r / %r)" % (
        what, int(bad.sum()), bad.numel(), int(bad.nonzero()[0]), float(a[bad][0]), float(b[bad][0]))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_worst):
        print("RATIO %-28s %.3f" % (k, _worst[k]))


DTN = ("fp32", "bf16", "fp16")


# ===================================================================================================================== urso_conv_weight_prep
PREP_SHAPES = [(1, 1, 1, 1, 1), (1, 1, 33, 31, 32), (3, 3, 40, 50, 56), (3, 3, 3, 5, 8), (1, 1, 256, 13, 16), (1, 1, 64, 64, 64)]


def _prep(hip, shape, dt, w, b, bn, with_wd=True):
    """One urso_conv_weight_prep on guarded outputs -> dict of output views."""
    KH, KW, Ci, N, npad = shape
    K = KH * KW * Ci
    out = {"wf": guarded(npad * K, dt), "biasf": guarded(npad), "scale": guarded(npad)}
    if with_wd:
        out["wd"] = guarded(npad * K, dt)
    bnd = [dev(t) for t in bn] if bn is not None else [None] * 4
    with X.ran("weight_prep_kernel"):
        hip.conv_weight_prep(KH, KW, Ci, N, npad, dt, dev(w), dev(b), bnd[0], bnd[1], bnd[2], bnd[3], EPS, out["wf"][1],
                             out["wd"][1] if with_wd else None, out["biasf"][1], out["scale"][1])
    for k, (buf, view) in out.items():
        assert_guard(buf, view.numel(), "weight_prep " + k)
    return {k: v[1] for k, v in out.items()}


def _check_fold(tag, got, ref, bnd, dt, N, what):
    """wf / wd / biasf / scale of one layer against fold64 within fold_bounds; the padded filters hold exactly 0 / 1."""
    for k in got:
        r = ref[k][0]
        check("%s %s%s" % (tag, k, " " + DTN[dt] if k in ("wf", "wd") else ""), got[k].reshape(r.shape), r, bnd[k], "%s %s" % (k, what))
    assert float(got["wf"].reshape(ref["wf"][0].shape)[N:].float().abs().sum()) == 0, "wf: padded filters not 0 " + what
    if "wd" in got:
        X.assert_zero_columns(got["wd"].reshape(ref["wd"][0].shape), N, "wd " + what)
    assert float(got["biasf"][N:].abs().sum()) == 0 and bool((got["scale"][N:] == 1).all()), "biasf / scale of the padded filters " + what


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("shape", PREP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_prep_elementwise(shape, dt):
    """urso_conv_weight_prep at the smallest shapes that reach each edge of the 32 x 32 tile walk (one past a tile in C and one short in N,
    ragged tiles with padded filters, a small 3x3, a head, whole tiles), with and without bias, BN and the wd output: the fold rounded
    once to `dt`.  A double rounding (s rounded to 16 bits before the product), unflipped wd taps or a missing eps are outside the bound
    (tests/test_exactprobe_cpu.py)."""
    hip = _hip()
    KH, KW, Ci, N, npad = shape
    w, b, bn = X.fold_inputs(KH, KW, Ci, N, seed=1)
    for bias in (True, False):
        for has_bn in (True, False):
            b_, bn_ = (b if bias else None), (bn if has_bn else None)
            ref = X.fold64(w, b_, bn_, EPS, npad)
            bnd = X.fold_bounds(ref, dt, bias, has_bn)
            X.assert_sensitive(ref["wf"][0], what="fold wf"); X.assert_sensitive(ref["wd"][0], what="fold wd"); X.assert_sensitive(ref["scale"][0], what="fold scale")
            if bias or has_bn:
                X.assert_sensitive(ref["biasf"][0], what="fold biasf")
            for with_wd in (True, False):
                got = _prep(hip, shape, dt, w, b_, bn_, with_wd)
                assert set(got) == set(ref) - (set() if with_wd else {"wd"})
                _check_fold("prep", got, ref, bnd, dt, N, "%s dt=%d bias=%d bn=%d wd=%d" % (shape, dt, bias, has_bn, with_wd))


def test_weight_prep_keeps_fp16_subnormals():
    """|w s| around 3e-6 in a block of filters, fp16: subnormals of spacing 2^-24.  The bound there is half that spacing (+ 5 U |w s|), so
    a store that flushes them to zero fails in nearly every element of the block."""
    hip = _hip()
    shape = (3, 3, 40, 50, 56)
    w, b, bn = X.fold_inputs(3, 3, 40, 50, seed=3, tiny_block=(16, 40))
    ref = X.fold64(w, b, bn, EPS, 56)
    blk = ref["wf"][0][16:40]
    assert float(blk.abs().max()) < 2.0 ** -14 and float(blk.abs().median()) > 1e-6
    got = _prep(hip, shape, 2, w, b, bn)
    _check_fold("prep", got, ref, X.fold_bounds(ref, 2, True, True), 2, 50, "fp16 subnormal block")
    stored = got["wf"].reshape(56, 3, 3, 40)[16:40].double().cpu()
    assert float((stored != 0).sum()) / stored.numel() > 0.9, "the subnormal block was flushed"


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 5, 64])
def test_stem_weight_pack_elementwise(N, dt):
    """urso_stem_weight_pack: the folded 7x7x3 filter in the packed [N][7][4][8] tap grid (X.stem_taps of fold64), pad taps and the molded
    zero channel exactly 0; biasf / scale as the plain preparation's."""
    hip = _hip()
    w, b, bn = X.fold_inputs(7, 7, 3, N, seed=2)
    for bias, has_bn in ((True, True), (False, True), (True, False)):
        b_, bn_ = (b if bias else None), (bn if has_bn else None)
        ref = X.fold64(w, b_, bn_, EPS, N)
        bnd = X.fold_bounds(ref, dt, bias, has_bn)
        grid = lambda t: X.stem_taps(t.permute(1, 2, 3, 0)).permute(3, 0, 1, 2).reshape(N, 7, 4, 8)       # [N][7][7][3] -> [N][7][kp][cp]
        X.assert_sensitive(ref["wf"][0], what="stem fold")
        out = {"wf": guarded(N * 224, dt), "biasf": guarded(N), "scale": guarded(N)}
        bnd_d = [dev(t) for t in bn_] if has_bn else [None] * 4
        with X.ran("stem_pack_kernel"):
            hip.stem_weight_pack(N, dt, dev(w), dev(b_), bnd_d[0], bnd_d[1], bnd_d[2], bnd_d[3], EPS, out["wf"][1], out["biasf"][1], out["scale"][1])
        for k, (buf, view) in out.items():
            assert_guard(buf, view.numel(), "stem_weight_pack " + k)
        tag = "N=%d dt=%d bias=%d bn=%d" % (N, dt, bias, has_bn)
        # (stem_taps leaves 0 in the pad taps of the bound as well: they must be exactly 0)
        check("stem pack wf " + DTN[dt], out["wf"][1].reshape(N, 7, 4, 8), grid(ref["wf"][0]), grid(bnd["wf"]), "wf " + tag)
        check("stem pack biasf", out["biasf"][1], ref["biasf"][0], bnd["biasf"], "biasf " + tag)
        check("stem pack scale", out["scale"][1], ref["scale"][0], bnd["scale"], "scale " + tag)


@pytest.mark.parametrize("N", [1, 5, 64])
def test_stem_wgrad_unpack_bit_exact(N):
    """urso_stem_wgrad_unpack: the 147 real taps of the packed [7][4][8][N] gradient, bit for bit; the pad taps (a sentinel) reach nothing."""
    hip = _hip()
    g = torch.Generator().manual_seed(N)
    packed = torch.randn(7, 8, 4, N, generator=g)                    # [ky][q = 2 kp + (cp >> 2)][c = cp & 3][n] == [7][4][8][N] in memory
    packed[:, 0] = X.PART_SENTINEL
    packed[:, :, 3] = X.PART_SENTINEL
    ob, out = guarded(147 * N)
    with X.ran("stem_unpack_kernel"):
        hip.stem_wgrad_unpack(N, dev(packed), out)
    assert_guard(ob, 147 * N, "stem_wgrad_unpack")
    X.assert_exact(out.reshape(7, 7, 3, N), X.stem_untaps(packed.double()), "stem_wgrad_unpack")
    X.assert_sensitive(X.stem_untaps(packed.double()), what="stem_wgrad_unpack")


# ===================================================================================================================== batched PB_PREP
# (KH, KW, C, N, npad, bias, bn, bias_from layer or None, wd output)
PB_LAYERS = [(3, 3, 64, 64, 64, True, True, None, True),            # 0  aligned: 64 x 64 form
             (1, 1, 68, 72, 72, False, True, None, True),           # 1  aligned, ragged 64-tiles, no bias
             (1, 1, 128, 60, 64, True, True, None, True),           # 2  aligned, padded filters
             (1, 1, 16, 13, 16, True, False, None, True),           # 3  unaligned: 32 form, no BN
             (3, 3, 3, 5, 8, True, True, None, True),               # 4  unaligned 3x3, padded filters
             (1, 1, 64, 64, 64, True, True, 0, True),               # 5  64 form + the folded bias of a layer with bias and BN
             (1, 1, 68, 60, 64, True, True, 1, False),              # 6  64 form + that of a layer with BN and no bias (more filters than this one); no wd
             (1, 1, 16, 13, 16, True, True, 4, True),               # 7  32 form + that of a layer with FEWER filters (5 < 13)
             (1, 1, 32, 32, 32, True, True, None, True)]            # 8  left out of the plan
PB_IDS = [5, 0, 3, 7, 2, 6, 4, 1]


def _aligned(L):
    return ((L[2] | L[3] | L[4]) & 3) == 0


def _set_ptrs(hip, d, **tensors):
    for f, t in tensors.items():
        setattr(d, f, hip.ptr(t))


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_batched_prep_elementwise(dt):
    """urso_param_batch_run(PB_PREP) over a permuted subset of nine descriptors: aligned layers on weight_prep_body64 (whole, ragged and
    padded 64-tiles), unaligned ones on the 32 x 32 body, a layer without BN, one without bias, one without wd, and three carrying
    bias_from (urso_param_desc::bias_from: a source with bias and BN, one with BN only and more filters, one with fewer filters).
    Every planned layer equals fold64 within fold_bounds; one without bias_from also equals urso_conv_weight_prep bit for bit; the layer
    left out of the plan keeps its NaN."""
    hip = _hip()
    assert sum(_aligned(L) for L in PB_LAYERS) >= 5 and sum(not _aligned(L) for L in PB_LAYERS) >= 3
    descs, data, outs = [], [], []
    for i, (KH, KW, Ci, N, npad, bias, has_bn, src, with_wd) in enumerate(PB_LAYERS):
        K = KH * KW * Ci
        w, b, bn = X.fold_inputs(KH, KW, Ci, N, seed=10 + i)
        b, bn = (b if bias else None), (bn if has_bn else None)
        t = dict(w=dev(w), b=dev(b))
        t.update(zip(("gamma", "beta", "mean", "var"), [dev(v) for v in bn] if has_bn else [None] * 4))
        o = {"wf": guarded(npad * K, dt), "biasf": guarded(npad), "scale": guarded(npad)}
        if with_wd:
            o["wd"] = guarded(npad * K, dt)
        d = hip.ParamDesc()
        hip.param_desc_init(d, KH, KW, Ci, N, npad, 1, EPS, WD)
        _set_ptrs(hip, d, **t)
        _set_ptrs(hip, d, **{k: v[1] for k, v in o.items()})
        d.bias_from = 0 if src is None else src + 1
        descs.append(d); data.append((w, b, bn, t)); outs.append(o)
    pb = hip.ParamBatch(descs, torch.device("cuda"))
    nb = pb.plan(hip.PB_PREP, "t", PB_IDS)
    want = sum((-(-L[2] // 64) * -(-L[4] // 64) if _aligned(L) else -(-L[2] // 32) * -(-L[4] // 32)) * L[0] * L[1] for L in (PB_LAYERS[i] for i in PB_IDS))
    assert nb == want, "PB_PREP plans %d blocks, batch_layer_blocks gives %d" % (nb, want)
    with X.ran("weight_prep_batch_kernel"):
        pb.run(hip.PB_PREP, "t", dt)
    for i, L in enumerate(PB_LAYERS):
        KH, KW, Ci, N, npad, bias, has_bn, src, with_wd = L
        w, b, bn, _ = data[i]
        if i not in PB_IDS:
            for k, (buf, _) in outs[i].items():
                assert_untouched(buf, "%s of layer %d, which is not in the plan," % (k, i))
            continue
        for k, (buf, view) in outs[i].items():
            assert_guard(buf, view.numel(), "PB_PREP layer %d %s" % (i, k))
        got = {k: v[1] for k, v in outs[i].items()}
        extra = None if src is None else (data[src][1], data[src][2], PB_LAYERS[src][3])
        ref = X.fold64(w, b, bn, EPS, npad, extra)
        bnd = X.fold_bounds(ref, dt, bias, has_bn, None if src is None else (PB_LAYERS[src][5], PB_LAYERS[src][6]))
        X.assert_sensitive(ref["wf"][0], what="fold wf"); X.assert_sensitive(ref["biasf"][0], what="fold biasf")
        tag = "batch prep" + (" 64" if _aligned(L) else " 32") + (" bias_from" if src is not None else "")
        _check_fold(tag, got, ref, bnd, dt, N, "layer %d %s dt=%d" % (i, L, dt))
        if src is not None:
            plain = X.fold64(w, b, bn, EPS, npad)["biasf"][0]
            m = min(PB_LAYERS[src][3], N)
            assert bool(((ref["biasf"][0] - plain)[:m] != 0).all()) and bool(((ref["biasf"][0] - plain)[m:] == 0).all())
            assert X.violations(got["biasf"][:m], plain[:m], bnd["biasf"][:m]) >= 0.9, "the probe cannot see bias_from"
        else:
            one = _prep(hip, L[:5], dt, w, b, bn, with_wd)
            for k in got:
                bits_equal(got[k], one[k], "PB_PREP against urso_conv_weight_prep: layer %d %s" % (i, k))


# ===================================================================================================================== PB_REDUCE + PB_FINALIZE_*
# (K, N, npad, bias, bn, trainable, bn_trainable)
RED_LAYERS = [(8, 8, 8, True, True, 1, 1),                # one block, a single row per lane
              (144, 24, 24, False, True, 1, 1),           # no bias
              (64, 13, 16, True, False, 1, 1),            # scalar path, padded stride, no BN
              (576, 64, 72, False, False, 1, 1),          # padded stride on the vector path, 4 k-slabs; neither gb nor ggamma
              (300, 8, 8, True, True, 1, 1),              # 2 k-slabs of 150 rows: the two-rows-at-a-time loop and its single-row tail
              (144, 24, 24, True, True, 0, 1),            # frozen layer
              (8, 8, 8, True, True, 1, 0)]                # frozen BN
RED_SPLITS = [1, 2, 5, 16, 17, 49, 100, 200, 400, 733]
GRADS = ("gw", "gb", "ggamma", "gbeta")


def test_split_counts_reach_every_lane_count():
    assert sorted({X.reduce_lanes(s) for s in RED_SPLITS if s > X.FUSE_REDUCE_MAX}) == [1, 2, 4, 8, 16]
    assert [s for s in RED_SPLITS if 1 < s <= X.FUSE_REDUCE_MAX] == [2, 5, 16]


def _red_blocks(L, splits, ks):
    """batch_layer_blocks (prep.hip) restated: (REDUCE, FINALIZE_MAT, FINALIZE_VEC) blocks of one layer."""
    K, N, npad = L[:3]
    red = 0
    if splits > X.FUSE_REDUCE_MAX:
        rcols = 256 // X.reduce_lanes(splits)
        red = -(-(-(-(K * npad) // 4)) // rcols) + -(-(-(-npad // 4)) // rcols)
    return red, -(-N // 64) * ks, -(-N // 256)


class _RedBatch(object):
    """The descriptor table of RED_LAYERS at one split count, its inputs on the host and its guarded outputs."""

    def __init__(self, hip, splits):
        self.hip, self.splits = hip, splits
        self.descs, self.host, self.out, self.flat, self.keep = [], [], [], [], []
        for i, (K, N, npad, bias, has_bn, tr, bntr) in enumerate(RED_LAYERS):
            flat, parts, colparts = X.partials_buffer(K, N, npad, splits, seed=i)
            g = torch.Generator().manual_seed(77 + i)
            h = dict(W=torch.randn(K, N, generator=g) / K ** 0.5, b=torch.randn(N, generator=g) if bias else None,
                     gamma=torch.rand(N, generator=g) + 0.5 if has_bn else None, mean=torch.randn(N, generator=g), var=torch.rand(N, generator=g) + 0.5,
                     parts=parts, colparts=colparts)
            d = hip.ParamDesc()
            hip.param_desc_init(d, 1, 1, K, N, npad, splits, EPS, WD)
            assert d.K == K and d.kb == -(-K // d.ks)
            o = {"dw_raw": guarded(K * npad), "colsum": guarded(npad), "gw": guarded(K * N)}
            if bias:
                o["gb"] = guarded(N)
            if has_bn:
                o["ggamma"], o["gbeta"] = guarded(N), guarded(N)
            fd = dev(flat)
            t = dict(w=dev(h["W"]), b=dev(h["b"]), gamma=dev(h["gamma"]), mean=dev(h["mean"]) if has_bn else None, var=dev(h["var"]) if has_bn else None,
                     dotpart=torch.full((d.ks * N + SLACK,), NAN, device="cuda"))
            _set_ptrs(hip, d, **t)
            _set_ptrs(hip, d, **{k: v[1] for k, v in o.items()})
            d.part = fd.data_ptr()
            d.colpart = fd.data_ptr() + 4 * splits * (K * npad + X.WGRAD_PART_PAD)
            assert fd.numel() == splits * (K * npad + X.WGRAD_PART_PAD) + splits * npad
            d.trainable, d.bn_trainable = tr, bntr
            self.descs.append(d); self.host.append(h); self.out.append(o); self.flat.append(fd); self.keep.append(t)
        self.pb = hip.ParamBatch(self.descs, torch.device("cuda"))
        self.ids = list(range(len(RED_LAYERS)))
        self.nb = {ph: self.pb.plan(ph, "t", self.ids) for ph in (hip.PB_REDUCE, hip.PB_FINALIZE_MAT, hip.PB_FINALIZE_VEC)}

    def clear(self, names):
        for o in self.out:
            for k in names:
                if k in o:
                    o[k][0].fill_(NAN)

    def reduce(self):
        if self.nb[self.hip.PB_REDUCE]:
            with X.ran("reduce_partials_batch_kernel"):
                self.pb.run(self.hip.PB_REDUCE, "t", 0)

    def finalize(self, sq=None, ls=None):
        hip = self.hip
        nbm = self.nb[hip.PB_FINALIZE_MAT]
        with X.ran("finalize_mat_batch_kernel"):
            self.pb.run(hip.PB_FINALIZE_MAT, "t", 0, sqpart=None if sq is None else sq[:nbm], ls=ls)
        with X.ran("finalize_vec_batch_kernel"):
            self.pb.run(hip.PB_FINALIZE_VEC, "t", 0, sqpart=None if sq is None else sq[nbm:nbm + self.nb[hip.PB_FINALIZE_VEC]], ls=ls)
        for i, o in enumerate(self.out):
            for k in GRADS:
                if k in o:
                    assert_guard(o[k][0], o[k][1].numel(), "layer %d %s" % (i, k))

    def grads(self):
        return [{k: o[k][1].clone() for k in GRADS if k in o} for o in self.out]


def _ls_state(k):
    return torch.tensor([2.0 ** k, 2.0 ** -k, 0.0, 0.0, 1.0, 2.0 ** 24, 0.0, 0.0], device="cuda")


@pytest.mark.parametrize("splits", RED_SPLITS)
def test_batched_reduce_and_finalize_elementwise(splits):
    """PB_REDUCE, PB_FINALIZE_MAT and PB_FINALIZE_VEC over seven layers whose partials are random numbers in the documented workspace
    layout (part[splits][K npad + 64] then colpart[splits][npad]; the gaps and the padded columns hold a finite sentinel that must reach
    no gradient).  splits 1: the finalisation reads `part`; 2 / 5 / 16: it sums the partials itself (the 4-at-a-time loop, its tail, the
    maximum); 17: one split-lane, a 16-batch and its tail; 49 / 100 / 200 / 400: 2 / 4 / 8 / 16 lanes, one past each threshold; 733:
    about the engine's largest.
      block counts: the plan returns batch_layer_blocks' counts; REDUCE plans nothing up to 16 splits.
      REDUCE:       dw_raw / colsum equal reduce32 (the documented order on the host) bit for bit, and the float64 sum within reduce_bound.
      gradients:    gw / gb / ggamma / gbeta against finalize64 of the float64 sum of the partials, within finalize_bounds widened by
                    reduce_depth(splits) = ceil(splits / SL) - 1 + SL - 1 roundings on the sums of the partials' magnitudes (gW, gb:
                    6 + depth; ggamma: dot depth + 6 + depth; gbeta: depth); frozen outputs exactly 0.
      bit identity: every gradient equals urso_param_grad_finalize run on the host's fp32 sum in that order (for 2 .. 16 splits the header's
                    "in REDUCE's order (bit-identical)" claim about the fused sums).
      _sq:          the same bits; exactly nblocks slots written; urso_sqnorm_final over them is the float64 sum of squares of what was
                    stored within tree_sum_bound; the layer with neither gb nor ggamma leaves 0 in its channel slot.
      _ls:          with state[INV_SCALE] = 2^-k, k = 0 / 7 / 15, and the partials multiplied by 2^k, every gradient bit and every slot equals
                    the plain run's (powers of two: exact)."""
    hip = _hip()
    rb = _RedBatch(hip, splits)
    D = X.reduce_depth(splits)
    want = [sum(_red_blocks(L, splits, d.ks)[j] for L, d in zip(RED_LAYERS, rb.descs)) for j in range(3)]
    got_nb = [rb.nb[ph] for ph in (hip.PB_REDUCE, hip.PB_FINALIZE_MAT, hip.PB_FINALIZE_VEC)]
    assert got_nb == want, "planned blocks %s, batch_layer_blocks %s" % (got_nb, want)
    assert (got_nb[0] == 0) == (splits <= X.FUSE_REDUCE_MAX)
    assert max(d.ks for d in rb.descs) > 1
    # ---- REDUCE
    rb.reduce()
    sums32 = []
    for i, (L, h, o) in enumerate(zip(RED_LAYERS, rb.host, rb.out)):
        K, N, npad = L[:3]
        s32 = (X.reduce32(h["parts"], splits), X.reduce32(h["colparts"], splits))
        sums32.append(s32)
        for name, s, p in (("dw_raw", s32[0], h["parts"]), ("colsum", s32[1], h["colparts"])):
            if splits <= X.FUSE_REDUCE_MAX:
                assert_untouched(o[name][0], "%s of layer %d (no reduction pass at %d splits)" % (name, i, splits))
                continue
            assert_guard(o[name][0], o[name][1].numel(), "REDUCE %s layer %d" % (name, i))
            bits_equal(o[name][1], s, "REDUCE %s of layer %d against reduce32" % (name, i))
            p64 = p.double()
            X.assert_sensitive(p64.sum(0), what="sum of partials")
            check("reduce " + name, o[name][1].reshape(s.shape), p64.sum(0), X.reduce_bound(p64.abs().sum(0), splits), "%s layer %d splits %d" % (name, i, splits))
    # ---- FINALIZE
    rb.finalize()
    plain = rb.grads()
    for i, (L, h, d) in enumerate(zip(RED_LAYERS, rb.host, rb.descs)):
        K, N, npad, bias, has_bn, tr, bntr = L
        p64, c64 = h["parts"].double()[:, :, :N], h["colparts"].double()[:, :N]
        ref = X.finalize64(p64.sum(0), c64.sum(0), h["W"], h["b"], h["gamma"], h["mean"], h["var"], EPS, WD, dw_mag=p64.abs().sum(0), cs_mag=c64.abs().sum(0))
        bnd = X.finalize_bounds(ref, K, N, npad, d.ks, sum_depth=D)
        assert set(ref) == set(plain[i])
        tag = "layer %d %s splits %d" % (i, L, splits)
        for name in ref:
            X.assert_sensitive(ref[name][0], what="finalize " + name)
            if (name in ("gw", "gb") and not tr) or (name in ("ggamma", "gbeta") and not bntr):
                X.assert_exact(plain[i][name].reshape(ref[name][0].shape), torch.zeros_like(ref[name][0]), "%s %s (frozen)" % (name, tag))
            else:
                check("batch finalize " + name, plain[i][name], ref[name][0], bnd[name], "%s %s" % (name, tag))
        # the per-layer entry point on the host's fp32 sum
        one = {k: guarded(v.numel()) for k, v in plain[i].items()}
        ws = torch.empty(hip.param_grad_finalize_ws_bytes(K, N) // 4 + 4, device="cuda")
        o = lambda k: one[k][1] if k in one else None
        hip.param_grad_finalize(K, N, npad, dev(sums32[i][0]), dev(sums32[i][1]), dev(h["W"]), dev(h["b"]), dev(h["gamma"]), dev(h["mean"]) if has_bn else None,
                                dev(h["var"]) if has_bn else None, EPS, WD, tr, bntr, o("gw"), o("gb"), o("ggamma"), o("gbeta"), ws)
        for k in one:
            assert_guard(one[k][0], one[k][1].numel(), "urso_param_grad_finalize " + k)
            bits_equal(plain[i][k], one[k][1], "%s of %s against urso_param_grad_finalize on the sequential fp32 sum" % (k, tag))
    # ---- _sq
    nbm, nbv = got_nb[1], got_nb[2]
    sqb, sq = guarded(nbm + nbv)
    rb.clear(GRADS)
    rb.finalize(sq=sq)
    assert_guard(sqb, nbm + nbv, "_sq slots")
    for i, g in enumerate(rb.grads()):
        for k in g:
            bits_equal(g[k], plain[i][k], "_sq form: %s of layer %d" % (k, i))
    stored = torch.cat([v.reshape(-1) for g in plain for v in g.values()]).double().cpu()
    sqwant = (stored ** 2).sum()
    depth = max(X.finalize_sq_depth(L[0], L[1], L[2], d.ks, nbm + nbv) for L, d in zip(RED_LAYERS, rb.descs))
    ob, o1 = guarded(1)
    hip.sqnorm_final(sq, o1)
    assert_guard(ob, 1, "sqnorm_final")
    check("batch finalize sq slots", o1[0], sqwant, X.store_bound(sqwant, X.tree_sum_bound(sqwant, depth), 0), "slots, splits %d" % splits)
    bare = [i for i, L in enumerate(RED_LAYERS) if not L[3] and not L[4]]
    assert bare == [3] and all(-(-L[1] // 256) == 1 for L in RED_LAYERS)
    assert float(sq[nbm + 3]) == 0.0 and float(sq[nbm + 2]) != 0.0, "channel slot of the layer with neither gb nor ggamma"
    slots_sq = sq.clone()
    # ---- _ls
    for k in (0, 7, 15):
        for fd in rb.flat:
            fd.mul_(2.0 ** k)
        rb.clear(GRADS + ("dw_raw", "colsum"))
        rb.reduce()
        sqb2, sq2 = guarded(nbm + nbv)
        rb.finalize(sq=sq2, ls=_ls_state(k))
        assert_guard(sqb2, nbm + nbv, "_ls slots")
        for fd in rb.flat:
            fd.mul_(2.0 ** -k)
        for i, g in enumerate(rb.grads()):
            for name in g:
                bits_equal(g[name], plain[i][name], "_ls form, scale 2^%d: %s of layer %d" % (k, name, i))
        bits_equal(sq2, slots_sq, "_ls form, scale 2^%d: the squared-norm slots" % k)
    # the loss-scaled form without slots
    rb.clear(GRADS)
    rb.reduce()                                               # (dw_raw / colsum still hold the sums of the partials times 2^15)
    rb.finalize(ls=_ls_state(0))
    for i, g in enumerate(rb.grads()):
        for name in g:
            bits_equal(g[name], plain[i][name], "_ls form without slots: %s of layer %d" % (name, i))


def test_batched_ls_and_sq_forms_refuse_what_they_cannot_do():
    """urso_param_batch_run_ls without a state, and the PREP / REDUCE phases through _ls and _sq, return URSO_EINVAL and launch nothing."""
    hip = _hip()
    rb = _RedBatch(hip, 17)
    lib, p = hip._lib, hip.ptr
    sqb, sq = guarded(64)
    st = _ls_state(0)
    nb_prep = rb.pb.plan(hip.PB_PREP, "t", rb.ids)
    assert nb_prep > 0 and rb.nb[hip.PB_REDUCE] > 0
    for ph in (hip.PB_FINALIZE_MAT, hip.PB_FINALIZE_VEC):
        t, nb = rb.pb.maps[(ph, "t")]
        assert lib.urso_param_batch_run_ls(ph, 0, p(rb.pb.dev), p(t), nb, p(sq), None, None) == EINVAL
        assert "state" in hip.last_error()
        assert lib.urso_param_batch_run_sq(ph, 0, p(rb.pb.dev), p(t), nb, None, None) == EINVAL
    for ph in (hip.PB_PREP, hip.PB_REDUCE):
        t, nb = rb.pb.maps[(ph, "t")]
        assert lib.urso_param_batch_run_ls(ph, 0, p(rb.pb.dev), p(t), nb, p(sq), p(st), None) == EINVAL
        assert lib.urso_param_batch_run_sq(ph, 0, p(rb.pb.dev), p(t), nb, p(sq), None) == EINVAL
    assert_untouched(sqb, "the slot buffer")
    for i, o in enumerate(rb.out):
        for k, (buf, _) in o.items():
            assert_untouched(buf, "%s of layer %d" % (k, i))


def test_param_grad_finalize_ls_elementwise():
    """urso_param_grad_finalize_ls, the per-layer loss-scaled finalisation (the stem's): with dw_raw / colsum multiplied by 2^k and
    state[INV_SCALE] = 2^-k it writes the bits and the slots of urso_param_grad_finalize_sq on the unscaled inputs, which are inside
    finalize_bounds; without slots, the bits of urso_param_grad_finalize; a NULL state is refused."""
    hip = _hip()
    K, N, ldn = 147, 64, 64
    g = torch.Generator().manual_seed(147)
    dw = torch.randn(K, ldn, generator=g); cs = torch.randn(N, generator=g) * 5
    W, b = torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    gamma, mean, var = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    ks = (hip.param_grad_finalize_ws_bytes(K, N) - 256) // (4 * N)
    nslots = hip.param_grad_finalize_sq_slots(K, N)
    fixed = [dev(t) for t in (W, b, gamma, mean, var)]

    def run(scale_k, sq, ls):
        out = {k: guarded(n) for k, n in (("gw", K * N), ("gb", N), ("ggamma", N), ("gbeta", N))}
        slots = guarded(nslots) if sq else (None, None)
        ws = torch.empty(hip.param_grad_finalize_ws_bytes(K, N) // 4 + 4, device="cuda")
        args = (K, N, ldn, dev(dw * 2.0 ** scale_k), dev(cs * 2.0 ** scale_k), fixed[0], fixed[1], fixed[2], fixed[3], fixed[4], EPS, WD, 1, 1,
                out["gw"][1], out["gb"][1], out["ggamma"][1], out["gbeta"][1], ws)
        with X.ran("finalize_mat_kernel"):
            if ls is not None:
                hip.param_grad_finalize_ls(*args, slots[1], ls)
            elif sq:
                hip.param_grad_finalize_sq(*args, slots[1])
            else:
                hip.param_grad_finalize(*args)
        for k, (buf, view) in out.items():
            assert_guard(buf, view.numel(), "finalize_ls " + k)
        if sq:
            assert_guard(slots[0], nslots, "finalize_ls slots")
        return {k: v[1] for k, v in out.items()}, slots[1]

    ref = X.finalize64(dw[:, :N], cs, W, b, gamma, mean, var, EPS, WD)
    bnd = X.finalize_bounds(ref, K, N, ldn, ks)
    base, base_slots = run(0, True, None)
    bare, _ = run(0, False, None)
    for k in (0, 7, 15):
        got, slots = run(k, True, _ls_state(k))
        for name in ref:
            X.assert_sensitive(ref[name][0], what="finalize " + name)
            check("finalize_ls " + name, got[name], ref[name][0], bnd[name], "%s scale 2^%d" % (name, k))
            bits_equal(got[name], base[name], "urso_param_grad_finalize_ls, scale 2^%d: %s" % (k, name))
        bits_equal(slots, base_slots, "urso_param_grad_finalize_ls, scale 2^%d: slots" % k)
        got, _ = run(k, False, _ls_state(k))
        for name in ref:
            bits_equal(got[name], bare[name], "urso_param_grad_finalize_ls without slots, scale 2^%d: %s" % (k, name))
    ob, out = guarded(K * N)
    ws = torch.empty(hip.param_grad_finalize_ws_bytes(K, N) // 4 + 4, device="cuda")
    p = hip.ptr
    rc = hip._lib.urso_param_grad_finalize_ls(K, N, ldn, p(dev(dw)), p(dev(cs)), p(fixed[0]), p(fixed[1]), p(fixed[2]), p(fixed[3]), p(fixed[4]), EPS, WD, 1, 1,
                                              p(out), None, None, None, p(ws), ws.numel() * 4, None, None, None)
    assert rc == EINVAL and "state" in hip.last_error()
    assert_untouched(ob, "gw")


# ===================================================================================================================== the engine's table
SMALL, CFG2 = (64, 128), (512, 640)


@pytest.mark.parametrize("dtype,train_bn,hw", [("bfloat16", False, SMALL), ("float16", False, SMALL), ("float32", False, SMALL), ("bfloat16", True, SMALL),
                                               ("bfloat16", False, CFG2)],
                         ids=["bf16", "fp16", "fp32", "bf16-batch-statistics", "bf16-512x640"])
def test_engine_prep_table_elementwise(dtype, train_bn, hw):
    """ResNet-50, 64 x 128, batch 4: after set_weights(initial_weights(randomize_bn=True)) and run_prep(), the wf / wd / biasf / scale of
    EVERY conv of the engine equal fold64 of that layer's own master tensors within fold_bounds -- a descriptor wired to another layer's
    tensor, or to the wrong BN, fails here and in no kernel-level probe.  The stem through X.stem_taps.  A projection shortcut computed
    inside another layer's launch is a member of eng.shortcut_folded (at least one in the 16-bit runs, none in fp32); where that launch is
    urso_conv_pointwise2 (Engine._fuse_entry_shortcuts) the consumer's descriptor carries bias_from and its biasf is compared with the
    shortcut as `extra`; where it is urso_conv_pair_shortcut (stage 2, Engine._fuse_pointwise_pairs) the launch takes both layers' biasf
    and each is its own layer's fold.  The two-segment kernel takes 5120 pixels or more, so at 64 x 128 no descriptor carries
    bias_from: the last case runs the preparation (nothing else) at 512 x 640, where the entry block of stage 4 does.
    Under batch statistics (TRAIN_BN None) a conv followed by BatchNorm is prepared UNFOLDED, as a plain conv + bias (its BN runs as
    its own kernels on the batch's statistics), so its reference has no BN."""
    from util import make_config
    from ursonet_amd.engine import Engine, initial_weights, BN_EPS
    hip = _hip()
    cfg = make_config(backbone="resnet50", h=hw[0], w=hw[1], batch=4, dtype=dtype)
    if train_bn:
        cfg.TRAIN_BN = None
    eng = Engine(cfg, "training", seed=3)
    assert eng.train_bn == train_bn
    Wt = initial_weights(eng.graph, seed=17, randomize_bn=True)
    eng.set_weights(Wt)
    eng.run_prep()
    torch.cuda.synchronize()
    dt = eng.dt
    by_desc = {c.desc_id: c for c in eng.convs.values() if not c.node.stem}
    folded, n_batch_bn = [], 0

    def tens(ln):
        return {k: torch.from_numpy(v) for k, v in Wt[ln].items()}

    def layer_bn(n_):
        q = tens(n_.bn) if n_.bn else None
        return (q["gamma"], q["beta"], q["moving_mean"], q["moving_variance"]) if q else None
    for name, c in eng.convs.items():
        node = c.node
        own = tens(name)
        w = own["kernel"] if own["kernel"].dim() == 4 else own["kernel"][None, None]
        b = own.get("bias") if node.bias else None
        bn = None if c.batch_bn else layer_bn(node)
        n_batch_bn += bool(c.batch_bn)
        assert tuple(w.shape[2:]) == (node.cin, c.N) and c.npad >= c.N
        extra, eflags = None, None
        if not node.stem and c.desc.bias_from:
            Sc = by_desc[c.desc.bias_from - 1]
            assert Sc.name in eng.shortcut_folded and not Sc.batch_bn
            es = tens(Sc.name)
            extra = (es.get("bias") if Sc.node.bias else None, layer_bn(Sc.node), Sc.N)
            eflags = (extra[0] is not None, extra[1] is not None)
            folded.append(name)
        ref = X.fold64(w, b, bn, BN_EPS, c.npad, extra)
        bnd = X.fold_bounds(ref, dt, b is not None, bn is not None, eflags)
        tag = "%s (%s)" % (name, dtype)
        if node.stem:
            grid = lambda t: X.stem_taps(t.permute(1, 2, 3, 0)).permute(3, 0, 1, 2).reshape(c.N, 7, 4, 8)
            check("engine wf " + DTN[dt], c.wf.reshape(c.N, 7, 4, 8), grid(ref["wf"][0]), grid(bnd["wf"]), "wf " + tag)
            assert c.wd is None
        else:
            check("engine wf " + DTN[dt], c.wf.reshape(ref["wf"][0].shape), ref["wf"][0], bnd["wf"], "wf " + tag)
            check("engine wd " + DTN[dt], c.wd.reshape(ref["wd"][0].shape), ref["wd"][0], bnd["wd"], "wd " + tag)
        check("engine biasf", c.biasf, ref["biasf"][0], bnd["biasf"], "biasf " + tag)
        check("engine scale", c.scale, ref["scale"][0], bnd["scale"], "scale " + tag)
        X.assert_sensitive(ref["wf"][0], what="fold wf " + name)
        if extra is not None:
            plain = X.fold64(w, b, bn, BN_EPS, c.npad)["biasf"][0]
            assert X.violations(c.biasf, plain, bnd["biasf"]) >= 0.9, "%s: the probe cannot see its shortcut's folded bias" % name
    assert len(eng.convs) >= 53
    if dt == hip.F32 or train_bn:
        assert not folded and not eng.shortcut_folded
    else:
        assert eng.shortcut_folded, "no projection shortcut of a 16-bit engine is computed inside another launch"
        assert folded or hw != CFG2, "no descriptor of the 512 x 640 engine carries bias_from"
    assert (n_batch_bn > 0) == train_bn
