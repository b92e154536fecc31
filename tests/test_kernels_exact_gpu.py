"""Exact-integer and rounded-once parity probes of the conv kernels (helpers: tests/exactprobe.py).

Every probe calls a kernel through the C ABI twice: with integer operands whose results are exact in the storage type
(compared BIT FOR BIT with a float64 reference, premise() proving that this is valid and assert_sensitive() that the data
can expose a wrong tap, channel or store), and with real operands pre-rounded to the storage type (every stored element
within half an ulp + the fp32 accumulation error of the float64 reference: one rounding, after the fused epilogue --
the model oracle.graph_ref.StorageRounding assumes).  Weights come from urso_conv_weight_prep without BatchNorm (scale 1,
so the folded filter is the pre-rounded one); outputs are filled with a sentinel first; a probe that forces a kernel
through an option asserts with ran() that the kernel it names actually ran."""
import math

import pytest
import torch
import torch.nn.functional as F

import exactprobe as X

pytestmark = pytest.mark.gpu

SENTINEL = -0.3125                 # exact in every storage type, never an integer result


def _hip():
    import ursonet_amd.hip as hip
    return hip


def dev(t, dt):
    return t.contiguous().to(X.tdtype(dt)).cuda()


def prep_weights(w_hwio, dt, bias):
    """urso_conv_weight_prep with bn = None: wf [N][kh][kw][C], wd [C][kh][kw][N] (flipped data-gradient filter), biasf."""
    hip = _hip()
    KH, KW, Ci, N = w_hwio.shape
    tdt = X.tdtype(dt)
    wf = torch.empty(N * KH * KW * Ci, dtype=tdt, device="cuda")
    wd = torch.empty(Ci * KH * KW * N, dtype=tdt, device="cuda")
    biasf = torch.empty(N, dtype=torch.float32, device="cuda")
    scale = torch.empty(N, dtype=torch.float32, device="cuda")
    hip.conv_weight_prep(KH, KW, Ci, N, N, dt, w_hwio.contiguous().cuda(), bias.contiguous().cuda(),
                         None, None, None, None, 1e-3, wf, wd, biasf, scale)
    return wf, wd, biasf


def full(shape, dt, v=SENTINEL):
    return torch.full(tuple(shape), v, dtype=X.tdtype(dt), device="cuda")


def _out_hw(H, W, k, s, pad, name):
    if name.endswith("tfsame"):
        return -(-H // s), -(-W // s)
    return (H + 2 * pad[0] - k) // s + 1, (W + 2 * pad[1] - k) // s + 1


def _conv64(x, w, s, pad, OH, OW):
    k = w.shape[0]
    H, W = x.shape[1:3]
    pb = max((OH - 1) * s + k - H - pad[0], 0)
    pr = max((OW - 1) * s + k - W - pad[1], 0)
    xp = F.pad(x.permute(0, 3, 1, 2), (pad[1], pr, pad[0], pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)


def _operands(shape, dt, exact, K, seed, scale=1.0, small=False, density=0.8):
    """One operand: integers planned for a K-term sum (small: a bias / residual / mask-sized integer), or real values rounded to dt."""
    if exact:
        if small:
            return X.int_operands(shape, dt, 3, density, seed)
        a, d = X.int_plan(K, dt)
        return X.int_operands(shape, dt, a, d, seed)
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale).to(X.tdtype(dt)).float()


class ConvRef(object):
    """Operands and float64 references of one conv layer: forward (+ bias + residual, ReLU), data gradient (+ add, mask of x),
    filter gradient and column sums; each with its magnitude tensor (the same operation on |operands|)."""

    def __init__(self, case, dt, exact, seed=0):
        B, H, W, Ci, N, k, s, pad, name = case
        OH, OW = _out_hw(H, W, k, s, pad, name)
        self.case, self.dt, self.exact = case, dt, exact
        self.OH, self.OW = OH, OW
        Kf, Kd = k * k * Ci, k * k * N
        self.Kf, self.Kd, self.Kw = Kf, Kd, B * OH * OW
        self.x = _operands((B, H, W, Ci), dt, exact, Kf, seed)
        self.w = _operands((k, k, Ci, N), dt, exact, Kf, seed + 1, 1 / math.sqrt(Kf))
        self.bias = _operands((N,), 0, exact, 0, seed + 2, 0.1, small=True)
        self.res = _operands((B, OH, OW, N), dt, exact, 0, seed + 3, small=True)
        self.dz = _operands((B, OH, OW, N), dt, exact, Kd, seed + 4)
        self.addt = _operands((B, H, W, Ci), dt, exact, 0, seed + 5, small=True)
        self.mk = _operands((B, H, W, Ci), dt, exact, 0, seed + 6, small=True, density=0.9)     # ReLU mask operand (exact zeros)
        d = lambda t: t.double()
        conv = lambda x, w: _conv64(x, w, s, pad, OH, OW)
        self.zc = conv(d(self.x), d(self.w))
        self.z = self.zc + d(self.bias) + d(self.res)                 # forward pre-activation with residual
        self.zn = self.zc + d(self.bias)                              # ... without
        mc = conv(d(self.x).abs(), d(self.w).abs())
        self.mz = mc + d(self.bias).abs() + d(self.res).abs()
        self.mzn = mc + d(self.bias).abs()
        xr = d(self.x).requires_grad_(True); wr = d(self.w).requires_grad_(True)
        (conv(xr, wr) * d(self.dz)).sum().backward()
        self.gx, self.gw = xr.grad, wr.grad
        xa = d(self.x).abs().requires_grad_(True); wa = d(self.w).abs().requires_grad_(True)
        (conv(xa, wa) * d(self.dz).abs()).sum().backward()
        self.mgx, self.mgw = xa.grad, wa.grad
        self.keep = (self.mk > 0).double()                            # ReLU mask of the layer input: mask > 0 (0 blocks)
        self.colsum = d(self.dz).sum(dim=(0, 1, 2))
        self.mcolsum = d(self.dz).abs().sum(dim=(0, 1, 2))

    def dgrad_last_channel_zeroed(self):
        """Data gradient (before add and mask) with the last channel of dz -- the reduction's input channel -- zeroed."""
        B, H, W, Ci, N, k, s, pad, name = self.case
        dz0 = self.dz.double().clone(); dz0[..., -1] = 0
        xr = self.x.double().requires_grad_(True)
        (_conv64(xr, self.w.double(), s, pad, self.OH, self.OW) * dz0).sum().backward()
        return xr.grad

    def last_channel_zeroed(self):
        B, H, W, Ci, N, k, s, pad, name = self.case
        x0 = self.x.double().clone(); x0[..., -1] = 0
        return _conv64(x0, self.w.double(), s, pad, self.OH, self.OW) + self.bias.double() + self.res.double()

    def check(self, got, ref, mag, K, what, out_dt=None, relu_pre=None, sens=True):
        """The probe of one stored output: exact (premise + sensitivity + bit equality) or rounded once."""
        odt = self.dt if out_dt is None else out_dt
        if self.exact:
            X.premise(odt, stored=[(what, ref)], mags=[(what, mag)])
            if sens:
                X.assert_sensitive(ref, pre64=relu_pre, what=what)
            X.assert_exact(got, ref, what)
            return 0.0
        return X.assert_rounded_once(got, ref, mag, odt, K, what)


def _record(family, r):
    """Prints |got - ref| / bound of a rounded-once probe (the bound's headroom, per family; shown with pytest -s)."""
    if r:
        print("rounded-once ratio %s %.3f" % (family, r))


def run_conv_layer(case, dt, exact, fwd_sym=None, dgrad_sym=None, residual=True, dgrad_add=True, family="igemm", wgrad=True):
    """conv_igemm forward (bias [+ residual] + ReLU), gather-form data gradient ([+ add] + mask), compact strided data gradient
    and its accumulate form (1x1 / stride 2), filter gradient + column sums -- under whatever options the caller set."""
    hip = _hip()
    R = ConvRef(case, dt, exact, seed=sum(map(ord, case[-1])) + 31 * dt)
    B, H, W, Ci, N, k, s, pad, name = case
    OH, OW = R.OH, R.OW
    wf, wd, biasf = prep_weights(R.w, dt, R.bias)
    x = dev(R.x, dt)
    # ---- forward
    g = hip.geom(B, H, W, Ci, OH, OW, N, k, k, s, s, pad[0], pad[1])
    y = full((B, OH, OW, N), dt)
    pre, mag = (R.z, R.mz) if residual else (R.zn, R.mzn)
    with (X.ran(fwd_sym) if fwd_sym else _nullctx()):
        hip.conv_igemm(g, dt, hip.EPI_RELU, x, wf, biasf, dev(R.res, dt) if residual else None, None, y)
    torch.cuda.synchronize()
    if exact:
        ref0 = R.last_channel_zeroed() - (0 if residual else R.res.double())
        X.assert_sensitive(F.relu(pre), F.relu(ref0), pre, "forward")
    _record(family, R.check(y, F.relu(pre), mag, R.Kf + 2, "forward", relu_pre=pre))
    # ---- data gradient: flipped taps, + add tensor, x 'x > 0'
    gd = hip.geom(B, OH, OW, N, H, W, Ci, k, k, 1, 1, k - 1 - pad[0], k - 1 - pad[1], s, s)
    dx = full((B, H, W, Ci), dt)
    dz, mk = dev(R.dz, dt), dev(R.mk, dt)
    add = R.addt.double() if dgrad_add else torch.zeros(1, dtype=torch.float64)
    with (X.ran(dgrad_sym) if dgrad_sym else _nullctx()):
        hip.conv_igemm(gd, dt, 0, dz, wd, None, dev(R.addt, dt) if dgrad_add else None, mk, dx)
    torch.cuda.synchronize()
    if exact:
        X.assert_sensitive((R.gx + add) * R.keep, (R.dgrad_last_channel_zeroed() + add) * R.keep, None, "data gradient")
    _record(family, R.check(dx, (R.gx + add) * R.keep, (R.mgx + add.abs()) * R.keep, R.Kd + 1, "data gradient"))
    if k == 1 and s == 2:
        # compact form (res{3,4,5}a_branch{2a,1}): GEMM over the output pixels, stored at the even pixels only
        gs = hip.geom(B, OH, OW, N, OH, OW, Ci, 1, 1, FH=H, FW=W, OSH=s, OSW=s)
        dx2 = full((B, H, W, Ci), dt)
        with (X.ran(dgrad_sym) if dgrad_sym else _nullctx()):
            hip.conv_igemm(gs, dt, 0, dz, wd, None, None, mk, dx2)
        torch.cuda.synchronize()
        first = (R.gx * R.keep)[:, ::2, ::2]
        _record(family, R.check(dx2[:, ::2, ::2], first, (R.mgx * R.keep)[:, ::2, ::2], R.Kd, "compact data gradient", sens=False))
        odd = torch.ones(H, W, dtype=torch.bool); odd[::2, ::2] = False
        assert bool((dx2.cpu()[:, odd].float() == SENTINEL).all()), "compact data gradient wrote an odd pixel"
        stored = dx2[:, ::2, ::2].double().cpu()
        with (X.ran(dgrad_sym) if dgrad_sym else _nullctx()):
            hip.conv_igemm(gs, dt, 0, dz, wd, None, dx2, mk, dx2)                 # in place: + what is stored there
        torch.cuda.synchronize()
        _record(family, R.check(dx2[:, ::2, ::2], stored + first, stored.abs() + (R.mgx * R.keep)[:, ::2, ::2], R.Kd + 1,
                                "compact data gradient, accumulate", sens=False))
        assert bool((dx2.cpu()[:, odd].float() == SENTINEL).all())
    if not wgrad:
        return R
    # ---- filter gradient (fp32) + column sums of dz
    ws = torch.empty(hip.conv_wgrad_ws_bytes(g, dt) // 4 + 16, dtype=torch.float32, device="cuda")
    dw = full((k, k, Ci, N), 0)
    cs = full((N,), 0)
    with X.ran("wgrad"):                                                        # which variant: test_wgrad_variants
        hip.conv_wgrad(g, dt, x, dz, ws, dw, cs)
    torch.cuda.synchronize()
    _record("wgrad", R.check(dw, R.gw, R.mgw, R.Kw, "filter gradient", out_dt=0, sens=False))
    _record("wgrad", R.check(cs, R.colsum, R.mcolsum, R.Kw, "column sums", out_dt=0, sens=False))
    return R


class _nullctx(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


MODES = [True, False]
MODE_IDS = ["exact", "rounded_once"]

# ---------------------------------------------------------------- generic implicit GEMM (conv_igemm.hip) and conv_pw.hip
GENERIC_CASES = [
    (3, 9, 11, 32, 160, 3, 1, (1, 1), "3x3_ragged"),
    (2, 16, 24, 128, 64, 1, 2, (0, 0), "1x1_s2"),
    (2, 16, 20, 64, 32, 3, 2, (0, 0), "3x3_s2_tfsame"),
    (2, 8, 8, 8, 24, 3, 1, (1, 1), "tinyC"),
    (2, 32, 40, 64, 256, 1, 1, (0, 0), "cap_1x1_64_256"),
]
ONLY_GENERIC = dict(pw_kernel=0, c3=0, hconv=0, bneck=0, dense=0, pair=0)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("case", GENERIC_CASES, ids=[c[-1] for c in GENERIC_CASES])
def test_igemm_kernel(case, dt, exact):
    hip = _hip()
    with hip.options(grid_cap=8 if case[-1].startswith("cap") else 0, **ONLY_GENERIC):
        run_conv_layer(case, dt, exact, "igemm_kernel", "igemm_kernel", family="igemm")


PW_CASES = [
    (2, 16, 20, 64, 256, 1, 1, (0, 0), "1x1_wideN"),
    (2, 12, 20, 64, 64, 3, 1, (1, 1), "3x3_same"),
    (2, 32, 40, 256, 64, 1, 1, (0, 0), "cap_1x1_256_64"),
]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case", PW_CASES, ids=[c[-1] for c in PW_CASES])
def test_pw_kernel(case, dt, exact):
    hip = _hip()
    opts = dict(ONLY_GENERIC, pw_kernel=2, pwx=0, grid_cap=8 if case[-1].startswith("cap") else 0)
    with hip.options(**opts):
        run_conv_layer(case, dt, exact, "pw_kernel", "pw_kernel", family="pw", wgrad=False)


# ---------------------------------------------------------------- 3x3 halo kernels (conv_halo.hip, conv_halo2.hip, stream-K)
HALO_CASES = [
    (2, 32, 40, 128, 128, 3, 1, (1, 1), "cap_3x3_128"),
    (16, 32, 40, 256, 256, 3, 1, (1, 1), "big_3x3_256"),
]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case", HALO_CASES, ids=[c[-1] for c in HALO_CASES])
def test_hconv_kernel(case, dt, exact):
    hip = _hip()
    with hip.options(hconv=2, hconv2=0, c3=0, grid_cap=8 if case[-1].startswith("cap") else 0):
        run_conv_layer(case, dt, exact, "hconv_kernel", "hconv_kernel", residual=False, dgrad_add=False, family="hconv", wgrad=False)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape", [32, 21])
@pytest.mark.parametrize("case", HALO_CASES, ids=[c[-1] for c in HALO_CASES])
def test_hconv2_kernel(case, shape, dt, exact):
    hip = _hip()
    B, H, W, Ci, N = case[:5]
    with hip.options(hconv=2, hconv2=2, hconv2_shape=shape, c3=0, grid_cap=8 if case[-1].startswith("cap") else 0):
        g = hip.geom(B, H, W, Ci, H, W, N, 3, 3, 1, 1, 1, 1)
        assert hip.conv_igemm_halo2_shape(g, dt, hip.EPI_RELU) == shape, "tile shape %d does not fit %s" % (shape, case[-1])
        run_conv_layer(case, dt, exact, "hconv2_kernel", "hconv2_kernel", residual=False, dgrad_add=False, family="hconv2", wgrad=False)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
def test_hconv_stream_k(dt, exact):
    """Stream-K hand-over (urso_conv_igemm_ws, hconv_dbg = 8): tiles cut by a run boundary are finished from fp32 partials,
    so the result is still rounded once."""
    hip = _hip()
    case = (3, 19, 23, 128, 128, 3, 1, (1, 1), "streamk_ragged")
    R = ConvRef(case, dt, exact, seed=77 + dt)
    B, H, W, Ci, N = case[:5]
    wf, wd, biasf = prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, H, W, N, 3, 3, 1, 1, 1, 1)
    ws = torch.zeros(hip.conv_igemm_halo_ws_bytes() // 4 + 16, dtype=torch.float32, device="cuda")
    ws[1024:] = float("nan")                      # the fp32 hand-over partials (conv_halo.hip: after the 4 KiB of flags)
    with hip.options(hconv=2, hconv2=0, grid_cap=24, c3=0, hconv_dbg=8):         # hconv2 (cost model) would take this shape
        assert hip.conv_igemm_halo_ok(g, dt, hip.EPI_RELU)
        y = full((B, H, W, N), dt)
        with X.ran("hconv_kernel"):
            hip.conv_igemm_ws(g, dt, hip.EPI_RELU, dev(R.x, dt), wf, biasf, None, None, y, ws)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ws[1024:]).any()), "no fp32 partial was handed over: the stream-K schedule did not engage"
        ws[1024:] = float("nan")
        ym = full((B, H, W, N), dt)
        msk = dev(R.addt, dt)
        with X.ran("hconv_kernel"):
            hip.conv_igemm_ws(g, dt, 0, dev(R.x, dt), wf, biasf, None, msk, ym, ws)
    torch.cuda.synchronize()
    assert int(ws[:1024].view(torch.int32).abs().max()) == 0, "hand-over flags not left zero"
    _record("hconv_streamk", R.check(y, F.relu(R.zn), R.mzn, R.Kf + 1, "stream-K forward", relu_pre=R.zn))
    keep = (R.addt > 0).double()
    assert bool(torch.isfinite(ws[1024:]).any()), "no fp32 partial was handed over (masked form)"
    if exact:
        X.assert_sensitive(F.relu(R.zn), F.relu(R.last_channel_zeroed() - R.res.double()), R.zn, "stream-K forward")
    _record("hconv_streamk", R.check(ym, R.zn * keep, R.mzn * keep, R.Kf + 1, "stream-K masked", sens=False))


# ---------------------------------------------------------------- register-filter 3x3 (conv_c3.hip)
C3_CASES = [
    ((2, 12, 20, 64, 64, 3, 1, (1, 1), "c3_narrow_image"), dict(c3=1), "c3_kernel"),
    ((3, 17, 45, 64, 64, 3, 1, (1, 1), "c3_ragged"), dict(c3=1, grid_cap=8), "c3_kernel"),
    # 8 x 16 tiles only where they cover more of the image than 4 x 32 tiles (c3w_best_tw): 21 x 40 (73 % vs 55 %), partial
    # tile rows and columns; 21 x 50 ties (68 %) and runs c3w_kernel on 4 x 32 tiles even with c3v = 1
    ((2, 21, 40, 128, 128, 3, 1, (1, 1), "c3v_ragged_16"), dict(c3=3, c3v=1), "c3v_kernel"),
    ((2, 21, 50, 128, 128, 3, 1, (1, 1), "c3w_ragged_halves"), dict(c3=3, c3v=0, grid_cap=8), "c3w_kernel"),
]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case,opts,sym", C3_CASES, ids=[c[0][-1] for c in C3_CASES])
def test_c3_kernels(case, opts, sym, dt, exact):
    hip = _hip()
    with hip.options(**opts):
        run_conv_layer(case, dt, exact, sym, sym, residual=False, dgrad_add=False, family=sym, wgrad=False)


# ---------------------------------------------------------------- big-tile pointwise (conv_pwx.hip)
PWX_FORMS = ["relu", "add_relu_bits", "mask_tensor", "add_maskbits", "maskbits", "add_relu"]
PWX_SHAPES = {"tiny_tails": (2, 9, 13, 128, 72, 0), "capped_multi_tile": (4, 32, 40, 256, 512, 8), "stage4_2a": (32, 32, 40, 1024, 256, 0)}


def _unpack_bits(bits, M, N):
    return ((bits.cpu().to(torch.int32).reshape(-1, 1) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(M, N)


# bit masks need N % 32 == 0 (tiny_tails: refused, test_bit_masks_refused_where_unsupported); the production-size shape runs the
# forward forms only (runtime budget)
PWX_CASES = [(sh, f) for sh in PWX_SHAPES for f in PWX_FORMS
             if not (PWX_SHAPES[sh][4] % 32 and ("bits" in f)) and not (sh == "stage4_2a" and f not in ("relu", "add_relu_bits"))]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape,form", PWX_CASES, ids=["%s-%s" % c for c in PWX_CASES])
def test_pwx_kernel(shape, form, dt, exact):
    hip = _hip()
    B, H, W, K, N, cap = PWX_SHAPES[shape]
    has_add, relu, emit = form.startswith("add"), "relu" in form, form.endswith("_bits")
    mbits, mtens = "maskbits" in form, form == "mask_tensor"
    M = B * H * W
    seed = K + N + dt + 7 * PWX_FORMS.index(form)
    x = _operands((M, K), dt, exact, K, seed)
    w = _operands((1, 1, K, N), dt, exact, K, seed + 1, 1 / math.sqrt(K))
    bias = _operands((N,), 0, exact, 0, seed + 2, 0.2, small=True)
    add = _operands((M, N), dt, exact, 0, seed + 3, small=True) if has_add else None
    wf, _, biasf = prep_weights(w, dt, bias)
    z = x.double() @ w.double().reshape(K, N)
    mag = x.double().abs() @ w.double().abs().reshape(K, N)
    if not (mbits or mtens):
        z, mag = z + bias.double(), mag + bias.double().abs()
    else:
        biasf = None                                                      # data-gradient forms carry no bias
    if add is not None:
        z, mag = z + add.double(), mag + add.double().abs()
    mask = None
    z0 = z - x[:, -1:].double() * w.double().reshape(K, N)[-1:]         # the last input channel zeroed
    ref = F.relu(z) if relu else z
    ref0 = F.relu(z0) if relu else z0
    if mbits:
        mask = X.rand_bits(M * N // 8, seed + 4)
        keep = _unpack_bits(mask, M, N).double()
        ref, mag, ref0 = ref * keep, mag * keep, ref0 * keep
        mask = mask.cuda()
    if mtens:
        mt = _operands((M, N), dt, True, 0, seed + 4, small=True)        # a tensor of exact zeros, positives and negatives
        keep = (mt > 0).double()
        ref, mag, ref0 = ref * keep, mag * keep, ref0 * keep
        mask = dev(mt, dt)
    flags = (hip.EPI_RELU if relu else 0) | (hip.EPI_EMIT_BITS if emit else 0) | (hip.EPI_MASK_BITS if mbits else 0)
    g = hip.geom(B, H, W, K, H, W, N, 1, 1)
    if exact:
        X.premise(dt, stored=[("pwx", ref)], mags=[("pwx", mag)])
        X.assert_sensitive(ref, ref0, z if relu else None, "pwx")
    for bn in (256, 128):
        y = full((B, H, W, N), dt)
        bits = torch.full((M * N // 8,), 0x55, dtype=torch.uint8, device="cuda") if emit else None
        with hip.options(pwx=2, pwx_bn=bn, pair=0, grid_cap=cap), X.ran("pwx_kernel"):
            hip.conv_igemm_ex(g, dt, flags, dev(x.reshape(B, H, W, K), dt), wf, biasf,
                              dev(add.reshape(B, H, W, N), dt) if add is not None else None, mask, y, bits)
        torch.cuda.synchronize()
        if exact:
            X.assert_exact(y.reshape(M, N), ref, "pwx bn=%d" % bn)
        else:
            _record("pwx", X.assert_rounded_once(y.reshape(M, N), ref, mag, dt, K + 2, "pwx bn=%d" % bn))
        if emit:
            got = _unpack_bits(bits, M, N)
            want = (y.reshape(M, N).cpu().float() > 0).to(torch.int32)
            assert torch.equal(got, want), "emitted ReLU bits differ from (stored output > 0) at %d elements" % int((got != want).sum())


# ---------------------------------------------------------------- dense heads (conv_dense.hip)
@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case", [(2, 512, 264, "relu"), (32, 1024, 8, "out_f32"), (32, 4096, 1024, "add_mask")],
                         ids=["batch2_ragged_N", "loc_final_padded", "dgrad_final_add_mask"])
def test_dense_kernel(case, dt, exact):
    hip = _hip()
    M, K, N, form = case
    seed = M + K + N + dt
    if exact:                                                     # few outputs: smaller sums, so that >= 1 % are exactly 0
        a, d = X.int_plan(K, dt, share=24)
        x, w = X.int_operands((M, K), dt, a, d, seed), X.int_operands((N, K), dt, a, d, seed + 1)
        x, w = X.fill_last_channel(x, seed + 5), X.fill_last_channel(w, seed + 6)
    else:
        x, w = _operands((M, K), dt, False, K, seed), _operands((N, K), dt, False, K, seed + 1, 1 / math.sqrt(K))
    bias = _operands((N,), 0, exact, 0, seed + 2, 0.3, small=True) if form in ("relu", "out_f32") else None
    add = _operands((M, N), dt, exact, 0, seed + 3, small=True) if "add" in form else None
    mt = _operands((M, N), dt, True, 0, seed + 4, small=True) if "mask" in form else None
    z = x.double() @ w.double().T
    mag = x.double().abs() @ w.double().abs().T
    if bias is not None:
        z, mag = z + bias.double(), mag + bias.double().abs()
    if add is not None:
        z, mag = z + add.double(), mag + add.double().abs()
    z0 = z - x[:, -1:].double() * w.double()[:, -1]                     # the last input channel zeroed
    ref = F.relu(z) if form == "relu" else z
    ref0 = F.relu(z0) if form == "relu" else z0
    if mt is not None:
        ref, mag, ref0 = ref * (mt > 0), mag * (mt > 0), ref0 * (mt > 0)
    out_dt = 0 if form == "out_f32" else dt
    flags = (hip.EPI_RELU if form == "relu" else 0) | (hip.EPI_OUT_F32 if form == "out_f32" else 0)
    g = hip.geom(M, 1, 1, K, 1, 1, N, 1, 1)
    y = full((M, 1, 1, N), out_dt)
    with hip.options(dense=1), X.ran("dense_kernel"):
        hip.conv_igemm(g, dt, flags, dev(x.reshape(M, 1, 1, K), dt), dev(w, dt), bias.cuda() if bias is not None else None,
                       dev(add.reshape(M, 1, 1, N), dt) if add is not None else None,
                       dev(mt.reshape(M, 1, 1, N), dt) if mt is not None else None, y)
    torch.cuda.synchronize()
    if exact:
        X.premise(out_dt, stored=[("dense", ref)], mags=[("dense", mag)])
        X.assert_sensitive(ref, ref0, z if form == "relu" else None, "dense")
        X.assert_exact(y.reshape(M, N), ref, "dense")
    else:
        _record("dense", X.assert_rounded_once(y.reshape(M, N), ref, mag, out_dt, K + 2, "dense"))


# ---------------------------------------------------------------- max-pool 3x3 / s2 / SAME with the fused ReLU mask
def _pool_ref(x):
    """float64 max-pool with the kernel's tie rule (first maximum in row-major window order wins) and its arg-max bytes."""
    B, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    xp = torch.full((B, H + 1, W + 1, C), -math.inf, dtype=torch.float64)
    xp[:, :H, :W] = x.double()
    best = torch.full((B, OH, OW, C), -math.inf, dtype=torch.float64)
    arg = torch.zeros((B, OH, OW, C), dtype=torch.int64)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]
            take = v > best
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.full_like(arg, ky * 3 + kx), arg)
    return best, arg


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("shape", [(3, 10, 20, 64), (1, 34, 70, 8)])
def test_maxpool_ties_and_relu_mask(shape, dt, exact):
    """Post-ReLU-like integers with many positive ties and zero windows: values, arg-max bytes (first maximum wins, bit 4 =
    window maximum <= 0) and the backward pass (sum of <= 4 window gradients per pixel, nothing through a window whose maximum
    is <= 0)."""
    hip = _hip()
    B, H, W, C = shape
    OH, OW = H // 2, W // 2
    seed = B + H + C + dt
    x = X.int_operands(shape, dt, 3, 0.35, seed)                  # integers in [-3, 3]: ties everywhere, all-nonpositive windows
    best, arg = _pool_ref(x)
    assert float((arg > 0).double().mean()) > 0.1 and bool(((best <= 0)).any()) and bool((best > 0).any())
    y = full((B, OH, OW, C), dt)
    am = torch.full((B, OH, OW, C), 0xEE, dtype=torch.uint8, device="cuda")
    with X.ran("maxpool_fwd_kernel"):
        hip.maxpool_fwd(B, H, W, C, dt, dev(x, dt), y, am)
    X.assert_exact(y, best, "pooled values")
    want_am = arg + 16 * (best <= 0).long()
    X.assert_exact(am.cpu().long().double(), want_am.double(), "arg-max bytes")
    dy = _operands((B, OH, OW, C), dt, exact, 4, seed + 1, small=True) if exact else _operands((B, OH, OW, C), dt, False, 0, seed + 1)
    live = (best > 0).double() * dy.double()                      # relu_mask = 1: windows with maximum <= 0 pass nothing
    ref = torch.zeros(B, H + 1, W + 1, C, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            sel = (arg == ky * 3 + kx).double()
            ref[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += sel * live
            mag[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += sel * live.abs()
    ref, mag = ref[:, :H, :W], mag[:, :H, :W]
    dx = full((B, H, W, C), dt)
    with X.ran("maxpool_bwd_kernel"):
        hip.maxpool_bwd(B, H, W, C, dt, y, dev(dy, dt), am, 1, dx)
    torch.cuda.synchronize()
    if exact:
        X.premise(dt, stored=[("dx", ref)], mags=[("dx", mag)])
        X.assert_exact(dx, ref, "pool gradient")
    else:
        _record("maxpool", X.assert_rounded_once(dx, ref, mag, dt, 4, "pool gradient"))


# ---------------------------------------------------------------- byte-row movers and input padding (exact by nature)
@pytest.mark.parametrize("shape", [(2, 6, 10, 16), (3, 34, 70, 48)])
def test_rows_subsample_expand_scatter(shape):
    hip = _hip()
    B, H, W, rb = shape
    src = X.rand_bits(B * H * W * rb, 1).reshape(B, H, W, rb)
    small = X.rand_bits(B * (H // 2) * (W // 2) * rb, 2).reshape(B, H // 2, W // 2, rb)
    sub = torch.full((B, H // 2, W // 2, rb), 0xA5, dtype=torch.uint8, device="cuda")
    with X.ran("subsample2_kernel"):
        hip.rows_subsample2(B, H, W, rb, src.cuda(), sub)
    assert torch.equal(sub.cpu(), src[:, ::2, ::2])
    exp = torch.full((B, H, W, rb), 0xA5, dtype=torch.uint8, device="cuda")
    with X.ran("expand2_kernel"):
        hip.rows_expand2(B, H, W, rb, small.cuda(), exp)
    want = torch.zeros(B, H, W, rb, dtype=torch.uint8)
    want[:, ::2, ::2] = small
    assert torch.equal(exp.cpu(), want), "rows_expand2: %d bytes wrong" % int((exp.cpu() != want).sum())
    sc = src.clone().cuda()
    with X.ran("scatter2_kernel"):
        hip.rows_scatter2(B, H, W, rb, small.cuda(), sc)
    want = src.clone()
    want[:, ::2, ::2] = small
    assert torch.equal(sc.cpu(), want), "rows_scatter2: %d bytes wrong (odd pixels must stay untouched)" % int((sc.cpu() != want).sum())


@pytest.mark.parametrize("geo", [(2, 5, 7, 3, 8, 12, 1, 2), (1, 30, 17, 3, 64, 64, 17, 0), (3, 16, 16, 1, 16, 16, 0, 0)])
def test_pad_images_u8(geo):
    hip = _hip()
    B, H, W, Cc, OH, OW, top, left = geo
    src = X.rand_bits(B * H * W * Cc, 3).reshape(B, H, W, Cc)
    dst = torch.full((B, OH, OW, Cc), 0xA5, dtype=torch.uint8, device="cuda")
    hip.pad_images_u8(B, H, W, Cc, OH, OW, top, left, src.cuda(), dst)
    torch.cuda.synchronize()
    want = F.pad(src.permute(0, 3, 1, 2), (left, OW - W - left, top, OH - H - top)).permute(0, 2, 3, 1)
    assert torch.equal(dst.cpu(), want), "pad_images_u8: %d bytes wrong" % int((dst.cpu() != want).sum())


# ---------------------------------------------------------------- weight-gradient variants of urso_conv_wgrad (fp32 out)
WGRAD_CASES = [
    ((2, 32, 40, 64, 64, 1, 1, (0, 0), "wg_1x1_64"), 0, dict(), "_Z12wgrad_kernel"),
    ((2, 32, 40, 64, 64, 1, 1, (0, 0), "wg_1x1_64"), 1, dict(wgrad_narrow=1), "wgrad_tr64_kernel"),
    ((2, 32, 40, 64, 64, 1, 1, (0, 0), "wg_1x1_64"), 1, dict(wgrad_narrow=0, wgrad_pipe=1), ("wgrad_tr_kernel", "Lb1EE")),
    ((3, 9, 11, 32, 160, 3, 1, (1, 1), "wg_3x3_ragged"), 2, dict(wgrad_pipe=0, wgrad_blocks=64), ("wgrad_tr_kernel", "Lb0EE")),
    ((2, 16, 24, 128, 64, 1, 2, (0, 0), "wg_1x1_s2"), 2, dict(wgrad_narrow=1), "wgrad_tr64_kernel"),
]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case,dt,opts,sym", WGRAD_CASES, ids=["%s-dt%d-%s" % (c[0][-1], c[1], "-".join("%s%d" % kv for kv in c[2].items()))
                                                              for c in WGRAD_CASES])
def test_wgrad_variants(case, dt, opts, sym, exact):
    """urso_conv_wgrad with each variant forced (narrow tile, pipelined fragment reads or not, the fp32 kernel; many / few splits)
    and urso_conv_wgrad_partial (the same split partials, summed here in float64): dW and the column sums."""
    hip = _hip()
    R = ConvRef(case, dt, exact, seed=sum(map(ord, case[-1])) + 5 * dt)
    B, H, W, Ci, N, k, s, pad, name = case
    g = hip.geom(B, H, W, Ci, R.OH, R.OW, N, k, k, s, s, pad[0], pad[1])
    x, dz = dev(R.x, dt), dev(R.dz, dt)
    with hip.options(c3=0, hwgrad=0, **opts):
        nbytes = hip.conv_wgrad_ws_bytes(g, dt)
        splits = hip.conv_wgrad_splits(g, dt)
        ws = torch.full((nbytes // 4 + 16,), float("nan"), dtype=torch.float32, device="cuda")
        dw, cs = full((k, k, Ci, N), 0), full((N,), 0)
        with X.ran(sym):
            hip.conv_wgrad(g, dt, x, dz, ws, dw, cs)
        torch.cuda.synchronize()
        _record("wgrad", R.check(dw, R.gw, R.mgw, R.Kw, "filter gradient", out_dt=0, sens=False))
        _record("wgrad", R.check(cs, R.colsum, R.mcolsum, R.Kw, "column sums", out_dt=0, sens=False))
        ws.fill_(float("nan"))
        with X.ran(sym):
            hip.conv_wgrad_partial(g, dt, x, dz, ws)
        torch.cuda.synchronize()
    cnt = k * k * Ci * N
    stride = cnt + hip.WGRAD_PART_PAD
    parts = ws[:splits * stride].reshape(splits, stride)[:, :cnt].double().cpu()
    assert bool(torch.isfinite(parts).all()), "a split partial was not written"
    _record("wgrad", R.check(parts.sum(0).reshape(k, k, Ci, N), R.gw, R.mgw, R.Kw, "filter gradient partials", out_dt=0, sens=False))


# ---------------------------------------------------------------- fused pointwise pairs (conv_pair.hip, conv_pairw.hip)
def _second_operand(mid64, K, dt, exact, seed, scale):
    """The second layer's filter: integers sparse enough that sums over the (integer) intermediate stay exact, or real."""
    if not exact:
        return _operands((scale[0], K), dt, False, K, seed, scale[1])
    ev = float((mid64 ** 2).mean()) or 1.0
    d = min(0.7, (X.INT_LIMIT[torch.bfloat16] / 12.0) ** 2 / (K * ev * 2.5))
    return X.fill_last_channel(X.int_operands((scale[0], K), dt, 2, d, seed), seed + 1)


def _mm(a, b):
    return a.double() @ b.double().T


PAIR_SHAPES = {"small": (3, 24, 40, 0), "capped": (2, 64, 80, 8)}


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("c", [64, 128], ids=["stage2", "stage3"])
@pytest.mark.parametrize("shape", list(PAIR_SHAPES), ids=list(PAIR_SHAPES))
def test_conv_pair(shape, c, dt, exact):
    """urso_conv_pair, forward (mode 0: mid = relu(src W1^T + b1 + add), emitted bits; dst = relu(mid W2^T + b2)) and backward
    (mode 1: mid = (src W1^T + add) * bits; dst = (mid W2^T) * (act > 0)).  mid and dst are both stored tensors, each rounded
    once (include/ursonet_hip.h: 'one rounding per stored tensor'): dst's reference is computed from the STORED mid -- the same
    rounding point StorageRounding models, every conv output being stored."""
    hip = _hip()
    B, H, W, cap = PAIR_SHAPES[shape]
    M, c4 = B * H * W, 4 * c
    seed = M + c + 11 * dt
    if exact:
        a, d = X.int_plan(c, dt, share=48)
        src, w1 = X.int_operands((M, c), dt, a, d, seed), X.int_operands((c4, c), dt, a, d, seed + 1)
    else:
        src, w1 = _operands((M, c), dt, False, c, seed), _operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    add = _operands((M, c4), dt, exact, 0, seed + 2, small=True)
    act = _operands((M, c), dt, exact, 0, seed + 3, small=True, density=0.9)
    b1 = _operands((c4,), 0, exact, 0, seed + 4, 0.3, small=True)
    b2 = _operands((c,), 0, exact, 0, seed + 5, 0.3, small=True)
    gbits = X.rand_bits(M * c4 // 8, seed + 6)
    keep1 = _unpack_bits(gbits, M, c4).double()
    for mode in (0, 1):
        if mode == 0:
            pre1, mag1 = _mm(src, w1) + b1.double() + add.double(), _mm(src.abs(), w1.abs()) + b1.double().abs() + add.double().abs()
            pre1_0 = pre1 - src[:, -1:].double() * w1.double()[:, -1]
            mid_ref, mid0 = F.relu(pre1), F.relu(pre1_0)
        else:
            pre1, mag1 = _mm(src, w1) + add.double(), _mm(src.abs(), w1.abs()) + add.double().abs()
            mid_ref, mag1 = pre1 * keep1, mag1 * keep1
            mid0 = (pre1 - src[:, -1:].double() * w1.double()[:, -1]) * keep1
        w2 = _second_operand(mid_ref, c4, dt, exact, seed + 7 + mode, (c, 1 / (2 * c ** 0.5)))
        mid = full((M, c4), dt); dst = full((M, c), dt)
        bits = torch.full((M * c4 // 8,), 0xAA, dtype=torch.uint8, device="cuda") if mode == 0 else gbits.cuda()
        with hip.options(grid_cap=cap), X.ran("pair_kernel"):
            hip.conv_pair(M, c, dt, mode, dev(src, dt), dev(w1, dt), b1.cuda() if mode == 0 else None, dev(add, dt), bits, mid,
                          dev(w2, dt), b2.cuda() if mode == 0 else None, dev(act, dt) if mode == 1 else None, dst)
        torch.cuda.synchronize()
        what = "mode %d" % mode
        if exact:
            X.premise(dt, stored=[(what + " mid", mid_ref)], mags=[(what + " mid", mag1)])
            X.assert_sensitive(mid_ref, mid0, pre1 if mode == 0 else None, what + " mid")
            X.assert_exact(mid, mid_ref, what + " mid")
        else:
            _record("pair", X.assert_rounded_once(mid, mid_ref, mag1, dt, c + 2, what + " mid"))
        m = mid.double().cpu()                                              # the second layer reads the stored mid
        if mode == 0:
            pre2, mag2 = _mm(m, w2) + b2.double(), _mm(m.abs(), w2.abs()) + b2.double().abs()
            dst_ref = F.relu(pre2)
        else:
            ka = (act > 0).double()
            pre2 = _mm(m, w2)
            dst_ref, mag2 = pre2 * ka, _mm(m.abs(), w2.abs()) * ka
        if exact:
            X.premise(dt, stored=[(what + " dst", dst_ref)], mags=[(what + " dst", mag2)])
            d0 = pre2 - m[:, -1:] * w2.double()[:, -1]
            X.assert_sensitive(dst_ref, F.relu(d0 + b2.double()) if mode == 0 else d0 * ka, pre2 + b2.double() if mode == 0 else None,
                               what + " dst")
            X.assert_exact(dst, dst_ref, what + " dst")
        else:
            _record("pair", X.assert_rounded_once(dst, dst_ref, mag2, dt, c4 + 1, what + " dst"))
        if mode == 0:
            got = _unpack_bits(bits, M, c4)
            assert torch.equal(got, (mid.cpu().float() > 0).to(torch.int32)), "emitted bits differ from (stored mid > 0)"


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape", list(PAIR_SHAPES), ids=list(PAIR_SHAPES))
def test_conv_pair_wgrad_and_dgrad_wgrad_pw(shape, dt, exact):
    """urso_conv_pair_wgrad (stage-2 backward pair + the block-closing layer's weight gradient u^T mid from the STORED mid, fp32 split
    partials) and urso_conv_dgrad_wgrad_pw (dx = dz Wd^T masked by x > 0, and the partials of x^T dz): partials summed in float64."""
    hip = _hip()
    B, H, W, cap = PAIR_SHAPES[shape]
    M, c, c4 = B * H * W, 64, 256
    seed = M + 3 * dt + 1
    if exact:
        a, d = X.int_plan(c, dt, share=48)
        src, w1 = X.int_operands((M, c), dt, a, d, seed), X.int_operands((c4, c), dt, a, d, seed + 1)
    else:
        src, w1 = _operands((M, c), dt, False, c, seed), _operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    add = _operands((M, c4), dt, exact, 0, seed + 2, small=True)
    u = _operands((M, c), dt, exact, 0, seed + 3, small=True, density=0.9)
    gbits = X.rand_bits(M * c4 // 8, seed + 4)
    keep1 = _unpack_bits(gbits, M, c4).double()
    pre1 = _mm(src, w1) + add.double()
    mid_ref = pre1 * keep1
    mag1 = (_mm(src.abs(), w1.abs()) + add.double().abs()) * keep1
    w2 = _second_operand(mid_ref, c4, dt, exact, seed + 5, (c, 1 / (2 * c ** 0.5)))
    with hip.options(grid_cap=cap):
        splits = hip.conv_pair_wgrad_splits(M, dt)
        stride = c * c4 + hip.WGRAD_PART_PAD
        part = torch.full((splits * stride,), float("nan"), device="cuda")
        colpart = torch.full((splits * c4,), float("nan"), device="cuda")
        mid, dst = full((M, c4), dt), full((M, c), dt)
        with X.ran("pairw_kernel"):
            hip.conv_pair_wgrad(M, dt, dev(src, dt), dev(w1, dt), dev(add, dt), gbits.cuda(), mid, dev(w2, dt), dev(u, dt), dst,
                                part, colpart, stride)
        torch.cuda.synchronize()
    m = mid.double().cpu()
    ka = (u > 0).double()
    dst_ref, mag2 = _mm(m, w2) * ka, _mm(m.abs(), w2.abs()) * ka
    dw_ref, dw_mag = u.double().T @ m, u.double().abs().T @ m.abs()
    cs_ref, cs_mag = m.sum(0), m.abs().sum(0)
    dw = part.reshape(splits, stride)[:, :c * c4].double().cpu().sum(0).reshape(c, c4)
    cs = colpart.reshape(splits, c4).double().cpu().sum(0)
    if exact:
        X.premise(dt, stored=[("mid", mid_ref), ("dst", dst_ref)], mags=[("mid", mag1), ("dst", mag2)])
        X.premise(0, stored=[("dW", dw_ref), ("colsum", cs_ref)], mags=[("dW", dw_mag), ("colsum", cs_mag)])
        X.assert_sensitive(mid_ref, (pre1 - src[:, -1:].double() * w1.double()[:, -1]) * keep1, None, "mid")
        for what, got, ref in (("mid", mid, mid_ref), ("dst", dst, dst_ref), ("dW", dw, dw_ref), ("colsum", cs, cs_ref)):
            X.assert_exact(got, ref, "conv_pair_wgrad " + what)
    else:
        _record("pair", X.assert_rounded_once(mid, mid_ref, mag1, dt, c + 1, "conv_pair_wgrad mid"))
        _record("pair", X.assert_rounded_once(dst, dst_ref, mag2, dt, c4, "conv_pair_wgrad dst"))
        _record("pair_wgrad", X.assert_rounded_once(dw, dw_ref, dw_mag, 0, M, "conv_pair_wgrad dW"))
        _record("pair_wgrad", X.assert_rounded_once(cs, cs_ref, cs_mag, 0, M, "conv_pair_wgrad colsum"))
    # single-layer form: dz = the stored mid, x = u, Wd = w2 [64][256]
    dx = full((M, c), dt)
    part.fill_(float("nan")); colpart.fill_(float("nan"))
    with hip.options(grid_cap=cap), X.ran("pairw_kernel"):
        hip.conv_dgrad_wgrad_pw(M, dt, mid, dev(w2, dt), dev(u, dt), 1, dx, part, colpart, stride)
    torch.cuda.synchronize()
    dw = part.reshape(splits, stride)[:, :c * c4].double().cpu().sum(0).reshape(c, c4)
    cs = colpart.reshape(splits, c4).double().cpu().sum(0)
    if exact:
        for what, got, ref in (("dx", dx, dst_ref), ("dW", dw, dw_ref), ("colsum", cs, cs_ref)):
            X.assert_exact(got, ref, "conv_dgrad_wgrad_pw " + what)
    else:
        _record("pair", X.assert_rounded_once(dx, dst_ref, mag2, dt, c4, "conv_dgrad_wgrad_pw dx"))
        _record("pair_wgrad", X.assert_rounded_once(dw, dw_ref, dw_mag, 0, M, "conv_dgrad_wgrad_pw dW"))
        _record("pair_wgrad", X.assert_rounded_once(cs, cs_ref, cs_mag, 0, M, "conv_dgrad_wgrad_pw colsum"))


# ---------------------------------------------------------------- two reduction segments (urso_conv_pointwise2, conv_pwx.hip SEG2)
@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("form", ["dgrad_bits", "forward_emit"])
@pytest.mark.parametrize("shape", [(3, 20, 24, 256, 320, 128, 16), (2, 32, 40, 256, 512, 1024, 0)], ids=["ragged_capped", "stage4_entry"])
def test_pointwise2(shape, form, dt, exact):
    """dst = mask(src0 W0^T + src1 W1^T) (data-gradient form, bit mask) and dst = relu(src0 W0^T + src1 W1^T + bias) with emitted bits
    (forward form, the shortcut inside): both segments summed in ONE fp32 accumulator, rounded once -- K = C0 + C1."""
    hip = _hip()
    B, OH, OW, C0, C1, N, cap = shape
    M = B * OH * OW
    seed = M + C0 + dt + (7 if form == "forward_emit" else 0)
    K = C0 + C1
    x0, x1 = _operands((M, C0), dt, exact, K, seed), _operands((M, C1), dt, exact, K, seed + 1)
    w0, w1 = _operands((N, C0), dt, exact, K, seed + 2, K ** -0.5), _operands((N, C1), dt, exact, K, seed + 3, K ** -0.5)
    z = _mm(x0, w0) + _mm(x1, w1)
    mag = _mm(x0.abs(), w0.abs()) + _mm(x1.abs(), w1.abs())
    z0 = z - x1[:, -1:].double() * w1.double()[:, -1]                    # the last input channel (of the second segment) zeroed
    dst = full((M, N), dt)
    if form == "dgrad_bits":
        flags, bias, bits = hip.EPI_MASK_BITS, None, X.rand_bits(M * N // 8, seed + 4)
        keep = _unpack_bits(bits, M, N).double()
        ref, mag, ref0, pre = z * keep, mag * keep, z0 * keep, None
        bits = bits.cuda()
    else:
        flags, bits = hip.EPI_RELU | hip.EPI_EMIT_BITS, torch.full((M * N // 8,), 0xAA, dtype=torch.uint8, device="cuda")
        bias = _operands((N,), 0, exact, 0, seed + 4, 0.3, small=True)
        ref, mag, ref0, pre = F.relu(z + bias.double()), mag + bias.double().abs(), F.relu(z0 + bias.double()), z + bias.double()
    with hip.options(pwx=2, grid_cap=cap):
        assert hip.conv_pointwise2_ok(B, OH, OW, C0, C1, N, dt, flags)
        with X.ran("pwx_kernel"):
            if form == "dgrad_bits":
                hip.conv_pointwise2(B, OH, OW, C0, C1, N, dt, flags, dev(x0, dt), dev(w0, dt), dev(x1, dt), dev(w1, dt), None, bits, dst)
            else:
                hip.conv_pointwise2(B, OH, OW, C0, C1, N, dt, flags, dev(x0, dt), dev(w0, dt), dev(x1, dt), dev(w1, dt), bias.cuda(), None,
                                    dst, bits)
    torch.cuda.synchronize()
    if exact:
        X.premise(dt, stored=[("pointwise2", ref)], mags=[("pointwise2", mag)])
        X.assert_sensitive(ref, ref0, pre, "pointwise2")
        X.assert_exact(dst, ref, "pointwise2 " + form)
    else:
        _record("pointwise2", X.assert_rounded_once(dst, ref, mag, dt, K + 1, "pointwise2 " + form))
    if form == "forward_emit":
        assert torch.equal(_unpack_bits(bits, M, N), (dst.cpu().float() > 0).to(torch.int32)), "emitted bits differ from (dst > 0)"
