"""Exact-integer and rounded-once parity probes of the conv kernels (helpers: tests/exactprobe.py).

Every probe calls a kernel through the C ABI twice: with integer operands whose results are exact in the storage type
(compared BIT FOR BIT with a float64 reference, premise() proving that this is valid and assert_sensitive() that the data
can expose a wrong tap, channel or store), and with real operands pre-rounded to the storage type (every stored element
within half an ulp + the fp32 accumulation error of the float64 reference: one rounding, after the fused epilogue --
the model oracle.graph_ref.StorageRounding assumes).  Weights come from urso_conv_weight_prep without BatchNorm (scale 1,
so the folded filter is the pre-rounded one); outputs are filled with a sentinel first; a probe that forces a kernel
through an option asserts with ran() that the kernel it names actually ran.

Families: the generic implicit GEMM, pointwise, halo, register-filter and big-tile pointwise kernels, the Dense head, the
max-pool, the weight-gradient variants, the fused pointwise pairs and the two-segment pointwise launch; the stem (weight
pack with a BatchNorm fold, unpooled, fused with ReLU + max-pool, weight gradient from dz and from the pool's gradient);
bottleneck_layer's forward and parity-class data gradient; the Dense heads in one launch (forward and weight gradients);
the batched weight gradients (grouped layers, two 3x3 layers in one launch, dz on a coarser grid); the launches around a stage's
first block and its end (forward pair with the projection shortcut inside, backward pair of the stage-entry block, the stage-closing
layer with its sampled second output, the compact add operand of the backward pairs) at every tiles-per-block count of their input
rings; the Winograd evaluation on integers.  The references of the larger layers are float64 on the device."""
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


def prep_weights(w_hwio, dt, bias, npad=None):
    """urso_conv_weight_prep with bn = None: wf [npad][kh][kw][C], wd [C][kh][kw][npad] (flipped data-gradient filter), biasf; filters
    N.. npad - 1 zero (npad defaults to N)."""
    hip = _hip()
    KH, KW, Ci, N = w_hwio.shape
    npad = npad or N
    tdt = X.tdtype(dt)
    wf = torch.empty(npad * KH * KW * Ci, dtype=tdt, device="cuda")
    wd = torch.empty(Ci * KH * KW * npad, dtype=tdt, device="cuda")
    biasf = torch.empty(npad, dtype=torch.float32, device="cuda")
    scale = torch.empty(npad, dtype=torch.float32, device="cuda")
    hip.conv_weight_prep(KH, KW, Ci, N, npad, dt, w_hwio.contiguous().cuda(), bias.contiguous().cuda(),
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


def run_conv_layer(case, dt, exact, fwd_sym=None, dgrad_sym=None, residual=True, dgrad_add=True, family="igemm", wgrad=True, fwd_flags=None,
                   forward_only=False):
    """conv_igemm forward (bias [+ residual] + ReLU), gather-form data gradient ([+ add] + mask), compact strided data gradient
    and its accumulate form (1x1 / stride 2), filter gradient + column sums -- under whatever options the caller set.
    fwd_flags: the forward launch's epilogue flags (default EPI_RELU); 0 is the bare conv + bias a batch-statistics BN layer
    launches (Engine._plan_conv_forward), whose reference has no ReLU.  forward_only: stop after the forward probe."""
    hip = _hip()
    fwd_flags = hip.EPI_RELU if fwd_flags is None else fwd_flags
    act = F.relu if (fwd_flags & hip.EPI_RELU) else (lambda t: t)
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
        hip.conv_igemm(g, dt, fwd_flags, x, wf, biasf, dev(R.res, dt) if residual else None, None, y)
    torch.cuda.synchronize()
    relu_pre = pre if (fwd_flags & hip.EPI_RELU) else None          # (no ReLU: no decision at zero to expose)
    if exact:
        ref0 = R.last_channel_zeroed() - (0 if residual else R.res.double())
        X.assert_sensitive(act(pre), act(ref0), relu_pre, "forward")
    _record(family, R.check(y, act(pre), mag, R.Kf + 2, "forward", relu_pre=relu_pre))
    if forward_only:
        return R
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
@pytest.mark.parametrize("kernel", ["hconv", "hconv2_32", "hconv2_21"])
@pytest.mark.parametrize("case", HALO_CASES, ids=[c[-1] for c in HALO_CASES])
def test_halo_kernels_plain(case, kernel, dt, exact):
    """flags = 0 -- bias only, no ReLU, no residual, no mask: the form in which a batch-statistics BN layer launches its conv (the raw z);
    reference zn without the ReLU."""
    hip = _hip()
    B, H, W, Ci, N = case[:5]
    cap = 8 if case[-1].startswith("cap") else 0
    if kernel == "hconv":
        opts, sym = dict(hconv=2, hconv2=0, c3=0, grid_cap=cap), "hconv_kernel"
    else:
        opts, sym = dict(hconv=2, hconv2=2, hconv2_shape=int(kernel[-2:]), c3=0, grid_cap=cap), "hconv2_kernel"
    with hip.options(**opts):
        g = hip.geom(B, H, W, Ci, H, W, N, 3, 3, 1, 1, 1, 1)
        assert hip.conv_igemm_halo_ok(g, dt, 0)
        if kernel != "hconv":
            assert hip.conv_igemm_halo2_shape(g, dt, 0) == opts["hconv2_shape"], "tile shape %s does not fit %s" % (kernel, case[-1])
        run_conv_layer(case, dt, exact, sym, residual=False, family=kernel + "_plain", fwd_flags=0, forward_only=True)


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


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
def test_hconv_stream_k_plain(dt, exact):
    """The stream-K hand-over with flags = 0 and no mask (the conv of a batch-statistics BN layer, which gets the hand-over workspace
    like a frozen layer): tiles finished from fp32 partials hold bias + sum, no ReLU, rounded once; the flags are left zero."""
    hip = _hip()
    case = (3, 19, 23, 128, 128, 3, 1, (1, 1), "streamk_ragged")
    R = ConvRef(case, dt, exact, seed=77 + dt)
    B, H, W, Ci, N = case[:5]
    wf, wd, biasf = prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, H, W, N, 3, 3, 1, 1, 1, 1)
    ws = torch.zeros(hip.conv_igemm_halo_ws_bytes() // 4 + 16, dtype=torch.float32, device="cuda")
    ws[1024:] = float("nan")
    with hip.options(hconv=2, hconv2=0, grid_cap=24, c3=0, hconv_dbg=8):
        assert hip.conv_igemm_halo_ok(g, dt, 0)
        y = full((B, H, W, N), dt)
        with X.ran("hconv_kernel"):
            hip.conv_igemm_ws(g, dt, 0, dev(R.x, dt), wf, biasf, None, None, y, ws)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws[1024:]).any()), "no fp32 partial was handed over: the stream-K schedule did not engage"
    assert int(ws[:1024].view(torch.int32).abs().max()) == 0, "hand-over flags not left zero"
    if exact:
        X.assert_sensitive(R.zn, R.last_channel_zeroed() - R.res.double(), None, "stream-K plain forward")
    _record("hconv_streamk_plain", R.check(y, R.zn, R.mzn, R.Kf + 1, "stream-K plain forward"))


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


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case,opts,sym", C3_CASES, ids=[c[0][-1] for c in C3_CASES])
def test_c3_kernels_plain(case, opts, sym, dt, exact):
    """flags = 0 (bias only: no ReLU, no residual, no mask), the launch of a batch-statistics BN layer's conv; reference zn without ReLU."""
    hip = _hip()
    with hip.options(**opts):
        run_conv_layer(case, dt, exact, sym, residual=False, family=sym + "_plain", fwd_flags=0, forward_only=True)


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
    _maxpool_case(shape, dt, exact)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
def test_maxpool_grid_stride(exact):
    """The same probe at (16, 256, 320, 64) in bf16: 2.6 M channel vectors against 8192 x 256 threads, so that both kernels' stride loops and
    the (b, tile, pixel, vector) decomposition of a large index run.  pool_loss_optim.hip, pool_blocks(): `size_t b = (total + 255) / 256;
    return (int)(b > 8192 ? 8192 : ...)` with total = B * H/2 * W/2 * C/VE, and the kernels' `i += gridDim.x * blockDim.x`."""
    B, H, W, C = shape = (16, 256, 320, 64)
    total = B * (H // 2) * (W // 2) * (C // 8)
    assert -(-total // (min((total + 255) // 256, 8192) * 256)) >= 2
    _maxpool_case(shape, 1, exact)


def _maxpool_case(shape, dt, exact):
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


@pytest.mark.parametrize("geo", [(2, 5, 7, 3, 8, 12, 1, 2), (1, 30, 17, 3, 64, 64, 17, 0), (3, 16, 16, 1, 16, 16, 0, 0),
                                 (8, 480, 640, 3, 512, 640, 16, 0), (2, 1200, 1920, 1, 1920, 1920, 360, 0)])
def test_pad_images_u8(geo):
    hip = _hip()
    B, H, W, Cc, OH, OW, top, left = geo
    # augment.hip, urso_pad_images_u8: `int bx = (int)((n + 255) / 256); if (bx > 2048) bx = 2048;` with n = OH * OW * C bytes per image, and
    # place_kernel's `i += (size_t)gridDim.x * blockDim.x`: the two frame-sized cases walk the stride loop twice and eight times
    n = OH * OW * Cc
    assert (-(-n // (min((n + 255) // 256, 2048) * 256)) >= 2) == (H >= 480)
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
    _conv_pair_case(PAIR_SHAPES[shape], c, dt, exact, compact=False)


# (B, H, W, grid_cap) of the compact-add probes: 64- / 32-pixel tiles straddle image rows (W = 40, 6) and images (H W = 240, 60: no
# multiple of a tile, the second smaller than one); (2, 24, 40) is PAIR_SHAPES["small"]'s image
COMPACT_GEOS = [(4, 6, 40, 0), (16, 10, 6, 8), (2, 24, 40, 0)]
COMPACT_IDS = ["%dx%dx%d" % g[:3] for g in COMPACT_GEOS]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("c", [64, 128], ids=["stage2", "stage3"])
@pytest.mark.parametrize("geo", COMPACT_GEOS, ids=COMPACT_IDS)
def test_conv_pair_compact_add(geo, c, dt, exact):
    """urso_conv_pair mode 1 with `add` given as the COMPACT [B][H/2][W/2][4c] gradient (add_hw = (H, W)): the same probe, against the
    float64 reference of the dense tensor with explicit zeros at the odd rows / columns (conv_pair.hip: the pixel map of the SPARSE
    loads; tests/test_exactprobe_cpu.py proves its arithmetic against divmod)."""
    _conv_pair_case(geo, c, dt, exact, compact=True)


def _conv_pair_case(geo, c, dt, exact, compact):
    hip = _hip()
    B, H, W, cap = geo
    M, c4 = B * H * W, 4 * c
    seed = M + c + 11 * dt
    if exact:
        a, d = X.int_plan(c, dt, share=48)
        src, w1 = X.int_operands((M, c), dt, a, d, seed), X.int_operands((c4, c), dt, a, d, seed + 1)
    else:
        src, w1 = _operands((M, c), dt, False, c, seed), _operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    if compact:                                                             # the kernel's operand; the reference adds the dense tensor
        add_k = _operands((B, H // 2, W // 2, c4), dt, exact, 0, seed + 2, small=True)
        add = X.compact_to_dense(add_k, H, W).reshape(M, c4)
        assert float((add != 0).float().mean()) > 0.1
    else:
        add = add_k = _operands((M, c4), dt, exact, 0, seed + 2, small=True)
    act = _operands((M, c), dt, exact, 0, seed + 3, small=True, density=0.9)
    b1 = _operands((c4,), 0, exact, 0, seed + 4, 0.3, small=True)
    b2 = _operands((c,), 0, exact, 0, seed + 5, 0.3, small=True)
    gbits = X.rand_bits(M * c4 // 8, seed + 6)
    keep1 = _unpack_bits(gbits, M, c4).double()
    for mode in ((1,) if compact else (0, 1)):                              # the forward form has no compact operand
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
            hip.conv_pair(M, c, dt, mode, dev(src, dt), dev(w1, dt), b1.cuda() if mode == 0 else None, dev(add_k, dt), bits, mid,
                          dev(w2, dt), b2.cuda() if mode == 0 else None, dev(act, dt) if mode == 1 else None, dst,
                          add_hw=(H, W) if compact else None)
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
    _conv_pair_wgrad_case(PAIR_SHAPES[shape], dt, exact, compact=False)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("geo", COMPACT_GEOS, ids=COMPACT_IDS)
def test_conv_pair_wgrad_compact_add(geo, dt, exact):
    """urso_conv_pair_wgrad with the COMPACT add operand (conv_pairw.hip's copy of the pixel map) against the float64 reference of the
    dense tensor with explicit zeros: mid, dst, the summed partials of u^T mid and the column sums."""
    _conv_pair_wgrad_case(geo, dt, exact, compact=True)


def _conv_pair_wgrad_case(geo, dt, exact, compact):
    hip = _hip()
    B, H, W, cap = geo
    M, c, c4 = B * H * W, 64, 256
    seed = M + 3 * dt + 1
    if exact:
        a, d = X.int_plan(c, dt, share=48)
        src, w1 = X.int_operands((M, c), dt, a, d, seed), X.int_operands((c4, c), dt, a, d, seed + 1)
    else:
        src, w1 = _operands((M, c), dt, False, c, seed), _operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    if compact:
        add_k = _operands((B, H // 2, W // 2, c4), dt, exact, 0, seed + 2, small=True)
        add = X.compact_to_dense(add_k, H, W).reshape(M, c4)
        assert float((add != 0).float().mean()) > 0.1
    else:
        add = add_k = _operands((M, c4), dt, exact, 0, seed + 2, small=True)
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
            hip.conv_pair_wgrad(M, dt, dev(src, dt), dev(w1, dt), dev(add_k, dt), gbits.cuda(), mid, dev(w2, dt), dev(u, dt), dst,
                                part, colpart, stride, add_hw=(H, W) if compact else None)
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
    if compact:                                                             # the single-layer form has no add operand
        return
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


# ---------------------------------------------------------------- the launches around a stage's first block (conv_pairs.hip, conv_pairx.hip)
# M = 64 ntiles under grid_cap = 8 is one block per XCD, XCD x owning tiles [x cpx, min((x + 1) cpx, ntiles)): per block
#   1: 1, then seven blocks without a tile      9: 2 2 2 2 1 0 0 0      19: 3 x 6, 1, 0      29: 4 x 7, 1      45: 6 x 7, 3
# and uncapped (45 tiles on 48 blocks) one tile or none -- every has_next / has_far pattern of the 3-stage and 2-stage input rings:
# the first tile with and without a next one, the steady state, the last two tiles of a drain.
PAIR_TILES = [(1, 8), (9, 8), (19, 8), (29, 8), (45, 8), (45, 0)]
PAIR_TILE_IDS = ["tiles%d_cap%d" % t for t in PAIR_TILES]


def _entry_tile_counts(ntiles, cap, dt):
    """Tiles per block of urso_conv_pair_wgrad_entry's launch: its grid is urso_conv_pair_wgrad_splits blocks."""
    hip = _hip()
    with hip.options(grid_cap=cap):
        splits = hip.conv_pair_wgrad_splits(64 * ntiles, dt)
    return X.tiles_per_block(ntiles, splits)


def test_pair_tile_shapes_reach_every_pipeline_phase():
    """The tile counts per block that PAIR_TILES reaches under the launch policies as they are now: {0, 1, 2, 3, 4, >= 6} for both
    kernels.  A change of the policy that shrinks this fails here instead of silently losing a prologue / steady / drain combination."""
    for name, counts in (("pairs_kernel", [X.tiles_per_block(n, X.pair_grid_blocks(n, cap)) for n, cap in PAIR_TILES]),
                         ("pairx_kernel", [_entry_tile_counts(n, cap, 1) for n, cap in PAIR_TILES])):
        seen = set(sum(counts, []))
        assert {0, 1, 2, 3, 4} <= seen and max(seen) >= 6, "%s: tiles per block reached %s" % (name, sorted(seen))
    assert _entry_tile_counts(9, 8, 1) == [2, 2, 2, 2, 1, 0, 0, 0] and _entry_tile_counts(45, 8, 2) == [6] * 7 + [3]
    assert X.pair_grid_blocks(45, 0) == 48 and sorted(set(X.tiles_per_block(45, 48))) == [0, 1]


def _differs(a, b):
    return float((a != b).sum()) / a.numel()


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("tiles", PAIR_TILES, ids=PAIR_TILE_IDS)
def test_conv_pair_shortcut(tiles, dt, exact):
    """urso_conv_pair_shortcut (pairs_kernel): mid = relu(src W1^T + xin Ws^T + (b1 + bs)) stored and rounded once -- ONE reduction of 128
    terms, the two biases added to each other in fp32 first (K = 128 + 2) -- and dst = relu(mid W2^T + b2) from the STORED mid (K = 256 + 1);
    with and without the emitted bit mask (bit for bit the same mid / dst; bits = stored mid > 0); a guard tile behind every output."""
    hip = _hip()
    ntiles, cap = tiles
    M, c, c4, G = 64 * ntiles, 64, 256, 64
    seed = 5 * M + 17 * dt + 3
    if exact:
        a, d = X.int_plan(2 * c, dt, share=48)
        src, xin = X.int_operands((M, c), dt, a, d, seed), X.int_operands((M, c), dt, a, d, seed + 1)
        w1 = X.fill_last_channel(X.int_operands((c4, c), dt, a, d, seed + 2), seed + 20)
        ws = X.fill_last_channel(X.int_operands((c4, c), dt, a, d, seed + 3), seed + 21)
    else:
        src, xin = _operands((M, c), dt, False, c, seed), _operands((M, c), dt, False, c, seed + 1)
        w1, ws = _operands((c4, c), dt, False, c, seed + 2, (2 * c) ** -0.5), _operands((c4, c), dt, False, c, seed + 3, (2 * c) ** -0.5)
    b1 = _operands((c4,), 0, exact, 0, seed + 4, 0.3, small=True)
    bs = _operands((c4,), 0, exact, 0, seed + 5, 0.3, small=True)
    b2 = _operands((c,), 0, exact, 0, seed + 6, 0.3, small=True)
    pre1, mag1 = X.pair_shortcut64(src, w1, b1, xin, ws, bs)
    mid_ref = F.relu(pre1)
    w2 = _second_operand(mid_ref, c4, dt, exact, seed + 7, (c, 1 / (2 * c ** 0.5)))
    outs = []
    with hip.options(grid_cap=cap), X.ran("pairs_kernel"):
        for emit in (True, False):
            mid, dst = full((M + G, c4), dt), full((M + G, c), dt)
            bits = torch.full(((M + G) * c4 // 8,), 0xAA, dtype=torch.uint8, device="cuda") if emit else None
            hip.conv_pair_shortcut(M, dt, dev(src, dt), dev(w1, dt), b1.cuda(), dev(xin, dt), dev(ws, dt), bs.cuda(), bits, mid,
                                   dev(w2, dt), b2.cuda(), dst)
            outs.append((mid, dst, bits))
    torch.cuda.synchronize()
    (mid, dst, bits), (mid_nb, dst_nb, _) = outs
    for name, t, v in (("mid", mid, SENTINEL), ("dst", dst, SENTINEL), ("mid (no bits)", mid_nb, SENTINEL), ("dst (no bits)", dst_nb, SENTINEL)):
        assert bool((t[M:].float() == v).all()), "%s: the guard tile behind the output was written" % name
    assert bool((bits[M * c4 // 8:] == 0xAA).all()), "bits: the guard tile behind the mask was written"
    assert torch.equal(mid, mid_nb) and torch.equal(dst, dst_nb), "the variant without a bit mask stores other values"
    mid, dst, bits = mid[:M], dst[:M], bits[:M * c4 // 8]
    if exact:
        X.premise(dt, stored=[("mid", mid_ref)], mags=[("mid", mag1)])
        X.assert_sensitive(mid_ref, F.relu(pre1 - src[:, -1:].double() * w1.double()[:, -1]), pre1, "mid (last channel of src)")
        X.assert_sensitive(mid_ref, F.relu(pre1 - xin[:, -1:].double() * ws.double()[:, -1]), pre1, "mid (last channel of xin)")
        assert _differs(F.relu(pre1 - bs.double()), mid_ref) >= 0.01, "dropping bias_s would not show"
        assert _differs(F.relu(X.pair_shortcut64(xin, w1, b1, src, ws, bs)[0]), mid_ref) >= 0.01, "swapping the segments would not show"
        X.assert_exact(mid, mid_ref, "mid")
    else:
        _record("pair_shortcut", X.assert_rounded_once(mid, mid_ref, mag1, dt, 2 * c + 2, "mid"))
    m = mid.double().cpu()                                                  # the second layer reads the stored mid
    pre2, mag2 = _mm(m, w2) + b2.double(), _mm(m.abs(), w2.abs()) + b2.double().abs()
    if exact:
        X.premise(dt, stored=[("dst", F.relu(pre2))], mags=[("dst", mag2)])
        X.assert_sensitive(F.relu(pre2), F.relu(pre2 - m[:, -1:] * w2.double()[:, -1]), pre2, "dst")
        X.assert_exact(dst, F.relu(pre2), "dst")
    else:
        _record("pair_shortcut", X.assert_rounded_once(dst, F.relu(pre2), mag2, dt, c4 + 1, "dst"))
    assert torch.equal(_unpack_bits(bits, M, c4), (mid.cpu().float() > 0).to(torch.int32)), "emitted bits differ from (stored mid > 0)"


def _relu_like(shape, dt, exact, seed):
    """A post-ReLU-like mask operand with exact zeros AND negatives (so that `> 0` is not `!= 0`): small integers of density 0.9, or real
    values of which a tenth are 0."""
    if exact:
        return X.int_operands(shape, dt, 3, 0.9, seed)
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(tuple(shape), generator=g).to(X.tdtype(dt)).float()
    return t * (torch.rand(tuple(shape), generator=g) < 0.9)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("mask_by_xin", [1, 0], ids=["dP_masked", "dP_unmasked"])
@pytest.mark.parametrize("tiles", PAIR_TILES, ids=PAIR_TILE_IDS)
def test_conv_pair_wgrad_entry(tiles, mask_by_xin, dt, exact):
    """urso_conv_pair_wgrad_entry (pairx_kernel), names as in conv_pairx.hip: mid = (G W1^T + dXb) bits never leaves LDS; stored are
    dst = (mid W2^T)(u > 0), dP = mid W3^T [(P > 0)], and per block the fp32 partials of dW2c = u^T mid, dWs = P^T mid and of the column
    sums (twice), summed here in float64.  Exact mode: the reference mid is exact and representable, so everything is bit for bit.
    Rounded once: mid is what urso_conv_pair_wgrad STORES for the same operands (itself probed against float64 here); the entry kernel's
    outputs are bounded against float64 products of that stored mid -- K = 256 for dst / dP, K = M for the partial sums -- as dst is
    referenced from the stored mid everywhere in this file.  Blocks without a tile must write zero partials."""
    hip = _hip()
    ntiles, cap = tiles
    M, c, c4 = 64 * ntiles, 64, 256
    seed = 7 * M + 13 * dt + 5
    if exact:
        a, d = X.int_plan(c, dt, share=48)
        src, w1 = X.int_operands((M, c), dt, a, d, seed), X.int_operands((c4, c), dt, a, d, seed + 1)
    else:
        src, w1 = _operands((M, c), dt, False, c, seed), _operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    add = _operands((M, c4), dt, exact, 0, seed + 2, small=True)
    u, P = _relu_like((M, c), dt, exact, seed + 3), _relu_like((M, c), dt, exact, seed + 4)
    gbits = X.rand_bits(M * c4 // 8, seed + 5)
    keep1 = _unpack_bits(gbits, M, c4).double()
    mid_ref = (_mm(src, w1) + add.double()) * keep1
    mag1 = (_mm(src.abs(), w1.abs()) + add.double().abs()) * keep1
    w2 = _second_operand(mid_ref, c4, dt, exact, seed + 6, (c, 1 / (2 * c ** 0.5)))
    w3 = _second_operand(mid_ref, c4, dt, exact, seed + 16, (c, 1 / (2 * c ** 0.5)))
    dsrc, dw1, dadd, dbits, dw2, dw3, du, dP = (dev(src, dt), dev(w1, dt), dev(add, dt), gbits.cuda(), dev(w2, dt), dev(w3, dt), dev(u, dt),
                                                dev(P, dt))
    with hip.options(grid_cap=cap):
        splits = hip.conv_pair_wgrad_splits(M, dt)
        counts = X.tiles_per_block(ntiles, splits)
        stride = c * c4 + hip.WGRAD_PART_PAD
        nan = lambda n: torch.full((n,), float("nan"), device="cuda")
        part, colpart, part_s, colpart_s = nan(splits * stride), nan(splits * c4), nan(splits * stride), nan(splits * c4)
        dst, dxin = full((M, c), dt), full((M, c), dt)
        with X.ran("pairx_kernel"):
            hip.conv_pair_wgrad_entry(M, dt, dsrc, dw1, dadd, dbits, dw2, du, dst, dw3, dP, mask_by_xin, dxin, part, colpart, part_s,
                                      colpart_s, stride)
        torch.cuda.synchronize()
        if exact:
            m = mid_ref
        else:
            mid, dst0 = full((M, c4), dt), full((M, c), dt)
            part0, colpart0 = nan(splits * stride), nan(splits * c4)
            with X.ran("pairw_kernel"):
                hip.conv_pair_wgrad(M, dt, dsrc, dw1, dadd, dbits, mid, dw2, du, dst0, part0, colpart0, stride)
            torch.cuda.synchronize()
            _record("pair_entry", X.assert_rounded_once(mid, mid_ref, mag1, dt, c + 1, "the stored mid of urso_conv_pair_wgrad"))
            m = mid.double().cpu()
    ref = X.pair_entry64(m, w2, w3, u, P, mask_by_xin)
    parts = {"dW2c": part, "dWs": part_s}
    cols = {"colsum": colpart, "colsum (shortcut)": colpart_s}
    got = {"dst": dst, "dP": dxin}
    for name, t in parts.items():
        t = t.reshape(splits, stride)[:, :c * c4].double().cpu()
        assert bool(torch.isfinite(t).all()), "%s: a split partial was not written" % name
        for blk, n in enumerate(counts):
            assert n > 0 or not bool(t[blk].any()), "%s: block %d owns no tile, its partial is not zero" % (name, blk)
        got[name] = t.sum(0).reshape(c, c4)
    for name, t in cols.items():
        t = t.reshape(splits, c4).double().cpu()
        assert bool(torch.isfinite(t).all()), "%s: a split partial was not written" % name
        for blk, n in enumerate(counts):
            assert n > 0 or not bool(t[blk].any()), "%s: block %d owns no tile, its partial is not zero" % (name, blk)
        got[name] = t.sum(0)
    ref["colsum (shortcut)"] = ref["colsum"]
    if exact:
        X.premise(dt, stored=[("mid", mid_ref), ("dst", ref["dst"][0]), ("dP", ref["dP"][0])],
                  mags=[("mid", mag1), ("dst", ref["dst"][1]), ("dP", ref["dP"][1])])
        X.premise(0, stored=[(k, ref[k][0]) for k in ("dW2c", "dWs", "colsum")], mags=[(k, ref[k][1]) for k in ("dW2c", "dWs", "colsum")])
        X.assert_sensitive(mid_ref, (_mm(src, w1) + add.double() - src[:, -1:].double() * w1.double()[:, -1]) * keep1, None, "mid")
        swapped = X.pair_entry64(m, w3, w2, P, u, mask_by_xin)                   # W2 <-> W3 and u <-> P: every reference changes
        for k in ("dst", "dP", "dW2c", "dWs"):
            assert _differs(swapped[k][0], ref[k][0]) >= 0.01, "%s: exchanging W2 / W3 and u / P would not show" % k
        if mask_by_xin:
            assert _differs(X.pair_entry64(m, w2, w3, u, P, 0)["dP"][0], ref["dP"][0]) >= 0.01, "ignoring the dP mask would not show"
        for k in ("dst", "dP", "dW2c", "dWs", "colsum", "colsum (shortcut)"):
            X.assert_exact(got[k], ref[k][0], "conv_pair_wgrad_entry " + k)
    else:
        for k in ("dst", "dP"):
            _record("pair_entry", X.assert_rounded_once(got[k], ref[k][0], ref[k][1], dt, c4, "conv_pair_wgrad_entry " + k))
        for k in ("dW2c", "dWs", "colsum", "colsum (shortcut)"):
            _record("pair_entry", X.assert_rounded_once(got[k], ref[k][0], ref[k][1], 0, M, "conv_pair_wgrad_entry " + k))


# ---------------------------------------------------------------- the stage-closing layer with its sampled second output (conv_pair.hip)
# (add, relu, emitted bits, grid_cap)
SAMPLED_FORMS = {"add_relu_bits": (True, True, True, 0), "add_relu_bits_capped": (True, True, True, 8), "relu_bits": (False, True, True, 0),
                 "add_relu": (True, True, False, 0), "add": (True, False, False, 0)}
# tiles of 64 / 32 pixels straddle image rows and images: H W = 240 is no multiple of either, 60 is smaller than a 64-pixel tile
SAMPLED_GEOS = [(8, 6, 40), (16, 10, 6)]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("form", list(SAMPLED_FORMS))
@pytest.mark.parametrize("geo", SAMPLED_GEOS, ids=["%dx%dx%d" % g for g in SAMPLED_GEOS])
@pytest.mark.parametrize("c", [64, 128, 256], ids=["stage2", "stage3", "stage4"])
def test_pointwise_sampled(c, geo, form, dt, exact):
    """urso_conv_pointwise_sampled (pair_kernel, single-layer form with the sampled copy): dst = act(src W^T + bias [+ add]) rounded once
    (K = c + 2, c + 1 without add), dst_sampled bit for bit dst[:, ::2, ::2] (the store's pixel map), bits = (stored dst > 0), a guard
    tile behind dst_sampled untouched."""
    hip = _hip()
    B, H, W = geo
    has_add, relu, emit, cap = SAMPLED_FORMS[form]
    N = 4 * c if c < 256 else 1024
    M, MS, G = B * H * W, B * (H // 2) * (W // 2), 64
    seed = c + M + 3 * dt + 7 * list(SAMPLED_FORMS).index(form)
    x = _operands((M, c), dt, exact, c, seed)
    w = _operands((N, c), dt, exact, c, seed + 1, c ** -0.5)
    bias = _operands((N,), 0, exact, 0, seed + 2, 0.2, small=True)
    add = _operands((M, N), dt, exact, 0, seed + 3, small=True) if has_add else None
    z, mag = _mm(x, w) + bias.double(), _mm(x.abs(), w.abs()) + bias.double().abs()
    if has_add:
        z, mag = z + add.double(), mag + add.double().abs()
    z0 = z - x[:, -1:].double() * w.double()[:, -1]                         # the last input channel zeroed
    ref, ref0 = (F.relu(z), F.relu(z0)) if relu else (z, z0)
    flags = (hip.EPI_RELU if relu else 0) | (hip.EPI_EMIT_BITS if emit else 0)
    g = hip.geom(B, H, W, c, H, W, N, 1, 1)
    dst, smp = full((B, H, W, N), dt), full((MS + G, N), dt)
    bits = torch.full((M * N // 8,), 0x55, dtype=torch.uint8, device="cuda") if emit else None
    with hip.options(grid_cap=cap):
        assert hip.conv_pointwise_sampled_ok(g, dt, flags, has_add)
        with X.ran("pair_kernel"):
            hip.conv_pointwise_sampled(g, dt, flags, dev(x, dt), dev(w, dt), bias.cuda(), dev(add, dt) if has_add else None, dst, bits, smp)
    torch.cuda.synchronize()
    assert bool((smp[MS:].float() == SENTINEL).all()), "the guard tile behind dst_sampled was written"
    smp = smp[:MS].reshape(B, H // 2, W // 2, N)
    if exact:
        X.premise(dt, stored=[("dst", ref)], mags=[("dst", mag)])
        X.assert_sensitive(ref, ref0, z if relu else None, "dst")
        X.assert_exact(dst.reshape(M, N), ref, "dst")
        X.assert_exact(smp, ref.reshape(B, H, W, N)[:, ::2, ::2], "dst_sampled")
    else:
        _record("pointwise_sampled", X.assert_rounded_once(dst.reshape(M, N), ref, mag, dt, c + (2 if has_add else 1), "dst"))
    want = dst[:, ::2, ::2]
    if not torch.equal(smp, want):
        X.assert_exact(smp, want.double().cpu(), "dst_sampled against dst[:, ::2, ::2]")
    if emit:
        assert torch.equal(_unpack_bits(bits, M, N), (dst.reshape(M, N).cpu().float() > 0).to(torch.int32)), "emitted bits differ from (stored dst > 0)"


# ---------------------------------------------------------------- Winograd F(2x2, 3x3), exact mode only (conv_winograd.hip)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape", [(2, 9, 15, 64, 64), (3, 17, 23, 128, 72)], ids=["c64", "odd_sizes_ragged_N"])
def test_winograd_exact(shape, dt):
    """urso_conv_winograd_fwd on integer operands with |v| <= 2: U = G g G^T is then a multiple of 1/4 with |U| <= 4.5 and V = B^T d B an
    integer with |V| <= 8 -- both exact in bf16 and f16 (premise proves it on the float64 transforms) -- and every fp32 sum is exact, so
    the output must equal the direct float64 conv BIT FOR BIT.  No rounded-once mode: on real data the transformed operands are rounded by
    design (tests/test_kernels_gpu.py keeps the normwise test)."""
    hip = _hip()
    B, H, W, C, N = shape
    seed = C + N + H + dt
    amax, d = X.int_plan(9 * C, dt)
    assert amax <= 2
    x, w = X.int_operands((B, H, W, C), dt, amax, d, seed), X.int_operands((3, 3, C, N), dt, amax, d, seed + 1)
    bias = X.int_operands((N,), None, 3, 0.8, seed + 2)
    pre = _conv64(x.double(), w.double(), 1, (1, 1), H, W) + bias.double()
    x0 = x.double().clone(); x0[..., -1] = 0
    pre0 = _conv64(x0, w.double(), 1, (1, 1), H, W) + bias.double()
    U, V = X.winograd_uv(w, x)
    assert float(U.abs().max()) <= 4.5 and float(V.abs().max()) <= 8
    X.assert_exact(X.winograd_out(U, V, H, W) + bias.double(), pre, "the float64 Winograd evaluation")
    mag = X.winograd_out(U, V, H, W, magnitude=True) + bias.double().abs()
    X.premise(dt, stored=[("U", U), ("V", V), ("y", F.relu(pre))], mags=[("y", mag)])
    X.assert_sensitive(F.relu(pre), F.relu(pre0), pre, "winograd")
    wf, _, biasf = prep_weights(w, dt, bias)
    g = hip.geom(B, H, W, C, H, W, N, 3, 3, 1, 1, 1, 1)
    ws = torch.full((hip.conv_winograd_ws_bytes(g, dt) // 4 + 16,), float("nan"), dtype=torch.float32, device="cuda")
    y = full((B, H, W, N), dt)
    with X.ran("wino_filter_kernel"):
        hip.conv_winograd_fwd(g, dt, hip.EPI_RELU, dev(x, dt), wf, biasf, y, ws)
    torch.cuda.synchronize()
    X.assert_exact(y, F.relu(pre), "winograd forward")


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


# ---------------------------------------------------------------- the stem (conv_stem.hip, conv_stemw.hip, prep.hip)
# pooled 10 x 17: partial 8 x 15 pool tiles and partial 8 x 32 conv tiles; pooled 17 x 31 on 18 tiles under grid_cap = 8: windows across
# the tile seams (stride 16 x 30, 17 x 32 conv pixels per tile), every block walks several tiles; conv grid 17 x 21: odd, the fused
# pool refuses it (unpooled path only)
STEM_CASES = [(2, 40, 68, 0, "partial_tiles"), (2, 68, 124, 8, "seams_capped"), (1, 34, 42, 0, "odd_grid")]
STEM_N = 64


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case", STEM_CASES, ids=[c[-1] for c in STEM_CASES])
def test_stem_kernels(case, dt, exact):
    """urso_stem_weight_pack with a BatchNorm fold that is exact but not the identity (scale 1 / sqrt(3 + 1) = 1/2), the unpooled stem
    (stem_kernel, bias + ReLU), the fused stem + ReLU + max-pool (stem_pool_kernel: values and arg-max bytes) and the weight gradient from
    the pool's gradient (stemw_kernel, pooled form) and from dz (urso_conv_wgrad) + urso_stem_wgrad_unpack -- against a float64 7x7 / s2 /
    pad-3 conv of the 3 real channels.  The pooled weight gradient's dz is the routed pool gradient rounded ONCE to the storage type: the
    kernel's LDS dz tile is bit for bit what urso_maxpool3x3s2_bwd writes (conv_stemw.hip)."""
    hip = _hip()
    B, H, W, cap, name = case
    N, OH, OW = STEM_N, H // 2, W // 2
    seed = H + W + 13 * dt
    if exact:
        a, d = X.int_plan(147, dt, share=24)
        x, w = X.int_operands((B, H, W, 3), dt, a, d, seed), X.int_operands((7, 7, 3, N), dt, a, d, seed + 1)
    else:
        x = _operands((B, H, W, 3), dt, False, 0, seed)
        w = 2 * _operands((7, 7, 3, N), dt, False, 0, seed + 1, 0.5 / 147 ** 0.5)     # w / 2 representable (fp16: not subnormal-cut)
    b = _operands((N,), dt, exact, 0, seed + 2, 0.3, small=True)
    beta = X.int_operands((N,), None, 3, 0.8, seed + 3) / 2            # folded bias b / 2 + beta - mean / 2: halves (exact in fp32)
    mean = X.int_operands((N,), None, 3, 0.8, seed + 4)
    x4 = torch.zeros(B, H, W, 4)
    x4[..., :3] = x                                                         # the molded input: RGB + a zero channel
    # ---- weight pack: BN with gamma 1, var 3, eps 1
    wf, biasf, scale = full((N * 224,), dt), full((N,), 0), full((N,), 0)
    hip.stem_weight_pack(N, dt, w.cuda(), b.cuda(), torch.ones(N, device="cuda"), beta.cuda(), mean.cuda(), torch.full((N,), 3.0, device="cuda"),
                         1.0, wf, biasf, scale)
    torch.cuda.synchronize()
    taps = X.stem_taps(w.double() * 0.5)
    bias64 = b.double() * 0.5 + beta.double() - mean.double() * 0.5
    X.premise(dt, stored=[("packed stem filter", taps)])
    X.premise(0, stored=[("folded stem bias", bias64)])
    X.assert_exact(scale, torch.full((N,), 0.5, dtype=torch.float64), "folded BN scale")
    X.assert_exact(wf.reshape(N, 7, 4, 8), taps.permute(3, 0, 1, 2).reshape(N, 7, 4, 8), "packed stem filter")
    X.assert_exact(biasf, bias64, "folded stem bias")
    # ---- forward, unpooled: the packed 7 x 4-pair geometry
    g = hip.geom(B, H, W // 2, 8, OH, OW, N, 7, 4, 2, 1, 3, 2)
    x4d = dev(x4, dt)
    z = X.stem_conv64(x4, taps) + bias64
    mag = X.stem_conv64(x4.abs(), taps.abs()) + bias64.abs()
    ref = F.relu(z)
    y = full((B, OH, OW, N), dt)
    with hip.options(stem=1, grid_cap=cap), X.ran("stem_kernel"):
        hip.conv_igemm(g, dt, hip.EPI_RELU, x4d, wf, biasf, None, None, y)
    torch.cuda.synchronize()
    if exact:
        x0 = x4.clone()
        x0[..., 2] = 0                                                      # the last REAL channel (channel 3 is the molded zero)
        X.premise(dt, stored=[("stem", ref)], mags=[("stem", mag)])
        X.assert_sensitive(ref, F.relu(X.stem_conv64(x0, taps) + bias64), z, "stem")
        X.assert_exact(y, ref, "stem")
    else:
        _record("stem", X.assert_rounded_once(y, ref, mag, dt, 148, "stem"))
    # ---- forward fused with ReLU + max-pool 3x3 / s2 / SAME (even grid: SAME pads the bottom and the right only)
    with hip.options(stem=1, stem_pool=1):
        pool_ok = hip.stem_conv_pool_ok(g, dt)
    assert pool_ok == (OH % 2 == 0 and OW % 2 == 0), "urso_stem_conv_pool_ok: %s for a %d x %d conv grid" % (pool_ok, OH, OW)
    ws = torch.full((hip.conv_wgrad_ws_bytes(g, dt) // 4 + 16,), float("nan"), device="cuda")
    Kw = B * OH * OW
    if pool_ok:
        PH, PW = OH // 2, OW // 2
        best, arg = _pool_ref(ref)
        pooled = full((B, PH, PW, N), dt)
        am = torch.full((B, PH, PW, N), 0xEE, dtype=torch.uint8, device="cuda")
        with hip.options(stem=1, stem_pool=1, grid_cap=cap), X.ran("stem_pool_kernel"):
            hip.stem_conv_pool(g, dt, x4d, wf, biasf, pooled, am)
        torch.cuda.synchronize()
        if exact:
            X.assert_exact(pooled, best, "fused stem + pool")
            X.assert_exact(am.cpu().double(), (arg + 16 * (best <= 0).long()).double(), "fused stem + pool arg-max bytes")
        else:          # rounding is monotone: the rounded maximum is the maximum of the rounded values (arg-max: ties, not compared)
            _record("stem_pool", X.assert_rounded_once(pooled, best, _pool_ref(mag)[0], dt, 148, "fused stem + pool"))
        dpool = _operands((B, PH, PW, N), dt, exact, 0, seed + 5, small=True)
        routed, _ = X.pool_route(dpool, am, OH, OW)
        dz = X.round_to(routed, dt)
        assert float((dz != 0).double().mean()) > 0.1
    else:
        dz = _operands((B, OH, OW, N), dt, exact, 0, seed + 5, small=True).double()
    # ---- weight gradient: packed [224][N] (pad taps included), unpacked [7][7][3][N], column sums
    gt = X.stem_wgrad64(x4, dz)
    gmag = X.stem_wgrad64(x4.abs(), dz.abs())
    cs_ref, cs_mag = dz.sum((0, 1, 2)), dz.abs().sum((0, 1, 2))

    def check(dwp, cs, what):
        dw = full((7, 7, 3, N), 0)
        hip.stem_wgrad_unpack(N, dwp, dw)
        torch.cuda.synchronize()
        for part, got, r, m in (("packed", dwp.reshape(7, 8, 4, N), gt, gmag), ("unpacked", dw, X.stem_untaps(gt), X.stem_untaps(gmag)),
                                ("column sums", cs, cs_ref, cs_mag)):
            if exact:
                X.premise(0, stored=[(part, r)], mags=[(part, m)])
                X.assert_exact(got, r, "%s %s" % (what, part))
            else:
                _record("stemw", X.assert_rounded_once(got, r, m, 0, Kw, "%s %s" % (what, part)))

    if pool_ok:
        dwp, cs = full((224 * N,), 0), full((N,), 0)
        with hip.options(stem=1, grid_cap=cap), X.ran("stemw_kernel"):
            hip.stem_wgrad_pooled(g, dt, x4d, dev(dpool, dt), am, ws, dwp, cs)
        torch.cuda.synchronize()
        check(dwp, cs, "pooled stem weight gradient")
        ws.fill_(float("nan"))
    dwp, cs = full((224 * N,), 0), full((N,), 0)
    with hip.options(stem=1, grid_cap=cap), X.ran("stemw_kernel"):
        hip.conv_wgrad(g, dt, x4d, dev(dz, dt), ws, dwp, cs)
    torch.cuda.synchronize()
    check(dwp, cs, "stem weight gradient")


# ---------------------------------------------------------------- bottleneck_layer (conv_bneck.hip, option bneck = 3)
BNECK_CASES = [(3, 16, 20, 128, 32, 0, "tfsame_small"), (32, 16, 20, 2048, 32, 0, "cfg2_full"), (2, 20, 30, 256, 32, 0, "cfg5_grid"),
               (2, 9, 11, 64, 32, 1, "odd_grid_pad1"), (2, 4, 4, 512, 32, 0, "cfg1_r18"), (2, 16, 20, 64, 24, 0, "n24")]


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("case", BNECK_CASES, ids=[c[-1] for c in BNECK_CASES])
def test_bneck_kernels(case, dt, exact):
    """3x3 / s2 / SAME (or pad 1), <= 32 filters padded to 32: the forward (bias, with and without ReLU; bneck_fwd_kernel where C % 512 == 0,
    the general kernel otherwise) with its padded output columns exactly 0, and the data gradient by parity class (bneck_dgrad_kernel: no
    mask, ReLU bit mask, mask tensor) with nonzero values in dz's padded columns, which the zero filter rows must keep out of dx.  References
    in float64 on the device."""
    hip = _hip()
    B, H, W, Ci, N, p, name = case
    npad, pad = 32, (p, p)
    OH, OW = _out_hw(H, W, 3, 2, pad, "tfsame" if p == 0 else name)
    seed = B + H + Ci + N + 3 * dt
    if exact:                                                     # 32 filters: smaller sums, so that >= 1 % of them are exactly 0
        a, d = X.int_plan(9 * Ci, dt, share=24)
        x, w = X.int_operands((B, H, W, Ci), dt, a, d, seed), X.int_operands((3, 3, N, Ci), dt, a, d, seed + 1)
        x, w = X.fill_last_channel(x, seed + 6), X.fill_last_channel(w, seed + 7).transpose(2, 3).contiguous()   # long sparse sums: see the last channel
    else:
        x, w = _operands((B, H, W, Ci), dt, False, 0, seed), _operands((3, 3, Ci, N), dt, False, 0, seed + 1, (9 * Ci) ** -0.5)
    bias = _operands((N,), 0, exact, 0, seed + 2, 0.3, small=True)
    dz = _operands((B, OH, OW, N), dt, exact, 9 * N, seed + 3)
    dzpad = X.int_operands((B, OH, OW, npad - N), dt, 3, 1.0, seed + 4)           # never 0
    mk = _operands((B, H, W, Ci), dt, exact, 0, seed + 5, small=True, density=0.9)
    wf, wd, biasf = prep_weights(w, dt, bias, npad)
    c = lambda t: t.cuda().double()
    conv = lambda a, b: _conv64(a, b, 2, pad, OH, OW)
    zc = conv(c(x), c(w))
    z, mag = zc + c(bias), conv(c(x).abs(), c(w).abs()) + c(bias).abs()
    x0 = c(x).clone()
    x0[..., -1] = 0
    z0 = conv(x0, c(w)) + c(bias)
    # ---- forward
    g = hip.geom(B, H, W, Ci, OH, OW, npad, 3, 3, 2, 2, p, p)
    ws = torch.empty(hip.conv_igemm_ws_bytes(g, dt) // 4 + 4, dtype=torch.float32, device="cuda")
    xd = dev(x, dt)
    for relu in (0, hip.EPI_RELU):
        y = full((B, OH, OW, npad), dt)
        with hip.options(bneck=3), (X.ran("bneck_fwd_kernel") if Ci % 512 == 0 else _nullctx()):
            hip.conv_igemm_ex(g, dt, relu, xd, wf, biasf, None, None, y, None, ws)
        torch.cuda.synchronize()
        X.assert_zero_columns(y, N, "bneck forward")
        ref, ref0 = (F.relu(z), F.relu(z0)) if relu else (z, z0)
        what = "bneck forward relu=%d" % bool(relu)
        if exact:
            X.premise(dt, stored=[(what, ref)], mags=[(what, mag)])
            X.assert_sensitive(ref.cpu(), ref0.cpu(), z.cpu() if relu else None, what)
            X.assert_exact(y[..., :N], ref.cpu(), what)
        else:
            _record("bneck_fwd", X.assert_rounded_once(y[..., :N], ref.cpu(), mag.cpu(), dt, 9 * Ci + 1, what))
    # ---- data gradient: dz [B, OH, OW, 32] -> dx [B, H, W, Ci], gather form with dilation 2
    xr, xa = c(x).requires_grad_(True), c(x).abs().requires_grad_(True)
    (conv(xr, c(w)) * c(dz)).sum().backward()
    (conv(xa, c(w).abs()) * c(dz).abs()).sum().backward()
    dz0 = c(dz).clone()
    dz0[..., -1] = 0                                                                # the last real filter's gradient
    x0r = c(x).requires_grad_(True)
    (conv(x0r, c(w)) * dz0).sum().backward()
    gx, mgx, gx0 = xr.grad.cpu(), xa.grad.cpu(), x0r.grad.cpu()
    gd = hip.geom(B, OH, OW, npad, H, W, Ci, 3, 3, 1, 1, 2 - p, 2 - p, 2, 2)
    dzd = dev(torch.cat([dz, dzpad], -1), dt)
    keep = (mk > 0).double()
    for mb in (0, 1, 2):                                  # no mask, ReLU bit mask, mask tensor (the destination's own activation)
        kp = keep if mb else torch.ones_like(keep)
        mask = (None, X.pack_bits(keep).cuda(), dev(mk, dt))[mb]
        dx = full((B, H, W, Ci), dt)
        with hip.options(bneck=3), X.ran("bneck_dgrad_kernel"):
            hip.conv_igemm_ex(gd, dt, hip.EPI_MASK_BITS if mb == 1 else 0, dzd, wd, None, None, mask, dx)
        torch.cuda.synchronize()
        what = "bneck data gradient mask=%s" % ("none", "bits", "tensor")[mb]
        if exact:
            X.premise(dt, stored=[(what, gx * kp)], mags=[(what, mgx * kp)])
            X.assert_sensitive(gx * kp, gx0 * kp, None, what)
            X.assert_exact(dx, gx * kp, what)
        else:
            _record("bneck_dgrad", X.assert_rounded_once(dx, gx * kp, mgx * kp, dt, 9 * N, what))


# ---------------------------------------------------------------- Dense heads in one launch (conv_dense.hip: urso_dense_multi / _wgrad_multi)
def _dense_operands(M, K, N, dt, exact, seed):
    if exact:                                                     # few outputs: smaller sums, so that >= 1 % are exactly 0
        a, d = X.int_plan(K, dt, share=24)
        x, w = X.int_operands((M, K), dt, a, d, seed), X.int_operands((N, K), dt, a, d, seed + 1)
        return X.fill_last_channel(x, seed + 5), X.fill_last_channel(w, seed + 6)
    return _operands((M, K), dt, False, K, seed), _operands((N, K), dt, False, K, seed + 1, K ** -0.5)


# (K0, K1, N, form): "relu" / "relu_shared" (bias + ReLU; _shared: the previous layer's input), "final" (fp32 output, bias, 8 outputs of
# which 6 real: zero filter rows and bias behind), "add_mask" (data gradient + add, masked), "two" (two reduction segments, no epilogue)
DENSE_LAUNCHES = {
    "four_heads": [(2560, 0, 1024, "relu"), (2560, 0, 1024, "relu_shared"), (1024, 0, 8, "final"), (4096, 0, 1024, "add_mask")],
    "short": [(1024, 0, 8, "final"), (512, 256, 264, "two"), (1024, 0, 520, "add_mask")],
    "two_segment": [(1024, 1024, 2560, "two")],
}


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M", [32, 5])
@pytest.mark.parametrize("launch", list(DENSE_LAUNCHES))
def test_dense_multi_kernel(launch, M, dt, exact):
    """hip.DenseMulti: every layer of one launch against float64.  A launch whose longest reduction is >= 2048 runs 16 waves per block,
    8 otherwise (asserted through the kernel's template argument); a two-segment layer (dZ_ori Wd_ori^T + dZ_loc Wd_loc^T) sums both
    segments in one fp32 accumulator and rounds once, K = K0 + K1."""
    hip = _hip()
    layers, checks = [], []
    for i, (K0, K1, N, form) in enumerate(DENSE_LAUNCHES[launch]):
        seed = 100 * i + M + K0 + N + dt
        x0, w0 = _dense_operands(M, K0, N, dt, exact, seed)
        if form == "final":
            w0[6:] = 0
        if form == "relu_shared":                                           # loc_dense_0 / ori_dense_0: the same input tensor
            x0 = layers[-1]["x0"]
        L = dict(x0=x0, src0=layers[-1]["src0"] if form == "relu_shared" else dev(x0, dt), wgt0=dev(w0, dt), K0=K0, N=N, M=M, flags=0)
        if form == "two":
            x1, w1 = _dense_operands(M, K1, N, dt, exact, seed + 10)
            z, mag = X.two_segment(x0, w0, x1, w1)
            z0 = z - x1[:, -1:].double() * w1.double()[:, -1]               # the last channel of the second segment zeroed
            L.update(src1=dev(x1, dt), wgt1=dev(w1, dt), K1=K1)
        else:
            z, mag = x0.double() @ w0.double().T, x0.double().abs() @ w0.double().abs().T
            z0 = z - x0[:, -1:].double() * w0.double()[:, -1]
        ref, ref0, pre = z, z0, None
        if form in ("relu", "relu_shared", "final"):
            bias = _operands((N,), 0, exact, 0, seed + 2, 0.3, small=True)
            if form == "final":
                bias[6:] = 0
            L["bias"] = bias.cuda()
            ref, ref0, mag = z + bias.double(), z0 + bias.double(), mag + bias.double().abs()
        if form.startswith("relu"):
            L["flags"] = hip.EPI_RELU
            pre, ref, ref0 = ref, F.relu(ref), F.relu(ref0)
        if form == "add_mask":
            add = _operands((M, N), dt, exact, 0, seed + 3, small=True)
            mt = _operands((M, N), dt, True, 0, seed + 4, small=True)
            keep = (mt > 0).double()
            ref, ref0, mag = (z + add.double()) * keep, (z0 + add.double()) * keep, (mag + add.double().abs()) * keep
            L.update(add=dev(add, dt), mask=dev(mt, dt))
        out_dt = 0 if form == "final" else dt
        if form == "final":
            L["flags"] = hip.EPI_OUT_F32
        L["dst"] = full((M, N), out_dt)
        layers.append(L)
        checks.append((L["dst"], ref, ref0, pre, mag, out_dt, K0 + K1 + 2, "%s layer %d (%s)" % (launch, i, form)))
    nw = "Li16EE" if max(k0 + k1 for k0, k1, _, _ in DENSE_LAUNCHES[launch]) >= 2048 else "Li8EE"
    with X.ran(("dense_multi_kernel", nw)):
        hip.DenseMulti([{k: v for k, v in L.items() if k != "x0"} for L in layers], dt).run()
    torch.cuda.synchronize()
    for dst, ref, ref0, pre, mag, out_dt, K, what in checks:
        if exact:
            X.premise(out_dt, stored=[(what, ref)], mags=[(what, mag)])
            X.assert_sensitive(ref, ref0, pre, what)
            X.assert_exact(dst, ref, what)
        else:
            _record("dense_multi", X.assert_rounded_once(dst, ref, mag, out_dt, K, what))


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("M", [32, 5])
def test_dense_wgrad_multi_kernel(M, dt, exact):
    """hip.DenseWgradMulti: dW = x^T dz (fp32) and the column sums of dz for four layers of the heads' shapes in one launch (a ragged
    2600 x 1000, the final layer's N = 8); nothing written behind K * N."""
    hip = _hip()
    layers, refs = [], []
    for i, (K, N) in enumerate([(2560, 1024), (1024, 8), (1024, 4096), (2600, 1000)]):
        seed = 10 * i + M + dt
        x, dz = _operands((M, K), dt, exact, M, seed), _operands((M, N), dt, exact, M, seed + 1)
        part, col = full((K * N + 64,), 0), full((N,), 0)
        layers.append(dict(x=dev(x, dt), dz=dev(dz, dt), part=part, colpart=col, M=M, K=K, N=N))
        refs.append((x.double().T @ dz.double(), x.double().abs().T @ dz.double().abs(), dz.double().sum(0), dz.double().abs().sum(0)))
    with X.ran("dense_wgrad_multi_kernel"):
        hip.DenseWgradMulti(layers, dt).run()
    torch.cuda.synchronize()
    for L, (rw, mw, rc, mc) in zip(layers, refs):
        K, N = L["K"], L["N"]
        what = "dense wgrad %d x %d" % (K, N)
        assert bool((L["part"][K * N:] == SENTINEL).all()), "%s: written behind K * N" % what
        for got, r, m, part in ((L["part"][:K * N].reshape(K, N), rw, mw, "dW"), (L["colpart"], rc, mc, "column sums")):
            if exact:
                X.premise(0, stored=[(what, r)], mags=[(what, m)])
                X.assert_exact(got, r, "%s %s" % (what, part))
            else:
                _record("dense_wgrad_multi", X.assert_rounded_once(got, r, m, 0, M, "%s %s" % (what, part)))


# ---------------------------------------------------------------- batched weight gradients (conv_wgrad.hip, conv_hwgrad.hip)
def _wgrad_operands(g, dt, exact, seed):
    """x [B][H][W][C] and dz [B][OH][OW][N] of a weight gradient over K = B OH OW pixels (exact: sparse integers), and the float64
    references on the device: dW, its magnitude, the column sums and theirs."""
    K = g.B * g.OH * g.OW
    x = _operands((g.B, g.H, g.W, g.C), dt, exact, K, seed)
    dz = _operands((g.B, g.OH, g.OW, g.N), dt, exact, K, seed + 1)
    xc, zc = x.cuda().double(), dz.cuda().double()
    k, s, pad = g.KH, g.SH, (g.PH, g.PW)
    r = (X.wgrad64(xc, zc, k, s, pad).cpu(), X.wgrad64(xc.abs(), zc.abs(), k, s, pad).cpu(), zc.sum((0, 1, 2)).cpu(), zc.abs().sum((0, 1, 2)).cpu())
    if exact:
        X.premise(0, stored=[("dW", r[0]), ("colsum", r[2])], mags=[("dW", r[1]), ("colsum", r[3])])
    return x, dz, r


def _check_partials(ws, splits, g, r, exact, what, K):
    """float64 sums of a layer's split partials (layout of urso_conv_wgrad_partial) and column-sum partials against the references."""
    kn = g.KH * g.KW * g.C * g.N
    stride = kn + _hip().WGRAD_PART_PAD
    part = ws[:splits * stride].reshape(splits, stride)[:, :kn].double().cpu().sum(0).reshape(g.KH, g.KW, g.C, g.N)
    col = ws[splits * stride:splits * stride + splits * g.N].reshape(splits, g.N).double().cpu().sum(0)
    for got, ref, mag, p in ((part, r[0], r[1], "dW"), (col, r[2], r[3], "column sums")):
        if exact:
            X.assert_exact(got, ref, "%s %s" % (what, p))
        else:
            _record("wgrad_batched", X.assert_rounded_once(got, ref, mag, 0, K, "%s %s" % (what, p)))


def _pw(M, C, N):
    return (1, 1, M, C, 1, M, N, 1, 1, 1, 1, 0, 0)


# the layer lists of test_grouped_weight_gradients: pointwise, strided 1x1, strided 3x3 and narrow-row 3x3 layers in one launch, ragged
# channel counts; the wide lists take wgrad_group_big_kernel under wgrad_big = 1
WG_LISTS = {
    "pair": [_pw(4096, 256, 128), _pw(4096, 128, 256)],
    "ragged_mixed_geometries": [_pw(8200, 1024, 256), _pw(8200, 256, 1024), _pw(4160, 136, 72), _pw(16384, 128, 512),
                                (4, 65, 81, 128, 33, 41, 136, 3, 3, 2, 2, 1, 1), (4, 64, 80, 256, 32, 40, 128, 1, 1, 2, 2, 0, 0),
                                (3, 40, 9, 128, 40, 9, 192, 3, 3, 1, 1, 1, 1)],
    "wide_stage4_stage5_mix": [_pw(40960, 256, 1024)] * 2 + [_pw(10240, 2048, 512), _pw(10240, 512, 2048)],
    "wide_ragged_mixed_geometries": [_pw(8200, 1024, 264), _pw(4160, 264, 520), (4, 65, 81, 256, 33, 41, 328, 3, 3, 2, 2, 1, 1),
                                     (4, 64, 80, 512, 32, 40, 256, 1, 1, 2, 2, 0, 0), (3, 40, 9, 128, 40, 9, 256, 3, 3, 1, 1, 1, 1)],
}


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("name", list(WG_LISTS))
def test_wgrad_group_kernels(name, dt, exact):
    """hip.WgradGroup: wgrad_group_kernel (wgrad_big = 0) with wgrad_ring 0 / 4 / 5 and, on the wide list, wgrad_group_big_kernel
    (wgrad_big = 1): per layer, the float64 sum of its split partials and column-sum partials against float64 x^T dz of the layer's full
    geometry; workspaces pre-filled with NaN (an unwritten split fails)."""
    hip = _hip()
    geoms = [hip.geom(*l) for l in WG_LISTS[name]]
    ops = [_wgrad_operands(g, dt, exact, 40 + 7 * i + dt) for i, g in enumerate(geoms)]
    xs, dzs = [dev(o[0], dt) for o in ops], [dev(o[1], dt) for o in ops]
    wide = name.startswith("wide")
    variants = [(0, ring, "wgrad_group_kernel") for ring in (0, 4, 5)] + ([(1, 0, "wgrad_group_big_kernel")] if wide else [])
    for big, ring, sym in variants:
        with hip.options(wgrad_big=big):
            grp = hip.WgradGroup(geoms, dt)
            assert grp.nblocks > 0
            KN = [g.KH * g.KW * g.C * g.N for g in geoms]
            wss = [torch.full((s * (kn + hip.WGRAD_PART_PAD) + s * g.N + 64,), float("nan"), device="cuda")
                   for s, kn, g in zip(grp.splits, KN, geoms)]
            grp.bind(xs, dzs, wss, "cuda")
        with hip.options(wgrad_ring=ring), X.ran(sym):
            grp.run()
        torch.cuda.synchronize()
        for i, g in enumerate(geoms):
            _check_partials(wss[i], grp.splits[i], g, ops[i][2], exact, "%s layer %d (big %d, ring %d)" % (name, i, big, ring), g.B * g.OH * g.OW)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shapes", [((4, 32, 40, 256, 256), (4, 32, 40, 256, 256)), ((4, 33, 41, 128, 128), (3, 17, 23, 256, 128)),
                                    ((8, 64, 80, 128, 128), (8, 32, 40, 256, 256))],
                         ids=["twins", "ragged_unequal", "stage3_with_stage4"])
def test_hwgrad2_kernel(shapes, dt, exact):
    """urso_conv_wgrad_partial2 (hwgrad2_kernel): two 3x3 / s1 / pad-1 weight gradients in one launch, each layer's partials against float64."""
    hip = _hip()
    gs = [hip.geom(B, H, W, C, H, W, N, 3, 3, 1, 1, 1, 1) for (B, H, W, C, N) in shapes]
    sp = hip.conv_wgrad_pair_splits(gs[0], gs[1], dt)
    assert sp is not None
    ops = [_wgrad_operands(g, dt, exact, 60 + 5 * i + dt) for i, g in enumerate(gs)]
    wss = [torch.full((s * (9 * g.C * g.N + hip.WGRAD_PART_PAD) + s * g.N + 64,), float("nan"), device="cuda") for s, g in zip(sp, gs)]
    with X.ran("hwgrad2_kernel"):
        hip.conv_wgrad_partial2(gs[0], gs[1], dt, dev(ops[0][0], dt), dev(ops[0][1], dt), wss[0], dev(ops[1][0], dt), dev(ops[1][1], dt), wss[1])
    torch.cuda.synchronize()
    for i, g in enumerate(gs):
        _check_partials(wss[i], sp[i], g, ops[i][2], exact, "hwgrad2 layer %d" % i, g.B * g.H * g.W)


@pytest.mark.parametrize("exact", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("shape", [(2, 16, 24, 64, 64, 3), (2, 32, 40, 128, 128, 3), (3, 16, 16, 64, 256, 1), (4, 128, 160, 64, 64, 3)],
                         ids=["c3x3_64", "c3x3_128", "pointwise_wide", "stage2_rows"])
def test_wgrad_coarse_grid_dz(shape, dt, exact):
    """urso_conv_wgrad with dz read on a coarser grid (FH / FW / OSH / OSW: element (2 oy, 2 ox) of a [B][H][W][N] tensor is output pixel
    (oy, ox) of the stride-2 layer) against float64 x^T dz of the COMPACT gradient; the positions between are never read (sentinel there)."""
    hip = _hip()
    B, H, W, Ci, N, k = shape
    pad = k // 2
    g = hip.geom(B, H, W, Ci, H // 2, W // 2, N, k, k, 2, 2, pad, pad, FH=H, FW=W, OSH=2, OSW=2)
    x, compact, r = _wgrad_operands(hip.geom(B, H, W, Ci, H // 2, W // 2, N, k, k, 2, 2, pad, pad), dt, exact, sum(shape) + dt)
    dense = full((B, H, W, N), dt)
    dense[:, ::2, ::2] = dev(compact, dt)
    ws = torch.full((hip.conv_wgrad_ws_bytes(g, dt) // 4 + 64,), float("nan"), device="cuda")
    dw, cs = full((k, k, Ci, N), 0), full((N,), 0)
    with X.ran("wgrad"):
        hip.conv_wgrad(g, dt, dev(x, dt), dense, ws, dw, cs)
    torch.cuda.synchronize()
    for got, ref, mag, p in ((dw, r[0], r[1], "dW"), (cs, r[2], r[3], "column sums")):
        if exact:
            X.assert_exact(got, ref, "coarse-grid dz " + p)
        else:
            _record("wgrad_coarse", X.assert_rounded_once(got, ref, mag, 0, B * (H // 2) * (W // 2), "coarse-grid dz " + p))
