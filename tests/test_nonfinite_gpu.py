"""NaN / inf propagation, kernel by kernel and through the Engine (contract and checker: tests/nonfinite.py; DESIGN.md "Non-finite values").

Kernel level: the operands are the real, pre-rounded operands of the rounded-once probes (tests/test_kernels_exact_gpu.py: ConvRef with
exact = False; the integer probes hold zeros on purpose and would break premise 1), the case tables, option sets and helpers are that
module's.  One element of an operand is replaced by each of the four poisons; several poisons share a launch where their dependency sets
are disjoint, which is asserted on the structural sets (which outputs read the element at all) -- and their union must be the dependency
set of the float64 pre-activation.  Forward: an input element, a residual element and an fp32 bias element, with ReLU and with flags = 0;
fp16 once more per family with operands scaled until the store overflows.  Backward: one interior dz element.

Engine level (ResNet-18, 64 x 128, batch 3, frozen BN): a NaN pixel through inference against oracle.graph_ref's forward, an fp16
forward overflow planted in a stage-3 kernel, and fp16 training under LOSS_SCALE = "dynamic" (the step with the NaN pixel is skipped)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exactprobe as X
import nonfinite as NF
import test_kernels_exact_gpu as TK
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

RELU, PLAIN = "relu", "plain"
OTHER_SENTINEL = 0.4375            # prefill of the poisoned launch (the clean one: TK.SENTINEL): an element neither launch writes differs
DT_IDS = {0: "fp32", 1: "bf16", 2: "fp16"}


def _hip():
    import ursonet_amd.hip as hip
    return hip


@functools.lru_cache(maxsize=None)
def _ref(case, dt):
    """The operands and float64 references of the rounded-once probe of `case` (computed once, shared, never modified)."""
    return TK.ConvRef(case, dt, False, seed=sum(map(ord, case[-1])) + 31 * dt)


def _stored(t, dt):
    """The host operand in its storage type (where a poison is written as a bit pattern)."""
    return t.contiguous().to(X.tdtype(dt))


def _corners(n, B, H, W, k, s):
    """n interior positions (b, y, x): every window that holds the element lies inside the image; on the strided grid; spread over the
    images first, then over two opposite corners, so that the windows of two of them never meet."""
    lo = -(-(k - 1) // s) * s
    hi_y, hi_x = ((H - 1 - (k - 1) - (s - 1)) // s) * s, ((W - 1 - (k - 1) - (s - 1)) // s) * s
    assert hi_y >= lo and hi_x >= lo, "no interior position"
    out = []
    for i in range(n):
        corner = (i // B) % 2
        out.append((i % B, hi_y if corner else lo, hi_x if corner else lo))
    assert len(set(out)) == n, "not enough room for %d poisons" % n
    return out


def _touched_fwd(case, R, pos):
    """Structural dependency of an input element: the output pixels whose window holds it (all filters)."""
    B, H, W, Ci, N, k, s, pad, _ = case
    ind = torch.zeros(B, H, W, 1, dtype=torch.float64)
    ind[pos] = 1
    t = TK._conv64(ind, torch.ones(k, k, 1, 1, dtype=torch.float64), s, pad, R.OH, R.OW) > 0
    return t.expand(B, R.OH, R.OW, N)


def _touched_bwd(case, R, pos):
    """Structural dependency of a dz element in the data gradient: the input pixels whose windows it belongs to (all channels)."""
    B, H, W, Ci, N, k, s, pad, _ = case
    xr = torch.zeros(B, H, W, 1, dtype=torch.float64, requires_grad=True)
    ind = torch.zeros(B, R.OH, R.OW, 1, dtype=torch.float64)
    ind[pos] = 1
    (TK._conv64(xr, torch.ones(k, k, 1, 1, dtype=torch.float64), s, pad, R.OH, R.OW) * ind).sum().backward()
    return (xr.grad > 0).expand(B, H, W, Ci)


def _gx64(case, R, dz64):
    """float64 data gradient of the layer for the output gradient dz64 (plain sums: a NaN reaches the windows of its pixel only)."""
    B, H, W, Ci, N, k, s, pad, _ = case
    xr = R.x.double().requires_grad_(True)
    return torch.autograd.grad((TK._conv64(xr, R.w.double(), s, pad, R.OH, R.OW) * dz64).sum(), xr)[0]


def _igemm(hip, g, dt, flags, src, wgt, bias, add, mask, dst, ws=None):
    if ws is None:
        hip.conv_igemm(g, dt, flags, src, wgt, bias, add, mask, dst)
    else:
        hip.conv_igemm_ws(g, dt, flags, src, wgt, bias, add, mask, dst, ws)


def _igemm_ex(hip, g, dt, flags, src, wgt, bias, add, mask, dst, ws=None):
    hip.conv_igemm_ex(g, dt, flags, src, wgt, bias, add, mask, dst, None)


def forward_parity(case, dt, mode, residual, sym, launch=_igemm, ws=None, after=None):
    """Forward launch of `case` (bias [+ residual], ReLU or flags = 0) on clean operands, with the four poisons in four input elements,
    and with four poisoned fp32 bias elements [and four poisoned residual elements in other channels].  ws(): a fresh workspace per
    launch; after(ws): a check of it.  Returns the ConvRef."""
    hip = _hip()
    R = _ref(case, dt)
    B, H, W, Ci, N, k, s, pad, name = case
    OH, OW = R.OH, R.OW
    flags = hip.EPI_RELU if mode == RELU else 0
    act = torch.relu if mode == RELU else (lambda t: t)
    wf, _, biasf = TK.prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, OH, OW, N, k, k, s, s, pad[0], pad[1])
    xs, rs = _stored(R.x, dt), _stored(R.res, dt)
    w64 = R.w.double()

    def run(x, bias, res, fill=OTHER_SENTINEL):
        y = TK.full((B, OH, OW, N), dt, fill)
        wsp = ws() if ws else None
        with X.ran(sym):
            launch(hip, g, dt, flags, x.cuda(), wf, bias, res.cuda() if residual else None, None, y, wsp)
        torch.cuda.synchronize()
        if after:
            after(wsp)
        return y.cpu()

    def pre64(x, bias, res):
        z = (R.zc if x is xs else TK._conv64(x.double(), w64, s, pad, OH, OW)) + bias.double().cpu()
        return z + res.double() if residual else z

    y_clean = run(xs, biasf, rs, TK.SENTINEL)
    pre_clean = R.z if residual else R.zn
    # ---- four poisoned input elements
    xp, touched = xs, []
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, H, W, k, s))):
        c = (3 * i + 1) % Ci
        NF.premise_nonzero(R.w[:, :, c, :], "%s: filter taps of input channel %d" % (name, c))
        xp = NF.put(xp, (b, y, x, c), pname)
        touched.append(_touched_fwd(case, R, (b, y, x)))
    NF.assert_disjoint(touched, name + " input poisons")
    pre_p = pre64(xp, biasf, rs)
    assert torch.equal(NF.dependency(pre_clean, pre_p), functools.reduce(torch.logical_or, touched)), "dependency set is not the windows' union"
    NF.assert_class_parity(run(xp, biasf, rs), y_clean, act(pre_p), NF.dependency(act(pre_clean), act(pre_p)), "%s %s input" % (name, mode))
    # ---- four poisoned bias elements, and four residual elements in other channels
    bp, rp, touched = biasf.clone(), rs, []
    for i, pname in enumerate(NF.POISON_NAMES):
        n = (5 * i + 1) % N
        bp = NF.put(bp, n, pname)
        t = torch.zeros(B, OH, OW, N, dtype=torch.bool); t[..., n] = True
        touched.append(t)
        if residual:
            at = (i % B, (i * 3 + 1) % OH, (i * 5 + 2) % OW, (5 * i + 3) % N)
            rp = NF.put(rp, at, pname)
            t = torch.zeros(B, OH, OW, N, dtype=torch.bool); t[at] = True
            touched.append(t)
    NF.assert_disjoint(touched, name + " bias and residual poisons")
    pre_p = pre64(xs, bp, rp)
    assert torch.equal(NF.dependency(pre_clean, pre_p), functools.reduce(torch.logical_or, touched))
    NF.assert_class_parity(run(xs, bp, rp), y_clean, act(pre_p), NF.dependency(act(pre_clean), act(pre_p)),
                           "%s %s bias%s" % (name, mode, " + residual" if residual else ""))
    return R


def store_overflow(case, dt, residual, sym, launch=_igemm, ws=None):
    """fp16, ReLU: x * 2**13 and w * 2**4 (both still fp16 values) put the pre-activations of a large share of the elements beyond
    +-65504; the positive ones are stored as +inf (the cast of torch), the negative ones are the ReLU's 0."""
    assert dt == 2
    hip = _hip()
    R = _ref(case, dt)
    B, H, W, Ci, N, k, s, pad, name = case
    x, w = R.x * 2.0 ** 13, R.w * 2.0 ** 4
    assert torch.equal(x.half().float(), x) and torch.equal(w.half().float(), w), "scaled operands are no fp16 values"
    wf, _, biasf = TK.prep_weights(w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, R.OH, R.OW, N, k, k, s, s, pad[0], pad[1])
    y = TK.full((B, R.OH, R.OW, N), dt)
    with X.ran(sym):
        launch(hip, g, dt, hip.EPI_RELU, TK.dev(x, dt), wf, biasf, TK.dev(R.res, dt) if residual else None, None, y, ws() if ws else None)
    torch.cuda.synchronize()
    pre = TK._conv64(x.double(), w.double(), s, pad, R.OH, R.OW) + R.bias.double()
    if residual:
        pre = pre + R.res.double()
    NF.assert_store_overflow(y, torch.relu(pre), torch.float16, name + " store overflow")
    neg = pre < -2 * 65504.0
    assert bool(neg.any()) and bool((y.cpu()[neg] == 0).all()), "ReLU of an overflowing negative pre-activation is not 0"


def dgrad_parity(case, dt, add, sym, launch=_igemm):
    """Gather-form data gradient (flipped filter, [+ add], x (mask > 0)) with the four poisons in four interior dz elements; for a
    1x1 / stride-2 layer the compact form as well (stored at the even pixels only)."""
    hip = _hip()
    R = _ref(case, dt)
    B, H, W, Ci, N, k, s, pad, name = case
    OH, OW = R.OH, R.OW
    _, wd, _ = TK.prep_weights(R.w, dt, R.bias)
    gd = hip.geom(B, OH, OW, N, H, W, Ci, k, k, 1, 1, k - 1 - pad[0], k - 1 - pad[1], s, s)
    dzs, mk = _stored(R.dz, dt), TK.dev(R.mk, dt)
    addd = TK.dev(R.addt, dt) if add else None
    add64 = R.addt.double() if add else torch.zeros(1, dtype=torch.float64)
    keep = R.mk > 0
    zero = torch.zeros(1, dtype=torch.float64)

    def run(dz, geom=gd, fill=OTHER_SENTINEL):
        dx = TK.full((B, H, W, Ci), dt, fill)
        with X.ran(sym):
            launch(hip, geom, dt, 0, dz.cuda(), wd, None, addd if geom is gd else None, mk, dx)
        torch.cuda.synchronize()
        return dx.cpu()

    dzp, touched = dzs, []
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, OH, OW, -(-k // s), 1))):
        n = (3 * i + 1) % N
        NF.premise_nonzero(R.w[:, :, :, n], "%s: filter taps of output channel %d" % (name, n))
        dzp = NF.put(dzp, (b, y, x, n), pname)
        touched.append(_touched_bwd(case, R, (b, y, x)))
    NF.assert_disjoint(touched, name + " dz poisons")
    gx, gx_p = _gx64(case, R, dzs.double()), _gx64(case, R, dzp.double())
    assert torch.equal(NF.dependency(gx, gx_p), functools.reduce(torch.logical_or, touched)), "dependency set is not the windows' union"
    ref_clean, ref_p = torch.where(keep, gx + add64, zero), torch.where(keep, gx_p + add64, zero)
    NF.assert_class_parity(run(dzp), run(dzs, fill=TK.SENTINEL), ref_p, NF.dependency(ref_clean, ref_p), name + " data gradient")
    if k == 1 and s == 2:
        gs = hip.geom(B, OH, OW, N, OH, OW, Ci, 1, 1, FH=H, FW=W, OSH=s, OSW=s)
        even = torch.zeros(B, H, W, Ci, dtype=torch.bool); even[:, ::2, ::2] = True
        sent = torch.full((1,), TK.SENTINEL, dtype=torch.float64)
        c_clean, c_p = torch.where(even, torch.where(keep, gx, zero), sent), torch.where(even, torch.where(keep, gx_p, zero), sent)
        NF.assert_class_parity(run(dzp, gs, TK.SENTINEL), run(dzs, gs, TK.SENTINEL), c_p, NF.dependency(c_clean, c_p), name + " compact data gradient")


# ====================================================================================================== forward and data gradient
def _by_name(cases, name):
    return next(c for c in cases if c[-1] == name)


IGEMM = [_by_name(TK.GENERIC_CASES, n) for n in ("3x3_ragged", "tinyC", "1x1_s2")]      # coalesced, scalar (N % 8), strided epilogues


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case", IGEMM, ids=[c[-1] for c in IGEMM])
def test_igemm_forward(case, dt, mode):
    with _hip().options(**TK.ONLY_GENERIC):
        forward_parity(case, dt, mode, True, "igemm_kernel")
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, True, "igemm_kernel")


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_igemm_fp32_out(dt):
    """EPI_OUT_F32 (the head layers' store): the poisoned fp32 outputs, and no 16-bit rounding on the way."""
    hip = _hip()
    case = _by_name(TK.GENERIC_CASES, "tinyC")
    R = _ref(case, dt)
    B, H, W, Ci, N, k, s, pad, name = case
    wf, _, biasf = TK.prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, R.OH, R.OW, N, k, k, s, s, pad[0], pad[1])
    xs = _stored(R.x, dt)

    def run(x, bias):
        y = TK.full((B, R.OH, R.OW, N), 0)
        with hip.options(**TK.ONLY_GENERIC), X.ran("igemm_kernel"):
            hip.conv_igemm(g, dt, hip.EPI_OUT_F32, x.cuda(), wf, bias, None, None, y)
        torch.cuda.synchronize()
        return y.cpu()
    xp, touched = xs, []
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, H, W, k, s))):
        NF.premise_nonzero(R.w[:, :, i, :], "filter taps")
        xp = NF.put(xp, (b, y, x, i), pname)
        touched.append(_touched_fwd(case, R, (b, y, x)))
    NF.assert_disjoint(touched)
    pre_p = TK._conv64(xp.double(), R.w.double(), s, pad, R.OH, R.OW) + R.bias.double()
    y_clean = run(xs, biasf)
    NF.assert_class_parity(run(xp, biasf), y_clean, pre_p, NF.dependency(R.zn, pre_p), "fp32-out forward")
    bp = biasf.clone()
    for i, pname in enumerate(NF.POISON_NAMES):
        bp = NF.put(bp, 5 * i + 1, pname)
    pre_p = R.zc + bp.double().cpu()
    NF.assert_class_parity(run(xs, bp), y_clean, pre_p, NF.dependency(R.zn, pre_p), "fp32-out forward, bias")


@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case", IGEMM, ids=[c[-1] for c in IGEMM])
def test_igemm_dgrad(case, dt):
    with _hip().options(**TK.ONLY_GENERIC):
        dgrad_parity(case, dt, True, "igemm_kernel")


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_splitk_finish(dt, mode):
    """3x3_s2_tfsame has 2 output tiles and >= 9 K-tiles: plan_splitk cuts K when the launch gets a workspace (asserted: the library
    asks for one and writes fp32 partials into it); bias, residual and ReLU then happen in splitk_finish_kernel."""
    hip = _hip()
    case = _by_name(TK.GENERIC_CASES, "3x3_s2_tfsame")
    B, H, W, Ci, N, k, s, pad, name = case
    R = _ref(case, dt)
    with hip.options(**TK.ONLY_GENERIC):
        g = hip.geom(B, H, W, Ci, R.OH, R.OW, N, k, k, s, s, pad[0], pad[1])
        nbytes = hip.conv_igemm_ws_bytes(g, dt)
        assert nbytes > 0, "this case no longer splits K: choose another"
        mark = 3.0e7

        def ws():
            return torch.full((nbytes // 4,), mark, dtype=torch.float32, device="cuda")

        def after(w):
            assert not bool((w == mark).any()), "the split-K partials were not all written: K was not split as planned"
        forward_parity(case, dt, mode, True, "igemm_kernel", ws=ws, after=after)
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, True, "igemm_kernel", ws=ws)


PW = [_by_name(TK.PW_CASES, n) for n in ("1x1_wideN", "3x3_same")]
PW_OPTS = dict(TK.ONLY_GENERIC, pw_kernel=2, pwx=0)


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case", PW, ids=[c[-1] for c in PW])
def test_pw_forward(case, dt, mode):
    with _hip().options(**PW_OPTS):
        forward_parity(case, dt, mode, True, "pw_kernel")
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, True, "pw_kernel")


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case", PW, ids=[c[-1] for c in PW])
def test_pw_dgrad(case, dt):
    with _hip().options(**PW_OPTS):
        dgrad_parity(case, dt, True, "pw_kernel")


HALO = _by_name(TK.HALO_CASES, "cap_3x3_128")
HALO_KERNELS = {"hconv": (dict(hconv=2, hconv2=0, c3=0, grid_cap=8), "hconv_kernel"),
                "hconv2_32": (dict(hconv=2, hconv2=2, hconv2_shape=32, c3=0, grid_cap=8), "hconv2_kernel"),
                "hconv2_21": (dict(hconv=2, hconv2=2, hconv2_shape=21, c3=0, grid_cap=8), "hconv2_kernel")}


def _halo_options(kernel, dt, flags):
    hip = _hip()
    opts, sym = HALO_KERNELS[kernel]
    B, H, W, Ci, N = HALO[:5]
    g = hip.geom(B, H, W, Ci, H, W, N, 3, 3, 1, 1, 1, 1)
    with hip.options(**opts):
        assert hip.conv_igemm_halo_ok(g, dt, flags)
        if "hconv2_shape" in opts:
            assert hip.conv_igemm_halo2_shape(g, dt, flags) == opts["hconv2_shape"]
    return opts, sym


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("kernel", list(HALO_KERNELS))
def test_halo_forward(kernel, dt, mode):
    hip = _hip()
    opts, sym = _halo_options(kernel, dt, hip.EPI_RELU if mode == RELU else 0)
    with hip.options(**opts):
        forward_parity(HALO, dt, mode, False, sym)
        if dt == 2 and mode == RELU:
            store_overflow(HALO, dt, False, sym)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("kernel", list(HALO_KERNELS))
def test_halo_dgrad(kernel, dt):
    hip = _hip()
    opts, sym = HALO_KERNELS[kernel]
    with hip.options(**opts):
        dgrad_parity(HALO, dt, False, sym)


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_stream_k_handover(dt, mode):
    """streamk_ragged under hconv_dbg = 8: tiles cut by a run boundary are finished from fp32 partials in the workspace, poisoned ones too."""
    hip = _hip()
    case = (3, 19, 23, 128, 128, 3, 1, (1, 1), "streamk_ragged")

    def ws():
        w = torch.zeros(hip.conv_igemm_halo_ws_bytes() // 4 + 16, dtype=torch.float32, device="cuda")
        w[1024:] = 3.0e7
        return w

    def after(w):
        assert bool((w[1024:] != 3.0e7).any()), "no fp32 partial was handed over: the stream-K schedule did not engage"
        assert int(w[:1024].view(torch.int32).abs().max()) == 0, "hand-over flags not left zero"
    with hip.options(hconv=2, hconv2=0, grid_cap=24, c3=0, hconv_dbg=8):
        forward_parity(case, dt, mode, False, "hconv_kernel", ws=ws, after=after)
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, False, "hconv_kernel", ws=ws)


def _c3_smallest():
    """The smallest case of test_c3_kernels per kernel."""
    best = {}
    for case, opts, sym in TK.C3_CASES:
        size = case[0] * case[1] * case[2] * case[3] * case[4]
        if sym not in best or size < best[sym][0]:
            best[sym] = (size, case, opts)
    return [(case, opts, sym) for sym, (_, case, opts) in sorted(best.items())]


C3 = _c3_smallest()


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case,opts,sym", C3, ids=[c[2] for c in C3])
def test_c3_forward(case, opts, sym, dt, mode):
    with _hip().options(**opts):
        forward_parity(case, dt, mode, False, sym)
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, False, sym)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
@pytest.mark.parametrize("case,opts,sym", C3, ids=[c[2] for c in C3])
def test_c3_dgrad(case, opts, sym, dt):
    with _hip().options(**opts):
        dgrad_parity(case, dt, False, sym)


def _pwx_case():
    name = min(TK.PWX_SHAPES, key=lambda n: math.prod(TK.PWX_SHAPES[n][:5]))
    B, H, W, K, N, cap = TK.PWX_SHAPES[name]
    return (B, H, W, K, N, 1, 1, (0, 0), "pwx_" + name), cap


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("bn", [256, 128])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_pwx_forward(dt, bn, mode):
    case, cap = _pwx_case()
    with _hip().options(pwx=2, pwx_bn=bn, pair=0, grid_cap=cap):
        forward_parity(case, dt, mode, True, "pwx_kernel", launch=_igemm_ex)
        if dt == 2 and mode == RELU:
            store_overflow(case, dt, True, "pwx_kernel", launch=_igemm_ex)


@pytest.mark.parametrize("bn", [256, 128])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_pwx_dgrad(dt, bn):
    """The mask_tensor form of test_pwx_kernel (no bias, no add, x (mask > 0)) as the data gradient of the 72 -> 128 layer: dz [M][128] times
    the flipped filter [72][128] is the shape's K = 128, N = 72 product."""
    (B, H, W, K, N), cap = _pwx_case()[0][:5], _pwx_case()[1]
    case = (B, H, W, N, K, 1, 1, (0, 0), "pwx_dgrad")
    with _hip().options(pwx=2, pwx_bn=bn, pair=0, grid_cap=cap):
        dgrad_parity(case, dt, False, "pwx_kernel", launch=_igemm_ex)


DENSE_FWD = (4, 1, 1, 512, 264, 1, 1, (0, 0), "dense_batch4_ragged_N")      # test_dense_kernel's relu form; a row per poison
DENSE_BWD = (32, 1, 1, 1024, 4096, 1, 1, (0, 0), "dense_dgrad_final")        # dz [32][4096] x wd [1024][4096]: test_dense_kernel's add_mask form


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_dense_forward(dt, mode):
    with _hip().options(dense=1):
        forward_parity(DENSE_FWD, dt, mode, False, "dense_kernel")
        if dt == 2 and mode == RELU:
            store_overflow(DENSE_FWD, dt, False, "dense_kernel")


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_dense_dgrad(dt):
    with _hip().options(dense=1):
        dgrad_parity(DENSE_BWD, dt, True, "dense_kernel")


BNECK = (2, 16, 20, 512, 32, 3, 2, (0, 0), "bneck_512_tfsame")        # C % 512 == 0: bneck_fwd_kernel (test_bneck_kernels' geometry, 32 filters)


def _bneck_launch(hip, g, dt, flags, src, wgt, bias, add, mask, dst, ws=None):
    hip.conv_igemm_ex(g, dt, flags, src, wgt, bias, add, mask, dst, None, ws)


@pytest.mark.parametrize("mode", [RELU, PLAIN])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_bneck_forward(dt, mode):
    hip = _hip()
    B, H, W, Ci, N = BNECK[:5]
    with hip.options(bneck=3):
        g = hip.geom(B, H, W, Ci, H // 2, W // 2, N, 3, 3, 2, 2, 0, 0)
        ws = lambda: torch.empty(hip.conv_igemm_ws_bytes(g, dt) // 4 + 4, dtype=torch.float32, device="cuda")
        forward_parity(BNECK, dt, mode, False, "bneck_fwd_kernel", launch=_bneck_launch, ws=ws)
        if dt == 2 and mode == RELU:
            store_overflow(BNECK, dt, False, "bneck_fwd_kernel", launch=_bneck_launch, ws=ws)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_bneck_dgrad(dt):
    """The data gradient by parity class (bneck_dgrad_kernel) with the mask tensor."""
    with _hip().options(bneck=3):
        dgrad_parity(BNECK, dt, False, "bneck_dgrad_kernel", launch=_igemm_ex)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_dense_multi(dt):
    """hip.DenseMulti, the four_heads launch of test_dense_multi_kernel at M = 5: bias + ReLU twice on a shared input, the fp32 final layer
    (6 real outputs: the zero filter rows behind them multiply the poison by 0 and are left out) and the masked data gradient with its add.
    The four poisons in four rows of every layer's input; then in four bias elements of every layer that has a bias; fp16: the store
    overflow of the 16-bit layers with x * 2**13 and w * 2**4."""
    hip = _hip()
    M = 5
    zero = torch.zeros(1, dtype=torch.float64)
    L = []
    for i, (K0, K1, N, form) in enumerate(TK.DENSE_LAUNCHES["four_heads"]):
        seed = 100 * i + M + K0 + N + dt
        x0, w0 = TK._dense_operands(M, K0, N, dt, False, seed)
        bias = add = mt = None
        if form == "final":
            w0[6:] = 0
        if form in ("relu", "relu_shared", "final"):
            bias = TK._operands((N,), 0, False, 0, seed + 2, 0.3)
            if form == "final":
                bias[6:] = 0
        if form == "add_mask":
            add, mt = TK._operands((M, N), dt, False, 0, seed + 3), TK._operands((M, N), dt, True, 0, seed + 4, small=True)
        shared = form == "relu_shared"
        L.append(dict(form=form, K0=K0, N=N, n=6 if form == "final" else N, odt=0 if form == "final" else dt, x=L[-1]["x"] if shared else x0,
                      w=w0, bias=bias, add=add, mt=mt, flags=hip.EPI_RELU if form.startswith("relu") else hip.EPI_OUT_F32 if form == "final" else 0))

    def ref64(l, x, bias, w):
        z = x.double() @ w.double().T
        if bias is not None:
            z = z + bias.double()
        if l["form"].startswith("relu"):
            z = torch.relu(z)
        if l["add"] is not None:
            z = torch.where(l["mt"] > 0, z + l["add"].double(), zero)
        return z[:, :l["n"]]

    def run(xs, biases, ws, fill):
        dsts = [TK.full((M, l["N"]), l["odt"], fill) for l in L]
        launch = []
        for l, x, bias, w, d in zip(L, xs, biases, ws, dsts):
            src = launch[-1]["src0"] if l["form"] == "relu_shared" else x.cuda()
            launch.append(dict(src0=src, wgt0=TK.dev(w, dt), K0=l["K0"], N=l["N"], M=M, flags=l["flags"], dst=d, bias=bias.cuda() if bias is not None else None,
                               add=TK.dev(l["add"], dt) if l["add"] is not None else None, mask=TK.dev(l["mt"], dt) if l["mt"] is not None else None))
        with X.ran(("dense_multi_kernel", "Li16EE")):
            hip.DenseMulti(launch, dt).run()
        torch.cuda.synchronize()
        return [d.cpu()[:, :l["n"]] for d, l in zip(dsts, L)]
    xs, biases, ws = [_stored(l["x"], dt) for l in L], [l["bias"] for l in L], [l["w"] for l in L]
    clean = run(xs, biases, ws, TK.SENTINEL)
    # ---- poisoned inputs (the shared input once)
    xp = []
    for l, x in zip(L, xs):
        if l["form"] == "relu_shared":
            xp.append(xp[-1])
            continue
        for j, pname in enumerate(NF.POISON_NAMES):
            NF.premise_nonzero(l["w"][:l["n"], 11 * j + 3], "dense filter column")
            x = NF.put(x, (j, 11 * j + 3), pname)
        xp.append(x)
    for j in range(4):
        NF.premise_nonzero(L[1]["w"][:, 11 * j + 3], "dense filter column (shared input)")
    got = run(xp, biases, ws, OTHER_SENTINEL)
    for l, c, g_, x0, x1, bias, w in zip(L, clean, got, xs, xp, biases, ws):
        rc, rp = ref64(l, x0, bias, w), ref64(l, x1, bias, w)
        NF.assert_class_parity(g_, c, rp, NF.dependency(rc, rp), "dense multi, %s, input" % l["form"])
    # ---- poisoned biases
    bp = []
    for l, bias in zip(L, biases):
        if bias is not None:
            for j, pname in enumerate(NF.POISON_NAMES):
                bias = NF.put(bias, j + 1, pname)                 # (the final layer has 6 real outputs)
        bp.append(bias)
    got = run(xs, bp, ws, OTHER_SENTINEL)
    for l, c, g_, x0, b0, b1, w in zip(L, clean, got, xs, biases, bp, ws):
        if b0 is None:
            assert torch.equal(NF._bits(g_), NF._bits(c)), "a layer without a bias changed"
            continue
        rc, rp = ref64(l, x0, b0, w), ref64(l, x0, b1, w)
        NF.assert_class_parity(g_, c, rp, NF.dependency(rc, rp), "dense multi, %s, bias" % l["form"])
    # ---- store overflow of the 16-bit layers
    if dt == 2:
        xo, wo = [_stored(l["x"] * 2.0 ** 13, dt) for l in L], [l["w"] * 2.0 ** 4 for l in L]
        assert all(bool(torch.isfinite(x).all()) for x in xo) and all(torch.equal(w.half().float(), w) for w in wo)
        got = run(xo, biases, wo, OTHER_SENTINEL)
        for l, g_, x, bias, w in zip(L, got, xo, biases, wo):
            if l["odt"] == 2:
                NF.assert_store_overflow(g_, ref64(l, x, bias, w), torch.float16, "dense multi, %s, store overflow" % l["form"])


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_emitted_relu_bits_of_a_stored_nan_are_clear(dt):
    """EPI_EMIT_BITS: bit = (stored output > 0), so a stored NaN sets none, +inf sets one, the ReLU's 0 of -inf none (pinned as it is)."""
    hip = _hip()
    case = _by_name(TK.PW_CASES, "1x1_wideN")
    R = _ref(case, dt)
    B, H, W, Ci, N, k, s, pad, name = case
    M = B * H * W
    wf, _, biasf = TK.prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, Ci, H, W, N, 1, 1)
    xp = _stored(R.x, dt)
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, H, W, 1, 1))):
        NF.premise_nonzero(R.w[:, :, i, :], "filter taps")
        xp = NF.put(xp, (b, y, x, i), pname)
    y = TK.full((B, H, W, N), dt)
    bits = torch.full((M * N // 8,), 0x55, dtype=torch.uint8, device="cuda")
    with hip.options(**TK.ONLY_GENERIC), X.ran("igemm_kernel"):
        hip.conv_igemm_ex(g, dt, hip.EPI_RELU | hip.EPI_EMIT_BITS, xp.cuda(), wf, biasf, None, None, y, bits)
    torch.cuda.synchronize()
    yc = y.cpu().reshape(M, N)
    cls = NF.classes(yc)
    assert int((cls == NF.NAN).sum()) == 2 * N and int((cls == NF.PINF).sum()) > 0
    got = TK._unpack_bits(bits, M, N)
    assert torch.equal(got, (yc.float() > 0).to(torch.int32)), "emitted ReLU bits differ from (stored output > 0)"
    assert int(got[cls == NF.NAN].sum()) == 0 and bool((got[cls == NF.PINF] == 1).all())


# ====================================================================================================== fused pointwise pairs
def _pair_checks(what, run, mid64, dst64, clean_in, poisoned_in, M, c4, mid_changes=True):
    """Two stored tensors per launch: mid against its float64 reference, dst against the float64 second layer of the STORED mid (the
    rounding point of test_conv_pair).  run(inputs, fill) -> (mid, dst, bits or None) on the host; mid64(*inputs), dst64(stored mid,
    *inputs).  mid_changes = False: the poison sits behind mid (the second bias), which then keeps every bit."""
    mid_c, dst_c, _ = run(clean_in, TK.SENTINEL)
    mid_p, dst_p, bits = run(poisoned_in, OTHER_SENTINEL)
    if mid_changes:
        rc, rp = mid64(*clean_in), mid64(*poisoned_in)
        NF.assert_class_parity(mid_p, mid_c, rp, NF.dependency(rc, rp), what + " mid")
    else:
        assert torch.equal(NF._bits(mid_p), NF._bits(mid_c)), what + ": mid changed"
    dc, dp = dst64(mid_c.double(), *clean_in), dst64(mid_p.double(), *poisoned_in)
    # a -inf that the first ReLU turned into 0 changes its row of dst by a finite amount: second-hand dependents, finite on both sides,
    # with no class to compare and no bits to keep; they are taken out (and must be finite)
    dep = NF.dependency(dc, dp)
    second_hand = dep & torch.isfinite(dp) & (dp != 0)
    assert bool(torch.isfinite(dst_p[second_hand].float()).all())
    NF.assert_class_parity(torch.where(second_hand, dst_c, dst_p), dst_c, dp, dep & ~second_hand, what + " dst")
    if bits is not None:
        assert torch.equal(TK._unpack_bits(bits, M, c4), (mid_p.float() > 0).to(torch.int32)), "emitted bits differ from (stored mid > 0)"
        assert int(TK._unpack_bits(bits, M, c4)[torch.isnan(mid_p)].sum()) == 0


def _pair_overflow(what, run, mid64, dst64, mid_in, dst_in):
    """fp16 store overflow of both stored tensors: mid_in overflows mid; dst_in keeps mid finite (asserted) and overflows dst."""
    mid, _, _ = run(mid_in, OTHER_SENTINEL)
    NF.assert_store_overflow(mid, mid64(*mid_in), torch.float16, what + " mid store overflow")
    mid, dst, _ = run(dst_in, OTHER_SENTINEL)
    assert bool(torch.isfinite(mid.float()).all()), "the stored mid must stay finite here"
    NF.assert_store_overflow(dst, dst64(mid.double(), *dst_in), torch.float16, what + " dst store overflow")


def _bias_poisons(bias, cols):
    out = bias
    for j, pname in enumerate(NF.POISON_NAMES):
        out = NF.put(out, 9 * j + 2, pname)
    if cols is not None:
        for j in range(4):
            NF.premise_nonzero(cols[:, 9 * j + 2], "second filter's column")
    return out


def _pair_operands(M, c, dt, seed):
    c4 = 4 * c
    src, w1 = TK._operands((M, c), dt, False, c, seed), TK._operands((c4, c), dt, False, c, seed + 1, c ** -0.5)
    add = TK._operands((M, c4), dt, False, 0, seed + 2)
    act = TK._operands((M, c), dt, True, 0, seed + 3, small=True, density=0.9)
    b1, b2 = TK._operands((c4,), 0, False, 0, seed + 4, 0.3), TK._operands((c,), 0, False, 0, seed + 5, 0.3)
    w2 = TK._operands((c, c4), dt, False, c4, seed + 7, 1 / (2 * c ** 0.5))
    return src, w1, add, act, b1, b2, w2


def _poison_rows(t, dt, w_cols):
    """The four poisons in four rows of the stored [M][c] operand t, spread over the rows; premise 1 on the filter columns they meet."""
    M = t.shape[0]
    out = _stored(t, dt)
    for j, pname in enumerate(NF.POISON_NAMES):
        ch = 3 * j + 1
        NF.premise_nonzero(w_cols[:, ch], "filter column %d" % ch)
        out = NF.put(out, ((j * M) // 4 + 5, ch), pname)
    return out


@pytest.mark.parametrize("c", [64, 128], ids=["stage2", "stage3"])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_conv_pair_forward(dt, c):
    """urso_conv_pair mode 0 (pair_kernel): mid = relu(src W1^T + b1 + add) with its emitted bits, dst = relu(mid W2^T + b2).  Poisoned
    src rows; poisoned elements of b1 (a column of mid, and through it every element of dst); of the residual `add`; of b2 (mid keeps its
    bits); fp16: the store overflow of mid and of dst."""
    hip = _hip()
    B, H, W, cap = TK.PAIR_SHAPES["small"]
    M, c4 = B * H * W, 4 * c
    src, w1, add, _, b1, b2, w2 = _pair_operands(M, c, dt, M + c + 11 * dt)

    def run(inp, fill):
        s, bias1, bias2, ad, wa, wb = inp
        mid, dst = TK.full((M, c4), dt, fill), TK.full((M, c), dt, fill)
        bits = torch.full((M * c4 // 8,), 0xAA, dtype=torch.uint8, device="cuda")
        with hip.options(grid_cap=cap), X.ran("pair_kernel"):
            hip.conv_pair(M, c, dt, 0, s.cuda(), TK.dev(wa, dt), bias1.cuda(), ad.cuda(), bits, mid, TK.dev(wb, dt), bias2.cuda(), None, dst)
        torch.cuda.synchronize()
        return mid.cpu(), dst.cpu(), bits.cpu()
    mid64 = lambda s, bias1, bias2, ad, wa, wb: torch.relu(TK._mm(s, wa) + bias1.double() + ad.double())
    dst64 = lambda m, s, bias1, bias2, ad, wa, wb: torch.relu(TK._mm(m, wb) + bias2.double())
    xs, ads = _stored(src, dt), _stored(add, dt)
    clean = (xs, b1, b2, ads, w1, w2)
    _pair_checks("pair forward, src", run, mid64, dst64, clean, (_poison_rows(src, dt, w1), b1, b2, ads, w1, w2), M, c4)
    _pair_checks("pair forward, b1", run, mid64, dst64, clean, (xs, _bias_poisons(b1, w2), b2, ads, w1, w2), M, c4)
    adp = ads
    for j, pname in enumerate(NF.POISON_NAMES):
        adp = NF.put(adp, ((j * M) // 4 + 9, 9 * j + 4), pname)
        NF.premise_nonzero(w2[:, 9 * j + 4], "second filter's column")
    _pair_checks("pair forward, add", run, mid64, dst64, clean, (xs, b1, b2, adp, w1, w2), M, c4)
    _pair_checks("pair forward, b2", run, mid64, dst64, clean, (xs, b1, _bias_poisons(b2, None), ads, w1, w2), M, c4, mid_changes=False)
    if dt == 2:
        _pair_overflow("pair forward", run, mid64, dst64, (_stored(src * 2.0 ** 13, dt), b1, b2, ads, w1 * 2.0 ** 4, w2),
                       (_stored(src * 2.0 ** 6, dt), b1, b2, ads, w1, w2 * 2.0 ** 15))


@pytest.mark.parametrize("c", [64, 128], ids=["stage2", "stage3"])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_conv_pair_backward(dt, c):
    """urso_conv_pair mode 1: mid = (src W1^T + add) where the bit mask is set, dst = (mid W2^T) where act > 0; poisoned rows of src (a dz)."""
    hip = _hip()
    B, H, W, cap = TK.PAIR_SHAPES["small"]
    M, c4 = B * H * W, 4 * c
    src, w1, add, act, _, _, w2 = _pair_operands(M, c, dt, M + c + 11 * dt)
    gbits = X.rand_bits(M * c4 // 8, 6 + dt)
    keep1, keep2 = TK._unpack_bits(gbits, M, c4) > 0, act > 0
    w1d, w2d, addd, actd, bitsd = TK.dev(w1, dt), TK.dev(w2, dt), TK.dev(add, dt), TK.dev(act, dt), gbits.cuda()
    zero = torch.zeros(1, dtype=torch.float64)

    def run(inp, fill):
        mid, dst = TK.full((M, c4), dt, fill), TK.full((M, c), dt, fill)
        with hip.options(grid_cap=cap), X.ran("pair_kernel"):
            hip.conv_pair(M, c, dt, 1, inp[0].cuda(), w1d, None, addd, bitsd, mid, w2d, None, actd, dst)
        torch.cuda.synchronize()
        return mid.cpu(), dst.cpu(), None
    mid64 = lambda s: torch.where(keep1, TK._mm(s, w1) + add.double(), zero)
    dst64 = lambda m, s: torch.where(keep2, TK._mm(m, w2), zero)
    _pair_checks("pair backward", run, mid64, dst64, (_stored(src, dt),), (_poison_rows(src, dt, w1),), M, c4)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_conv_pair_shortcut(dt):
    """urso_conv_pair_shortcut (pairs_kernel) on one 64-pixel tile, the smallest tiles-per-block count of PAIR_TILES: mid = relu(src W1^T +
    xin Ws^T + b1 + bs), dst = relu(mid W2^T + b2).  Poisoned rows of src and, in another launch, of xin; poisoned elements of b1, of bs
    and of b2; fp16: the store overflow of mid and of dst."""
    hip = _hip()
    (ntiles, cap), c, c4, G = TK.PAIR_TILES[0], 64, 256, 64
    M = 64 * ntiles
    seed = 5 * M + 17 * dt + 3
    src, xin = TK._operands((M, c), dt, False, c, seed), TK._operands((M, c), dt, False, c, seed + 1)
    w1, ws = TK._operands((c4, c), dt, False, c, seed + 2, (2 * c) ** -0.5), TK._operands((c4, c), dt, False, c, seed + 3, (2 * c) ** -0.5)
    b1, bs, b2 = (TK._operands((n,), 0, False, 0, seed + 4 + i, 0.3) for i, n in enumerate((c4, c4, c)))
    w2 = TK._operands((c, c4), dt, False, c4, seed + 7, 1 / (2 * c ** 0.5))

    def run(inp, fill):
        s, x, ba, bb, bc, wa, wb = inp
        mid, dst = TK.full((M + G, c4), dt, fill), TK.full((M + G, c), dt, fill)
        bits = torch.full(((M + G) * c4 // 8,), 0xAA, dtype=torch.uint8, device="cuda")
        with hip.options(grid_cap=cap), X.ran("pairs_kernel"):
            hip.conv_pair_shortcut(M, dt, s.cuda(), TK.dev(wa, dt), ba.cuda(), x.cuda(), TK.dev(ws, dt), bb.cuda(), bits, mid, TK.dev(wb, dt),
                                   bc.cuda(), dst)
        torch.cuda.synchronize()
        assert bool((mid[M:].float() == fill).all()) and bool((dst[M:].float() == fill).all()), "the guard tile behind the output was written"
        return mid[:M].cpu(), dst[:M].cpu(), bits[:M * c4 // 8].cpu()
    mid64 = lambda s, x, ba, bb, bc, wa, wb: torch.relu(TK._mm(s, wa) + TK._mm(x, ws) + ba.double() + bb.double())
    dst64 = lambda m, s, x, ba, bb, bc, wa, wb: torch.relu(TK._mm(m, wb) + bc.double())
    xs, xi = _stored(src, dt), _stored(xin, dt)
    clean = (xs, xi, b1, bs, b2, w1, w2)
    _pair_checks("shortcut pair, src", run, mid64, dst64, clean, (_poison_rows(src, dt, w1), xi, b1, bs, b2, w1, w2), M, c4)
    _pair_checks("shortcut pair, xin", run, mid64, dst64, clean, (xs, _poison_rows(xin, dt, ws), b1, bs, b2, w1, w2), M, c4)
    _pair_checks("shortcut pair, b1", run, mid64, dst64, clean, (xs, xi, _bias_poisons(b1, w2), bs, b2, w1, w2), M, c4)
    _pair_checks("shortcut pair, bs", run, mid64, dst64, clean, (xs, xi, b1, _bias_poisons(bs, w2), b2, w1, w2), M, c4)
    _pair_checks("shortcut pair, b2", run, mid64, dst64, clean, (xs, xi, b1, bs, _bias_poisons(b2, None), w1, w2), M, c4, mid_changes=False)
    if dt == 2:
        _pair_overflow("shortcut pair", run, mid64, dst64, (_stored(src * 2.0 ** 13, dt), xi, b1, bs, b2, w1 * 2.0 ** 4, w2),
                       (_stored(src * 2.0 ** 6, dt), xi, b1, bs, b2, w1, w2 * 2.0 ** 15))


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_conv_pair_wgrad_and_dgrad_wgrad_pw(dt):
    """urso_conv_pair_wgrad (pairw_kernel): the backward pair with poisoned rows of its dz, and the block-closing layer's weight gradient
    u^T mid + column sums from the STORED mid (split partials, summed here in float64); then urso_conv_dgrad_wgrad_pw on that stored mid as
    its dz.  u is real and non-zero (it multiplies the poisoned rows in u^T mid) and serves as the mask u > 0 as well."""
    hip = _hip()
    B, H, W, cap = TK.PAIR_SHAPES["small"]
    M, c, c4 = B * H * W, 64, 256
    src, w1, add, _, _, _, w2 = _pair_operands(M, c, dt, M + 3 * dt + 1)
    u = TK._operands((M, c), dt, False, 0, M + 3 * dt + 4)
    NF.premise_nonzero(u, "u")
    gbits = X.rand_bits(M * c4 // 8, 4 + dt)
    keep1, keep2 = TK._unpack_bits(gbits, M, c4) > 0, u > 0
    zero = torch.zeros(1, dtype=torch.float64)
    w1d, w2d, addd, ud, bitsd = TK.dev(w1, dt), TK.dev(w2, dt), TK.dev(add, dt), TK.dev(u, dt), gbits.cuda()
    with hip.options(grid_cap=cap):
        splits = hip.conv_pair_wgrad_splits(M, dt)
    stride = c * c4 + hip.WGRAD_PART_PAD

    def sums(part, colpart):
        return part.reshape(splits, stride)[:, :c * c4].double().cpu().sum(0).reshape(c, c4), colpart.reshape(splits, c4).double().cpu().sum(0)

    def run(s, fill):
        part, colpart = torch.full((splits * stride,), float("nan"), device="cuda"), torch.full((splits * c4,), float("nan"), device="cuda")
        mid, dst, dx = TK.full((M, c4), dt, fill), TK.full((M, c), dt, fill), TK.full((M, c), dt, fill)
        with hip.options(grid_cap=cap), X.ran("pairw_kernel"):
            hip.conv_pair_wgrad(M, dt, s.cuda(), w1d, addd, bitsd, mid, w2d, ud, dst, part, colpart, stride)
        torch.cuda.synchronize()
        pair = (mid.cpu(), dst.cpu()) + sums(part, colpart)
        part.fill_(float("nan")); colpart.fill_(float("nan"))
        with hip.options(grid_cap=cap), X.ran("pairw_kernel"):
            hip.conv_dgrad_wgrad_pw(M, dt, mid, w2d, ud, 1, dx, part, colpart, stride)
        torch.cuda.synchronize()
        return pair, (dx.cpu(),) + sums(part, colpart)
    mid64 = lambda s_: torch.where(keep1, TK._mm(s_, w1) + add.double(), zero)
    xs = _stored(src, dt)
    xp = _poison_rows(src, dt, w1)
    (mid_c, dst_c, dw_c, cs_c), (dx_c, dw2_c, cs2_c) = run(xs, TK.SENTINEL)
    (mid_p, dst_p, dw_p, cs_p), (dx_p, dw2_p, cs2_p) = run(xp, OTHER_SENTINEL)
    assert bool(torch.isfinite(dw_c).all()) and bool(torch.isfinite(cs_c).all())
    rc, rp = mid64(xs), mid64(xp)
    NF.assert_class_parity(mid_p, mid_c, rp, NF.dependency(rc, rp), "conv_pair_wgrad mid")
    mc, mp = mid_c.double(), mid_p.double()                            # everything behind reads the stored mid
    refs = lambda m: (torch.where(keep2, TK._mm(m, w2), zero), u.double().T @ m, m.sum(0))
    (dst_rc, dw_rc, cs_rc), (dst_rp, dw_rp, cs_rp) = refs(mc), refs(mp)
    for what, got, cl, r0, r1 in (("conv_pair_wgrad dst", dst_p, dst_c, dst_rc, dst_rp), ("conv_pair_wgrad dW", dw_p, dw_c, dw_rc, dw_rp),
                                  ("conv_pair_wgrad colsum", cs_p, cs_c, cs_rc, cs_rp), ("conv_dgrad_wgrad_pw dx", dx_p, dx_c, dst_rc, dst_rp),
                                  ("conv_dgrad_wgrad_pw dW", dw2_p, dw2_c, dw_rc, dw_rp), ("conv_dgrad_wgrad_pw colsum", cs2_p, cs2_c, cs_rc, cs_rp)):
        NF.assert_class_parity(got, cl, r1, NF.dependency(r0, r1), what)


@pytest.mark.parametrize("mask_by_xin", [1, 0], ids=["dP_masked", "dP_unmasked"])
@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_conv_pair_wgrad_entry(dt, mask_by_xin):
    """urso_conv_pair_wgrad_entry (pairx_kernel), the backward pair of a stage-entry block, on one 64-pixel tile (the smallest
    tiles-per-block count of PAIR_TILES): mid = (G W1^T + dXb) where the bit mask is set never leaves LDS; stored are dst = (mid W2^T)
    where u > 0, dP = mid W3^T [where P > 0] and per block the fp32 partials of dW2c = u^T mid, dWs = P^T mid and the column sums (twice).
    Poisoned rows of G.  The reference mid is what urso_conv_pair_wgrad STORES for the same operands (as in test_conv_pair_wgrad_entry;
    its class parity is test_conv_pair_wgrad_and_dgrad_wgrad_pw's); u and P are real and non-zero: they multiply the poisoned rows."""
    hip = _hip()
    (ntiles, cap), c, c4 = TK.PAIR_TILES[0], 64, 256
    M = 64 * ntiles
    seed = 7 * M + 13 * dt + 5
    src, w1, add, _, _, _, w2 = _pair_operands(M, c, dt, seed)
    w3 = TK._operands((c, c4), dt, False, c4, seed + 16, 1 / (2 * c ** 0.5))
    u, P = TK._operands((M, c), dt, False, 0, seed + 3), TK._operands((M, c), dt, False, 0, seed + 4)
    NF.premise_nonzero(u, "u"); NF.premise_nonzero(P, "P"); NF.premise_nonzero(w2, "W2"); NF.premise_nonzero(w3, "W3")
    gbits = X.rand_bits(M * c4 // 8, seed + 5)
    zero = torch.zeros(1, dtype=torch.float64)
    dw1, dadd, dbits, dw2, dw3, du, dP = TK.dev(w1, dt), TK.dev(add, dt), gbits.cuda(), TK.dev(w2, dt), TK.dev(w3, dt), TK.dev(u, dt), TK.dev(P, dt)
    with hip.options(grid_cap=cap):
        splits = hip.conv_pair_wgrad_splits(M, dt)
    stride = c * c4 + hip.WGRAD_PART_PAD
    nan = lambda n: torch.full((n,), float("nan"), device="cuda")

    def run(s, fill):
        part, colpart, part_s, colpart_s = nan(splits * stride), nan(splits * c4), nan(splits * stride), nan(splits * c4)
        dst, dxin, mid, dst0 = TK.full((M, c), dt, fill), TK.full((M, c), dt, fill), TK.full((M, c4), dt, fill), TK.full((M, c), dt, fill)
        with hip.options(grid_cap=cap):
            with X.ran("pairx_kernel"):
                hip.conv_pair_wgrad_entry(M, dt, s.cuda(), dw1, dadd, dbits, dw2, du, dst, dw3, dP, mask_by_xin, dxin, part, colpart, part_s,
                                          colpart_s, stride)
            torch.cuda.synchronize()
            out = {"dst": dst.cpu(), "dP": dxin.cpu()}
            for name, t in (("dW2c", part), ("dWs", part_s)):
                out[name] = t.reshape(splits, stride)[:, :c * c4].double().cpu().sum(0).reshape(c, c4)
            for name, t in (("colsum", colpart), ("colsum (shortcut)", colpart_s)):
                out[name] = t.reshape(splits, c4).double().cpu().sum(0)
            part0, colpart0 = nan(splits * stride), nan(splits * c4)
            with X.ran("pairw_kernel"):
                hip.conv_pair_wgrad(M, dt, s.cuda(), dw1, dadd, dbits, mid, dw2, du, dst0, part0, colpart0, stride)
            torch.cuda.synchronize()
        return out, mid.double().cpu()

    def ref64(m):
        r = {"dst": torch.where(u > 0, TK._mm(m, w2), zero), "dP": torch.where(P > 0, TK._mm(m, w3), zero) if mask_by_xin else TK._mm(m, w3),
             "dW2c": u.double().T @ m, "dWs": P.double().T @ m, "colsum": m.sum(0)}
        r["colsum (shortcut)"] = r["colsum"]
        return r
    (clean, mid_c), (got, mid_p) = run(_stored(src, dt), TK.SENTINEL), run(_poison_rows(src, dt, w1), OTHER_SENTINEL)
    assert all(bool(torch.isfinite(t.double()).all()) for t in clean.values()), "a split partial of the clean launch was not written"
    assert int((~torch.isfinite(mid_p)).sum()) > 0
    rc, rp = ref64(mid_c), ref64(mid_p)
    for k in ("dst", "dP", "dW2c", "dWs", "colsum", "colsum (shortcut)"):
        NF.assert_class_parity(got[k], clean[k], rp[k], NF.dependency(rc[k], rp[k]), "conv_pair_wgrad_entry " + k)


# ====================================================================================================== stem, max-pool, BatchNorm
STEM = TK.STEM_CASES[0]                                 # partial_tiles: 2 x 40 x 68, pooled 10 x 17


def _stem_setup(dt):
    """Operands of test_stem_kernels' rounded-once probe with an identity BatchNorm (var 1 - eps: scale 1), packed by the library."""
    hip = _hip()
    B, H, W, cap, name = STEM
    N = TK.STEM_N
    seed = H + W + 13 * dt
    x = TK._operands((B, H, W, 3), dt, False, 0, seed)
    w = TK._operands((7, 7, 3, N), dt, False, 0, seed + 1, 1 / 147 ** 0.5)
    b = TK._operands((N,), 0, False, 0, seed + 2, 0.3)
    x4 = torch.zeros(B, H, W, 4)
    x4[..., :3] = x
    wf, biasf, scale = TK.full((N * 224,), dt), TK.full((N,), 0), TK.full((N,), 0)
    one, zero = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    hip.stem_weight_pack(N, dt, w.cuda(), b.cuda(), one, zero, zero, one, 0.0, wf, biasf, scale)
    torch.cuda.synchronize()
    taps = X.stem_taps(w.double())
    X.assert_exact(wf.reshape(N, 7, 4, 8), taps.permute(3, 0, 1, 2).reshape(N, 7, 4, 8), "packed stem filter")
    X.assert_exact(biasf, b.double(), "stem bias")
    g = hip.geom(B, H, W // 2, 8, H // 2, W // 2, N, 7, 4, 2, 1, 3, 2)
    return x4, taps, b.double(), wf, biasf, g


def _stem_poisons(x4, dt, taps):
    """A NaN of either sign in two interior pixels of real channels.  The packed filter holds one zero pad tap per row, which multiplies
    every pixel once: premise 1 cannot hold for an infinity in the input (0 x inf), so the infinities go into the bias instead."""
    xs = _stored(x4, dt)
    assert bool((X.stem_untaps(taps) != 0).all())
    xs = NF.put(xs, (0, 14, 21, 1), "nan_pos")
    return NF.put(xs, (1, 25, 46, 2), "nan_neg")


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_stem_unpooled(dt):
    hip = _hip()
    B, H, W, cap, name = STEM
    N, OH, OW = TK.STEM_N, H // 2, W // 2
    x4, taps, b64, wf, biasf, g = _stem_setup(dt)

    def run(x, bias):
        y = TK.full((B, OH, OW, N), dt)
        with hip.options(stem=1, grid_cap=cap), X.ran("stem_kernel"):
            hip.conv_igemm(g, dt, hip.EPI_RELU, x.cuda(), wf, bias, None, None, y)
        torch.cuda.synchronize()
        return y.cpu()
    xs = _stored(x4, dt)
    y_clean = run(xs, biasf)
    clean = torch.relu(X.stem_conv64(x4, taps) + b64)
    xp = _stem_poisons(x4, dt, taps)
    ref = torch.relu(X.stem_conv64(xp.double(), taps) + b64)
    NF.assert_class_parity(run(xp, biasf), y_clean, ref, NF.dependency(clean, ref), "stem, NaN pixels")
    bp = biasf.clone()
    for i, pname in enumerate(NF.POISON_NAMES):
        bp = NF.put(bp, 9 * i + 2, pname)
    ref = torch.relu(X.stem_conv64(x4, taps) + bp.double().cpu())
    NF.assert_class_parity(run(xs, bp), y_clean, ref, NF.dependency(clean, ref), "stem, bias poisons")
    # store overflow: x * 2**13, w * 2**4
    if dt == 2:
        xo = x4 * 2.0 ** 13
        wo = X.stem_untaps(taps).float() * 2.0 ** 4
        assert torch.equal(xo.half().float(), xo) and torch.equal(wo.half().float(), wo)
        wf2, bf2, sc2 = TK.full((N * 224,), dt), TK.full((N,), 0), TK.full((N,), 0)
        one, zero = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
        hip.stem_weight_pack(N, dt, wo.cuda(), b64.float().cuda(), one, zero, zero, one, 0.0, wf2, bf2, sc2)
        y = TK.full((B, OH, OW, N), dt)
        with hip.options(stem=1, grid_cap=cap), X.ran("stem_kernel"):
            hip.conv_igemm(g, dt, hip.EPI_RELU, TK.dev(xo, dt), wf2, bf2, None, None, y)
        torch.cuda.synchronize()
        NF.assert_store_overflow(y, torch.relu(X.stem_conv64(xo, X.stem_taps(wo.double())) + b64), torch.float16, "stem store overflow")


def _pool64(x):
    """F.max_pool2d 3x3 / s2 / TF-SAME in float64 (pads the bottom and the right with -inf); keeps a NaN."""
    xp = F.pad(x.double().permute(0, 3, 1, 2), (0, 1, 0, 1), value=-math.inf)
    return F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_stem_fused_with_pool(dt):
    """stem_pool_kernel pools over integer keys: a NaN of either sign in a window must come out as NaN, +inf as +inf, and the ReLU's
    0 of a -inf must not win; every other pooled element keeps its bits."""
    hip = _hip()
    B, H, W, cap, name = STEM
    N, OH, OW = TK.STEM_N, H // 2, W // 2
    x4, taps, b64, wf, biasf, g = _stem_setup(dt)
    with hip.options(stem=1, stem_pool=1):
        assert hip.stem_conv_pool_ok(g, dt)

    def run(x, bias):
        pooled = TK.full((B, OH // 2, OW // 2, N), dt)
        am = torch.full((B, OH // 2, OW // 2, N), 0xEE, dtype=torch.uint8, device="cuda")
        with hip.options(stem=1, stem_pool=1, grid_cap=cap), X.ran("stem_pool_kernel"):
            hip.stem_conv_pool(g, dt, x.cuda(), wf, bias, pooled, am)
        torch.cuda.synchronize()
        return pooled.cpu(), am.cpu()
    xs = _stored(x4, dt)
    p_clean, am_clean = run(xs, biasf)
    clean = _pool64(torch.relu(X.stem_conv64(x4, taps) + b64))
    xp = _stem_poisons(x4, dt, taps)
    ref = _pool64(torch.relu(X.stem_conv64(xp.double(), taps) + b64))
    dep = NF.dependency(clean, ref)
    got, am = run(xp, biasf)
    NF.assert_class_parity(got, p_clean, ref, dep, "fused stem + pool, NaN pixels")
    assert torch.equal(am[~dep], am_clean[~dep]), "arg-max bytes outside the dependency set changed"
    bp = biasf.clone()
    for i, pname in enumerate(NF.POISON_NAMES):
        bp = NF.put(bp, 9 * i + 2, pname)
    ref = _pool64(torch.relu(X.stem_conv64(x4, taps) + bp.double().cpu()))
    NF.assert_class_parity(run(xs, bp)[0], p_clean, ref, NF.dependency(clean, ref), "fused stem + pool, bias poisons")
    if dt == 2:                                                 # store overflow: x * 2**13, w * 2**4, through the pack and the integer keys
        xo = x4 * 2.0 ** 13
        wo = X.stem_untaps(taps).float() * 2.0 ** 4
        assert torch.equal(xo.half().float(), xo) and torch.equal(wo.half().float(), wo)
        wf, sc2 = TK.full((N * 224,), dt), TK.full((N,), 0)
        one, zero = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
        hip.stem_weight_pack(N, dt, wo.cuda(), b64.float().cuda(), one, zero, zero, one, 0.0, wf, biasf, sc2)
        pooled = run(_stored(xo, dt), biasf)[0]
        NF.assert_store_overflow(pooled, _pool64(torch.relu(X.stem_conv64(xo, X.stem_taps(wo.double())) + b64)), torch.float16,
                                 "fused stem + pool store overflow")


POOL_SHAPE = (3, 10, 20, 64)


def _pool_input(dt):
    """Post-ReLU-like reals (zeros and positives).  Around the NaN of each sign: a larger finite value earlier and later in the window
    scan, and a +inf in the same window; one window holds +inf alone."""
    g = torch.Generator().manual_seed(3 + dt)
    x = _stored(torch.relu(torch.randn(POOL_SHAPE, generator=g)), dt)
    clean = x.clone()
    for b, c, pname in ((0, 5, "nan_pos"), (1, 9, "nan_neg")):
        for t in (x, clean):
            t[b, 4, 8, c] = 7.0                       # before the NaN in the scan of window (2, 4) (and in windows (1, 3), (1, 4), (2, 3))
            t[b, 6, 10, c] = 9.0                      # after it
        clean[b, 5, 9, c] = 0.5
        x[b, 5, 10, c] = math.inf
        clean[b, 5, 10, c] = 11.0
        x = NF.put(x, (b, 5, 9, c), pname)            # odd pixel: the windows (2, 4) only ... and none else
    x[2, 2, 2, 3] = math.inf
    clean[2, 2, 2, 3] = 5.0
    return x, clean


@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_maxpool_forward(dt):
    hip = _hip()
    B, H, W, C = POOL_SHAPE
    x, clean = _pool_input(dt)

    def run(t):
        y = TK.full((B, H // 2, W // 2, C), dt)
        am = torch.full((B, H // 2, W // 2, C), 0xEE, dtype=torch.uint8, device="cuda")
        with X.ran("maxpool_fwd_kernel"):
            hip.maxpool_fwd(B, H, W, C, dt, t.cuda(), y, am)
        torch.cuda.synchronize()
        return y.cpu(), am.cpu()
    ref = _pool64(x)
    dep = NF.dependency(_pool64(clean), ref)
    assert int((NF.classes(ref) == NF.NAN).sum()) == 2 and int((NF.classes(ref) == NF.PINF).sum()) >= 1
    (got, am), (got_clean, am_clean) = run(x), run(clean)
    NF.assert_class_parity(got, got_clean, ref, dep, "max-pool")
    assert torch.equal(am[~dep], am_clean[~dep]), "arg-max bytes outside the dependency set changed"


@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_maxpool_backward(dt):
    """One dy element per poison, each in a window whose maximum is positive (asserted): it reaches the one pixel its arg-max byte names."""
    hip = _hip()
    B, H, W, C = POOL_SHAPE
    OH, OW = H // 2, W // 2
    g = torch.Generator().manual_seed(11 + dt)
    x = _stored(torch.relu(torch.randn(POOL_SHAPE, generator=g)), dt)
    dy = _stored(torch.randn(B, OH, OW, C, generator=g), dt)
    y = TK.full((B, OH, OW, C), dt)
    am = torch.full((B, OH, OW, C), 0xEE, dtype=torch.uint8, device="cuda")
    hip.maxpool_fwd(B, H, W, C, dt, x.cuda(), y, am)
    torch.cuda.synchronize()
    amc = am.cpu().long()

    def ref64(d):
        out = torch.zeros(B, H + 1, W + 1, C, dtype=torch.float64)
        zero = torch.zeros(1, dtype=torch.float64)
        for ky in range(3):
            for kx in range(3):
                out[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += torch.where(amc == 3 * ky + kx, d.double(), zero)      # bit 4 set: no tap matches
        return out[:, :H, :W]

    def run(d):
        dx = TK.full((B, H, W, C), dt)
        with X.ran("maxpool_bwd_kernel"):
            hip.maxpool_bwd(B, H, W, C, dt, y, d.cuda(), am, 1, dx)
        torch.cuda.synchronize()
        return dx.cpu()
    dyp = dy
    for i, pname in enumerate(NF.POISON_NAMES):
        at = (i % B, 1 + i, 2 + 2 * i, 7 * i + 1)
        assert float(y.cpu()[at]) > 0 and int(amc[at]) < 16, "the poisoned window is not live"
        dyp = NF.put(dyp, at, pname)
    ref = ref64(dyp)
    dep = NF.dependency(ref64(dy), ref)
    assert int(dep.sum()) == 4
    NF.assert_class_parity(run(dyp), run(dy), ref, dep, "max-pool gradient")


BN_MN = (37 * 8, 64)


def _bn_operands(dt):
    M, N = BN_MN
    g = torch.Generator().manual_seed(17 + dt)
    z = _stored(torch.randn(M, N, generator=g) * 2 + 0.5, dt)
    res, gy = _stored(torch.randn(M, N, generator=g), dt), _stored(torch.randn(M, N, generator=g), dt)
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    mean, var = torch.randn(N, generator=g) * 0.3 + 0.5, torch.rand(N, generator=g) + 3.5
    return z, res, gy, gamma, beta, mean, var


@pytest.mark.parametrize("relu", [1, 0], ids=[RELU, PLAIN])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_bn_apply(dt, relu):
    """y = relu?(gamma (z - mean) rstd + beta + res): the four poisons in four z elements and in four residual elements."""
    hip = _hip()
    M, N = BN_MN
    z, res, _, gamma, beta, mean, var = _bn_operands(dt)
    eps = 1e-3
    act = torch.relu if relu else (lambda t: t)
    dv = [t.cuda() for t in (mean, var, gamma, beta)]

    def run(zz, rr, v=var, fill=OTHER_SENTINEL):
        y = TK.full((M, N), dt, fill)
        with X.ran("bn_apply_kernel"):
            hip.bn_apply(M, N, dt, zz.cuda(), dv[0], v.cuda(), dv[2], dv[3], eps, rr.cuda(), relu, y)
        torch.cuda.synchronize()
        return y.cpu()

    def ref64(zz, rr, v=var):
        s = gamma.double() * torch.rsqrt(v.double() + X.f32v(eps))
        return act((zz.double() - mean.double()) * s + beta.double() + rr.double())
    NF.premise_nonzero(gamma, "gamma")
    zp, rp = z, res
    for i, pname in enumerate(NF.POISON_NAMES):
        zp = NF.put(zp, (11 * i + 3, 9 * i + 1), pname)
        rp = NF.put(rp, (13 * i + 5, 9 * i + 4), pname)
    ref = ref64(zp, rp)
    dep = NF.dependency(ref64(z, res), ref)
    assert int(dep.sum()) >= 6
    NF.assert_class_parity(run(zp, rp), run(z, res, fill=TK.SENTINEL), ref, dep, "bn_apply")
    if dt == 2 and relu:
        # z * 2**11 is still an fp16 value; a variance of 2**-8 makes rstd ~ 16, so gamma (z - mean) rstd passes 65504 for |z| > ~ 1
        big, small_var = _stored(z.float() * 2.0 ** 11, dt), torch.full((N,), 2.0 ** -8)
        assert bool(torch.isfinite(big).all())
        NF.assert_store_overflow(run(big, res, small_var), ref64(big, res, small_var), torch.float16, "bn_apply store overflow")


@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_relu_of_negative_zero_is_positive_zero(dt):
    """relu_f sends -0 to +0, as the hardware maximum did: gamma < 0, z = mean and beta = -0 give the pre-activation (+0)(-s) + (-0) = -0;
    with the ReLU the stored bits are those of +0, without it the -0 stays."""
    hip = _hip()
    M, N = 16, 64
    z, mean, gamma = torch.full((M, N), 1.5), torch.full((N,), 1.5), torch.full((N,), -1.0)
    beta, var = torch.full((N,), -0.0), torch.ones(N)
    for relu in (1, 0):
        y = TK.full((M, N), dt)
        hip.bn_apply(M, N, dt, TK.dev(z, dt), mean.cuda(), var.cuda(), gamma.cuda(), beta.cuda(), 0.0, None, relu, y)
        torch.cuda.synchronize()
        assert bool((y.cpu() == 0).all()) and bool((NF.sign_bit(y.cpu()) == (relu == 0)).all()), "relu = %d: wrong sign of zero" % relu


@pytest.mark.parametrize("dt", [0, 1, 2], ids=DT_IDS.get)
def test_bn_backward(dt):
    """A NaN of either sign in one element of the incoming gradient: dbeta, dgamma of its channel and the channel's whole dz column are
    NaN, every other channel keeps its bits.  (An infinity gives inf - inf inside dz = k (g - dbeta / M - xhat dgamma / M) whatever the
    kernel does: its class is no property of the kernel, so it is not tried.)"""
    hip = _hip()
    M, N = BN_MN
    z, _, gy, gamma, _, mean, var = _bn_operands(dt)
    eps = 1e-3
    ws = torch.empty(hip.bn_ws_bytes(M, N) // 8 + 8, dtype=torch.float64, device="cuda")
    dv = [t.cuda() for t in (mean, var, gamma)]

    def run(gg):
        db, dg, gb, gga, dz = TK.full((N,), 0), TK.full((N,), 0), TK.full((N,), 0), TK.full((N,), 0), TK.full((M, N), dt)
        with X.ran("bn_colreduce_kernel"):
            hip.bn_backward(M, N, dt, gg.cuda(), z.cuda(), dv[0], dv[1], dv[2], eps, ws, db, dg, 1, gb, gga, dz)
        torch.cuda.synchronize()
        return db.cpu(), dg.cpu(), dz.cpu()
    gp = NF.put(NF.put(gy, (40, 3), "nan_pos"), (201, 50), "nan_neg")
    clean, got = run(gy), run(gp)
    col = torch.zeros(N, dtype=torch.bool); col[3] = col[50] = True
    for name, c, t in zip(("dbeta", "dgamma", "dz"), clean, got):
        nan = torch.isnan(t)
        assert bool(nan[..., col].all()), "%s of a poisoned channel is not NaN" % name
        assert torch.equal(NF._bits(t[..., ~col]), NF._bits(c[..., ~col])), "%s of a clean channel changed" % name


# ====================================================================================================== weight gradients
@pytest.mark.parametrize("case,dt,opts,sym", TK.WGRAD_CASES, ids=["%s-dt%d-%s" % (c[0][-1], c[1], "-".join("%s%d" % kv for kv in c[2].items()))
                                                                   for c in TK.WGRAD_CASES])
def test_wgrad_variants(case, dt, opts, sym):
    """urso_conv_wgrad, every variant of test_wgrad_variants: the four poisons in interior dz elements of four output channels; filter
    gradient and column sums of those channels take the class of the float64 sums, the others keep their bits."""
    hip = _hip()
    R = TK.ConvRef(case, dt, False, seed=sum(map(ord, case[-1])) + 5 * dt)
    B, H, W, Ci, N, k, s, pad, name = case
    g = hip.geom(B, H, W, Ci, R.OH, R.OW, N, k, k, s, s, pad[0], pad[1])
    NF.premise_nonzero(R.x, "layer input")
    dzs = _stored(R.dz, dt)
    dzp = dzs
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, R.OH, R.OW, -(-k // s), 1))):
        dzp = NF.put(dzp, (b, y, x, 7 * i + 2), pname)
    xd = TK.dev(R.x, dt)

    def run(dz):
        with hip.options(c3=0, hwgrad=0, **opts):
            ws = torch.full((hip.conv_wgrad_ws_bytes(g, dt) // 4 + 16,), float("nan"), dtype=torch.float32, device="cuda")
            dw, cs = TK.full((k, k, Ci, N), 0), TK.full((N,), 0)
            with X.ran(sym):
                hip.conv_wgrad(g, dt, xd, dz.cuda(), ws, dw, cs)
            torch.cuda.synchronize()
        return dw.cpu(), cs.cpu()
    wr = R.w.double().requires_grad_(True)
    gw_p = torch.autograd.grad((TK._conv64(R.x.double(), wr, s, pad, R.OH, R.OW) * dzp.double()).sum(), wr)[0]
    cs_p = dzp.double().sum(dim=(0, 1, 2))
    (dw, cs), (dw_clean, cs_clean) = run(dzp), run(dzs)
    dep = NF.dependency(R.gw, gw_p)
    want = torch.zeros(k, k, Ci, N, dtype=torch.bool)
    want[..., [2, 9, 16, 23]] = True
    assert torch.equal(dep, want), "every tap of a poisoned channel depends on the poison, nothing else does"
    NF.assert_class_parity(dw, dw_clean, gw_p, dep, name + " filter gradient")
    NF.assert_class_parity(cs, cs_clean, cs_p, NF.dependency(R.colsum, cs_p), name + " column sums")


def _partial_sums(ws, splits, g):
    """float64 sums of a layer's split partials and column-sum partials (the layout of urso_conv_wgrad_partial)."""
    kn = g.KH * g.KW * g.C * g.N
    stride = kn + _hip().WGRAD_PART_PAD
    part = ws[:splits * stride].reshape(splits, stride)[:, :kn].double().cpu().sum(0).reshape(g.KH, g.KW, g.C, g.N)
    col = ws[splits * stride:splits * stride + splits * g.N].reshape(splits, g.N).double().cpu().sum(0)
    return part, col


def _batched_wgrad(geoms, dt, seed, launch, what):
    """Several layers' weight gradients in one launch (split partials, summed here in float64): the four poisons in interior dz elements
    of four output channels of every layer.  launch(xs, dzs) -> [(workspace, splits)] per layer."""
    ops = [TK._wgrad_operands(g, dt, False, seed + 7 * i) for i, g in enumerate(geoms)]
    xs = [TK.dev(o[0], dt) for o in ops]
    clean, poisoned = [], []
    for g, (x, dz, r) in zip(geoms, ops):
        NF.premise_nonzero(x, "layer input")
        dzs = _stored(dz, dt)
        dzp = dzs
        m = -(-g.KH // g.SH) - 1                                  # interior margin: the dz element's window lies inside the input
        for i, pname in enumerate(NF.POISON_NAMES):               # (distinct channels: the pixels need not differ)
            at = (i % g.B, m + (5 * i) % (g.OH - 2 * m), m + (7 * i) % (g.OW - 2 * m), 7 * i + 2)
            dzp = NF.put(dzp, at, pname)
        clean.append(dzs); poisoned.append(dzp)
    got_c = launch(xs, [t.cuda() for t in clean])
    got_p = launch(xs, [t.cuda() for t in poisoned])
    for i, (g, (x, dz, r)) in enumerate(zip(geoms, ops)):
        zp = poisoned[i].cuda().double()
        gw_p, cs_p = X.wgrad64(x.cuda().double(), zp, g.KH, g.SH, (g.PH, g.PW)).cpu(), zp.sum((0, 1, 2)).cpu()
        (dw_c, col_c), (dw_p, col_p) = _partial_sums(*got_c[i], g), _partial_sums(*got_p[i], g)
        assert bool(torch.isfinite(dw_c).all()) and bool(torch.isfinite(col_c).all()), "a split partial of the clean launch was not written"
        dep = NF.dependency(r[0], gw_p)
        want = torch.zeros_like(dep); want[..., [2, 9, 16, 23]] = True
        assert torch.equal(dep, want)
        NF.assert_class_parity(dw_p, dw_c, gw_p, dep, "%s layer %d dW" % (what, i))
        NF.assert_class_parity(col_p, col_c, cs_p, NF.dependency(r[2], cs_p), "%s layer %d column sums" % (what, i))


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_wgrad_group(dt):
    """hip.WgradGroup (wgrad_group_kernel) on the `pair` list of test_wgrad_group_kernels."""
    hip = _hip()
    geoms = [hip.geom(*l) for l in TK.WG_LISTS["pair"]]

    def launch(xs, dzs):
        with hip.options(wgrad_big=0):
            grp = hip.WgradGroup(geoms, dt)
            assert grp.nblocks > 0
            wss = [torch.full((s * (g.KH * g.KW * g.C * g.N + hip.WGRAD_PART_PAD) + s * g.N + 64,), float("nan"), device="cuda")
                   for s, g in zip(grp.splits, geoms)]
            grp.bind(xs, dzs, wss, "cuda")
        with hip.options(wgrad_ring=0), X.ran("wgrad_group_kernel"):
            grp.run()
        torch.cuda.synchronize()
        return list(zip(wss, grp.splits))
    _batched_wgrad(geoms, dt, 40 + dt, launch, "grouped wgrad")


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_hwgrad2(dt):
    """urso_conv_wgrad_partial2 (hwgrad2_kernel): the ragged_unequal pair of test_hwgrad2_kernel."""
    hip = _hip()
    gs = [hip.geom(B, H, W, C, H, W, N, 3, 3, 1, 1, 1, 1) for (B, H, W, C, N) in ((4, 33, 41, 128, 128), (3, 17, 23, 256, 128))]
    sp = hip.conv_wgrad_pair_splits(gs[0], gs[1], dt)
    assert sp is not None

    def launch(xs, dzs):
        wss = [torch.full((s * (9 * g.C * g.N + hip.WGRAD_PART_PAD) + s * g.N + 64,), float("nan"), device="cuda") for s, g in zip(sp, gs)]
        with X.ran("hwgrad2_kernel"):
            hip.conv_wgrad_partial2(gs[0], gs[1], dt, xs[0], dzs[0], wss[0], xs[1], dzs[1], wss[1])
        torch.cuda.synchronize()
        return list(zip(wss, sp))
    _batched_wgrad(gs, dt, 60 + dt, launch, "hwgrad2")


def test_finalize_into_gradients_and_norm_slots():
    """urso_param_grad_finalize_sq on the stem's shape (K = 147, N = 64): the four poisons in four elements of dw_raw and one NaN in the
    column sums.  gW, gb, ggamma, gbeta take the class of finalize64's closed form, every other element keeps its bits, and the squared-norm
    slots -- what the step's normsq is summed from -- are not all finite."""
    hip = _hip()
    K, N, ldn, eps, wd = 147, 64, 64, 1e-3, 1e-4
    g = torch.Generator().manual_seed(147)
    dw, cs = torch.randn(K, ldn, generator=g), torch.randn(N, generator=g) * 5
    W, b = torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    gamma, mean, var = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    NF.premise_nonzero(W, "W (ggamma sums W dw_raw)")
    nslots = hip.param_grad_finalize_sq_slots(K, N)
    fixed = [t.cuda() for t in (W, b, gamma, mean, var)]

    def run(dw_, cs_, fill):
        out = {k: torch.full((n,), fill, device="cuda") for k, n in (("gw", K * N), ("gb", N), ("ggamma", N), ("gbeta", N))}
        slots = torch.full((nslots,), fill, device="cuda")
        ws = torch.empty(hip.param_grad_finalize_ws_bytes(K, N) // 4 + 4, device="cuda")
        with X.ran("finalize_mat_kernel"):
            hip.param_grad_finalize_sq(K, N, ldn, dw_.cuda(), cs_.cuda(), fixed[0], fixed[1], fixed[2], fixed[3], fixed[4], eps, wd, 1, 1,
                                       out["gw"], out["gb"], out["ggamma"], out["gbeta"], ws, slots)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}, slots.cpu()
    dwp = dw
    for i, pname in enumerate(NF.POISON_NAMES):
        dwp = NF.put(dwp, (31 * i + 5, 11 * i + 3), pname)
    csp = NF.put(cs, 50, "nan_neg")
    clean, slots_c = run(dw, cs, TK.SENTINEL)
    got, slots = run(dwp, csp, OTHER_SENTINEL)
    assert bool(torch.isfinite(slots_c).all())
    ref_c, ref_p = X.finalize64(dw[:, :N], cs, W, b, gamma, mean, var, eps, wd), X.finalize64(dwp[:, :N], csp, W, b, gamma, mean, var, eps, wd)
    for name in ("gw", "gb", "ggamma", "gbeta"):
        rp = ref_p[name][0].reshape(-1)
        NF.assert_class_parity(got[name], clean[name], rp, NF.dependency(ref_c[name][0].reshape(-1), rp), "finalize " + name)
    assert not bool(torch.isfinite(slots).all()) and not math.isfinite(float(slots.double().sum())), "the squared-norm slots hide the poison"


@pytest.mark.parametrize("dt", [1, 2], ids=DT_IDS.get)
def test_winograd_keeps_other_tiles(dt):
    """conv_winograd.hip (opt-in, URSO_WINOGRAD = 1).  Its input transform takes differences over a 4 x 4 window, so an infinity
    legitimately turns into NaN over the whole 2 x 2 output tile: class parity is not asked.  What is: every element that depends on the
    poison and whose float64 reference is non-finite is non-finite, and the output tiles whose window does not hold the poisoned pixel
    keep every bit."""
    hip = _hip()
    case = (2, 9, 15, 64, 64, 3, 1, (1, 1), "wino_c64")
    B, H, W, C, N = case[:5]
    R = _ref(case, dt)
    wf, _, biasf = TK.prep_weights(R.w, dt, R.bias)
    g = hip.geom(B, H, W, C, H, W, N, 3, 3, 1, 1, 1, 1)

    def run(x, fill):
        ws = torch.full((hip.conv_winograd_ws_bytes(g, dt) // 4 + 16,), float("nan"), dtype=torch.float32, device="cuda")
        y = TK.full((B, H, W, N), dt, fill)
        with X.ran("wino_filter_kernel"):
            hip.conv_winograd_fwd(g, dt, hip.EPI_RELU, x.cuda(), wf, biasf, y, ws)
        torch.cuda.synchronize()
        return y.cpu()
    xs = _stored(R.x, dt)
    xp, tiles = xs, torch.zeros(B, H, W, N, dtype=torch.bool)
    for i, (pname, (b, y, x)) in enumerate(zip(NF.POISON_NAMES, _corners(4, B, H, W, 3, 1))):
        NF.premise_nonzero(R.w[:, :, 3 * i + 1, :], "filter taps")
        xp = NF.put(xp, (b, y, x, 3 * i + 1), pname)
        for ty in range((H + 1) // 2):
            for tx in range((W + 1) // 2):
                if 2 * ty - 1 <= y <= 2 * ty + 2 and 2 * tx - 1 <= x <= 2 * tx + 2:
                    tiles[b, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
    ref = torch.relu(TK._conv64(xp.double(), R.w.double(), 1, (1, 1), H, W) + R.bias.double())
    dep = NF.dependency(torch.relu(R.zn), ref)
    assert bool((tiles | ~dep).all()), "a dependent element lies outside the poisoned tiles"
    got, clean = run(xp, OTHER_SENTINEL), run(xs, TK.SENTINEL)
    must = dep & (NF.classes(ref) != NF.FINITE)
    assert int(must.sum()) > 0 and not bool(torch.isfinite(got[must].float()).any()), "a dependent element of the Winograd output is finite"
    assert torch.equal(NF._bits(got)[~tiles], NF._bits(clean)[~tiles]), "the poison reached an output tile that does not read it"


# ====================================================================================================== the Engine
GEOM = dict(backbone="resnet18", h=64, w=128, batch=3)          # tests/test_loss_scale_gpu.py
HEADS = dict(regress_ori=True, regress_loc=True)
TORCH_DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
NAN_BITS = {"nan_pos": 0x7FC00000, "nan_neg": 0xFFC00000}


@functools.lru_cache(maxsize=None)
def _batch(seed):
    cfg = make_config(dtype="float32", **GEOM, **HEADS)
    img, loc, ori, _ = synthetic_batch(cfg, 3, seed=seed)
    return img, loc, ori


def _with_nan_pixel(img, sign):
    out = np.array(img, dtype=np.float32, copy=True)
    out.view(np.uint32)[1, 30, 61, 1] = NAN_BITS[sign]
    assert np.isnan(out[1, 30, 61, 1]) and np.isnan(out).sum() == 1
    return out


def _oracle_forward(w, img, cfg, tdt, hook=None):
    from oracle import graph_ref as G
    with torch.no_grad():
        loc, ori = G.forward(G.to_torch(w, requires_grad=False), torch.tensor(img), cfg, relu_hook=hook, q=G.StorageRounding(tdt))
    return loc, ori


def _engine_outputs(eng, img):
    eng.load_batch(img)
    eng.forward()
    torch.cuda.synchronize()
    return [t.clone().cpu() for t in eng.outputs()]


@pytest.mark.parametrize("stem_pool", [1, 0])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_engine_inference_keeps_a_nan_pixel(dtype, stem_pool):
    """One NaN pixel (either sign) in image 1 of a molded float batch: wherever oracle.graph_ref's outputs are non-finite the engine's are
    too (torch.relu and F.max_pool2d keep a NaN), and images 0 and 2 -- frozen BN: no image reads another -- keep every bit."""
    from ursonet_amd.engine import Engine
    hip = _hip()
    cfg = make_config(dtype=dtype, **GEOM, **HEADS)
    img = _batch(11)[0]
    with hip.options(stem_pool=stem_pool):
        eng = Engine(cfg, "inference", seed=3, randomize_bn=True)
        assert any("maxpool" in (l or "") for l in eng.labels["fwd"]), eng.labels["fwd"][:4]
        fused = any((l or "").endswith("+maxpool") for l in eng.labels["fwd"])
        assert fused == bool(stem_pool), "stem_pool = %d did not choose the stem's launch" % stem_pool
        w = eng.get_weights()
        clean = _engine_outputs(eng, img)
        assert all(bool(torch.isfinite(t).all()) for t in clean)
        for sign in ("nan_pos", "nan_neg"):
            bad = _with_nan_pixel(img, sign)
            got = _engine_outputs(eng, bad)
            want = _oracle_forward(w, bad, cfg, TORCH_DT[dtype])
            assert not bool(torch.isfinite(want[0][1]).any()) and not bool(torch.isfinite(want[1][1]).any()), "the oracle lost the NaN"
            for name, g_, w_, c_ in zip(("loc", "ori"), got, want, clean):
                lost = ~torch.isfinite(w_) & torch.isfinite(g_)
                assert not bool(lost.any()), "%s %s: %d outputs are finite where the oracle's are not: %s" % (
                    sign, name, int(lost.sum()), g_[1].tolist())
                assert torch.equal(NF._bits(g_[[0, 2]]), NF._bits(c_[[0, 2]])), "%s %s: the NaN of image 1 reached another image" % (sign, name)


def test_engine_fp16_forward_overflow_reaches_the_outputs():
    """stage3_unit1_conv1's kernel x 2**p, p raised until the oracle's stored fp16 activation behind it (its ReLU's output, rounded to
    fp16) holds inf in every image -- the asserted premise.  The next layer sums +inf x w over both signs of w: NaN, which the oracle's
    ReLUs keep to the outputs.  The engine's outputs are non-finite wherever the oracle's are."""
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype="float16", **GEOM, **HEADS)
    img = _batch(11)[0]
    eng = Engine(cfg, "inference", seed=3, randomize_bn=True)
    w = eng.get_weights()
    layer = "stage3_unit1_conv1"
    base = np.array(w[layer]["kernel"], copy=True)
    seen = {}

    def hook(site, pre):
        if site == layer:
            seen["inf"] = torch.isinf(torch.relu(pre).to(torch.float16)).flatten(1).any(1)
        return None
    for p in range(4, 40, 2):
        w[layer]["kernel"] = base * np.float32(2.0 ** p)
        want = _oracle_forward(w, img, cfg, torch.float16, hook)
        if bool(seen["inf"].all()):
            break
    assert bool(seen["inf"].all()) and float(np.abs(w[layer]["kernel"]).max()) < 65504, "no power of two overflows the stored activation"
    print("stage-3 kernel x 2**%d: the oracle's fp16 activation holds inf in every image" % p)
    assert not bool(torch.isfinite(want[0]).all()) and not bool(torch.isfinite(want[1]).all())
    eng.set_weights(w)
    got = _engine_outputs(eng, img)
    for name, g_, w_ in zip(("loc", "ori"), got, want):
        lost = ~torch.isfinite(w_) & torch.isfinite(g_)
        assert not bool(lost.any()), "%s: %d of %d outputs are finite where the oracle's are not: %s" % (name, int(lost.sum()), lost.numel(), g_.tolist())


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(NF._bits(a), NF._bits(b))


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_engine_training_skips_the_step_with_a_nan_pixel(optimizer):
    """fp16, LOSS_SCALE = "dynamic".  The clean batch is replayed until a step is applied (at most 30 replays: the scale halves from its
    default until nothing overflows), so the scale is one the network trains at.  Then the same batch with one NaN pixel: the squared
    norm is non-finite; weights, momentum (Adam: both moments, vhat, t) keep every bit and the loss-scale state is
    next_state(state, False).  The clean batch after it is applied."""
    from ursonet_amd.engine import Engine
    from ursonet_amd import loss_scale as LS
    cfg = make_config(dtype="float16", **GEOM, **HEADS)
    cfg.OPTIMIZER, cfg.TRAIN_BN, cfg.LOSS_SCALE = optimizer, False, "dynamic"
    eng = Engine(cfg, "training", seed=3, randomize_bn=True)
    img, loc, ori = _batch(11)

    def state():
        t = [eng.flat_w, eng.flat_v]
        if eng.adam:
            t += [eng.flat_v2, eng.flat_vhat, eng.hyper]
        return [x.clone() for x in t]
    eng.load_batch(img, loc, ori)
    w0 = eng.flat_w.clone()
    for _ in range(30):
        eng.step(); torch.cuda.synchronize()
        if not _same_bits(eng.flat_w, w0):
            break
    assert not _same_bits(eng.flat_w, w0) and bool(torch.isfinite(eng.normsq).all()), "no step of the clean batch was applied"
    eng.load_batch(_with_nan_pixel(img, "nan_neg"), loc, ori)
    before, ls0 = state(), eng.ls_state.tolist()
    eng.step(); torch.cuda.synchronize()
    assert not bool(torch.isfinite(eng.normsq).all()), "normsq %r is finite: the NaN pixel was lost on the way" % eng.normsq.tolist()
    for name, x, y in zip(("weights", "momentum", "m", "vhat", "hyper"), before, state()):
        assert _same_bits(x, y), "the skipped step changed %s" % name
    ls1 = LS.next_state(ls0, False)
    assert eng.ls_state.tolist() == ls1 and ls1[LS.SKIPPED_TOTAL] == ls0[LS.SKIPPED_TOTAL] + 1 and eng.loss_scale()["last_step_skipped"]
    eng.load_batch(img, loc, ori)
    eng.step(); torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.normsq).all()) and eng.ls_state.tolist() == LS.next_state(ls1, True)
    assert not _same_bits(eng.flat_w, before[0]) and bool(torch.isfinite(eng.flat_w).all()), "the clean step after the skipped one was not applied"
