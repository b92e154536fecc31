"""The exact-integer and rounded-once helpers (tests/exactprobe.py) have teeth: torch "simulated kernels" compute a 3x3 conv
layer (+ bias + residual) and its filter gradient correctly -- fp32 accumulation, one round-to-nearest-even store -- and
with the faults a hand-written kernel can have.  The correct kernel must pass, every fault must fail:

* rounding faults (truncating store, double rounding, 16-bit split partials) on real operands pre-rounded to the storage
  type: assert_rounded_once;
* structural faults (one wrong element, a dropped final pixel tile, transposed 3x3 taps) on exact integer operands:
  assert_exact, and on the real operands: assert_rounded_once.

Integer data cannot show a rounding fault by construction (premise() makes every value exact), which is why the GPU probes
run both kinds of data."""
import math

import pytest
import torch
import torch.nn.functional as F

import exactprobe as X

DTS = [torch.bfloat16, torch.float16]
B, H, W, C, N = 2, 12, 20, 128, 64
KCONV = 9 * C
TILE = 64                               # pixels of the simulated kernel's last tile


def conv64(x, w):
    """NHWC x HWIO, 3x3 stride 1 pad 1, in float64."""
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(3, 2, 0, 1).double(), padding=1).permute(0, 2, 3, 1)


def conv32(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2).float(), w.permute(3, 2, 0, 1).float(), padding=1).permute(0, 2, 3, 1).double()


def rne(v, t):
    return v.to(t).to(torch.float64)


def trunc(v, t):
    """Store that truncates toward zero instead of rounding to nearest even."""
    v = v.to(torch.float64)
    r = rne(v, t)
    up = r.abs() > v.abs()
    step = X.ulp(r, t)
    small = X.ulp(r.abs() - step, t)          # below a power of two the spacing halves
    return torch.where(up, r - torch.sign(r) * torch.minimum(step, small), r)


def split_partials(x, w, t, chunks=4):
    """Reduction split over channel chunks whose fp32 partials are stored in 16 bits, then summed."""
    cs = C // chunks
    acc = torch.zeros(B, H, W, N, dtype=torch.float64)
    for i in range(chunks):
        acc = acc + rne(conv32(x[..., i * cs:(i + 1) * cs], w[:, :, i * cs:(i + 1) * cs]), t)
    return acc.float().double()


def one_wrong(y, ref, t, exact):
    """y with one element off by one unit (the element where y is closest to ref, i.e. hardest to see)."""
    y = y.clone().reshape(-1)
    if exact:
        y[y.numel() // 3] += 1
    else:
        i = int(((y - ref.reshape(-1)).abs() / X.ulp(ref.reshape(-1), t)).argmin())
        y[i] += X.ulp(y[i:i + 1], t)[0]
    return y.reshape(ref.shape)


def dropped_tile(y):
    y = y.clone().reshape(-1, N)
    y[-TILE:] = 0
    return y.reshape(B, H, W, N)


def layer(t, exact, seed=0):
    if exact:
        amax, d = X.int_plan(KCONV, t)
        x = X.int_operands((B, H, W, C), t, amax, d, seed)
        w = X.int_operands((3, 3, C, N), t, amax, d, seed + 1)
        bias = X.int_operands((N,), t, 3, 0.8, seed + 2)
        res = X.int_operands((B, H, W, N), t, 3, 0.8, seed + 3)
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, H, W, C, generator=g).to(t).float()
        w = (torch.randn(3, 3, C, N, generator=g) / math.sqrt(KCONV)).to(t).float()
        bias = torch.randn(N, generator=g) * 0.1
        res = torch.randn(B, H, W, N, generator=g).to(t).float()
    ref = conv64(x, w) + bias.double() + res.double()
    mag = conv64(x.abs(), w.abs()) + bias.double().abs() + res.double().abs()
    return x, w, bias, res, ref, mag


def simulated_conv(kind, t, x, w, bias, res, ref):
    b, r = bias.double(), res.double()
    if kind == "correct":
        return rne(conv32(x, w) + b + r, t)
    if kind == "truncating_store":
        return trunc(conv32(x, w) + b + r, t)
    if kind == "double_rounding":
        return rne(rne(conv32(x, w) + b, t) + r, t)
    if kind == "split_partials_16bit":
        return rne(split_partials(x, w, t) + b + r, t)
    if kind == "taps_transposed":
        return rne(conv32(x, w.transpose(0, 1)) + b + r, t)
    good = rne(conv32(x, w) + b + r, t)
    if kind == "one_wrong_element":
        return one_wrong(good, ref, t, exact=bool(torch.equal(x, x.round())))
    if kind == "dropped_final_tile":
        return dropped_tile(good)
    raise ValueError(kind)


ROUNDING_FAULTS = ["truncating_store", "double_rounding", "split_partials_16bit"]
STRUCTURAL_FAULTS = ["one_wrong_element", "dropped_final_tile", "taps_transposed"]


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_correct_conv_passes_both_checks(t):
    x, w, bias, res, ref, mag = layer(t, exact=False)
    ratio = X.assert_rounded_once(simulated_conv("correct", t, x, w, bias, res, ref), ref, mag, t, KCONV + 2)
    assert ratio <= 1.0
    x, w, bias, res, ref, mag = layer(t, exact=True)
    X.premise(t, stored=[("y", ref)], mags=[("y", mag)])
    X.assert_sensitive(ref, conv64(x[..., :-1], w[:, :, :-1]) + bias.double() + res.double())
    X.assert_exact(simulated_conv("correct", t, x, w, bias, res, ref), ref)


@pytest.mark.parametrize("kind", ROUNDING_FAULTS + STRUCTURAL_FAULTS)
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_rounded_once_rejects_every_fault(t, kind):
    x, w, bias, res, ref, mag = layer(t, exact=False)
    got = simulated_conv(kind, t, x, w, bias, res, ref)
    with pytest.raises(AssertionError, match="rounded-once bound"):
        X.assert_rounded_once(got, ref, mag, t, KCONV + 2)


@pytest.mark.parametrize("kind", STRUCTURAL_FAULTS)
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_exact_rejects_every_structural_fault(t, kind):
    x, w, bias, res, ref, mag = layer(t, exact=True)
    got = simulated_conv(kind, t, x, w, bias, res, ref)
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_exact(got, ref)


# ---- filter gradient: dW[k][n] = sum over M pixels of x[m][k] dz[m][n], fp32 output
M, KW, NW, SPLITS = 4096, 64, 64, 32


def wgrad_case(t, exact, seed=5):
    if exact:
        amax, d = X.int_plan(M, torch.float32, share=64)
        x = X.int_operands((M, KW), t, amax, d, seed)
        dz = X.int_operands((M, NW), t, amax, d, seed + 1)
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(M, KW, generator=g).to(t).float()
        dz = torch.randn(M, NW, generator=g).to(t).float()
    return x, dz, x.double().T @ dz.double(), x.double().abs().T @ dz.double().abs()


def simulated_wgrad(kind, t, x, dz, ref):
    f32 = lambda a: a.float().double()
    parts = [f32(x[s::SPLITS].T @ dz[s::SPLITS]) for s in range(SPLITS)]        # fp32 partial per split
    if kind == "correct":
        return f32(sum(parts))
    if kind == "split_partials_16bit":
        return f32(sum(rne(p, t) for p in parts))
    if kind == "one_wrong_element":                    # one dW element misses the product of one pixel (its largest)
        good = f32(sum(parts))
        i = int((x[:, 0].abs() * dz[:, 0].abs()).argmax())
        good[0, 0] -= float(x[i, 0]) * float(dz[i, 0])
        return good
    if kind == "dropped_final_tile":
        return f32(x[:-TILE].T @ dz[:-TILE])
    if kind == "transposed":
        return f32(sum(parts)).T.contiguous()
    raise ValueError(kind)


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_correct_filter_gradient_passes_both_checks(t):
    x, dz, ref, mag = wgrad_case(t, exact=False)
    assert X.assert_rounded_once(simulated_wgrad("correct", t, x, dz, ref), ref, mag, torch.float32, M) <= 1.0
    x, dz, ref, mag = wgrad_case(t, exact=True)
    X.premise(torch.float32, stored=[("dW", ref)], mags=[("dW", mag)])
    X.assert_exact(simulated_wgrad("correct", t, x, dz, ref), ref)


@pytest.mark.parametrize("kind", ["split_partials_16bit", "one_wrong_element", "dropped_final_tile", "transposed"])
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_filter_gradient_faults_rejected(t, kind):
    x, dz, ref, mag = wgrad_case(t, exact=False)
    with pytest.raises(AssertionError, match="rounded-once bound"):
        X.assert_rounded_once(simulated_wgrad(kind, t, x, dz, ref), ref, mag, torch.float32, M)
    if kind != "split_partials_16bit":            # integer partials are exact in 16 bits as well: the real-valued probe's job
        x, dz, ref, mag = wgrad_case(t, exact=True)
        with pytest.raises(AssertionError, match="elements wrong"):
            X.assert_exact(simulated_wgrad(kind, t, x, dz, ref), ref)


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_premise_refuses_unrepresentable_data(t):
    lim = X.INT_LIMIT[t]
    ok = torch.tensor([float(lim), -float(lim), 3.0], dtype=torch.float64)
    X.premise(t, stored=[("y", ok)], mags=[("y", ok.abs())])
    with pytest.raises(AssertionError, match="not representable"):
        X.premise(t, stored=[("y", torch.tensor([float(lim + 1)], dtype=torch.float64))])
    with pytest.raises(AssertionError, match="not representable"):
        X.premise(t, stored=[("mid", torch.tensor([0.1], dtype=torch.float64))])
    with pytest.raises(AssertionError, match="2\\^24"):
        X.premise(t, mags=[("y", torch.tensor([2.0 ** 24], dtype=torch.float64))])
    # the plan for a long reduction keeps a real layer's sums inside the limit
    x, w, bias, res, ref, mag = layer(t, exact=True)
    X.premise(t, stored=[("y", ref)], mags=[("y", mag)])


def test_insensitive_data_is_refused():
    ref = torch.zeros(100, dtype=torch.float64)
    ref[:10] = 1
    with pytest.raises(AssertionError, match="nonzero"):
        X.assert_sensitive(ref)
    ref[:50] = 1
    with pytest.raises(AssertionError, match="last input channel"):
        X.assert_sensitive(ref, ref.clone())
    with pytest.raises(AssertionError, match="exactly 0"):
        X.assert_sensitive(ref, pre64=torch.ones(1000, dtype=torch.float64))


@pytest.mark.parametrize("t", [torch.bfloat16, torch.float16, torch.float32])
def test_ulp_and_truncation_model(t):
    v = torch.tensor([1.0, 1.5, 3.0, 1000.0], dtype=torch.float64)
    p = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}[t]
    assert torch.equal(X.ulp(v, t), torch.tensor([2.0 ** (1 - p), 2.0 ** (1 - p), 2.0 ** (2 - p), 2.0 ** (10 - p)], dtype=torch.float64))
    r = torch.randn(10000, dtype=torch.float64) * 7
    tr = trunc(r, t)
    assert bool((tr.abs() <= r.abs()).all()) and torch.equal(rne(tr, t), tr)
    assert bool(((r - tr).abs() < X.ulp(r, t)).all())


def test_exact_refuses_a_reference_of_another_layout():
    ref = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    with pytest.raises(AssertionError, match="shape"):
        X.assert_exact(ref.T.contiguous().float(), ref)
    with pytest.raises(AssertionError, match="shape"):
        X.assert_rounded_once(ref.T.contiguous().float(), ref, ref.abs(), torch.bfloat16, 4)
