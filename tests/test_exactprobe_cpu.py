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


# ---- the packed stem, the max-pool's gradient routing, padded filter columns, two-segment reductions
SB, SH, SW, SN = 2, 12, 20, 8                  # molded input [SB][SH][SW][4], conv output [SB][SH/2][SW/2][SN]


def stem_case(t, exact, seed=11, up=1):
    """Molded input [SB][up SH][up SW][4] and a [7][7][3][SN] filter (up = 2: the conv output is SH x SW)."""
    g = torch.Generator().manual_seed(seed)
    x4 = torch.zeros(SB, up * SH, up * SW, 4)
    if exact:
        x4[..., :3] = X.int_operands((SB, up * SH, up * SW, 3), t, 3, 0.6, seed)
        w = X.int_operands((7, 7, 3, SN), t, 3, 0.6, seed + 1)
    else:
        x4[..., :3] = torch.randn(SB, up * SH, up * SW, 3, generator=g).to(t).float()
        w = (torch.randn(7, 7, 3, SN, generator=g) / 12).to(t).float()
    return x4, w


def test_stem_taps_match_the_kernel_pack_and_a_plain_7x7_conv():
    """stem_taps is the layout of urso_stem_weight_pack (its index formula, element by element) and stem_conv64 with it is the 7x7 /
    s2 / ZeroPadding2D(3) conv of the 3 real channels; stem_untaps inverts stem_taps."""
    x4, w = stem_case(torch.bfloat16, exact=True)
    packed = X.stem_taps(w).permute(3, 0, 1, 2).reshape(-1)
    for i in range(packed.numel()):                    # prep.hip stem_pack_kernel: i = ((n * 7 + ky) * 4 + kp) * 8 + cp
        cp, kp, ky, n = i & 7, (i >> 3) & 3, (i >> 5) % 7, i // 224
        q, c = 2 * kp + (cp >> 2), cp & 3
        want = float(w[ky, q - 1, c, n]) if q >= 1 and c < 3 else 0.0
        assert float(packed[i]) == want, i
    plain = F.conv2d(F.pad(x4[..., :3].double().permute(0, 3, 1, 2), (3, 3, 3, 3)), w.double().permute(3, 2, 0, 1), stride=2)
    assert torch.equal(X.stem_conv64(x4, X.stem_taps(w)), plain[:, :, :SH // 2, :SW // 2].permute(0, 2, 3, 1))
    assert torch.equal(X.stem_untaps(X.stem_taps(w)), w.double())


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_stem_unpack_counting_a_pad_tap_is_rejected(t):
    """A weight-gradient unpack that reads window pixel q = kx (the pad tap q = 0 counted, the last real tap dropped) instead of kx + 1."""
    for exact in (True, False):
        x4, _ = stem_case(t, exact)
        g = torch.Generator().manual_seed(3)
        dz = (X.int_operands((SB, SH // 2, SW // 2, SN), t, 3, 0.8, 4) if exact else torch.randn(SB, SH // 2, SW // 2, SN, generator=g).to(t)).double()
        gt, mag = X.stem_wgrad64(x4, dz), X.stem_wgrad64(x4.abs(), dz.abs())
        got = gt.float().double()                       # fp32 output of a correct kernel
        assert float(gt[:, :, 3].abs().max()) == 0 and float(gt[:, 0].abs().max()) > 0    # the zero channel; the pad tap sees pixels
        ref, rmag = X.stem_untaps(gt), X.stem_untaps(mag)
        if exact:
            X.assert_exact(X.stem_untaps(got), ref)
            with pytest.raises(AssertionError, match="elements wrong"):
                X.assert_exact(got[:, :7, :3], ref)
        else:
            X.assert_rounded_once(X.stem_untaps(got), ref, rmag, torch.float32, SB * SH * SW // 4)
            with pytest.raises(AssertionError, match="rounded-once bound"):
                X.assert_rounded_once(got[:, :7, :3], ref, rmag, torch.float32, SB * SH * SW // 4)


def pool_case(t, seed=21):
    """Post-ReLU conv output with ties and all-zero windows, its pooled gradient and arg-max bytes (urso_maxpool3x3s2_fwd's encoding)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.relu(X.int_operands((SB, SH, SW, SN), t, 3, 0.5, seed))
    best = torch.full((SB, SH // 2, SW // 2, SN), -math.inf, dtype=torch.float64)
    arg = torch.zeros(best.shape, dtype=torch.int64)
    yp = torch.full((SB, SH + 1, SW + 1, SN), -math.inf, dtype=torch.float64)
    yp[:, :SH, :SW] = y.double()
    for ky in range(3):
        for kx in range(3):
            v = yp[:, ky:ky + SH:2, kx:kx + SW:2]
            take = v > best
            best, arg = torch.where(take, v, best), torch.where(take, torch.full_like(arg, 3 * ky + kx), arg)
    am = (arg + 16 * (best <= 0).long()).to(torch.uint8)
    dpool = torch.randn(best.shape, generator=g).to(t).double()
    return am, dpool


def route_neighbour(dpool, am):
    """A router that sends a window's gradient to the pixel right of its arg-max where that is kx = 0 (always inside the image)."""
    a = am.to(torch.int64)
    tap = a & 15
    return X.pool_route(dpool, (tap + (tap % 3 == 0).long() + (a & 16)).to(torch.uint8), SH, SW)[0]


def route_rounding_every_add(dpool, am, t):
    """A router that rounds to the storage type after every window it adds (instead of once per conv pixel)."""
    B_, PH, PW, C_ = dpool.shape
    out = torch.zeros(B_, SH + 1, SW + 1, C_, dtype=torch.float64)
    a = am.to(torch.int64)
    for ky in range(3):
        for kx in range(3):
            sel = (((a & 16) == 0) & ((a & 15) == 3 * ky + kx)).double()
            out[:, ky:ky + 2 * PH:2, kx:kx + 2 * PW:2] = X.round_to(out[:, ky:ky + 2 * PH:2, kx:kx + 2 * PW:2] + sel * dpool, t)
    return out[:, :SH, :SW]


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_pool_route_and_its_faults(t):
    """pool_route: every live window's gradient reaches its arg-max pixel, dead windows (bit 4) nothing; the stem's weight gradient from
    the routed gradient rounded once rejects a router that picks a neighbouring tap, a gradient left unrounded and one rounded twice."""
    am, dpool = pool_case(t)
    routed, mag = X.pool_route(dpool, am, SH, SW)
    live = (am.long() & 16) == 0
    assert 0.05 < float((~live).double().mean()) < 0.95
    assert abs(float(routed.sum()) - float((dpool * live).sum())) < 1e-9 and torch.equal(mag.sum(), (dpool.abs() * live).sum())
    dz = X.round_to(routed, t)
    assert not torch.equal(dz, routed) and int((mag > 0).sum()) > int((routed != 0).sum()) // 2
    x4, _ = stem_case(t, exact=False, up=2)
    ref, rmag = X.stem_wgrad64(x4, dz), X.stem_wgrad64(x4.abs(), dz.abs())
    K = SB * SH * SW
    X.assert_rounded_once(X.stem_wgrad64(x4, dz).float(), ref, rmag, torch.float32, K)
    for bad in (X.round_to(route_neighbour(dpool, am), t), routed, route_rounding_every_add(dpool, am, t)):
        assert not torch.equal(bad, dz)
        with pytest.raises(AssertionError, match="rounded-once bound"):
            X.assert_rounded_once(X.stem_wgrad64(x4, bad).float(), ref, rmag, torch.float32, K)
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_exact(route_neighbour(dpool.round(), am), X.pool_route(dpool.round(), am, SH, SW)[0])


def test_padded_filter_columns_must_be_zero():
    y = torch.zeros(2, 3, 4, 32)
    y[..., :24] = torch.randn(2, 3, 4, 24)
    X.assert_zero_columns(y, 24)
    y[1, 2, 3, 30] = 2.0 ** -20
    with pytest.raises(AssertionError, match="padded columns"):
        X.assert_zero_columns(y, 24)


def test_pack_bits_element_order():
    keep = (torch.rand(64, generator=torch.Generator().manual_seed(2)) > 0.5).to(torch.int32)
    bits = X.pack_bits(keep)
    assert torch.equal(((bits.to(torch.int32).reshape(-1, 1) >> torch.arange(8)) & 1).reshape(-1), keep)


@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_two_segment_rounded_between_segments_is_rejected(t):
    """Two reduction segments summed in one fp32 accumulator and rounded once pass; rounding segment 1 to the storage type before adding
    segment 2 (the two-launch form) does not."""
    g = torch.Generator().manual_seed(8)
    Mr, K0, K1, Nn = 32, 1024, 1024, 256
    x0, x1 = (torch.randn(Mr, K0, generator=g).to(t).float(), torch.randn(Mr, K1, generator=g).to(t).float())
    w0, w1 = ((torch.randn(Nn, K0, generator=g) / 32).to(t).float(), (torch.randn(Nn, K1, generator=g) / 32).to(t).float())
    ref, mag = X.two_segment(x0, w0, x1, w1)
    s0, s1 = (x0 @ w0.T).double(), (x1 @ w1.T).double()                  # fp32 segment sums
    X.assert_rounded_once(rne((s0 + s1).float().double(), t), ref, mag, t, K0 + K1)
    with pytest.raises(AssertionError, match="rounded-once bound"):
        X.assert_rounded_once(rne(rne(s0, t) + s1, t), ref, mag, t, K0 + K1)


def test_wgrad64_is_the_filter_gradient_of_a_strided_padded_conv():
    g = torch.Generator().manual_seed(9)
    for (Bq, Hq, Wq, Cq, Nq, k, s, pad) in [(2, 9, 11, 5, 7, 3, 2, (1, 1)), (2, 8, 10, 4, 6, 3, 2, (0, 0)), (1, 6, 6, 3, 4, 1, 2, (0, 0)),
                                            (2, 5, 7, 3, 5, 3, 1, (1, 1))]:
        OH, OW = ((Hq + 2 * pad[0] - k) // s + 1, (Wq + 2 * pad[1] - k) // s + 1) if pad[0] or s == 1 else (-(-Hq // s), -(-Wq // s))
        x = torch.randn(Bq, Hq, Wq, Cq, generator=g, dtype=torch.float64)
        dz = torch.randn(Bq, OH, OW, Nq, generator=g, dtype=torch.float64)
        w = torch.zeros(k, k, Cq, Nq, dtype=torch.float64, requires_grad=True)
        pb, pr = max((OH - 1) * s + k - Hq - pad[0], 0), max((OW - 1) * s + k - Wq - pad[1], 0)
        y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pad[1], pr, pad[0], pb)), w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
        (y * dz).sum().backward()
        assert float((X.wgrad64(x, dz, k, s, pad) - w.grad).abs().max()) < 1e-12
