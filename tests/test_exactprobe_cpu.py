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


# =====================================================================================================================
# The step-tail references and bounds (losses, norm, optimizers, finalisation, batch-statistics BatchNorm): each accepts a plain
# fp32 restatement of the operation and rejects the planted faults below (>= 1 % of elements outside the bound; the dropped tail
# and the dropped sweep need one).
XENT_K = [1, 63, 64, 65, 257, 512, 4095, 4096, 4097, 13824, 16383, 16384, 16385, 32768]


def flush16(v, t):
    """16-bit store that flushes subnormal results to zero."""
    r = rne(v, t)
    return torch.where(r.abs() < 2.0 ** X._EMIN[t], torch.zeros_like(r), r)


def test_xent_restatement_inside_bound_on_every_probe_input():
    """exp as exp2(x * 1.442695) + pairwise fp32 sums stays inside softmax_xent_bounds on every input of the GPU probe; the largest
    ratios (printed) is recorded in the pull request."""
    worst = {"loss": 0.0, "row": 0.0, "dz fp32": 0.0, "dz bf16": 0.0, "dz fp16": 0.0}
    for K in XENT_K:
        for Bn in (1, 32):
            for psum in (1.0, 0.6):
                z, p = X.xent_inputs(Bn, K, psum)
                for relu in (0, 1):
                    if relu and K >= 63:
                        assert float((z == 0).sum()) / z.numel() >= 0.01
                    for dt in (0, 1, 2):
                        ref = X.softmax_xent64(z, p, 1.0, relu)
                        bnd = X.softmax_xent_bounds(z, p, 1.0, relu, dt)
                        got = X.softmax_xent32(z, p, 1.0, relu, dt)
                        for name, g, r, b in zip(("loss", "row", "dz " + ("fp32", "bf16", "fp16")[dt]), got, ref, bnd):
                            worst[name] = max(worst[name], X.assert_within(g, r, b, "%s K=%d B=%d" % (name, K, Bn)))
                    if K >= 63 and not relu:
                        assert float((ref[2] != 0).sum()) / ref[2].numel() >= 0.25
    print("softmax_xent restatement, largest ratio to the bound:", worst)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dt", [1, 2])
def test_xent_faults_rejected(dt):
    t = X.tdtype(dt)
    Bn, K = 32, 13824
    z, p = X.xent_inputs(Bn, K, 0.6)
    for relu in (0, 1):
        _, _, ref = X.softmax_xent64(z, p, 1.0, relu)
        bnd = X.softmax_xent_bounds(z, p, 1.0, relu, dt)[2]
        f32 = X.softmax_xent32(z, p, 1.0, relu, 0)[2].double()
        assert X.violations(rne(f32, t), ref, bnd) == 0
        # softmax * sum(p) - p (the gradient of the row loss with softmax scaled by the labels' mass)
        soft = torch.softmax(z.double(), 1)
        wrong = (soft * 0.6 - p.double()) / Bn
        if relu:
            wrong = wrong * (z > 0)
        assert X.violations(rne(wrong, t), ref, bnd) >= 0.01
        assert X.violations(trunc(f32, t), ref, bnd) >= 0.01                       # truncating store
        if dt == 2:
            assert X.violations(flush16(f32, t), ref, bnd) >= 0.01                 # subnormals flushed
            assert X.violations(rne(rne(f32, torch.bfloat16), t), ref, bnd) >= 0.01   # rounded to bf16, then to fp16
    # ReLU mask taken as z >= 0: the exact zeros (half of the logits) keep their gradient
    _, _, ref = X.softmax_xent64(z, p, 1.0, 1)
    bnd = X.softmax_xent_bounds(z, p, 1.0, 1, dt)[2]
    unmasked = X.softmax_xent32(z, p, 1.0, 0, dt)[2]
    assert X.violations(unmasked, ref, bnd) >= 0.01
    # the row loss with the labels' mass dropped (lse - sum p z)
    _, row, _ = X.softmax_xent64(z, p, 1.0, 0)
    wrong_row = torch.logsumexp(z.double(), 1) - (p.double() * z.double()).sum(1)
    assert X.violations(wrong_row.float(), row, X.softmax_xent_bounds(z, p, 1.0, 0, dt)[1]) >= 0.5


def test_fp16_subnormal_share_of_the_benchmark_softmax_gradient():
    """At B = 32, K = 24^3 nearly every nonzero fp16 gradient is subnormal (the numbers of the issue)."""
    z, p = X.xent_inputs(32, 13824, 1.0)
    _, _, ref = X.softmax_xent64(z, p, 1.0, 0)
    nz = ref != 0
    sub = nz & (ref.abs() < 2.0 ** -14)
    assert float(sub.sum()) / float(nz.sum()) > 0.9
    assert float((rne(ref, torch.float16)[nz] == 0).sum()) / float(nz.sum()) < 0.05


def _head(Bn, D, ld, seed, tiny=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randn(Bn, D, generator=g)
    x = torch.randn(Bn, ld, generator=g)
    for i in range(tiny):
        x[3 * i + 1] *= 1e-7                          # |x|^2 <= 1e-12: the clamp branch, with a nonzero dot
    return gt, x


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_regression_losses_accept_fp32_and_reject_faults(dt):
    t = X.tdtype(dt)
    for Bn, D in ((1, 3), (5, 3), (32, 4), (300, 3)):
        gt, x = _head(Bn, D, 8, Bn + D)
        f = lambda v: v.float()
        # rel_l2 / mse restated in fp32
        e = gt - x[:, :D]
        nd, ng = X.pairwise_sum32((e * e).reshape(-1)).sqrt(), X.pairwise_sum32((gt * gt).reshape(-1)).sqrt()
        loss, g, _ = X.rel_l2_64(gt, x, 0.7)
        bl, bg, _ = X.rel_l2_bounds(gt, x, 0.7, dt)
        got = F.pad(f(torch.tensor(-0.7)) / (nd * ng) * e, (0, 8 - D)).to(t)
        assert X.violations(got, g, bg) == 0 and X.violations(f(torch.tensor(0.7)) * nd / ng, loss, bl) == 0
        assert float((g[:, :D] != 0).sum()) / g[:, :D].numel() >= 0.25
        if dt and Bn == 300:                          # a truncating 16-bit store
            assert X.violations(trunc(F.pad(f(torch.tensor(-0.7)) / (nd * ng) * e, (0, 8 - D)).double(), t), g, bg) >= 0.01
        loss, g = X.mse64(gt, x, 0.7)
        bl, bg = X.mse_bounds(gt, x, 0.7, dt)
        e = x[:, :D] - gt
        got = F.pad(torch.tensor(2 * 0.7, dtype=torch.float32) / (Bn * D) * e, (0, 8 - D)).to(t)
        assert X.violations(got, g, bg) == 0
        assert X.violations(torch.tensor(0.7, dtype=torch.float32) * X.pairwise_sum32((e * e).reshape(-1)) / (Bn * D), loss, bl) == 0
        assert X.violations((got.double() * 1.01).to(t), g, bg) >= 0.25 * D / 8


@pytest.mark.parametrize("normalize", [0, 1])
def test_absdot_reference_and_clamp_branch(normalize):
    Bn, D, ld = 300, 4, 8
    gt, x = _head(Bn, D, ld, 7, tiny=10)
    gt[0], x[0] = 0, 0
    gt[0, 0], x[0, 1] = 1, 1                          # dot == 0 exactly: zero gradient, loss term 1
    x[2] = 0                                          # a row of zeros
    q, loss, dx, dot, _ = X.absdot64(gt, x, 0.9, normalize)
    assert float(dot[0]) == 0 and float(dx[0].abs().sum()) == 0 and float(dx[2].abs().sum()) == 0
    assert float((dx[:, D:] != 0).sum()) == 0
    # against autograd of the definition (rows away from the clamp)
    xr = x.double().clone().requires_grad_(True)
    xv = xr[:, :D]
    qq = xv * torch.rsqrt((xv * xv).sum(1, keepdim=True).clamp_min(X.ABSDOT_CLAMP)) if normalize else xv
    (X.f32v(0.9) * (1 - (gt.double() * qq).sum(1).abs()).mean()).backward()
    big = (x[:, :D].double() ** 2).sum(1) > 1e-6
    assert float((xr.grad[big] - dx[big]).abs().max()) <= 1e-12 * float(dx.abs().max())
    for dt in (0, 1, 2):
        bq, bl, bdx = X.absdot_bounds(gt, x, 0.9, normalize, dt)
        # fp32 restatement
        xv = x[:, :D]
        ss = (xv * xv).sum(1, keepdim=True)
        rinv = torch.rsqrt(ss.clamp_min(1e-12)) if normalize else torch.ones_like(ss)
        q32 = xv * rinv
        d32 = (gt * q32).sum(1, keepdim=True)
        dq = -torch.sign(d32) * torch.tensor(np.float32(0.9) / np.float32(Bn)) * gt
        proj = q32 * (q32 * dq).sum(1, keepdim=True)
        good = rinv * (dq - torch.where(ss > 1e-12, proj, torch.zeros_like(proj))) if normalize else dq
        assert X.violations(q32, q, bq) == 0
        assert X.violations(F.pad(good, (0, ld - D)).to(X.tdtype(dt)), dx, bdx) == 0
        assert X.violations(torch.tensor(np.float32(0.9)) * (1 - d32.abs()).mean(), loss, bl) == 0
        if normalize:                                 # without the clamp branch: the 10 tiny rows are wrong (10 x 4 of 300 x 8 values)
            nocl = rinv * (dq - proj)
            assert X.violations(F.pad(nocl, (0, ld - D)).to(X.tdtype(dt)), dx, bdx) >= 0.01


import numpy as np  # noqa: E402


def test_adam_lr_t_measured():
    """The measured error behind ADAM_LRT_REL (4 x the largest deviation of the float32 restatement of lr_t)."""
    worst = max(abs(float(X.adam_lr_t32(1e-3, 0.9, 0.999, t)) - X.adam_lr_t64(1e-3, 0.9, 0.999, t)) / X.adam_lr_t64(1e-3, 0.9, 0.999, t)
                for t in (1, 2, 3))
    assert worst <= X.ADAM_LRT_MEASURED and X.ADAM_LRT_REL == 4 * X.ADAM_LRT_MEASURED and worst >= 0.5 * X.ADAM_LRT_MEASURED


@pytest.mark.parametrize("case", ["unclipped", "clipped", "noclip", "mom0"])
def test_sgd_reference_accepts_fp32_and_rejects_faults(case):
    n = 1_000_003
    w, g, v, lr, mom, clip = X.sgd_data(n, case)
    nsq = float(X.pairwise_sum32(g * g))
    assert abs(nsq - float((g.double() ** 2).sum())) <= float(X.tree_sum_bound((g.double() ** 2).sum(), 21))
    w64, v64, bw, bv, ratio = X.sgd64(w, g, v, lr, mom, clip, nsq)
    assert ratio >= 0.1, ratio                                              # a wrong step shows in v
    norm = nsq ** 0.5
    assert clip == 0 or abs(norm - clip) > 0.01 * clip
    w32, v32 = X.sgd32(w, g, v, lr, mom, clip, nsq)
    assert X.violations(w32, w64, bw) == 0 and X.violations(v32, v64, bv) == 0
    assert float((v64 != 0).sum()) / n >= 0.25
    wf, vf = X.sgd32(w, g, v, lr, mom, clip, nsq, lr_factor=1.01)           # lr wrong by 1 %
    assert X.violations(vf, v64, bv) >= 0.01 and X.violations(wf, w64, bw) >= 0.01
    wf, vf = X.sgd32(w, g, v, lr, mom, clip, nsq, keep_from=n - n % 4, keep_to=n)      # the last n % 4 elements not updated
    assert X.violations(vf, v64, bv) > 0 and X.violations(wf, w64, bw) > 0
    wf, vf = X.sgd32(w, g, v, lr, mom, clip, nsq, keep_from=n // 2, keep_to=n)         # elements past the first sweep not updated
    assert X.violations(vf, v64, bv) > 0.4 and X.violations(wf, w64, bw) > 0.4


def test_adam_reference_accepts_fp32_and_rejects_faults():
    n = 10007
    g_ = torch.Generator().manual_seed(3)
    w = torch.randn(n, generator=g_)
    m, v, vh = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    f = np.float32
    for t in (1, 2, 3):
        hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-7, 5.0, float(t), float(f(1) - f(0.9)), float(f(1) - f(0.999))], dtype=torch.float32)
        g = torch.randn(n, generator=g_) * (3.0 if t == 2 else 0.01)        # step 2 is clipped
        nsq = float(X.pairwise_sum32(g * g))
        assert (nsq ** 0.5 >= 5.0) == (t == 2)
        ref = X.adam64(w, g, m, v, vh, hyper, nsq)
        got = X.adam32(w, g, m, v, vh, hyper, nsq)
        for name, val in zip(("w", "m", "v", "vhat"), got):
            assert X.violations(val, *ref[name]) == 0, (t, name)
        if t == 2:                                                          # v updated from the unclipped gradient
            bad = X.adam32(w, g, m, v, vh, hyper, nsq, v_from_unclipped=True)
            assert X.violations(bad[2], *ref["v"]) >= 0.01 and X.violations(bad[0], *ref["w"]) >= 0.01
            h2 = hyper.clone(); h2[0] *= 1.01                               # lr wrong by 1 %, clipped step
            assert X.violations(X.adam32(w, g, m, v, vh, h2, nsq)[0], *ref["w"]) >= 0.01
        w, m, v, vh = got


@pytest.mark.parametrize("bias,bn", [(True, True), (False, True), (True, False), (False, False)])
def test_finalize_closed_form_equals_autograd(bias, bn, monkeypatch):
    """finalize64 == float64 autograd through oracle.graph_ref.conv2d + frozen batchnorm + the L2 term (1e-12 relative); eps is the
    fp32 value the entry point receives, in both."""
    from oracle import graph_ref as G
    monkeypatch.setattr(G, "BN_EPS", X.f32v(G.BN_EPS))
    torch.manual_seed(11)
    Bn, Hh, Ww, Ci, Nn = 2, 6, 5, 8, 12
    d = torch.float64
    x = torch.randn(Bn, Ci, Hh, Ww, dtype=d)
    P = {"kernel": torch.randn(3, 3, Ci, Nn, dtype=d).requires_grad_(True)}
    if bias:
        P["bias"] = torch.randn(Nn, dtype=d).requires_grad_(True)
    Q = {"gamma": (torch.rand(Nn, dtype=d) + 0.5).requires_grad_(True), "beta": torch.randn(Nn, dtype=d).requires_grad_(True),
         "moving_mean": torch.randn(Nn, dtype=d), "moving_variance": torch.rand(Nn, dtype=d) + 0.5}
    zc = G.conv2d(x, P, 1, "same")
    z = G.batchnorm(zc, Q, False) if bn else zc
    dz = torch.randn_like(z)
    wd = X.f32v(1e-2)
    reg = wd * (P["kernel"] ** 2).sum() / P["kernel"].numel() + (wd * (P["bias"] ** 2).sum() / Nn if bias else 0.0)
    ((z * dz).sum() + reg).backward()
    xp = F.pad(x, (1, 1, 1, 1))
    dw_raw = torch.stack([torch.stack([torch.einsum("bchw,bnhw->cn", xp[:, :, ky:ky + Hh, kx:kx + Ww], dz) for kx in range(3)]) for ky in range(3)])
    K = 9 * Ci
    ref = X.finalize64(dw_raw.reshape(K, Nn), dz.sum(dim=(0, 2, 3)), P["kernel"].detach().reshape(K, Nn), P["bias"].detach() if bias else None,
                       Q["gamma"].detach() if bn else None, Q["moving_mean"], Q["moving_variance"], X.f32v(G.BN_EPS), 1e-2)
    want = {"gw": P["kernel"].grad.reshape(K, Nn)}
    if bias:
        want["gb"] = P["bias"].grad
    if bn:
        want["ggamma"], want["gbeta"] = Q["gamma"].grad, Q["beta"].grad
    assert set(ref) == set(want)
    for k_, wv in want.items():
        assert float((ref[k_][0] - wv).abs().max()) <= 1e-12 * float(wv.abs().max()), k_


@pytest.mark.parametrize("KNl", [(144, 24, 24), (2048, 3, 8), (4608, 512, 512)])
def test_finalize_bounds_accept_fp32_and_reject_missing_term(KNl):
    K, Nn, ldn = KNl
    torch.manual_seed(K + Nn)
    dw, cs, Wt = torch.randn(K, Nn), torch.randn(Nn) * 5, torch.randn(K, Nn) / K ** 0.5
    b, gamma, mean, var = torch.randn(Nn), torch.rand(Nn) + 0.5, torch.randn(Nn), torch.rand(Nn) + 0.5
    ks = max(min(-(-512 // -(-Nn // 64)), 32, max(K // 128, 1)), 1)
    ref = X.finalize64(dw, cs, Wt, b, gamma, mean, var, 1e-3, 1e-2)
    bnd = X.finalize_bounds(ref, K, Nn, ldn, ks)
    got = X.finalize32(dw, cs, Wt, b, gamma, mean, var, 1e-3, 1e-2)
    for k_ in ref:
        assert X.violations(got[k_], ref[k_][0], bnd[k_]) == 0, k_
        assert float((ref[k_][0] != 0).sum()) / ref[k_][0].numel() >= 0.25
    bad = X.finalize32(dw, cs, Wt, b, gamma, mean, var, 1e-3, 1e-2, gamma_term=False)      # ggamma without (b - mean) colsum
    assert X.violations(bad["ggamma"], ref["ggamma"][0], bnd["ggamma"]) >= 0.9
    # a helper broken the same way is caught by the correct restatement
    broken = X.finalize64(dw, cs, Wt, b, gamma, mean, var, 1e-3, 1e-2, gamma_term=False)
    assert X.violations(got["ggamma"], broken["ggamma"][0], bnd["ggamma"]) >= 0.9


def _bn_case(M, Nn, dt, seed=0):
    g = torch.Generator().manual_seed(seed + M + Nn)
    t = X.tdtype(dt)
    z = torch.randn(M, Nn, generator=g) * 2 + torch.randn(Nn, generator=g)
    z[:, 0] = 0.75                                                          # a constant channel: the variance clamps at 0
    z[:, 1] = torch.randn(M, generator=g) + 1000.0                          # mean 1000, unit spread
    return (z.to(t), torch.randn(M, Nn, generator=g).to(t), torch.rand(Nn, generator=g) + 0.5, torch.randn(Nn, generator=g),
            torch.randn(Nn, generator=g), torch.rand(Nn, generator=g) + 0.5, torch.randn(M, Nn, generator=g).to(t))


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_bn_references_accept_fp32_and_reject_faults(dt):
    M, Nn, eps, mom = 2048, 16, 1e-3, 0.99
    t = X.tdtype(dt)
    z, res, gamma, beta, mm, mv, gy = _bn_case(M, Nn, dt)
    zf = z.float()
    st = X.bn_stats64(z, mm, mv, mom, eps)
    mean32, var32 = zf.double().mean(0).float(), zf.double().var(0, unbiased=False).float()
    assert X.violations(mean32, *st["mean"]) == 0 and X.violations(var32, *st["var"]) == 0
    f = torch.float32
    momt, one = torch.tensor(mom, dtype=f), torch.tensor(1.0, dtype=f)
    corr = M / (M - (1 + X.f32v(eps)))
    assert X.violations(mm * momt + mean32 * (one - momt), *st["mmean"]) == 0
    assert X.violations(mv * momt + (zf.double().var(0, unbiased=False) * corr).float() * (one - momt), *st["mvar"]) == 0
    # the moving variance without the M / (M - (1 + eps)) factor: all but the constant channel
    assert X.violations(mv * momt + var32 * (one - momt), *st["mvar"]) >= 0.9
    rstd = torch.rsqrt(var32 + torch.tensor(eps, dtype=f))
    for relu in (0, 1):
        y64, by = X.bn_apply64(z, mean32, var32, gamma, beta, eps, res, relu, dt)
        y32 = (zf - mean32) * (gamma * rstd) + beta + res.float()
        y32 = torch.relu(y32) if relu else y32
        assert X.violations(y32.to(t), y64, by) == 0
        assert float((y64 != 0).sum()) / y64.numel() >= 0.25
        bad = y32.clone(); bad[:, 5] *= 1.005                               # one channel scaled by 1.005
        assert X.violations(bad.to(t), y64, by) >= (0.01 if not relu else 0.005)
        assert X.violations(trunc(y32, t), y64, by) >= (0.01 if dt else 0)
    g = gy.float()
    xh = (zf - mean32) * rstd
    db32, dg32 = g.double().sum(0).float(), (g * xh).double().sum(0).float()
    bw = X.bn_backward64(gy, z, mean32, var32, gamma, eps, dt, db32, dg32)
    assert X.violations(db32, *bw["dbeta"]) == 0 and X.violations(dg32, *bw["dgamma"]) == 0
    invM = torch.tensor(1.0 / M, dtype=f)
    dz32 = (gamma * rstd) * (g - db32 * invM - xh * dg32 * invM)
    assert X.violations(dz32.to(t), *bw["dz"]) == 0
    bad = dz32.clone(); bad[:, 5] *= 1.005
    assert X.violations(bad.to(t), *bw["dz"]) >= 0.01


# =====================================================================================================================
# The launches around a stage's first block and its end: the pixel map of the compact / sampled forms, the tile partition,
# and simulated kernels of urso_conv_pair_shortcut, urso_conv_pair_wgrad_entry, urso_conv_pointwise_sampled and the
# Winograd evaluation -- the clean simulation passes the GPU probes' checks, each planted defect is rejected.
import numpy as np


def _assert_pixel_map(H, W, p):
    b, y, x = X.pixel_map_f32(p, H, W)
    p64 = np.asarray(p, dtype=np.int64)
    wb, rem = np.divmod(p64, H * W)
    wy, wx = np.divmod(rem, W)
    bad = (b != wb) | (y != wy) | (x != wx)
    assert not bad.any(), "H %d W %d: pixel %d maps to (%d, %d, %d), divmod gives (%d, %d, %d)" % (
        (H, W, int(p64[bad][0])) + tuple(int(v[bad][0]) for v in (b, y, x, wb, wy, wx)))


def test_pixel_map_equals_divmod_for_every_small_even_image():
    """(int)((float)p * rcp) + one correction, as conv_pair.hip and conv_pairw.hip locate a pixel: every even H, W in 2 .. 162 and every
    p of four images."""
    for H in range(2, 163, 2):
        for W in range(2, 163, 2):
            _assert_pixel_map(H, W, np.arange(4 * H * W, dtype=np.int32))


@pytest.mark.parametrize("H,W", [(128, 160), (64, 80), (32, 40), (256, 320), (6, 40), (10, 6), (10, 22), (2, 2)])
def test_pixel_map_equals_divmod_up_to_the_largest_tensor(H, W):
    """p up to 2^22 (the entry points accept M * 512 bytes < 2 GiB): within +-2 of every multiple of W and of H W, and 10^5 random pixels."""
    top = 2 ** 22
    near = lambda step: (np.arange(0, top + 1, step, dtype=np.int64)[:, None] + np.arange(-2, 3)).reshape(-1)
    rng = np.random.RandomState(H + W)
    p = np.concatenate([near(W), near(H * W), rng.randint(0, top, 100000), [0, top - 1]])
    p = np.unique(p[(p >= 0) & (p < top)]).astype(np.int32)
    _assert_pixel_map(H, W, p)


def test_pixel_map_check_rejects_a_map_without_the_correction():
    """The same arithmetic without the +-1 step is wrong already at the first pixel of the second 10 x 22 image (f32(1 / 220) rounds down):
    the correction is needed, and the comparison with divmod can fail."""
    H, W = 10, 22
    p = np.arange(4 * H * W, dtype=np.int32)
    b = (p.astype(np.float32) * (np.float32(1.0) / np.float32(H * W))).astype(np.int32)
    assert b[H * W] == 0 and (b != p // (H * W)).any()
    _assert_pixel_map(H, W, p)


def test_tiles_per_block_of_the_pair_probes():
    """The table of tests/test_kernels_exact_gpu.py (PAIR_TILES): one block per XCD under grid_cap = 8."""
    want = {1: [1] + [0] * 7, 9: [2, 2, 2, 2, 1, 0, 0, 0], 19: [3] * 6 + [1, 0], 29: [4] * 7 + [1], 45: [6] * 7 + [3]}
    for n, counts in want.items():
        assert X.pair_grid_blocks(n, 8) == 8 and X.tiles_per_block(n, 8) == counts
    assert X.pair_grid_blocks(45, 0) == 48 and X.pair_grid_blocks(45, 16) == 16 and X.pair_grid_blocks(3, 0) == 8
    u = X.tiles_per_block(45, 48)                       # blockIdx.x = 8 lb + xcd: XCD 7 owns 3 tiles, its blocks lb = 3 .. 5 none
    assert sum(u) == 45 and [u[8 * lb + 7] for lb in range(6)] == [1, 1, 1, 0, 0, 0]
    assert X.tiles_per_block(45, 16) == [3] * 7 + [2] + [3] * 7 + [1]
    d = X.compact_to_dense(torch.arange(2 * 2 * 3 * 1, dtype=torch.float32).reshape(2, 2, 3, 1) + 1, 4, 6)
    assert float(d.sum()) == 78 and float(d[:, 1::2].abs().sum()) == 0 and float(d[:, :, 1::2].abs().sum()) == 0 and float(d[1, 2, 4, 0]) == 12


# ---- urso_conv_pair_shortcut
PM, PC, PC4 = 4 * 64, 64, 256                 # four 64-pixel tiles


def shortcut_case(t, exact, seed=21):
    if exact:
        a, d = X.int_plan(2 * PC, t, share=48)
        src, xin = X.int_operands((PM, PC), t, a, d, seed), X.int_operands((PM, PC), t, a, d, seed + 1)
        w1 = X.fill_last_channel(X.int_operands((PC4, PC), t, a, d, seed + 2), seed + 8)
        ws = X.fill_last_channel(X.int_operands((PC4, PC), t, a, d, seed + 3), seed + 9)
        b1, bs, b2 = X.int_operands((PC4,), t, 3, 0.8, seed + 4), X.int_operands((PC4,), t, 3, 0.8, seed + 5), X.int_operands((PC,), t, 3, 0.8, seed + 6)
        mid = F.relu(X.pair_shortcut64(src, w1, b1, xin, ws, bs)[0])
        dn = min(0.7, (256 / 12.0) ** 2 / (PC4 * float((mid ** 2).mean()) * 2.5))
        w2 = X.fill_last_channel(X.int_operands((PC, PC4), t, 2, dn, seed + 7), seed + 10)
    else:
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        src, xin = r(PM, PC).to(t).float(), r(PM, PC).to(t).float()
        w1, ws = (r(PC4, PC) / (2 * PC) ** 0.5).to(t).float(), (r(PC4, PC) / (2 * PC) ** 0.5).to(t).float()
        w2 = (r(PC, PC4) / (2 * PC ** 0.5)).to(t).float()
        b1, bs, b2 = r(PC4) * 0.3, r(PC4) * 0.3, r(PC) * 0.3
    return dict(src=src, xin=xin, w1=w1, ws=ws, w2=w2, b1=b1, bs=bs, b2=b2)


def simulated_shortcut(kind, t, o):
    """fp32 accumulation, one rounding per stored tensor -- or one of the faults."""
    f = lambda a: a.float()
    src, xin, w1, ws = o["src"], o["xin"], o["w1"], o["ws"]
    if kind == "segments_swapped":
        src, xin = xin, src
    bsum = f(o["b1"]) + (0 if kind == "bias_s_dropped" else f(o["bs"]))
    if kind == "shortcut_rounded_first":                 # the two-launch path: the shortcut conv's output is stored, then added
        sc = rne(f(xin) @ f(ws).T + f(o["bs"]), t)
        mid = rne(F.relu((f(src) @ f(w1).T + f(o["b1"])).double() + sc), t)
    else:
        mid = rne(F.relu(f(src) @ f(w1).T + f(xin) @ f(ws).T + bsum), t)
    dst = rne(F.relu(mid.float() @ f(o["w2"]).T + f(o["b2"])), t)
    if kind == "dst_tile_from_previous_tile":            # a ring slot reused too early
        dst = dst.clone()
        dst[128:192] = dst[64:128]
    return mid, dst


def check_shortcut(mid, dst, t, o, exact):
    """The comparisons of test_conv_pair_shortcut (tests/test_kernels_exact_gpu.py)."""
    pre1, mag1 = X.pair_shortcut64(o["src"], o["w1"], o["b1"], o["xin"], o["ws"], o["bs"])
    if exact:
        X.premise(t, stored=[("mid", F.relu(pre1))], mags=[("mid", mag1)])
        X.assert_exact(mid, F.relu(pre1), "mid")
    else:
        X.assert_rounded_once(mid, F.relu(pre1), mag1, t, 2 * PC + 2, "mid")
    pre2 = mid @ o["w2"].double().T + o["b2"].double()
    mag2 = mid.abs() @ o["w2"].double().abs().T + o["b2"].double().abs()
    if exact:
        X.premise(t, stored=[("dst", F.relu(pre2))], mags=[("dst", mag2)])
        X.assert_exact(dst, F.relu(pre2), "dst")
    else:
        X.assert_rounded_once(dst, F.relu(pre2), mag2, t, PC4 + 1, "dst")


SHORTCUT_FAULTS = ["bias_s_dropped", "segments_swapped", "shortcut_rounded_first", "dst_tile_from_previous_tile"]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded_once"])
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_shortcut_pair_simulation(t, exact):
    o = shortcut_case(t, exact)
    check_shortcut(*simulated_shortcut("correct", t, o), t, o, exact)
    for kind in SHORTCUT_FAULTS:
        if exact and kind == "shortcut_rounded_first":   # integers are exact at every rounding point: the real-valued probe's job
            continue
        with pytest.raises(AssertionError, match="elements wrong"):
            check_shortcut(*simulated_shortcut(kind, t, o), t, o, exact)


# ---- urso_conv_pair_wgrad_entry
def entry_case(t, exact, seed=31):
    if exact:
        a, d = X.int_plan(PC, t, share=48)
        src, w1 = X.int_operands((PM, PC), t, a, d, seed), X.int_operands((PC4, PC), t, a, d, seed + 1)
        add = X.int_operands((PM, PC4), t, 3, 0.8, seed + 2)
        u, p = X.int_operands((PM, PC), t, 3, 0.9, seed + 3), X.int_operands((PM, PC), t, 3, 0.9, seed + 4)
    else:
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        src, w1, add = r(PM, PC).to(t).float(), (r(PC4, PC) / PC ** 0.5).to(t).float(), r(PM, PC4).to(t).float()
        u, p = (r(PM, PC) * (torch.rand(PM, PC, generator=g) < 0.9)).to(t).float(), (r(PM, PC) * (torch.rand(PM, PC, generator=g) < 0.9)).to(t).float()
    keep = ((X.rand_bits(PM * PC4 // 8, seed + 5).to(torch.int32).reshape(-1, 1) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(PM, PC4).double()
    mid_ref = (src.double() @ w1.double().T + add.double()) * keep
    mag1 = (src.double().abs() @ w1.double().abs().T + add.double().abs()) * keep
    if exact:
        dn = min(0.7, (256 / 12.0) ** 2 / (PC4 * float((mid_ref ** 2).mean()) * 2.5))
        w2 = X.fill_last_channel(X.int_operands((PC, PC4), t, 2, dn, seed + 6), seed + 7)
        w3 = X.fill_last_channel(X.int_operands((PC, PC4), t, 2, dn, seed + 8), seed + 9)
    else:
        w2, w3 = (r(PC, PC4) / (2 * PC ** 0.5)).to(t).float(), (r(PC, PC4) / (2 * PC ** 0.5)).to(t).float()
    return dict(src=src, w1=w1, add=add, u=u, p=p, keep=keep, w2=w2, w3=w3, mid_ref=mid_ref, mag1=mag1)


def simulated_entry(kind, t, o, mask_p=1):
    """mid rounded once into the LDS tile; dst / dP rounded once; fp32 partial sums per 64-pixel tile, summed in float64."""
    f = lambda a: a.float()
    mid = rne((f(o["src"]) @ f(o["w1"]).T + f(o["add"])).double() * o["keep"], t)
    w2, w3 = (o["w3"], o["w2"]) if kind == "w2_w3_exchanged" else (o["w2"], o["w3"])
    ku = (o["u"] > 0).double()
    kp = (o["p"] > 0).double() if (mask_p and kind != "dP_mask_ignored") else 1.0
    out = {"dst": rne((mid.float() @ f(w2).T).double() * ku, t), "dP": rne((mid.float() @ f(w3).T).double() * kp, t)}
    tiles = range(PM // 64)
    tsum = lambda a, skip=None: sum((f(a[64 * i:64 * i + 64]).T @ mid[64 * i:64 * i + 64].float()).double() for i in tiles if i != skip)
    out["dW2c"] = tsum(o["u"])
    out["dWs"] = tsum(o["p"], skip=2 if kind == "dWs_misses_a_tile" else None)
    out["colsum"] = sum(mid[64 * i:64 * i + 64].float().sum(0).double() for i in tiles)
    out["colsum (shortcut)"] = out["colsum"].clone()     # "copied from the first layer's": the same values by definition
    return mid, out


def check_entry(mid, got, t, o, exact, mask_p=1):
    """The comparisons of test_conv_pair_wgrad_entry: exact against the products of the exact mid; rounded once against the products of the
    STORED mid (itself within the rounded-once bound of the float64 mid)."""
    if exact:
        m = o["mid_ref"]
        X.premise(t, stored=[("mid", m)], mags=[("mid", o["mag1"])])
    else:
        X.assert_rounded_once(mid, o["mid_ref"], o["mag1"], t, PC + 1, "mid")
        m = mid
    ref = X.pair_entry64(m, o["w2"], o["w3"], o["u"], o["p"], mask_p)
    ref["colsum (shortcut)"] = ref["colsum"]
    for k in ("dst", "dP", "dW2c", "dWs", "colsum", "colsum (shortcut)"):
        st = t if k in ("dst", "dP") else torch.float32
        if exact:
            X.premise(st, stored=[(k, ref[k][0])], mags=[(k, ref[k][1])])
            X.assert_exact(got[k], ref[k][0], k)
        else:
            X.assert_rounded_once(got[k], ref[k][0], ref[k][1], st, PC4 if k in ("dst", "dP") else PM, k)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded_once"])
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_entry_pair_simulation(t, exact):
    o = entry_case(t, exact)
    for mask_p in (1, 0):
        check_entry(*simulated_entry("correct", t, o, mask_p), t, o, exact, mask_p)
    for kind in ("w2_w3_exchanged", "dP_mask_ignored", "dWs_misses_a_tile"):
        with pytest.raises(AssertionError, match="elements wrong"):
            check_entry(*simulated_entry(kind, t, o), t, o, exact)


def test_entry_pair_probe_cannot_tell_the_two_column_sums_apart():
    """A kernel that wrote the second layer's column sums as a COPY of the first layer's is a correct kernel: both layers' dz is the same mid
    (conv_pairx.hip stores one accumulator twice), so the references are the same tensor.  The probe covers each buffer's values, block
    slices and NaN pre-fill -- not which accumulator fed it; nothing else could, and nothing needs to."""
    o = entry_case(torch.bfloat16, True)
    mid, got = simulated_entry("correct", torch.bfloat16, o)
    ref = X.pair_entry64(o["mid_ref"], o["w2"], o["w3"], o["u"], o["p"], 1)
    assert torch.equal(got["colsum (shortcut)"], got["colsum"]) and torch.equal(ref["colsum"][0], o["mid_ref"].sum(0))
    check_entry(mid, got, torch.bfloat16, o, True)
    got["colsum (shortcut)"] = got["colsum"] * 0        # ... while a buffer that was never accumulated is rejected
    with pytest.raises(AssertionError, match="elements wrong"):
        check_entry(mid, got, torch.bfloat16, o, True)


# ---- urso_conv_pointwise_sampled
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounded_once"])
@pytest.mark.parametrize("t", DTS, ids=["bf16", "fp16"])
def test_sampled_copy_simulation(t, exact):
    """dst_sampled must be dst[:, ::2, ::2] bit for bit: the copy taken at odd columns, or one image's rows shifted by one, is rejected (on
    integer and on real data: it is a comparison of stored values)."""
    Bq, Hq, Wq, c, N = 4, 6, 10, 64, 256
    if exact:
        a, d = X.int_plan(c, t)
        x, w = X.int_operands((Bq * Hq * Wq, c), t, a, d, 41), X.int_operands((N, c), t, a, d, 42)
    else:
        g = torch.Generator().manual_seed(43)
        x, w = torch.randn(Bq * Hq * Wq, c, generator=g).to(t).float(), (torch.randn(N, c, generator=g) / 8).to(t).float()
    z = x.double() @ w.double().T
    dst = rne(F.relu(x @ w.T), t).reshape(Bq, Hq, Wq, N)
    if exact:
        X.premise(t, stored=[("dst", F.relu(z))], mags=[("dst", x.double().abs() @ w.double().abs().T)])
        X.assert_exact(dst.reshape(-1, N), F.relu(z), "dst")
    else:
        X.assert_rounded_once(dst.reshape(-1, N), F.relu(z), x.double().abs() @ w.double().abs().T, t, c + 1, "dst")
    good = dst[:, ::2, ::2].clone()
    X.assert_exact(good, dst[:, ::2, ::2], "dst_sampled")
    shifted = good.clone()
    shifted[2] = dst[2, 1::2, ::2]
    for bad in (dst[:, ::2, 1::2], shifted):
        with pytest.raises(AssertionError, match="elements wrong"):
            X.assert_exact(bad, dst[:, ::2, ::2], "dst_sampled")


# ---- Winograd F(2x2, 3x3)
@pytest.mark.parametrize("shape", [(2, 9, 15, 16, 8), (1, 4, 6, 8, 8), (3, 17, 23, 24, 16)])
def test_winograd_operands_and_evaluation(shape):
    """winograd_uv / winograd_out evaluate the 3x3 / stride-1 / pad-1 conv exactly on integers with |v| <= 2 (odd sizes: the last tiles'
    second row / column is dropped), U is a multiple of 1/4 with |U| <= 4.5 and V an integer with |V| <= 8 -- representable in bf16 and
    f16 -- and a filter transform that forgets a factor 1/2 is rejected."""
    Bq, Hq, Wq, c, N = shape
    x, w = X.int_operands((Bq, Hq, Wq, c), None, 2, 0.6, 51), X.int_operands((3, 3, c, N), None, 2, 0.6, 52)
    ref = conv64(x, w)
    U, V = X.winograd_uv(w, x)
    assert torch.equal(4 * U, (4 * U).round()) and float(U.abs().max()) <= 4.5
    assert torch.equal(V, V.round()) and float(V.abs().max()) <= 8
    for t in DTS:
        X.premise(t, stored=[("U", U), ("V", V)])
    X.assert_exact(X.winograd_out(U, V, Hq, Wq), ref, "winograd")
    assert bool((X.winograd_out(U, V, Hq, Wq, magnitude=True) >= ref.abs()).all())
    Ubad = U.clone()
    Ubad[1] *= 2
    with pytest.raises(AssertionError, match="elements wrong"):
        X.assert_exact(X.winograd_out(Ubad, V, Hq, Wq), ref, "winograd")
    worst = X.winograd_uv(torch.full((3, 3, 1, 1), 2.0), torch.tensor([2.0, -2.0]).repeat(4, 2).reshape(1, 4, 4, 1) * torch.tensor([1.0, 1, -1, -1]).reshape(1, 4, 1, 1))
    assert float(worst[0].abs().max()) == 4.5 and float(worst[1].abs().max()) <= 8


# =====================================================================================================================
# Weight preparation (fold64 / fold_bounds) and the split reduction (reduce32 / reduce_bound): each bound accepts a plain fp32
# restatement and rejects the faults a preparation or reduction kernel can have.
FOLD_SHAPES = [(1, 1, 1, 1, 1), (1, 1, 33, 31, 32), (3, 3, 40, 50, 56), (3, 3, 3, 5, 8), (1, 1, 64, 64, 64)]


@pytest.mark.parametrize("t", [torch.bfloat16, torch.float16, torch.float32])
def test_ulp_is_the_subnormal_spacing_below_the_smallest_normal(t):
    """X.ulp below 2^emin: the constant subnormal spacing 2^(emin - (p - 1)) -- 2^-24 for fp16 -- down to 0; rounding a value there to the
    type moves it by at most half of it, and the first normal binade has the same spacing."""
    p, emin = X._SIG_BITS[t], X._EMIN[t]
    sub = 2.0 ** (emin - (p - 1))
    if t == torch.float16:
        assert sub == 2.0 ** -24
    v = torch.tensor([0.0, sub / 3, sub, 3e-6 if t == torch.float16 else 100 * sub, 2.0 ** emin * 0.999, 2.0 ** emin, 2.0 ** emin * 1.5],
                     dtype=torch.float64)
    assert torch.equal(X.ulp(v, t), torch.full_like(v, sub))
    assert float(X.ulp(torch.tensor([2.0 ** (emin + 1)], dtype=torch.float64), t)) == 2 * sub
    r = torch.rand(10000, dtype=torch.float64) * 2.0 ** emin
    assert float((rne(r, t) - r).abs().max()) <= sub / 2 and float((rne(r, t) - r).abs().max()) > sub / 4
    assert torch.equal(X.store_bound(torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), t), torch.tensor([sub / 2], dtype=torch.float64))


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_bounds_accept_fp32_and_reject_faults(shape, dt):
    KH, KW, Ci, Nn, npad = shape
    eps = 1e-3
    w, b, bn = X.fold_inputs(KH, KW, Ci, Nn, seed=1)
    _, eb, ebn = X.fold_inputs(1, 1, 4, max(Nn - 2, 1), seed=2)
    eN = max(Nn - 2, 1)
    big = Nn >= 5
    for bias in (True, False):
        for has_bn in (True, False):
            for extra in (None, (eb, ebn, eN), (None, ebn, eN), (eb, None, eN)):
                b_, bn_ = (b if bias else None), (bn if has_bn else None)
                ref = X.fold64(w, b_, bn_, eps, npad, extra)
                bnd = X.fold_bounds(ref, dt, bias, has_bn, None if extra is None else (extra[0] is not None, extra[1] is not None))
                got = X.fold32(w, b_, bn_, eps, npad, dt, extra)
                for k in ref:
                    assert X.violations(got[k], ref[k][0], bnd[k]) == 0, (k, bias, has_bn)
                # the definition's exact values in the padded filters
                assert float(ref["wf"][0][Nn:].abs().sum()) == 0 and float(ref["wd"][0][..., Nn:].abs().sum()) == 0
                assert float(ref["biasf"][0][Nn:].abs().sum()) == 0 and bool((ref["scale"][0][Nn:] == 1).all())
                if npad > Nn:
                    bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, pad_scale=0.0)
                    assert X.violations(bad["scale"], ref["scale"][0], bnd["scale"]) >= (npad - Nn) / float(npad)
                    bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, pad_scale=1.0 + 2.0 ** -23)
                    assert X.violations(bad["scale"], ref["scale"][0], bnd["scale"]) >= (npad - Nn) / float(npad)
                if KH * KW > 1:
                    bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, flip=False)
                    assert X.violations(bad["wd"], ref["wd"][0], bnd["wd"]) >= 0.5
                    assert X.violations(bad["wf"], ref["wf"][0], bnd["wf"]) == 0
                if extra is not None and big:
                    bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, use_extra=False)
                    assert X.violations(bad["biasf"], ref["biasf"][0], bnd["biasf"]) >= 0.9 * eN / npad
                if has_bn and big:
                    for st in (torch.bfloat16, torch.float16):        # s rounded to 16 bits before the product: a double rounding
                        bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, s_round=st)
                        # expected share: mean |shift of w s| / ulp of the store.  s rounded to the store's own type: a quarter of an ulp
                        # on average -> ~0.25; fp16's s (2^-13 on average) under a bf16 store (ulp 2^-8 .. 2^-7): ~0.02; otherwise ~1
                        floor = 0.01 if (dt == 1 and st == torch.float16) else (0.15 if X.tdtype(dt) == st else 0.5)
                        assert X.violations(bad["wf"], ref["wf"][0], bnd["wf"]) >= floor * Nn / npad, (dt, st)
                        assert X.violations(bad["wd"], ref["wd"][0], bnd["wd"]) >= floor * Nn / npad, (dt, st)
                        assert X.violations(bad["scale"], ref["scale"][0], bnd["scale"]) >= 0.9 * Nn / npad
                    bad = X.fold32(w, b_, bn_, eps, npad, dt, extra, use_eps=False)
                    assert X.violations(bad["scale"], ref["scale"][0], bnd["scale"]) >= 0.9 * Nn / npad
                    assert X.violations(bad["wf"], ref["wf"][0], bnd["wf"]) >= 0.01
                    assert X.violations(bad["biasf"], ref["biasf"][0], bnd["biasf"]) >= 0.5 * Nn / npad


def test_fold_bound_rejects_flushed_fp16_subnormals():
    """|w s| around 3e-6 in a block of filters: fp16 subnormals (spacing 2^-24 = 6e-8).  A store rounding them is inside the bound, one
    flushing them to zero is outside in nearly every element of the block."""
    KH, KW, Ci, Nn, npad = 3, 3, 40, 50, 56
    w, b, bn = X.fold_inputs(KH, KW, Ci, Nn, seed=3, tiny_block=(16, 40))
    ref = X.fold64(w, b, bn, 1e-3, npad)
    bnd = X.fold_bounds(ref, 2, True, True)
    blk = ref["wf"][0][16:40]
    assert float(blk.abs().max()) < 2.0 ** -14 and float(blk.abs().median()) > 1e-6
    got = X.fold32(w, b, bn, 1e-3, npad, 2)
    assert X.violations(got["wf"], ref["wf"][0], bnd["wf"]) == 0 and X.violations(got["wd"], ref["wd"][0], bnd["wd"]) == 0
    f32 = X.fold32(w, b, bn, 1e-3, npad, 0)
    flushed = flush16(f32["wf"].double(), torch.float16)
    assert X.violations(flushed[16:40], blk, bnd["wf"][16:40]) >= 0.9
    assert X.violations(flush16(f32["wd"].double(), torch.float16), ref["wd"][0], bnd["wd"]) >= 0.9 * 24 / npad


def test_fold64_agrees_with_the_layout_test_of_the_suite():
    """fold64 restates what tests/test_kernels_gpu.py::test_weight_prep_layouts builds by hand (1e-12), and X.stem_taps of it is the
    packed stem filter of a folded 7x7 layer."""
    KH, KW, Ci, Nn, NP = 3, 3, 40, 50, 56
    w, b, bn = X.fold_inputs(KH, KW, Ci, Nn, seed=4)
    d = lambda v: v.double()
    s = d(bn[0]) / torch.sqrt(d(bn[3]) + X.f32v(1e-3))
    wfr = torch.zeros(NP, KH, KW, Ci, dtype=torch.float64); wfr[:Nn] = (d(w) * s).permute(3, 0, 1, 2)
    wdr = torch.zeros(Ci, KH, KW, NP, dtype=torch.float64); wdr[..., :Nn] = (d(w) * s).flip(0, 1).permute(2, 0, 1, 3)
    ref = X.fold64(w, b, bn, 1e-3, NP)
    assert float((ref["wf"][0] - wfr).abs().max()) <= 1e-12 and float((ref["wd"][0] - wdr).abs().max()) <= 1e-12
    assert float((ref["biasf"][0][:Nn] - (s * d(b) + d(bn[1]) - d(bn[2]) * s)).abs().max()) <= 1e-12
    assert bool((ref["biasf"][0].abs() <= sum(ref["biasf"][1]) * (1 + 1e-12)).all()) and len(ref["biasf"][1]) == 6
    w7, b7, bn7 = X.fold_inputs(7, 7, 3, 5, seed=5)
    r7 = X.fold64(w7, b7, bn7, 1e-3, 5)
    taps = X.stem_taps(r7["wf"][0].permute(1, 2, 3, 0))
    assert torch.equal(X.stem_untaps(taps), r7["wf"][0].permute(1, 2, 3, 0)) and float(taps[:, 0].abs().sum()) == 0 and float(taps[:, :, 3].abs().sum()) == 0


REDUCE_SPLITS = [1, 2, 5, 16, 17, 49, 100, 200, 400, 733]


def test_reduce_lanes_thresholds():
    assert [X.reduce_lanes(s) for s in REDUCE_SPLITS] == [1, 1, 1, 1, 1, 2, 4, 8, 16, 16]
    assert [X.reduce_lanes(s) for s in (48, 96, 192, 384)] == [1, 2, 4, 8]
    assert [X.reduce_depth(s) for s in (1, 2, 16, 49, 733)] == [0, 1, 15, 25, 45 + 15]


@pytest.mark.parametrize("splits", REDUCE_SPLITS)
def test_reduce32_inside_bound_and_faults_rejected(splits):
    """reduce32 over the documented workspace layout equals the float64 sum within reduce_bound; a dropped partial and partials read at
    stride K npad (without WGRAD_PART_PAD) are outside it; the order matters to the bits (a sequential sum differs from the lane
    order somewhere once there is more than one lane)."""
    K, Nn, npad = 24, 13, 16
    flat, parts, colparts = X.partials_buffer(K, Nn, npad, splits, seed=splits)
    stride = K * npad + X.WGRAD_PART_PAD
    assert flat.numel() == splits * stride + splits * npad
    view = flat[:splits * stride].reshape(splits, stride)
    assert torch.equal(view[:, :K * npad].reshape(splits, K, npad), parts) and bool((view[:, K * npad:] == X.PART_SENTINEL).all())
    assert torch.equal(flat[splits * stride:].reshape(splits, npad), colparts)
    for p in (parts, colparts):
        ref, mag = p.double().sum(0), p.double().abs().sum(0)
        bnd = X.reduce_bound(mag, splits)
        got = X.reduce32(p, splits)
        assert got.dtype == torch.float32 and X.violations(got, ref, bnd) == 0
        X.assert_sensitive(ref, what="sum of partials")
        if splits == 1:
            assert torch.equal(got, p[0]) and float(bnd.abs().max()) == 0
            continue
        real = (slice(None), slice(0, Nn)) if p is parts else (slice(0, Nn),)
        dropped = X.reduce32(torch.cat([p[:splits // 2], torch.zeros_like(p[:1]), p[splits // 2 + 1:]]), splits)
        assert X.violations(dropped[real], ref[real], bnd[real]) >= 0.9
    if splits > 1:
        wrong = torch.stack([flat[q * K * npad:(q + 1) * K * npad] for q in range(splits)]).reshape(splits, K, npad)
        ref, mag = parts.double().sum(0), parts.double().abs().sum(0)
        assert X.violations(X.reduce32(wrong, splits)[:, :Nn], ref[:, :Nn], X.reduce_bound(mag, splits)[:, :Nn]) >= 0.9
    if X.reduce_lanes(splits) > 1:
        seq = torch.zeros_like(parts[0])
        for q in range(splits):
            seq = seq + parts[q]
        assert not torch.equal(seq, X.reduce32(parts, splits))


def test_finalize_bounds_widened_by_the_partial_sums():
    """finalize64 with the partials' summed magnitudes + finalize_bounds(sum_depth) accepts the finalisation of an fp32 sum of partials
    (reduce32's order) against the float64 sum's closed form, and rejects a dropped partial in every gradient."""
    K, Nn, npad, splits = 144, 24, 24, 17
    _, parts, colparts = X.partials_buffer(K, Nn, npad, splits, seed=9)
    g = torch.Generator().manual_seed(5)
    Wt, b = torch.randn(K, Nn, generator=g) / K ** 0.5, torch.randn(Nn, generator=g)
    gamma, mean, var = torch.rand(Nn, generator=g) + 0.5, torch.randn(Nn, generator=g), torch.rand(Nn, generator=g) + 0.5
    p64, c64 = parts.double()[:, :, :Nn], colparts.double()[:, :Nn]
    ref = X.finalize64(p64.sum(0), c64.sum(0), Wt, b, gamma, mean, var, 1e-3, 1e-2, dw_mag=p64.abs().sum(0), cs_mag=c64.abs().sum(0))
    plain = X.finalize64(p64.sum(0), c64.sum(0), Wt, b, gamma, mean, var, 1e-3, 1e-2)
    for k in ref:
        assert torch.equal(ref[k][0], plain[k][0]) and bool((ref[k][1] >= plain[k][1] * (1 - 1e-12)).all())
    D = X.reduce_depth(splits)
    assert D == 16
    bnd = X.finalize_bounds(ref, K, Nn, npad, 1, sum_depth=D)
    got = X.finalize32(X.reduce32(parts)[:, :Nn], X.reduce32(colparts)[:Nn], Wt, b, gamma, mean, var, 1e-3, 1e-2)
    less = torch.cat([parts[:3], parts[4:]]), torch.cat([colparts[:3], colparts[4:]])
    bad = X.finalize32(X.reduce32(less[0])[:, :Nn], X.reduce32(less[1])[:Nn], Wt, b, gamma, mean, var, 1e-3, 1e-2)
    for k in ref:
        assert X.violations(got[k], ref[k][0], bnd[k]) == 0, k
        assert X.violations(bad[k], ref[k][0], bnd[k]) >= 0.9, k
