"""Exact-integer and rounded-once probes of the conv kernels (plain helpers, imported like tests/util.py).

Two ways to compare a kernel with a float64 reference of the same operation, both far tighter than a normwise gate:

* exact: integer operands small enough that every product and every fp32 partial sum is exact (|partial| < 2^24) and
  every stored value is representable in the storage type (premise() proves both).  A correct kernel then equals the
  reference bit for bit whatever its summation order, so one wrong element, tap, channel or store is a failure.
* rounded once: real operands already rounded to the storage type.  A correct kernel accumulates in fp32 and rounds
  each stored output once (after its fused epilogue), so every element lies within half an ulp of the exact value plus
  the fp32 accumulation error (assert_rounded_once).  A truncating store, a double rounding or 16-bit partial sums
  break that bound (tests/test_exactprobe_cpu.py shows it on simulated kernels).

int_operands() / int_plan() make the integer data; ran() asserts which kernel a call actually launched.  The references of the
packed stem (stem_taps, stem_conv64), of the max-pool's gradient routing (pool_route), of weight gradients (wgrad64) and of
two-segment reductions (two_segment) live here too, each with a CPU test that it rejects the fault it is there to expose.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

# storage types by the library's dtype codes (URSO_F32 / URSO_BF16 / URSO_F16) or by torch dtype
_TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
_SIG_BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}       # significand bits, implicit bit included
_EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}    # exponent of the smallest normal
# every integer of magnitude <= this is exact in the type
INT_LIMIT = {torch.float32: 2 ** 24, torch.bfloat16: 2 ** 8, torch.float16: 2 ** 11}
ACC_FACTOR = 4.0            # fp32 accumulation term of assert_rounded_once: ACC_FACTOR * sqrt(K) * 2^-24 * magnitude


def tdtype(dt):
    return _TDT[dt] if isinstance(dt, int) else dt


def ulp(a, dt):
    """Spacing of the storage type at |a| (float64 tensor); below the smallest normal, the subnormal spacing."""
    t = tdtype(dt)
    a = a.abs().to(torch.float64).clamp_min(2.0 ** _EMIN[t])
    return torch.exp2(torch.floor(torch.log2(a)) - (_SIG_BITS[t] - 1))


def int_plan(K, dt, share=12):
    """(amax, density) for int_operands() of BOTH operands of a K-term dot product whose results must stay exact in `dt`:
    the standard deviation of a sum is about min(INT_LIMIT, 256) / share (premise() still has to prove the maximum).  The
    bf16 limit also for the wider types keeps sums small enough that ~2 % of them are exactly 0 (a ReLU decision at 0)."""
    lim = min(INT_LIMIT[tdtype(dt)], INT_LIMIT[torch.bfloat16])
    sigma = lim / float(share)
    for amax in (2, 3, 4, 6, 8):
        ev2 = (amax + 1) * (2 * amax + 1) / 6.0                 # E[v^2] of the nonzero values
        d = sigma / (math.sqrt(K) * ev2)
        if d <= 0.7 or amax == 8:
            return amax, float(min(max(d, 0.04), 0.7))
    raise AssertionError("unreachable")


def int_operands(shape, dt=None, amax=2, density=0.5, seed=0):
    """Integer-valued float32 CPU tensor in [-amax, amax]: a `density` fraction of nonzero entries, uniform over the
    nonzero integers, iid -- so no row, column, tap or channel equals another (a swap or a transpose changes the result).
    `dt` only checks that amax is exact in the storage type."""
    if dt is not None:
        assert amax <= INT_LIMIT[tdtype(dt)], "amax %d not exact in %s" % (amax, tdtype(dt))
    g = torch.Generator().manual_seed(int(seed))
    mag = torch.randint(1, amax + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    keep = torch.rand(tuple(shape), generator=g) < density
    return (mag * sign * keep).to(torch.float32)


def fill_last_channel(t, seed=0):
    """t with the zeros of its LAST channel (last dimension) replaced by +-1: in a long, sparse reduction with few outputs (the
    Dense heads) the last input channel would otherwise rarely contribute, and dropping it (a K-tail fault) would go unseen."""
    g = torch.Generator().manual_seed(int(seed))
    t = t.clone()
    last = t[..., -1]
    sign = (torch.randint(0, 2, tuple(last.shape), generator=g) * 2 - 1).to(t.dtype)
    t[..., -1] = torch.where(last == 0, sign, last)
    return t


def rand_bits(nbytes, seed=0):
    """Random bit-mask bytes (uint8 CPU tensor)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, 256, (int(nbytes),), dtype=torch.uint8, generator=g)


def premise(dt, stored=(), mags=()):
    """Conditions under which an exact comparison is valid; fails with the first that does not hold.
    stored: (name, float64 tensor) of every value the kernel stores in `dt` (outputs and intermediates such as a pair's
    `mid`) -- each must be exactly representable.  mags: (name, float64 tensor) of the same operations applied to |operands|
    -- every fp32 partial sum is bounded by them and must stay below 2^24."""
    t = tdtype(dt)
    for name, v in stored:
        v = v.to(torch.float64)
        back = v.to(t).to(torch.float64)
        bad = back != v
        assert not bool(bad.any()), ("premise: %s has %d values not representable in %s (max |v| %g, limit for integers %d): "
                                     "shrink amax / density" % (name, int(bad.sum()), t, float(v.abs().max()), INT_LIMIT[t]))
    for name, m in mags:
        mx = float(m.to(torch.float64).abs().max()) if m.numel() else 0.0
        assert mx < 2.0 ** 24, "premise: partial sums of %s may reach %g >= 2^24: not exact in fp32" % (name, mx)


def _coords(idx, shape):
    names = "byxc" if len(shape) == 4 else "".join("abcdefgh"[:len(shape)])
    return "(" + ", ".join("%s=%d" % (n, i) for n, i in zip(names, np.unravel_index(idx, shape))) + ")"


def _report(what, bad, got, ref, extra=None, show=6):
    flat = bad.reshape(-1).nonzero().reshape(-1)
    lines = ["%s: %d of %d elements wrong" % (what, flat.numel(), bad.numel())]
    g, r = got.reshape(-1), ref.reshape(-1)
    for i in flat[:show].tolist():
        s = "  %s got %r expected %r" % (_coords(i, tuple(bad.shape)), float(g[i]), float(r[i]))
        if extra is not None:
            s += " (bound %.3g)" % float(extra.reshape(-1)[i])
        lines.append(s)
    return "\n".join(lines)


def _host64(t):
    return t.detach().to("cpu").to(torch.float64)


def assert_exact(got, ref64, what="output"):
    """Bit-for-bit equality of a kernel output with its float64 reference (shapes must match)."""
    got = _host64(got)
    ref64 = ref64.to(torch.float64)
    assert got.shape == ref64.shape, "%s: shape %s, reference %s" % (what, tuple(got.shape), tuple(ref64.shape))
    if not torch.equal(got, ref64):
        bad = (got != ref64) & ~(torch.isnan(got) & torch.isnan(ref64))
        raise AssertionError(_report(what, bad, got, ref64))


def rounded_once_bound(ref64, mag64, dt, K):
    """0.5 ulp_dt at the computed value + the fp32 accumulation error of K products: the largest deviation of a kernel that
    sums in fp32 (any order) and rounds the result to `dt` once."""
    acc = ACC_FACTOR * math.sqrt(max(int(K), 1)) * 2.0 ** -24 * mag64.to(torch.float64).abs()
    return 0.5 * ulp(ref64.to(torch.float64).abs() + acc, dt) + acc


def assert_rounded_once(got, ref64, mag64, dt, K, what="output"):
    """Elementwise |got - ref| <= rounded_once_bound(); `dt` is the type the output is STORED in (fp32 for filter gradients
    and out_f32 heads).  Returns the largest |got - ref| / bound (recorded by the tests)."""
    got = _host64(got)
    ref64, mag64 = ref64.to(torch.float64), mag64.to(torch.float64)
    assert got.shape == ref64.shape == mag64.shape, "%s: shape %s, reference %s, magnitude %s" % (
        what, tuple(got.shape), tuple(ref64.shape), tuple(mag64.shape))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    bound = rounded_once_bound(ref64, mag64, dt, K)
    err = (got - ref64).abs()
    bad = err > bound
    if bool(bad.any()):
        raise AssertionError(_report("%s (rounded-once bound, K=%d, %s)" % (what, K, tdtype(dt)), bad, got, ref64, bound))
    return float((err / bound.clamp_min(1e-300)).max())


def assert_sensitive(ref64, ref64_lastc=None, pre64=None, what="output"):
    """Integer data that can expose a fault: >= 25 % of outputs nonzero; >= 1 % of pre-activations exactly 0 (where a ReLU
    applies); the reference with the LAST input channel zeroed differs in >= 1 % of outputs."""
    n = ref64.numel()
    nz = float((ref64 != 0).sum()) / n
    assert nz >= 0.25, "%s: only %.1f %% of outputs nonzero" % (what, 100 * nz)
    if pre64 is not None:
        z = float((pre64 == 0).sum()) / pre64.numel()
        assert z >= 0.01, "%s: only %.2f %% of pre-activations are exactly 0" % (what, 100 * z)
    if ref64_lastc is not None:
        d = float((ref64_lastc != ref64).sum()) / n
        assert d >= 0.01, "%s: zeroing the last input channel changes only %.2f %% of outputs" % (what, 100 * d)


@contextlib.contextmanager
def ran(symbol_substring):
    """Asserts that every library entry point called inside the block launched a kernel whose device symbol contains
    `symbol_substring` (the launch profiler names each call by the first kernel it launched), and at least one was called.
    A tuple: every one of its substrings (e.g. a kernel name and a template argument of its mangled symbol)."""
    subs = symbol_substring if isinstance(symbol_substring, tuple) else (symbol_substring,)
    import ursonet_amd.hip as hip
    torch.cuda.synchronize()
    hip.prof_collect_ex()                       # drop older records
    hip.prof_enable(1)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        recs = hip.prof_collect_ex()
        hip.prof_enable(0)
    syms = [r[5] for r in recs]
    assert syms, "no library call was profiled (expected %s)" % symbol_substring
    assert all(all(u in s for u in subs) for s in syms), "expected every call to launch %s, launched %s" % (" + ".join(subs), syms)


def round_to(t, dt):
    """float64 t rounded once to the storage type (round to nearest even), back in float64."""
    return t.to(torch.float64).to(tdtype(dt)).to(torch.float64)


def pack_bits(keep):
    """Bit-mask bytes of a 0 / 1 tensor in element order (bit i of byte j = element 8 j + i): the ReLU bit masks of the library."""
    k = keep.reshape(-1, 8).to(torch.int32)
    return (k << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def assert_zero_columns(y, n, what="output"):
    """The padded output columns n.. of y (last dimension) are exactly 0 (zero filter rows, zero bias)."""
    pad = _host64(y)[..., n:]
    bad = pad != 0
    assert not bool(bad.any()), "%s: %d values of the padded columns %d.. are not 0 (max |v| %g)" % (
        what, int(bad.sum()), n, float(pad.abs().max()))


# ---- the packed stem (urso_stem_weight_pack / conv_stem.hip): 7x7 taps of 3 channels as 7 rows x 4 pixel pairs x 8 (pixel, channel)
def stem_taps(w):
    """[7][7][3][N] filter -> the packed 7 x 8 x 4 tap grid [7][8][4][N]: window pixel q = kx + 1 (q = 0 is a pad tap) and channel
    c (c = 3 is the molded zero channel); pad taps are 0.  Permuted to [N][7][8][4] and reshaped to [N][7][4][8] it is the layout
    of urso_stem_weight_pack's filter (pixel pair kp = q >> 1, cp = 4 (q & 1) + c)."""
    N = w.shape[3]
    t = torch.zeros(7, 8, 4, N, dtype=torch.float64)
    t[:, 1:, :3] = w.to(torch.float64)
    return t


def stem_untaps(t):
    """The 147 real taps [7][7][3][N] of a [7][8][4][N] tap grid (urso_stem_wgrad_unpack)."""
    return t[:, 1:, :3]


def stem_conv64(x4, taps):
    """float64 stem on the molded input [B][H][W][4] with a [7][8][4][N] tap grid: stride 2, ZeroPadding2D(3) -- window pixel q of
    output column ox is input column 2 ox - 4 + q -- so the real taps give the 7x7 / s2 / pad-3 conv of the 3 channels.  [B][H/2][W/2][N]."""
    B, H, W, _ = x4.shape
    xp = F.pad(x4.to(torch.float64).permute(0, 3, 1, 2), (4, 3, 3, 3))
    y = F.conv2d(xp, taps.to(torch.float64).permute(3, 2, 0, 1), stride=2)
    return y[:, :, :H // 2, :W // 2].permute(0, 2, 3, 1)


def stem_wgrad64(x4, dz):
    """float64 gradient of stem_conv64 with respect to its [7][8][4][N] tap grid (x^T dz over the B * H/2 * W/2 pixels)."""
    taps = torch.zeros(7, 8, 4, dz.shape[3], dtype=torch.float64, requires_grad=True)
    (stem_conv64(x4, taps) * dz.to(torch.float64)).sum().backward()
    return taps.grad


def pool_route(dpool, am, H, W):
    """The max-pool 3x3 / s2 / SAME gradient in float64: every pooled element goes to the conv pixel its arg-max byte names (tap in
    bits 0-3 = 3 ky + kx of window (2 py, 2 px)); a byte with bit 4 set (window maximum <= 0: the ReLU in front) routes nothing.
    Returns (sum reaching each conv pixel [B][H][W][C], the same sum of magnitudes) -- unrounded: the kernels store it rounded ONCE."""
    B, PH, PW, C = dpool.shape
    dp = dpool.to(torch.float64)
    a = am.to("cpu").to(torch.int64)
    live = (a & 16) == 0
    out = torch.zeros(B, 2 * PH + 1, 2 * PW + 1, C, dtype=torch.float64)
    mag = torch.zeros_like(out)
    for ky in range(3):
        for kx in range(3):
            sel = (live & ((a & 15) == 3 * ky + kx)).to(torch.float64)
            out[:, ky:ky + 2 * PH:2, kx:kx + 2 * PW:2] += sel * dp
            mag[:, ky:ky + 2 * PH:2, kx:kx + 2 * PW:2] += sel * dp.abs()
    assert float(mag[:, H:].abs().sum()) == 0 and float(mag[:, :, W:].abs().sum()) == 0, "an arg-max byte points outside the conv output"
    return out[:, :H, :W], mag[:, :H, :W]


# ---- weight gradients and two-segment reductions
def wgrad64(x, dz, k, s, pad):
    """float64 filter gradient x^T dz of a k x k / stride-s conv with top / left padding pad (bottom / right as far as the output grid
    needs): [k][k][C][N].  Runs on the operands' device (float64 GEMMs; exact for integer data below 2^53)."""
    B, H, W, C = x.shape
    _, OH, OW, N = dz.shape
    pb = max((OH - 1) * s + k - H - pad[0], 0)
    pr = max((OW - 1) * s + k - W - pad[1], 0)
    xp = F.pad(x.to(torch.float64).permute(0, 3, 1, 2), (pad[1], pr, pad[0], pb))
    cols = F.unfold(xp, k, stride=s)                                     # [B][C k k][L], L >= OH OW
    L = cols.shape[2]
    nw = (xp.shape[3] - k) // s + 1
    cols = cols.reshape(B, C * k * k, L // nw, nw)[:, :, :OH, :OW].reshape(B, C * k * k, OH * OW)
    g = torch.einsum("bkl,bln->kn", cols, dz.to(torch.float64).reshape(B, OH * OW, N))
    return g.reshape(C, k, k, N).permute(1, 2, 0, 3)


def two_segment(x0, w0, x1, w1):
    """(x0 w0^T + x1 w1^T, |x0| |w0|^T + |x1| |w1|^T) in float64: ONE reduction of K0 + K1 terms, rounded once when stored."""
    d = lambda t: t.to(torch.float64)
    return d(x0) @ d(w0).T + d(x1) @ d(w1).T, d(x0).abs() @ d(w0).abs().T + d(x1).abs() @ d(w1).abs().T
