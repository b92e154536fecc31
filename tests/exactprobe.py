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
two-segment reductions (two_segment) live here too, each with a CPU test that it rejects the fault it is there to expose; so do
those of the launches around a stage's first block (pair_shortcut64, pair_entry64), the tile partition of the pair launches
(tiles_per_block), the pixel map of the compact / sampled forms (pixel_map_f32) and the Winograd operands (winograd_uv).

The second half holds the float64 references and counted bounds of the step's tail (losses, global norm, optimizers, gradient
finalisation, batch-statistics BatchNorm) that tests/test_step_tail_exact_gpu.py compares the kernels with, and those of the weight
preparation (fold64 / fold_bounds) and of the split reduction (reduce32 / reduce_bound) for tests/test_param_passes_exact_gpu.py.
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


# ---- the launches around a stage's first block and its end (conv_pairs.hip, conv_pairx.hip, the sampled / compact forms of conv_pair.hip)
def tiles_per_block(ntiles, nblocks):
    """Tiles each block of a pair launch walks, by blockIdx.x (the kernels' own partition): XCD x = blockIdx.x & 7 owns tiles
    [x cpx, min((x + 1) cpx, ntiles)), cpx = ceil(ntiles / 8); its nblocks / 8 blocks stride through that segment."""
    assert nblocks >= 8 and nblocks % 8 == 0
    bpx, cpx = nblocks // 8, -(-ntiles // 8)
    out = []
    for blk in range(nblocks):
        x, lb = blk & 7, blk >> 3
        first, end = x * cpx + lb, min((x + 1) * cpx, ntiles)
        out.append(0 if first >= end else -(-(end - first) // bpx))
    assert sum(out) == ntiles
    return out


def pair_grid_blocks(ntiles, grid_cap):
    """Blocks of a stage-2 pair launch of `ntiles` tiles under option grid_cap (0: none), as long as the device's CU cap does not
    bind (ntiles <= 8 x the CUs / 8): 8 x min(ceil(ntiles / 8), ceil(grid_cap / 8))."""
    bpx = -(-ntiles // 8)
    if grid_cap > 0:
        bpx = min(bpx, -(-grid_cap // 8))
    return 8 * max(bpx, 1)


def pixel_map_f32(p, H, W):
    """NumPy float32 restatement of the index arithmetic by which the compact-add loads and the sampled store locate pixel p of a
    [B][H][W] grid (conv_pair.hip, conv_pairw.hip): b = int(f32(p) * f32(1 / (H W))), one +-1 correction, the same for (y, x).
    p: int32 array.  -> (b, y, x) int32 arrays."""
    f = np.float32
    p = np.asarray(p, dtype=np.int32)
    hw = np.int32(H * W)
    w = np.int32(W)
    rcp_hw, rcp_w = f(1.0) / f(H * W), f(1.0) / f(W)
    b = (p.astype(f) * rcp_hw).astype(np.int32)
    rem = p - b * hw
    lo, hi = rem < 0, rem >= hw
    b = b + hi.astype(np.int32) - lo.astype(np.int32)
    rem = rem - np.where(hi, hw, 0).astype(np.int32) + np.where(lo, hw, 0).astype(np.int32)
    y = (rem.astype(f) * rcp_w).astype(np.int32)
    x = rem - y * w
    lo, hi = x < 0, x >= w
    y = y + hi.astype(np.int32) - lo.astype(np.int32)
    x = x - np.where(hi, w, 0).astype(np.int32) + np.where(lo, w, 0).astype(np.int32)
    return b, y, x


def compact_to_dense(compact, H, W):
    """[B][H/2][W/2][C] -> [B][H][W][C] with the compact rows at even (y, x) and explicit zeros elsewhere."""
    B, _, _, C = compact.shape
    dense = torch.zeros(B, H, W, C, dtype=compact.dtype)
    dense[:, ::2, ::2] = compact
    return dense


def pair_shortcut64(src, w1, b1, xin, ws, bs):
    """Pre-activation of the forward pair with the projection shortcut inside, src W1^T + xin Ws^T + (b1 + bs), and its magnitude:
    ONE reduction of 128 terms + the two biases.  float64 [M][256] each."""
    z, mag = two_segment(src, w1, xin, ws)
    d = lambda t: t.to(torch.float64)
    return z + d(b1) + d(bs), mag + d(b1).abs() + d(bs).abs()


def pair_entry64(mid, w2, w3, u, p, mask_p):
    """The five products of the backward pair of the stage-entry block from ITS mid [M][256] (float64, as the kernel holds it in LDS):
    dst = (mid W2^T) (u > 0), dP = mid W3^T [(P > 0)], dW2c = u^T mid, dWs = P^T mid, colsum = 1^T mid.
    -> dict name -> (reference, magnitude)."""
    d = lambda t: t.to(torch.float64)
    mid, w2, w3, u, p = d(mid), d(w2), d(w3), d(u), d(p)
    ku = (u > 0).to(torch.float64)
    kp = (p > 0).to(torch.float64) if mask_p else torch.ones_like(p)
    am = mid.abs()
    return {"dst": ((mid @ w2.T) * ku, (am @ w2.abs().T) * ku),
            "dP": ((mid @ w3.T) * kp, (am @ w3.abs().T) * kp),
            "dW2c": (u.T @ mid, u.abs().T @ am),
            "dWs": (p.T @ mid, p.abs().T @ am),
            "colsum": (mid.sum(0), am.sum(0))}


_WG = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)        # G: filter transform
_WBT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)  # B^T: input transform
_WAT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)                              # A^T: output transform


def winograd_uv(g, d):
    """float64 operands of the Winograd F(2x2, 3x3) evaluation of a 3x3 / stride-1 / pad-1 conv: U = G g G^T [4][4][C][N] of the
    filter g [3][3][C][N], V = B^T d B [B][TH][TW][4][4][C] of the 4x4 patches (stride 2, zero padding) of the input d [B][H][W][C]."""
    g, d = g.to(torch.float64), d.to(torch.float64)
    U = torch.einsum("ir,rscn,js->ijcn", _WG, g, _WG)
    B, H, W, C = d.shape
    TH, TW = (H + 1) // 2, (W + 1) // 2
    dp = F.pad(d.permute(0, 3, 1, 2), (1, 2 * TW + 1 - W, 1, 2 * TH + 1 - H))             # rows / columns -1 .. 2 T
    pat = dp.unfold(2, 4, 2).unfold(3, 4, 2)                                               # [B][C][TH][TW][4][4]
    V = torch.einsum("ir,bcyxrs,js->byxijc", _WBT, pat, _WBT)
    return U, V


def winograd_out(U, V, H, W, magnitude=False):
    """A^T (sum_c U V) A of winograd_uv's operands, cropped to [B][H][W][N]: equals the direct conv (proved on the CPU).
    magnitude: the same sums of |U| |V| through |A| -- a bound of every fp32 partial sum of the evaluation."""
    At = _WAT.abs() if magnitude else _WAT
    Mf = torch.einsum("byxijc,ijcn->byxijn", V.abs() if magnitude else V, U.abs() if magnitude else U)
    Y = torch.einsum("ri,byxijn,sj->byrxsn", At, Mf, At)
    B, TH, _, TW, _, N = Y.shape
    return Y.reshape(B, 2 * TH, 2 * TW, N)[:, :H, :W]


# =====================================================================================================================
# The tail of a training step: losses, global norm, optimizers, gradient finalisation, batch-statistics BatchNorm.
# Every reference mirrors the operation's DEFINITION in float64 (not the kernel's loop order); every bound is counted
# from the operation: half an ulp of the storage type at the reference + U = 2^-24 times the magnitude of each fp32
# intermediate times the number of roundings on its path (FMA contraction only lowers it).  Differences of larger
# numbers are charged with the SUM of the magnitudes of their terms.  Each docstring states its count.
U32 = 2.0 ** -24
EXP_FLOOR = 2.0 ** -120             # absolute floor for fp32 denormals the exp unit may flush


def d64(t):
    return t.detach().to("cpu").to(torch.float64) if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t), dtype=torch.float64)


def f32v(x):
    """The float32 value of a Python scalar, as float64 (what a `float` argument of the C ABI carries)."""
    return float(np.float32(x))


def store_bound(ref64, err64, dt):
    """err + half an ulp of the storage type at (|ref| + err): the value is rounded ONCE when stored."""
    return 0.5 * ulp(ref64.abs() + err64, dt) + err64


def assert_within(got, ref64, bound64, what="output"):
    """Elementwise |got - ref| <= bound over the WHOLE extent (no masking); returns the largest ratio to the bound
    (0 / 0 counts as 0: an element whose bound is 0 must be exact)."""
    got = _host64(got).reshape(ref64.shape)
    ref64, bound64 = ref64.to(torch.float64), bound64.to(torch.float64)
    assert got.shape == ref64.shape == bound64.shape, "%s: shapes %s %s %s" % (what, tuple(got.shape), tuple(ref64.shape), tuple(bound64.shape))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % what
    err = (got - ref64).abs()
    bad = err > bound64
    if bool(bad.any()):
        raise AssertionError(_report(what, bad, got, ref64, bound64))
    return float(torch.where(err > 0, err / bound64.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.0


def violations(got, ref64, bound64):
    """Share of elements outside the bound (the CPU rejection tests count it)."""
    got = _host64(got).reshape(ref64.shape)
    bad = ((got - ref64).abs() > bound64) | ~torch.isfinite(got)
    return float(bad.sum()) / max(bad.numel(), 1)


def pairwise_sum32(t, dim=-1):
    """fp32 sum by halving (a tree of depth ceil(log2 n)): the summation of the simulated kernels."""
    t = t.to(torch.float32).movedim(dim, -1)
    while t.shape[-1] > 1:
        if t.shape[-1] & 1:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


# ---- sums of nonnegative terms
def tree_sum_bound(ref64, depth):
    """A sum of nonnegative fp32 terms through an addition tree whose longest chain has `depth` roundings (the product that
    makes a term counts as one): relative depth U / (1 - depth U)."""
    return ref64.abs() * (depth * U32 / (1.0 - depth * U32))


def block_sum_depth(nthreads=256):
    """wave_sum (6 xor-shuffle additions over 64 lanes) + the serial addition of the block's waves."""
    return 6 + nthreads // 64


def sqnorm_depth(n):
    """urso_sqnorm (pool_loss_optim.hip): 1024 x 256 threads sweep float4s: square 1 + 3 additions inside the float4 + one
    addition to the thread's sum per sweep (ceil(n / 4 / 262144)) + 2 for the ragged tail (square, addition; block 0) +
    block sum 10; the final pass adds 1024 parts: 4 per thread + block sum 10."""
    sweeps = max(-(-(n // 4) // (1024 * 256)), 1)
    return 1 + 3 + sweeps + 2 + block_sum_depth() + 4 + block_sum_depth()


def sqnorm_final_depth(nparts):
    """urso_sqnorm_final: ceil(nparts / 256) additions per thread + block sum 10."""
    return -(-nparts // 256) + block_sum_depth()


# ---- softmax cross-entropy with soft labels (TF: dz = (softmax - p) weight / B; row loss lse sum(p) - sum(p z))
def xent_inputs(B, K, psum, seed=0):
    """(logits, labels) float32 [B][K] of the loss probes: post-ReLU logits (about half exactly 0) in the engine's range; soft
    labels that sum to `psum`; row 0 all zero; row 1 (if B > 1) with one logit of 80 (every other term underflows); the last
    row's maximum is its last element."""
    g = torch.Generator().manual_seed(1000 * int(seed) + K + B)
    z = torch.relu(torch.randn(B, K, generator=g) * 2)
    z[0] = 0
    if B > 1:
        z[1, K // 3] = 80.0
    z[B - 1, K - 1] = z[B - 1].max() + 1.5
    p = torch.softmax(torch.randn(B, K, generator=g) * 4, 1) * psum
    return z.contiguous(), p.to(torch.float32).contiguous()


def softmax_sum_depth(K):
    """Longest chain of additions of a row sum in urso_softmax_xent_fwd_bwd: K <= 4096: 4 per thread + 6 (wave) + 16 waves;
    K <= 16384: 16 + 6 + 16; larger: ceil(K / 256) per thread + block sum 10."""
    if K <= 4096:
        return 4 + 6 + 16
    if K <= 16384:
        return 16 + 6 + 16
    return -(-K // 256) + block_sum_depth()


def softmax_xent64(z, p, weight, relu_mask, B=None):
    """-> (loss, row_loss [B], dz [B][K]) in float64.  The scale weight / B is the fp32 quotient the entry point passes on."""
    z, p = d64(z), d64(p)
    B = z.shape[0] if B is None else B
    gs = float(np.float32(weight) / np.float32(B))
    lse = torch.logsumexp(z, 1)
    row = lse * p.sum(1) - (p * z).sum(1)
    dz = (torch.softmax(z, 1) - p) * gs
    if relu_mask:
        dz = torch.where(z > 0, dz, torch.zeros_like(dz))
    return row.sum() * gs, row, dz


def softmax_xent_bounds(z, p, weight, relu_mask, dt):
    """-> (bound of loss, of row_loss, of dz) for fp32 arithmetic with the exp unit, D = softmax_sum_depth(K).
    term e = exp(x), x = z - max <= 0:        (|x| + 4) U e + 2^-120   (x rounded 1, x log2e 1 + the constant, exp2 1 ulp = 2)
    sum S:                                    sum of the terms' errors + D U S
    softmax = e (1 / S):                      err_e / S + softmax (err_S / S + 2 U)            (reciprocal 1, product 1)
    dz = (softmax - p) gs:                    gs err_softmax + 3 U gs (softmax + |p|)          (difference 1, product 1, gs itself 1)
    row = lse sp - spz, lse = max + log S:    |sp| (err_S / S + 2 U |log S| + U |lse|)  (logf 1 ulp = 2, addition 1)
                                              + |lse| (D + 1) U sum|p| + (D + 2) U sum|p z| + U (|lse sp| + |spz|)
    loss = gs sum(row):                       gs (sum of the rows' errors + (ceil(B / 256) + 10 + 2) U sum|row|)
    dz is stored in `dt` (half an ulp on top), the losses in fp32."""
    z, p = d64(z), d64(p)
    B, K = z.shape
    D = softmax_sum_depth(K)
    gs = float(np.float32(weight) / np.float32(B))
    m = z.max(1, keepdim=True).values
    x = z - m
    e = torch.exp(x)
    S = e.sum(1, keepdim=True)
    err_e = (x.abs() + 4) * U32 * e + EXP_FLOOR
    err_S = err_e.sum(1, keepdim=True) + D * U32 * S
    soft = e / S
    err_soft = err_e / S + soft * (err_S / S + 2 * U32)
    err_dz = gs * err_soft + 3 * U32 * gs * (soft + p.abs())
    if relu_mask:
        err_dz = torch.where(z > 0, err_dz, torch.zeros_like(err_dz))
    _, row, dz = softmax_xent64(z, p, weight, relu_mask)
    logS, sp, spz = torch.log(S[:, 0]), p.sum(1), (p * z).sum(1)
    lse = m[:, 0] + logS
    sabs, spzabs = p.abs().sum(1), (p * z).abs().sum(1)
    err_row = (sp.abs() * (err_S[:, 0] / S[:, 0] + 2 * U32 * logS.abs() + U32 * lse.abs())
               + lse.abs() * (D + 1) * U32 * sabs + (D + 2) * U32 * spzabs + U32 * ((lse * sp).abs() + spz.abs()))
    err_loss = gs * (err_row.sum() + (-(-B // 256) + block_sum_depth() + 2) * U32 * row.abs().sum())
    return store_bound(row.sum() * gs, err_loss, 0), store_bound(row, err_row, 0), store_bound(dz, err_dz, dt)


def softmax_xent32(z, p, weight, relu_mask, dt, exp2=True):
    """Plain fp32 restatement (the simulated kernel): exp as exp2(x * 1.442695), pairwise fp32 sums, gradient rounded once."""
    z, p = z.to(torch.float32), p.to(torch.float32)
    B = z.shape[0]
    gs = torch.tensor(np.float32(weight) / np.float32(B))
    m = z.max(1, keepdim=True).values
    x = z - m
    e = torch.exp2(x * torch.tensor(1.442695, dtype=torch.float32)) if exp2 else torch.exp(x)
    S = pairwise_sum32(e)[:, None]
    dz = (e * (1.0 / S) - p) * gs
    if relu_mask:
        dz = torch.where(z > 0, dz, torch.zeros_like(dz))
    row = (m[:, 0] + torch.log(S[:, 0])) * pairwise_sum32(p) - pairwise_sum32(p * z)
    return pairwise_sum32(row) * gs, row, dz.to(tdtype(dt))


# ---- the regression losses on [B][D] heads stored with row stride ld (columns D.. of the gradient are exactly 0)
def _pad_cols(g, ld):
    return F.pad(g, (0, ld - g.shape[1]))


def rel_l2_64(gt, pred, weight, gscale=1.0):
    """||gt - pred||_F / ||gt||_F over the batch: -> (loss, dpred [B][ld], (sd, sg)); pred is [B][ld], its columns D.. are ignored.
    The gradient is -weight gscale (gt - pred) / (nd ng)."""
    gt, pred = d64(gt), d64(pred)
    D, ld, w = gt.shape[1], pred.shape[1], f32v(weight)
    e = gt - pred[:, :D]
    sd, sg = (e * e).sum(), (gt * gt).sum()
    nd, ng = sd.sqrt(), sg.sqrt()
    return w * nd / ng, _pad_cols(-w * f32v(gscale) / (nd * ng) * e, ld), torch.stack([sd, sg])


def rel_l2_bounds(gt, pred, weight, dt, gscale=1.0):
    """S = ceil(B D / 256) + 10 (+ 3: difference 1, square 1, first addition) roundings on each squared norm, relative.
    loss = w nd / ng: half of each norm's error ((S + 3) U in all) + 2 square roots + product + quotient = (S + 7) U.
    gradient c (gt - pred), c = -w gscale / (nd ng): (S + 3) + 2 + product 1 + quotient 1 + gscale 1, difference 1,
    product 1 = (S + 10) U relative, + half an ulp of `dt`.  -> (loss, gradient, norms)."""
    loss, g, norms = rel_l2_64(gt, pred, weight, gscale)
    S = -(-gt.numel() // 256) + block_sum_depth()
    return (store_bound(loss, (S + 7) * U32 * loss.abs(), 0), store_bound(g, (S + 10) * U32 * g.abs(), dt),
            store_bound(norms, tree_sum_bound(norms, S + 3), 0))


def mse64(gt, pred, weight):
    """weight mean((pred - gt)^2) -> (loss, dpred [B][ld] = 2 weight (pred - gt) / (B D))."""
    gt, pred = d64(gt), d64(pred)
    B, D = gt.shape
    e = pred[:, :D] - gt
    w = f32v(weight)
    return w * (e * e).sum() / (B * D), _pad_cols(2 * w / (B * D) * e, pred.shape[1])


def mse_bounds(gt, pred, weight, dt):
    """gradient: quotient in c 1, difference 1, product 1 = 3 U relative + half an ulp of `dt`;
    loss: S = ceil(B ld / 256) + 10 additions + 3 (difference, square, first addition) + product 1 + quotient 1 = (S + 5) U."""
    loss, g = mse64(gt, pred, weight)
    S = -(-pred.numel() // 256) + block_sum_depth()
    return store_bound(loss, (S + 5) * U32 * loss.abs(), 0), store_bound(g, 3 * U32 * g.abs(), dt)


ABSDOT_CLAMP = float(np.float32(1e-12))


def absdot64(gt, x, weight, normalize, clamp_branch=True):
    """q = x / sqrt(max(|x|^2, 1e-12)) (normalize) or x; loss = weight mean(1 - |gt . q|); dq = -sign(dot) gt weight / B with
    sign(0) = 0; dx = rinv (dq - q (q . dq)), and rinv dq on a clamped row (|x|^2 <= 1e-12: q = x rinv has no norm
    constraint).  gt None: the inference form, only q.  -> (q [B][D], loss, dx [B][ld], dot [B], magnitude of dx's terms)."""
    x = d64(x)
    B, ld = x.shape
    D = gt.shape[1] if gt is not None else None
    if D is None:
        raise ValueError("pass D through absdot_q64 for the inference form")
    xv = x[:, :D]
    ss = (xv * xv).sum(1, keepdim=True)
    clamped = ~(ss > ABSDOT_CLAMP)
    rinv = torch.rsqrt(ss.clamp_min(ABSDOT_CLAMP)) if normalize else torch.ones_like(ss)
    q = xv * rinv
    gt = d64(gt)
    w = f32v(weight)
    dot = (gt * q).sum(1, keepdim=True)
    dq = -torch.sign(dot) * gt * (w / B)
    qdq = (q * dq).sum(1, keepdim=True)
    proj = q * qdq
    if normalize and clamp_branch:
        proj = torch.where(clamped, torch.zeros_like(proj), proj)
    dx = rinv * (dq - proj) if normalize else dq
    mag = rinv * (dq.abs() + (proj != 0) * q.abs() * (q * dq).abs().sum(1, keepdim=True)) if normalize else dq.abs()
    return q, w * (1 - dot.abs()).mean(), _pad_cols(dx, ld), dot[:, 0], _pad_cols(mag, ld)


def absdot_q64(x, D, normalize):
    """The inference form (gt = None): q alone."""
    xv = d64(x)[:, :D]
    ss = (xv * xv).sum(1, keepdim=True)
    return xv * (torch.rsqrt(ss.clamp_min(ABSDOT_CLAMP)) if normalize else 1.0)


def absdot_bounds(gt, x, weight, normalize, dt):
    """R = D + 4 roundings on q = x rinv, relative (|x|^2: D + 1 roundings, halved by the root; rsqrt 1 ulp = 2; product 1);
    0 without normalisation (q = x, dx = dq).
    dot = sum gt q: (R + D + 1) U sum|gt q|.     loss: w (mean of the dots' errors + (ceil(B / 256) + 10 + 3) U mean|1 - |dot||).
    dx = rinv (dq - q qdq): on the sum of the magnitudes rinv (|dq| + |q| sum|q dq|):
      c = -sign w / B 1, dq 1, rinv R, q R, qdq R + D + 1, difference 1, two products 2  ->  (3 R + D + 6) U;  dq alone: 2 U.
    -> (q, loss, dx) bounds; dx stored in `dt`."""
    q, loss, dx, dot, mag = absdot64(gt, x, weight, normalize)
    B, D = q.shape
    R = D + 4 if normalize else 0
    gtq = (d64(gt) * q).abs().sum(1)
    err_dot = (R + D + 1) * U32 * gtq
    w = f32v(weight)
    err_loss = w * (err_dot.mean() + (-(-B // 256) + block_sum_depth() + 3) * U32 * (1 - dot.abs()).abs().mean())
    err_dx = ((3 * R + D + 6) if normalize else 2) * U32 * mag
    return store_bound(q, R * U32 * q.abs(), 0), store_bound(loss, err_loss, 0), store_bound(dx, err_dx, dt)


# ---- optimizers.  normsq is an ARGUMENT: the GPU tests pass the value the device wrote (checked on its own)
def sgd_data(n, case, seed=0):
    """(w, g, v, lr, mom, clip) of the SGD probes, float32; the median of |step g| / |mom v| is >= 0.1 in every case (a wrong
    step size shows in v), and the gradient norm is a factor 2 away from clip.  case: 'unclipped', 'clipped', 'noclip'
    (clip = 0 with a large gradient), 'mom0'."""
    g_ = torch.Generator().manual_seed(int(seed) + n)
    w = torch.randn(n, generator=g_)
    v = torch.randn(n, generator=g_) * 0.01
    g = torch.randn(n, generator=g_) * (10.0 if case == "noclip" else 0.1)
    norm = float(g.double().pow(2).sum().sqrt())
    clip = {"unclipped": 2.0 * norm, "clipped": 0.5 * norm, "noclip": 0.0, "mom0": 2.0 * norm}[case]
    return w, g, v, 0.05, (0.0 if case == "mom0" else 0.9), float(np.float32(clip))


def clip_factor64(normsq, clip):
    norm = math.sqrt(float(normsq))
    clip = f32v(clip)
    return clip / norm if (clip > 0 and norm >= clip) else 1.0


def sgd64(w, g, v, lr, mom, clip, normsq):
    """keras SGD(momentum, clipnorm) with the global norm: step = lr c, c = clip / norm if clip > 0 and norm >= clip else 1;
    v' = mom v - step g; w' = w + v'.  -> (w', v', bound of w', bound of v', median |step g| / |mom v|).
    Roundings: step: square root 1, quotient 1, product 1 = 3; v': mom v 1, step g 3 + 1, difference 1 on the sum of the
    magnitudes -> U (2 |mom v| + 5 |step g|); w': the error of v' + U (|w| + |v'|); both stored in fp32."""
    w, g, v = d64(w), d64(g), d64(v)
    step, mom = f32v(lr) * clip_factor64(normsq, clip), f32v(mom)
    a, b = mom * v, step * g
    v2 = a - b
    w2 = w + v2
    err_v = U32 * (2 * a.abs() + 5 * b.abs())
    err_w = err_v + U32 * (w.abs() + v2.abs())
    ratio = float((b.abs() / a.abs().clamp_min(1e-300)).median()) if mom != 0 else float("inf")
    return w2, v2, store_bound(w2, err_w, 0), store_bound(v2, err_v, 0), ratio


def sgd32(w, g, v, lr, mom, clip, normsq, lr_factor=1.0, keep_from=None, keep_to=None):
    """fp32 restatement (the simulated kernel); lr_factor plants a wrong learning rate, [keep_from, keep_to) is left
    un-updated (a dropped tail or grid sweep)."""
    f = np.float32
    norm = np.sqrt(f(normsq))
    c = f(clip) / norm if (f(clip) > 0 and norm >= f(clip)) else f(1)
    step = torch.tensor(f(f(lr) * f(lr_factor)) * c)
    v2 = v * torch.tensor(f(mom)) - g * step
    w2 = w + v2
    if keep_from is not None:
        v2[keep_from:keep_to] = v[keep_from:keep_to]
        w2[keep_from:keep_to] = w[keep_from:keep_to]
    return w2, v2


# Adam's lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) goes through powf, whose error is amplified by the cancellation in 1 - b2^t
# (b2 = 0.999): not derivable from rounding counts.  MEASURED: the float32 NumPy restatement adam_lr_t32() against float64 on
# the probes' hyper-parameters (lr 1e-3, b1 0.9, b2 0.999, t = 1, 2, 3) is off by at most 3.42e-6 relative
# (tests/test_exactprobe_cpu.py::test_adam_lr_t_measured recomputes it); allowed: 4 x that.
ADAM_LRT_MEASURED = 3.42e-6
ADAM_LRT_REL = 4 * ADAM_LRT_MEASURED


def adam_lr_t32(lr, b1, b2, t):
    f = np.float32
    return f(lr) * (np.sqrt(f(1) - np.power(f(b2), f(t), dtype=f)) / (f(1) - np.power(f(b1), f(t), dtype=f)))


def adam_lr_t64(lr, b1, b2, t):
    lr, b1, b2 = f32v(lr), f32v(b1), f32v(b2)
    return lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)


def adam64(w, g, m, v, vhat, hyper, normsq, v_from_unclipped=False):
    """Keras 2 Adam(amsgrad=True, clipnorm): hyper = (lr, b1, b2, eps, clip, t AFTER the tick, 1 - b1, 1 - b2) as the device holds
    them (fp32 values).  gc = g c; m' = b1 m + c1 gc; v' = b2 v + c2 gc^2; vhat' = max(vhat, v'); w' = w - lr_t m' / (sqrt(vhat') + eps).
    -> dict name -> (reference, bound).  Roundings: c: square root 1 + quotient 1, gc: + 1 = 3 (0 when not clipped -- kept);
    m': U (2 |b1 m| + 5 |c1 gc|);  v': U (2 |b2 v| + 9 |c2 gc^2|) (gc^2: 6 + 1, product 1, addition 1);  vhat': that of v';
    update u = lr_t m' / (sqrt(vhat') + eps): relative ADAM_LRT_REL (measured, see above) + err_m / |m'| + err_vhat / (2 vhat')
    + 4 U (root, addition, product, quotient);  w': err_u + U (|w| + |u|)."""
    w, g, m, v, vhat = d64(w), d64(g), d64(m), d64(v), d64(vhat)
    lr, b1, b2, eps, clip, t, c1, c2 = [float(h) for h in d64(hyper)[:8]]
    gc = g * clip_factor64(normsq, clip)
    gv = g if v_from_unclipped else gc
    a, b = b1 * m, c1 * gc
    m2 = a + b
    p, q = b2 * v, c2 * gv * gv
    v2 = p + q
    vh2 = torch.maximum(vhat, v2)
    den = vh2.sqrt() + eps
    u = adam_lr_t64(lr, b1, b2, t) * m2 / den
    w2 = w - u
    err_m = U32 * (2 * a.abs() + 5 * b.abs())
    err_v = U32 * (2 * p.abs() + 9 * q.abs())
    err_u = u.abs() * (ADAM_LRT_REL + 4 * U32) + adam_lr_t64(lr, b1, b2, t) * (err_m / den + m2.abs() * err_v / (2 * vh2.sqrt().clamp_min(1e-300) * den * den))
    err_w = err_u + U32 * (w.abs() + u.abs())
    return {"w": (w2, store_bound(w2, err_w, 0)), "m": (m2, store_bound(m2, err_m, 0)),
            "v": (v2, store_bound(v2, err_v, 0)), "vhat": (vh2, store_bound(vh2, err_v, 0))}


def adam32(w, g, m, v, vhat, hyper, normsq, v_from_unclipped=False):
    """fp32 restatement of the update (the simulated kernel)."""
    f = np.float32
    lr, b1, b2, eps, clip, t, c1, c2 = [f(h) for h in hyper[:8].tolist()]
    norm = np.sqrt(f(normsq))
    c = torch.tensor(clip / norm if (clip > 0 and norm >= clip) else f(1))
    gc = g * c
    gv = g if v_from_unclipped else gc
    m2 = torch.tensor(b1) * m + torch.tensor(c1) * gc
    v2 = torch.tensor(b2) * v + torch.tensor(c2) * (gv * gv)
    vh2 = torch.maximum(vhat, v2)
    w2 = w - torch.tensor(adam_lr_t32(lr, b1, b2, t)) * m2 / (vh2.sqrt() + torch.tensor(eps))
    return w2, m2, v2, vh2


# ---- parameter-gradient finalisation of a conv / dense layer with its frozen BatchNorm folded in
def finalize64(dw_raw, colsum, W, b, gamma, mean, var, eps, wd, gamma_term=True, dw_mag=None, cs_mag=None):
    """Closed form; s = gamma / sqrt(var + eps) (1 without BN), dw_raw [K][N] (the padded columns already dropped):
      gW = s dw_raw + 2 wd / (K N) W;  gb = s colsum + 2 wd / N b;
      ggamma = (sum_k W dw_raw + (b - mean) colsum) / sqrt(var + eps);  gbeta = colsum.
    b / gamma None: absent.  -> dict name -> (reference, magnitude of the terms).  (tests/test_exactprobe_cpu.py proves it
    equal to float64 autograd through conv -> frozen BatchNorm + the L2 term.)
    dw_mag / cs_mag: where dw_raw / colsum are themselves fp32 sums of split partials, the sums of the partials' magnitudes; they
    replace |dw_raw| / |colsum| in the magnitudes (finalize_bounds(..., sum_depth) charges the partial sums' roundings to them)."""
    dw, cs, W = d64(dw_raw), d64(colsum), d64(W)
    K, N = W.shape
    eps, wd = f32v(eps), f32v(wd)
    rstd = torch.rsqrt(d64(var) + eps) if gamma is not None else None
    s = d64(gamma) * rstd if gamma is not None else torch.ones(N, dtype=torch.float64)
    regc, regb = 2 * wd / (float(K) * float(N)), 2 * wd / float(N)
    dwm = d64(dw_mag) if dw_mag is not None else dw.abs()
    csm = d64(cs_mag) if cs_mag is not None else cs.abs()
    out = {"gw": (s * dw + regc * W, s.abs() * dwm + (regc * W).abs())}
    if b is not None:
        out["gb"] = (s * cs + regb * d64(b), s.abs() * csm + (regb * d64(b)).abs())
    if gamma is not None:
        bm = (d64(b) if b is not None else 0.0) - d64(mean)
        extra = bm * cs if gamma_term else torch.zeros_like(cs)
        out["ggamma"] = (rstd * ((W * dw).sum(0) + extra), rstd * ((W.abs() * dwm).sum(0) + torch.as_tensor(bm).abs() * csm))
        out["gbeta"] = (cs.clone(), csm.clone())
    return out


BN_SCALE_ROUNDINGS = 4      # s = gamma rsqrt(var + eps) in fp32: addition 1, rsqrt 1 ulp = 2, product 1 (finalize_bounds, fold_bounds)


def finalize_bounds(ref, K, N, ldn, ks, sum_depth=0):
    """Roundings (ks = row slabs of the launch, kb = ceil(K / ks) rows each; vector body when (N | ldn) % 4 == 0):
      gW, gb: s = gamma rsqrt(var + eps): addition 1, rsqrt 1 ulp = 2, product 1 = 4; s d 1; the L2 factor 2, its product 1;
              sum 1  ->  6 U on |s d| + |reg W|.
      ggamma: the dot sum_k W d: product 1 + ceil(kb / 16) additions per row lane + 15 lanes (vector) or ceil(kb / 4) + 3
              (scalar), + the slabs: ceil(ks / 4) + 2; (b - mean) colsum: 2; sum 1; rstd 3, product 1
              ->  (dot depth + 6) U on rstd (sum|W d| + |(b - mean) colsum|).
      gbeta = colsum: exact.        All stored in fp32.  -> dict name -> bound.
    sum_depth > 0 (the batched passes: d and colsum are fp32 sums of split partials, reduce_depth(splits) roundings on their longest
    chain; `ref` then comes from finalize64(..., dw_mag, cs_mag)): every count grows by sum_depth -- gW, gb: 6 + sum_depth;
    ggamma: dot depth + 6 + sum_depth; gbeta: sum_depth."""
    kb = -(-K // ks)
    ddot = 1 + ((-(-kb // 16) + 15) if ((N | ldn) & 3) == 0 else (-(-kb // 4) + 3)) + -(-ks // 4) + 2
    cnt = {"gw": 6 + sum_depth, "gb": 6 + sum_depth, "ggamma": ddot + 6 + sum_depth, "gbeta": sum_depth}
    return {k: store_bound(r, cnt[k] * U32 * mag, 0) if cnt[k] else torch.zeros_like(r) for k, (r, mag) in ref.items()}


def finalize_sq_depth(K, N, ldn, ks, nslots):
    """Sum of squares through the _sq slots and urso_sqnorm_final: a block's slot: square 1 + 3 inside a float4 + ceil(kb / 16)
    additions per thread (vector; scalar: 1 + ceil(kb / 4)) + block sum 10; the channel block: 3 squares' sum + block sum;
    then sqnorm_final_depth(nslots)."""
    kb = -(-K // ks)
    per = (4 + -(-kb // 16)) if ((N | ldn) & 3) == 0 else (1 + -(-kb // 4))
    return per + block_sum_depth() + sqnorm_final_depth(nslots)


def finalize32(dw_raw, colsum, W, b, gamma, mean, var, eps, wd, gamma_term=True):
    """fp32 restatement (the simulated kernel), pairwise column dots."""
    f = torch.float32
    K, N = W.shape
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=f)) if gamma is not None else None
    s = gamma * rstd if gamma is not None else torch.ones(N)
    regc = torch.tensor(np.float32(2.0) * np.float32(wd) / (np.float32(K) * np.float32(N)))
    regb = torch.tensor(np.float32(2.0) * np.float32(wd) / np.float32(N))
    out = {"gw": s * dw_raw + regc * W}
    if b is not None:
        out["gb"] = s * colsum + regb * b
    if gamma is not None:
        bm = (b if b is not None else torch.zeros(N)) - mean
        out["ggamma"] = rstd * (pairwise_sum32(W * dw_raw, 0) + (bm * colsum if gamma_term else 0.0))
        out["gbeta"] = colsum.clone()
    return out


# ---- weight preparation: the frozen BatchNorm folded into filter and bias, in the MFMA layouts (urso_conv_weight_prep, PB_PREP)
def _bn_scale64(bn, eps, N):
    if bn is None:
        return torch.ones(N, dtype=torch.float64)
    return d64(bn[0]) * torch.rsqrt(d64(bn[3]) + f32v(eps))


def _folded_bias64(b, bn, eps, N):
    """(b s + beta - mean s, the list of its terms' magnitudes) of one layer, [N] float64."""
    s = _bn_scale64(bn, eps, N)
    z = torch.zeros(N, dtype=torch.float64)
    bs = d64(b) * s if b is not None else z
    beta, ms = (d64(bn[1]), d64(bn[2]) * s) if bn is not None else (z, z)
    return bs + beta - ms, (bs.abs(), beta.abs(), ms.abs())


def fold_inputs(KH, KW, C, N, seed=0, tiny_block=None):
    """(w [KH][KW][C][N], b [N], (gamma, beta, mean, var)) float32 of the preparation probes: BN tensors as the finalisation probes'
    (gamma and var in [0.5, 1.5]: s is no power of two), random mean / beta / bias.  tiny_block = (n0, n1): the filters n0 .. n1 are
    scaled so that |w s| there is around 3e-6, fp16 subnormals (a store that flushes them fails the bound)."""
    g = torch.Generator().manual_seed(1000 * int(seed) + 7 * KH * KW * C + N)
    w = torch.randn(KH, KW, C, N, generator=g) / (KH * KW * C) ** 0.5
    b = torch.randn(N, generator=g)
    bn = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g), torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5)
    if tiny_block is not None:
        n0, n1 = tiny_block
        w[..., n0:n1] = torch.randn(KH, KW, C, n1 - n0, generator=g) * 3e-6
    return w.contiguous(), b, bn


def fold64(w, b, bn, eps, npad, extra=None):
    """The definition of the weight preparation in float64.  w [KH][KW][C][N] (HWIO), b [N] or None, bn = (gamma, beta, mean, var)
    or None, eps the fp32 value the entry point receives; s = gamma / sqrt(var + eps) (1 without BN):
      wf [npad][KH][KW][C]: wf[n][tap][c] = w[tap][c][n] s[n];   wd [C][KH][KW][npad]: wd[c][taps - 1 - tap][n] = w[tap][c][n] s[n];
      biasf [npad] = b s + beta - mean s (+ the folded bias of `extra` = another layer's (b, bn, N) for n < extra's N:
      urso_param_desc::bias_from);   scale [npad] = s.
    Filters N .. npad: wf / wd / biasf exactly 0, scale exactly 1.
    -> dict name -> (reference, magnitude); biasf's magnitude is the TUPLE (|b s|, |beta|, |mean s|, |b' s'|, |beta'|, |mean' s'|)
    of its terms (primes: extra's), each [npad], which fold_bounds charges one by one."""
    w = d64(w)
    KH, KW, C, N = w.shape
    assert npad >= N
    s = _bn_scale64(bn, eps, N)
    p = w * s
    wf = torch.zeros(npad, KH, KW, C, dtype=torch.float64)
    wf[:N] = p.permute(3, 0, 1, 2)
    wd = torch.zeros(C, KH, KW, npad, dtype=torch.float64)
    wd[..., :N] = p.flip(0, 1).permute(2, 0, 1, 3)
    pad = lambda t, v=0.0: torch.cat([t, torch.full((npad - N,), v, dtype=torch.float64)])
    bf, terms = _folded_bias64(b, bn, eps, N)
    z = torch.zeros(N, dtype=torch.float64)
    eterms = (z, z, z)
    if extra is not None:
        eb, ebn, eN = extra
        m = min(int(eN), N)
        ebf, et = _folded_bias64(eb, ebn, eps, int(eN))
        head = lambda t: torch.cat([t[:m], torch.zeros(N - m, dtype=torch.float64)])
        bf = bf + head(ebf)
        eterms = tuple(head(t) for t in et)
    scale = pad(s, 1.0)
    return {"wf": (wf, wf.abs()), "wd": (wd, wd.abs()), "biasf": (pad(bf), tuple(pad(t) for t in terms + eterms)),
            "scale": (scale, torch.cat([s.abs(), torch.zeros(npad - N, dtype=torch.float64)]))}


def fold_bounds(ref, dt, bias, bn, extra=None):
    """Counted fp32 roundings of the preparation (derived from the operation, not measured); bias / bn: whether the layer has them,
    extra: None or (extra has bias, extra has BN).  S = BN_SCALE_ROUNDINGS = 4 on s = gamma rsqrt(var + eps) (finalize_bounds'
    count: addition 1, rsqrt 1 ulp = 2, product 1); without BN s is the constant 1 and a product with it is exact: 0.
      scale = s:        S U |s|  (0 without BN; the padded filters' 1 is exact), stored in fp32.
      wf, wd = w s:     S + the product 1 = 5 U |w s| (0 without BN), then rounded ONCE to `dt`: + half an ulp of `dt`.
      biasf:            b s: S + product 1 = 5 U |b s| (0 without BN);  mean s: 5 U |mean s|;  beta - mean s: 1 U (|beta| + |mean s|);
                        the sum of b s and that difference: 1 U (|b s| + |beta| + |mean s|), only when both are there;
                        extra's folded bias, computed on its own: the same counts on ITS terms;  adding it: 1 U on all six terms.
                        Stored in fp32.
    A padded filter has magnitude 0 everywhere, so its bound is half an ulp at its reference (0, or 1 for scale): no other value of the
    storage type lies inside it, and the definition's exact 0 / 1 is what is asserted."""
    S = BN_SCALE_ROUNDINGS if bn else 0
    out = {}
    r, mag = ref["scale"]
    out["scale"] = store_bound(r, S * U32 * mag, 0) if S else torch.zeros_like(r)
    for k in ("wf", "wd"):
        r, mag = ref[k]
        out[k] = store_bound(r, ((S + 1) if bn else 0) * U32 * mag, dt)
    r, (bs, beta, ms, ebs, ebeta, ems) = ref["biasf"]

    def own(bs, beta, ms, has_b, has_bn):
        if not has_bn:
            return torch.zeros_like(bs)                      # b * 1 or nothing: exact
        e = 5 * ms + (beta + ms)
        if has_b:
            e = e + 5 * bs + (bs + beta + ms)
        return e
    err = own(bs, beta, ms, bias, bn)
    if extra is not None:
        err = err + own(ebs, ebeta, ems, extra[0], extra[1]) + (bs + beta + ms + ebs + ebeta + ems)
    out["biasf"] = store_bound(r, U32 * err, 0) if (bn or extra is not None) else torch.zeros_like(r)
    return out


def fold32(w, b, bn, eps, npad, dt, extra=None, flip=True, s_round=None, use_eps=True, use_extra=True, pad_scale=1.0):
    """Plain fp32 restatement of the preparation (the simulated kernel) -> dict name -> tensor (wf / wd in `dt`, biasf / scale fp32).
    Faults: flip=False leaves wd's taps unflipped; s_round = a 16-bit type rounds s to it before the products; use_eps=False leaves
    eps out; use_extra=False leaves extra's folded bias out; pad_scale: scale of the padded filters."""
    f = torch.float32
    w = w.to(f)
    KH, KW, C, N = w.shape
    e = torch.tensor(eps if use_eps else 0.0, dtype=f)

    def sc(bn_, n):
        s_ = bn_[0].to(f) * torch.rsqrt(bn_[3].to(f) + e) if bn_ is not None else torch.ones(n)
        return s_.to(s_round).to(f) if s_round is not None else s_

    def fb(b_, bn_, n):
        s_ = sc(bn_, n)
        v = b_.to(f) * s_ if b_ is not None else torch.zeros(n)
        return v + (bn_[1].to(f) - bn_[2].to(f) * s_) if bn_ is not None else v
    s = sc(bn, N)
    p = w * s
    wf = torch.zeros(npad, KH, KW, C); wf[:N] = p.permute(3, 0, 1, 2)
    wd = torch.zeros(C, KH, KW, npad); wd[..., :N] = (p.flip(0, 1) if flip else p).permute(2, 0, 1, 3)
    bf = torch.zeros(npad); bf[:N] = fb(b, bn, N)
    if extra is not None and use_extra:
        m = min(int(extra[2]), N)
        bf[:m] += fb(extra[0], extra[1], int(extra[2]))[:m]
    scale = torch.full((npad,), pad_scale, dtype=f); scale[:N] = s
    return {"wf": wf.to(tdtype(dt)), "wd": wd.to(tdtype(dt)), "biasf": bf, "scale": scale}


# ---- the split reduction of weight-gradient partials (reduce_partials_body, conv_wgrad.hip) and the sums fused into the finalisation
WGRAD_PART_PAD = 64                # URSO_WGRAD_PART_PAD: floats between consecutive partial tensors
FUSE_REDUCE_MAX = 16               # URSO_FUSE_REDUCE_MAX: up to here the finalisation sums the partials itself


PART_SENTINEL = 3.0e7              # finite filler of the gaps between partials and of the padded columns: must reach no gradient


def partials_buffer(K, N, npad, splits, seed=0):
    """Random weight-gradient partials in the documented workspace layout (urso_conv_wgrad_partial): one flat fp32 buffer holding
    part[splits][K * npad + WGRAD_PART_PAD] followed by colpart[splits][npad]; the WGRAD_PART_PAD floats behind every partial and the
    padded columns N .. npad of both hold PART_SENTINEL.  -> (flat, parts [splits][K][npad], colparts [splits][npad]), the last two
    being copies in their logical shapes (sentinel columns included)."""
    g = torch.Generator().manual_seed(100003 * int(seed) + 31 * K + 7 * npad + splits)
    stride = K * npad + WGRAD_PART_PAD
    parts = torch.full((splits, K, npad), PART_SENTINEL)
    parts[:, :, :N] = torch.randn(splits, K, N, generator=g)
    colparts = torch.full((splits, npad), PART_SENTINEL)
    colparts[:, :N] = torch.randn(splits, N, generator=g) * 5
    flat = torch.full((splits * stride + splits * npad,), PART_SENTINEL)
    flat[:splits * stride].reshape(splits, stride)[:, :K * npad] = parts.reshape(splits, K * npad)
    flat[splits * stride:] = colparts.reshape(-1)
    return flat, parts, colparts


def reduce_lanes(splits):
    """urso_reduce_lanes (csrc/common.h): split-lanes of the reduction kernel."""
    return 16 if splits > 384 else (8 if splits > 192 else (4 if splits > 96 else (2 if splits > 48 else 1)))


def reduce32(parts, splits=None):
    """Host fp32 emulation of reduce_partials_body's documented order over parts [splits][...] (fp32): SL = reduce_lanes(splits);
    lane sl adds its contiguous run of ceil(splits / SL) partials in order, starting from +0; the lanes are then added in lane order
    (one lane: its sum is the result).  Pure additions, so a kernel in that order matches bit for bit.  The sums the finalisation
    fuses (2 .. 16 splits) are the one-lane case: sequential from +0."""
    parts = parts.to(torch.float32)
    splits = parts.shape[0] if splits is None else int(splits)
    assert parts.shape[0] == splits
    SL = reduce_lanes(splits)
    per = -(-splits // SL)
    lanes = []
    for sl in range(SL):
        t = torch.zeros_like(parts[0])
        for k in range(sl * per, min(splits, (sl + 1) * per)):
            t = t + parts[k]
        lanes.append(t)
    t = lanes[0]
    for other in lanes[1:]:
        t = t + other
    return t


def reduce_depth(splits):
    """Roundings on the longest chain of reduce32: ceil(splits / SL) - 1 inside a lane (+0 + the first partial is exact) + SL - 1
    additions of the lanes."""
    SL = reduce_lanes(splits)
    return -(-splits // SL) - 1 + SL - 1


def reduce_bound(mag64, splits):
    """|fp32 sum in reduce32's order - float64 sum| <= D U / (1 - D U) sum|terms|, D = reduce_depth(splits): every rounding is half
    an ulp of a partial sum, none of which exceeds sum|terms|.  splits = 1: 0 (a copy)."""
    D = reduce_depth(splits)
    return d64(mag64) * (D * U32 / (1.0 - D * U32))


# ---- batch-statistics BatchNorm over [M][N]
def bn_stats64(z, mmean, mvar, momentum, eps, corrected=True):
    """mean, biased variance (clamped at 0), and Keras' moving statistics: mmean' = mmean mom + mean (1 - mom);
    mvar' = mvar mom + var M / (M - (1 + eps)) (1 - mom).  -> dict name -> (reference, bound).
    The kernel sums in float64 (M terms: M 2^-53 on the sums' magnitudes, var = E[z^2] - mean^2 charged with both terms), rounds
    mean / var to fp32 once; the moving updates run in fp32 on those rounded values: (1 - mom) 1, two products 2, sum 1 ->
    U (2 |old mom| + 3 |new (1 - mom)|) + the rounding of the batch value (1 - mom) / 2 ulp."""
    z = d64(z)
    M = z.shape[0]
    mom, eps = f32v(momentum), f32v(eps)
    D = M * 2.0 ** -53
    mean = z.mean(0)
    ez2 = (z * z).mean(0)
    var = (ez2 - mean * mean).clamp_min(0)
    err_mean, err_var = D * z.abs().mean(0), 3 * D * (ez2 + mean * mean)
    out = {"mean": (mean, store_bound(mean, err_mean, 0)), "var": (var, store_bound(var, err_var, 0))}
    corr = M / (M - (1 + eps)) if corrected else 1.0
    for name, old, new, e_new in (("mmean", d64(mmean), mean, err_mean), ("mvar", d64(mvar), var * corr, err_var * corr)):
        a, b = old * mom, new * (1 - mom)
        e_new = store_bound(new, e_new + 2.0 ** -52 * new.abs(), 0)             # the batch value itself is rounded to fp32
        out[name] = (a + b, store_bound(a + b, U32 * (2 * a.abs() + 3 * b.abs()) + (1 - mom) * e_new, 0))
    return out


def bn_apply64(z, mean, var, gamma, beta, eps, res, relu, dt, scale_channel=None):
    """y = relu?(gamma (z - mean) rstd + beta + res) with the mean / var the device holds (fp32 values) -> (y, bound).
    s = gamma rsqrt(var + eps): 4 roundings (addition, rsqrt 1 ulp = 2, product); z - mean 1; product 1; + beta 1; + res 1:
    U (8 |(z - mean) s| + 2 |beta| + |res|), + half an ulp of `dt`."""
    z = d64(z)
    s = d64(gamma) * torch.rsqrt(d64(var) + f32v(eps))
    t = (z - d64(mean)) * s
    y = t + d64(beta)
    err = U32 * (8 * t.abs() + 2 * d64(beta).abs())
    if res is not None:
        y = y + d64(res)
        err = err + U32 * d64(res).abs()
    if relu:
        y = y.clamp_min(0)
    return y, store_bound(y, err, dt)


def bn_backward64(g, z, mean, var, gamma, eps, dt, dbeta=None, dgamma=None):
    """dbeta = sum g; dgamma = sum g xhat, xhat = (z - mean) rstd; dz = gamma rstd (g - dbeta / M - xhat dgamma / M), with the
    device's mean / var and -- for dz -- the device's dbeta / dgamma when given.  -> dict name -> (reference, bound).
    dbeta: float64 sums, rounded once.  dgamma: each term g xhat in fp32: difference 1, rstd 3, product 1, product 1 = 6 U on
    sum|g xhat|, rounded once.  dz on gamma rstd (|g| + |dbeta / M| + |xhat dgamma / M|): k = gamma rstd 4 + its product 1;
    dbeta / M 2 (1 / M, product); xhat 5, dgamma 1, 1 / M 2; two differences 2  ->  14 U, + half an ulp of `dt`."""
    g, z = d64(g), d64(z)
    M = z.shape[0]
    rstd = torch.rsqrt(d64(var) + f32v(eps))
    xh = (z - d64(mean)) * rstd
    db, dg = g.sum(0), (g * xh).sum(0)
    D = M * 2.0 ** -53
    out = {"dbeta": (db, store_bound(db, D * g.abs().sum(0), 0)),
           "dgamma": (dg, store_bound(dg, (6 * U32 + D) * (g * xh).abs().sum(0), 0))}
    db_, dg_ = (d64(dbeta) if dbeta is not None else db), (d64(dgamma) if dgamma is not None else dg)
    k = d64(gamma) * rstd
    dz = k * (g - db_ / M - xh * dg_ / M)
    mag = k.abs() * (g.abs() + (db_ / M).abs() + (xh * dg_ / M).abs())
    out["dz"] = (dz, store_bound(dz, 14 * U32 * mag, dt))
    return out
