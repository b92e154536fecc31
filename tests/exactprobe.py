"""Exact-integer and rounded-once probes of the conv kernels (plain helpers, imported like tests/util.py).

Two ways to compare a kernel with a float64 reference of the same operation, both far tighter than a normwise gate:

* exact: integer operands small enough that every product and every fp32 partial sum is exact (|partial| < 2^24) and
  every stored value is representable in the storage type (premise() proves both).  A correct kernel then equals the
  reference bit for bit whatever its summation order, so one wrong element, tap, channel or store is a failure.
* rounded once: real operands already rounded to the storage type.  A correct kernel accumulates in fp32 and rounds
  each stored output once (after its fused epilogue), so every element lies within half an ulp of the exact value plus
  the fp32 accumulation error (assert_rounded_once).  A truncating store, a double rounding or 16-bit partial sums
  break that bound (tests/test_exactprobe_cpu.py shows it on simulated kernels).

int_operands() / int_plan() make the integer data; ran() asserts which kernel a call actually launched.
"""
import contextlib
import math

import numpy as np
import torch

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
