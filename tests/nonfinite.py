"""Class parity of non-finite values between a kernel and its float64 reference (tests/test_nonfinite_cpu.py, tests/test_nonfinite_gpu.py).

One operand element is replaced by a poison: a NaN with the sign bit clear, a NaN with the sign bit set, +inf or -inf.  The
DEPENDENCY SET is the set of output elements whose float64 reference changes.  Two premises make the IEEE result unambiguous:
every co-operand the poisoned element is multiplied with is non-zero (premise_nonzero), and the element lies where all its taps
are in bounds (the caller's choice of position).  Then every dependent pre-activation is NaN or sign(co-operand) x inf, whatever
the order of the sum, and no kernel can legitimately differ through 0 x inf.  assert_class_parity checks:

  * on the dependency set the device output has the CLASS (NaN, +inf, -inf, finite) of the reference on the same poisoned
    operands; payload and sign of a NaN are free; where the class is finite the value is exactly 0 (ReLU of -inf, a blocked
    mask element);
  * outside it every stored bit equals the same launch on the clean operands (a sentinel prefill still shows unwritten elements).

The float64 reference is built from plain sums, torch.relu and F.max_pool2d, all of which keep a NaN."""
import torch

NAN, PINF, NINF, FINITE = 0, 1, 2, 3
CLASS_NAMES = ("NaN", "+inf", "-inf", "finite")
POISON_NAMES = ("nan_pos", "nan_neg", "pinf", "ninf")

_INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_BITS = {      # quiet NaN sign clear / sign set, +inf, -inf
    torch.float64: (0x7FF8000000000000, -0x0008000000000000, 0x7FF0000000000000, -0x0010000000000000),
    torch.float32: (0x7FC00000, 0xFFC00000 - (1 << 32), 0x7F800000, 0xFF800000 - (1 << 32)),
    torch.bfloat16: (0x7FC0, 0xFFC0 - (1 << 16), 0x7F80, 0xFF80 - (1 << 16)),
    torch.float16: (0x7E00, 0xFE00 - (1 << 16), 0x7C00, 0xFC00 - (1 << 16)),
}


def poisons(dtype):
    """{name: 0-d tensor of dtype} of the four poisons, built from their bit patterns (so the NaN's sign bit is what the name says)."""
    return {n: torch.tensor([b], dtype=_INT[dtype]).view(dtype)[0] for n, b in zip(POISON_NAMES, _BITS[dtype])}


def sign_bit(t):
    """The sign bit of every element, NaNs included."""
    return t.contiguous().view(_INT[t.dtype]) < 0


def put(t, index, name):
    """A copy of t with t[index] = the poison `name` of t's dtype, written as a bit pattern (no arithmetic touches the NaN's sign)."""
    out = t.detach().clone().contiguous()
    out.view(_INT[t.dtype])[index] = _BITS[t.dtype][POISON_NAMES.index(name)]
    return out


def classes(t):
    """Class of every element: NAN, PINF, NINF or FINITE (int8 tensor of t's shape, on the CPU)."""
    t = t.detach().cpu()
    c = torch.full(t.shape, FINITE, dtype=torch.int8)
    c[torch.isnan(t)] = NAN
    c[torch.isposinf(t)] = PINF
    c[torch.isneginf(t)] = NINF
    return c


def _same(a, b):
    """Elementwise 'the same float64 value' with NaN == NaN."""
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def dependency(ref_clean, ref_poisoned):
    """Boolean mask of the elements whose float64 reference changes when the operand is poisoned."""
    assert ref_clean.dtype == torch.float64 and ref_poisoned.dtype == torch.float64
    assert bool(torch.isfinite(ref_clean).all()), "the clean reference must be finite"
    return ~_same(ref_clean, ref_poisoned)


def premise_nonzero(co_operands, what="co-operands"):
    """Premise 1: everything the poisoned element is multiplied with is non-zero (0 x inf = NaN would make the class depend on the kernel)."""
    co = co_operands.detach().cpu()
    assert co.numel() > 0, "%s: no co-operand" % what
    assert bool(torch.isfinite(co.double()).all()), "%s: a co-operand is not finite" % what
    n = int((co == 0).sum())
    assert n == 0, "%s: %d of %d co-operands are zero; the class of 0 x inf is not pinned" % (what, n, co.numel())


def assert_disjoint(deps, what="poisons"):
    """Several poisons in one launch: their dependency sets must not meet."""
    total = torch.zeros_like(deps[0], dtype=torch.int32)
    for d in deps:
        total += d.to(torch.int32)
    assert int(total.max()) <= 1, "%s: dependency sets overlap at %d elements" % (what, int((total > 1).sum()))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT[t.dtype])


def assert_class_parity(got, got_clean, ref_poisoned, dep, what="output"):
    """The contract of this module's docstring.  got, got_clean: the launch on the poisoned / clean operands (same dtype and shape);
    ref_poisoned: the float64 reference, rounded to nothing (its class is what counts); dep: dependency(...)."""
    got, got_clean, ref = got.detach().cpu(), got_clean.detach().cpu(), ref_poisoned.detach().cpu()
    assert got.shape == ref.shape == got_clean.shape == dep.shape, (what, got.shape, got_clean.shape, ref.shape, dep.shape)
    assert int(dep.sum()) > 0, "%s: the poison reaches no output element (vacuous)" % what
    assert bool((classes(ref)[dep] != FINITE).any()), "%s: no dependent element of the reference is non-finite (vacuous)" % what
    cg, cr = classes(got), classes(ref)
    bad = dep & (cg != cr)
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        lines = ["  %s: got %r (%s), reference %s" % (tuple(i), float(got[tuple(i)]), CLASS_NAMES[int(cg[tuple(i)])], CLASS_NAMES[int(cr[tuple(i)])])
                 for i in idx]
        raise AssertionError("%s: %d of %d dependent elements have another class than the float64 reference\n%s"
                             % (what, int(bad.sum()), int(dep.sum()), "\n".join(lines)))
    fin = dep & (cr == FINITE)
    if bool(fin.any()):
        # a dependent element that stays finite is a ReLU of -inf or a blocked mask element: exactly zero
        assert bool((ref[fin] == 0).all()), "%s: a finite dependent reference element is not 0; premises violated" % what
        nz = fin & (got.double() != 0)
        assert not bool(nz.any()), "%s: %d dependent elements whose reference is 0 hold %r ..." % (what, int(nz.sum()), float(got[nz][0]))
    out = ~dep
    diff = out & (_bits(got) != _bits(got_clean))
    if bool(diff.any()):
        i = tuple(diff.nonzero()[0].tolist())
        raise AssertionError("%s: %d elements outside the dependency set differ from the clean launch; first %s: %r, clean %r"
                             % (what, int(diff.sum()), i, float(got[i]), float(got_clean[i])))


def assert_store_overflow(got, pre64, dtype, what="output"):
    """Store overflow: where |pre64| rounds past the largest finite value of dtype, the stored value is the infinity torch's cast
    gives, never the saturated maximum.  Asserts that the case holds such elements."""
    want = pre64.to(dtype)
    over = torch.isinf(want) & torch.isfinite(pre64)
    assert int(over.sum()) > 0, "%s: no pre-activation overflows %s (vacuous)" % (what, dtype)
    assert bool((pre64[over].abs() > torch.finfo(dtype).max).all())
    got = got.detach().cpu()
    bad = over & (classes(got) != classes(want))
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d overflowing elements are not stored as the infinity of the cast; first %s: %r for %r"
                             % (what, int(bad.sum()), int(over.sum()), i, float(got[i]), float(pre64[i])))
