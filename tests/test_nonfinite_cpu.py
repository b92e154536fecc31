"""The class-parity checker of tests/nonfinite.py is not vacuous: on a small float64 conv + bias + ReLU (and a max-pool) in torch it
accepts torch.relu / F.max_pool2d and rejects six wrong epilogues, each the shape of a real kernel bug."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite as NF

B, H, W, C, N = 2, 9, 10, 3, 4
POS = (1, 4, 5, 1)                 # interior: all 3x3 taps of the poisoned input element are in bounds


def _operands(dtype=torch.float64):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, C, N, generator=g, dtype=torch.float64)
    w[w == 0] = 0.5
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    return x, w, bias


def _pre(x, w, bias):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1) + bias


def _relu(y):
    return torch.relu(y)


def _fmax(y):                      # (a) C's fmaxf(y, 0): a NaN is dropped
    return torch.fmax(y, torch.zeros_like(y))


def _nan_to_inf(y):                # (b)
    return torch.relu(torch.where(torch.isnan(y), torch.full_like(y, float("inf")), y))


def _smear(y):                     # (c) the poison spreads over the 4 x 4 tile it lies in
    out = torch.relu(y).clone()
    bad = ~torch.isfinite(y)
    for b, oy, ox, n in bad.nonzero().tolist():
        if not bool(torch.isfinite(out[b, oy, ox, n])):
            tile = out[b, oy & ~3:(oy & ~3) + 4, ox & ~3:(ox & ~3) + 4, n]
            tile[torch.isfinite(y[b, oy & ~3:(oy & ~3) + 4, ox & ~3:(ox & ~3) + 4, n])] = out[b, oy, ox, n]      # the independent ones
    return out


def _pool(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, padding=1).permute(0, 2, 3, 1)


def _pool_skip_nan(x):             # (e) `if (v > best)`: a NaN never wins
    return _pool(torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x))


def _pool_keep_positive_nan(x):    # (f) integer keys: only a NaN with the sign bit clear is the largest key
    neg_nan = torch.isnan(x) & NF.sign_bit(x)
    return _pool(torch.where(neg_nan, torch.full_like(x, -float("inf")), x))


def _check_epilogue(epi, name):
    x, w, bias = _operands()
    NF.premise_nonzero(w[:, :, POS[3], :], "filter taps of the poisoned channel")
    clean = _pre(x, w, bias)
    xp = NF.put(x, POS, name)
    dep = NF.dependency(torch.relu(clean), torch.relu(_pre(xp, w, bias)))
    assert int(dep.sum()) > 0
    NF.assert_class_parity(epi(_pre(xp, w, bias)), epi(clean), torch.relu(_pre(xp, w, bias)), dep, name)


@pytest.mark.parametrize("name", NF.POISON_NAMES)
def test_relu_is_accepted(name):
    _check_epilogue(_relu, name)


def test_poisons_are_what_they_say():
    for dtype in (torch.float64, torch.float32, torch.bfloat16, torch.float16):
        p = NF.poisons(dtype)
        assert list(p) == list(NF.POISON_NAMES)
        vals = torch.stack([p[n] for n in NF.POISON_NAMES])
        assert NF.classes(vals).tolist() == [NF.NAN, NF.NAN, NF.PINF, NF.NINF]
        assert NF.sign_bit(vals).tolist() == [False, True, False, True]
        t = NF.put(torch.zeros(3, dtype=dtype), 1, "nan_neg")
        assert bool(torch.isnan(t[1])) and bool(NF.sign_bit(t)[1]) and float(t[0]) == 0 and float(t[2]) == 0


@pytest.mark.parametrize("name", ["nan_pos", "nan_neg"])
def test_fmax_is_rejected(name):
    with pytest.raises(AssertionError, match="another class"):
        _check_epilogue(_fmax, name)


@pytest.mark.parametrize("name", ["nan_pos", "nan_neg"])
def test_nan_turned_into_inf_is_rejected(name):
    with pytest.raises(AssertionError, match="another class"):
        _check_epilogue(_nan_to_inf, name)


@pytest.mark.parametrize("name", NF.POISON_NAMES)
def test_smear_over_a_tile_is_rejected(name):
    with pytest.raises(AssertionError, match="outside the dependency set"):
        _check_epilogue(_smear, name)


def test_saturating_cast_is_rejected():
    x, w, bias = _operands()
    pre = _pre(x, w, bias) * 65504.0                                   # some |pre| > 65504: the fp16 store overflows
    NF.assert_store_overflow(torch.relu(pre).to(torch.float16), torch.relu(pre), torch.float16, "torch cast")
    sat = torch.relu(pre).clamp(max=65504.0).to(torch.float16)         # (d)
    with pytest.raises(AssertionError, match="not stored as the infinity"):
        NF.assert_store_overflow(sat, torch.relu(pre), torch.float16, "saturating cast")
    with pytest.raises(AssertionError, match="vacuous"):
        NF.assert_store_overflow(torch.relu(pre * 1e-6).to(torch.float16), torch.relu(pre * 1e-6), torch.float16, "no overflow")


def _check_pool(pool, name):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 8, 8, C, generator=g, dtype=torch.float64).abs()
    x[1, 3, 3, 1] = 50.0                                               # larger finite values and +inf share the NaN's windows
    x[1, 4, 5, 1] = float("inf")
    clean_in = x.clone(); clean_in[1, 4, 5, 1] = 60.0
    xp = NF.put(x, (1, 4, 4, 1), name)
    ref = _pool(xp)
    dep = NF.dependency(_pool(clean_in), ref)
    NF.assert_class_parity(pool(xp), pool(clean_in), ref, dep, name)


@pytest.mark.parametrize("name", ["nan_pos", "nan_neg"])
def test_max_pool_is_accepted(name):
    _check_pool(_pool, name)


@pytest.mark.parametrize("name", ["nan_pos", "nan_neg"])
def test_pool_that_skips_nan_is_rejected(name):
    with pytest.raises(AssertionError, match="another class"):
        _check_pool(_pool_skip_nan, name)


def test_pool_that_keeps_only_a_positive_nan_is_rejected():
    _check_pool(_pool_keep_positive_nan, "nan_pos")                    # this half it gets right ...
    with pytest.raises(AssertionError, match="another class"):
        _check_pool(_pool_keep_positive_nan, "nan_neg")                # ... and this one it loses


def test_vacuous_cases_are_refused():
    x, w, bias = _operands()
    clean = torch.relu(_pre(x, w, bias))
    with pytest.raises(AssertionError, match="vacuous"):
        NF.assert_class_parity(clean, clean, clean, torch.zeros_like(clean, dtype=torch.bool), "nothing poisoned")
    w0 = w.clone(); w0[1, 1, POS[3], 2] = 0
    with pytest.raises(AssertionError, match="are zero"):
        NF.premise_nonzero(w0[:, :, POS[3], :], "a zero tap")
    d = torch.zeros(4, dtype=torch.bool); d[1] = True
    e = torch.zeros(4, dtype=torch.bool); e[1:3] = True
    with pytest.raises(AssertionError, match="overlap"):
        NF.assert_disjoint([d, e])
    NF.assert_disjoint([d, ~e])
