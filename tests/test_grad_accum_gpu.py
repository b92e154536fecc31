"""Gradient accumulation on the GPU (Config.GRAD_ACCUM_STEPS).

Kernel level: urso_grad_accum (copy, add) and urso_grad_accum_close bit for bit against ursonet_amd.grad_accum.first32 / add32 / close32 in
guarded buffers (every ragged-tail case of a 16-byte access, one block, many blocks, the grid-stride loop, buffers off the 16-byte
boundary), and the close launch's slots against a float64 sum over each block's documented element set.
Engine level (resnet18, 64 x 64, batch 2: 11.3 M parameters, so the step's own launches walk their grid-stride loop): the plan is the
parent's with the key at 1, the gradient in front of the optimizer is the written recurrence of the micro-batches' gradients and the
update is the one a reference engine makes of it, nothing moves before the close, graph replay equals the eager step, a poisoned
micro-step under loss scaling costs exactly one optimizer step, the weights' average counts optimizer steps, batch-statistics BN advances
per micro-batch, the refusals, and UrsoNet.train() draws k batches per optimizer step.

NaN results: IEEE 754 leaves the payload and sign of a NaN result to the implementation, so the add and the close are compared bit for bit
wherever the emulation's result is not a NaN, and NaN for NaN where it is.  The copy moves integers: every bit, NaN payloads included."""
import os
import re

import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats in front of and behind every buffer under test (256 bytes: the buffer itself stays 16-byte aligned)
GUARD_BITS = 0x7FA5A5A5          # a NaN with a payload: an arithmetic pass over it would show, and so would a copy
# the ragged tail on each side of a 16-byte access, one block, more than one block; + one size past 4096 blocks x 256 threads x 4 elements,
# the only one at which the grid-stride loop takes a second turn
SIZES = [1, 3, 4, 5, 255, 256, 257, 4096 + 1, 2 ** 20 + 3, 2 ** 22 + 2 ** 12 + 1]
T, MAX_BLOCKS = 256, 4096        # the documented grid (include/ursonet_ext.h)
U = 2.0 ** -24


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _GA():
    from ursonet_amd import grad_accum
    return grad_accum


def _values(n, seed, finite=False):
    """Normal-range random fp32 values over twelve decades, with +inf, -inf and NaNs (two payloads) sprinkled in where n allows."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32)
    x[np.abs(x) < 1e-30] = 1.0
    if n >= 255 and not finite:
        k = rng.choice(n, size=8, replace=False)
        x[k[0]], x[k[1]], x[k[2]] = np.inf, -np.inf, np.nan
        x.view(np.int32)[k[3]] = 0x7FC12345
        x.view(np.int32)[k[4]] = np.int32(-4194305)          # 0xFFBFFFFF: a negative signalling NaN
    return x


def _guarded(values, shift=0):
    """(whole device buffer, the view under test): GUARD words, `shift` more, the values, GUARD words.  shift moves the view off the
    16-byte boundary by 4 x shift bytes."""
    n = values.size
    whole = torch.full((GUARD + shift + n + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    view = whole[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.from_numpy(values.view(np.int32)))
    return whole, view.view(torch.float32)


def _guards_intact(whole, n, shift=0):
    g = whole.cpu().numpy()
    return bool((g[:GUARD + shift] == GUARD_BITS).all() and (g[GUARD + shift + n:] == GUARD_BITS).all())


def _put(view, values):
    """Every bit of `values` into the fp32 view, NaN payloads included (they move as 32-bit integers)."""
    view.view(torch.int32).copy_(torch.from_numpy(values.view(np.int32)))


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _assert_bits(got, want, what):
    """got: fp32 device tensor; want: the emulation's float32 array.  Bit for bit off the NaNs, NaN for NaN on them."""
    got = got.detach().cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs in other places"
    bad = got.view(np.int32)[~nan] != want.view(np.int32)[~nan]
    assert not bad.any(), "%s: %d of %d elements differ from the emulation" % (what, int(bad.sum()), got.size)


def _copy_add_close(n, shifts, seed):
    """The three launches in guarded buffers at one size and placement: the copy over an accumulator full of other values, the add, and the
    close at c = 1/2, 1/3, 1/8, each from the same accumulator."""
    hip, GA = _hip(), _GA()
    g1, g2, g3, junk = (_values(n, seed + j) for j in range(4))
    what = "n = %d shifts %s" % (n, shifts)
    ag, av = _guarded(junk, shifts[1])
    gg, gv = _guarded(g1, shifts[0])
    assert gv.data_ptr() % 16 == 4 * shifts[0] and av.data_ptr() % 16 == 4 * shifts[1]
    hip.grad_accum(n, gv, av, True)
    torch.cuda.synchronize()
    acc = GA.first32(g1)
    assert np.array_equal(_bits(av), acc.view(np.int32)), what + ": the copy moves every bit"
    assert np.array_equal(_bits(gv), g1.view(np.int32)) and _guards_intact(ag, n, shifts[1]) and _guards_intact(gg, n, shifts[0])
    _put(gv, g2)
    hip.grad_accum(n, gv, av, False)
    torch.cuda.synchronize()
    acc = GA.add32(acc, g2)
    _assert_bits(av, acc, what + ", add")
    assert np.array_equal(_bits(gv), g2.view(np.int32)) and _guards_intact(ag, n, shifts[1]) and _guards_intact(gg, n, shifts[0])
    acc_bits = _bits(av).copy()
    acc_dev = av.cpu().numpy()                                               # (the device's NaNs, where there are any: close32 sees what the launch sees)
    parts = hip.grad_accum_parts(n)
    for k in (2, 3, 8):
        c = GA.inv32(k)
        _put(gv, g3)
        sg, sv = _guarded(np.full(parts, -1.0, np.float32))
        hip.grad_accum_close(n, gv, av, c, sv)
        torch.cuda.synchronize()
        _assert_bits(gv, GA.close32(acc_dev, g3, c), what + ", close at 1/%d" % k)
        assert np.array_equal(_bits(av), acc_bits), what + ": the close only reads acc"
        assert _guards_intact(ag, n, shifts[1]) and _guards_intact(gg, n, shifts[0]) and _guards_intact(sg, parts)
        assert not bool((sv == -1.0).any()), what + ": every slot is written"


# ===================================================================================================================== kernel level
@pytest.mark.parametrize("n", SIZES)
def test_copy_add_and_close_bit_for_bit(n):
    _copy_add_close(n, (0, 0), 1000 + n)


@pytest.mark.parametrize("n", [1, 3, 5, 257, 4096 + 1])
@pytest.mark.parametrize("shifts", [(1, 1), (3, 3), (2, 0), (0, 1)])
def test_buffers_off_the_16_byte_boundary(n, shifts):
    """4-byte alignment is all the entry points ask for: both buffers off the boundary alike (a scalar head, then vectors) and differently
    (scalars alone) give the same bits and leave the guards alone."""
    _copy_add_close(n, shifts, 2000 + n)


def _block_layout(n, addr_g, addr_a):
    """(block of every element, terms of the busiest thread per block) from the documented grid shape (include/ursonet_ext.h)."""
    B = min(MAX_BLOCKS, -(-(-(-n // 4)) // T))
    if addr_g % 16 == addr_a % 16:
        head = min(n, ((16 - addr_g % 16) % 16) // 4)
        nvec = (n - head) // 4
    else:
        head, nvec = n, 0
    tail0 = head + 4 * nvec
    thread = np.empty(n, dtype=np.int64)
    thread[head:tail0] = np.repeat(np.arange(nvec, dtype=np.int64) % (B * T), 4)
    scalars = np.concatenate([np.arange(head), np.arange(tail0, n)])
    thread[scalars] = np.arange(scalars.size, dtype=np.int64) % (B * T)
    per_thread = np.bincount(thread, minlength=B * T)
    return B, thread // T, per_thread.reshape(B, T).max(axis=1)


@pytest.mark.parametrize("n,shifts", [(1, (0, 0)), (5, (0, 0)), (257, (0, 0)), (4096 + 1, (0, 0)), (4096 + 1, (3, 3)), (4096 + 1, (2, 0)),
                                      (2 ** 20 + 3, (0, 0)), (2 ** 22 + 2 ** 12 + 1, (0, 0)), (2 ** 22 + 2 ** 12 + 1, (1, 1))])
def test_the_slots_are_each_blocks_sum_of_squares(n, shifts):
    """On finite inputs sqpart[b] is the sum of the squares of what block b stored.  The bound is counted from the kernel's operation order: a
    term's square is rounded once, then it passes through at most terms - 1 adds of its thread's running sum, the 6 levels of the wave's
    shuffle and at most 3 adds of the 4 wave partials (the first add of each chain, to 0, is exact): at most m = terms + 6 + 4 roundings,
    all terms non-negative, so |slot - exact| <= gamma_m * exact with gamma_m = m u / (1 - m u), u = 2^-24 (+ one quantum per term for
    squares that underflow).  urso_sqnorm_final adds ceil(B / 256) slots per thread, 6 shuffle levels and 4 partials on top."""
    hip, GA = _hip(), _GA()
    acc, g = _values(n, 31 + n, finite=True), _values(n, 32 + n, finite=True)
    ag, av = _guarded(acc, shifts[1])
    gg, gv = _guarded(g, shifts[0])
    B, block, terms = _block_layout(n, gv.data_ptr(), av.data_ptr())
    assert B == hip.grad_accum_parts(n)
    sg, sv = _guarded(np.full(B, -1.0, np.float32))
    c = GA.inv32(3)
    hip.grad_accum_close(n, gv, av, c, sv)
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    hip.sqnorm_final(sv, out)
    torch.cuda.synchronize()
    stored = gv.cpu().numpy()
    assert np.array_equal(stored.view(np.int32), GA.close32(acc, g, c).view(np.int32)) and np.isfinite(stored).all()
    exact = np.bincount(block, weights=stored.astype(np.float64) ** 2, minlength=B)
    count = np.bincount(block, minlength=B)
    m = terms + 6 + 4
    tol = m * U / (1.0 - m * U) * exact + count * 2.0 ** -149
    got = sv.cpu().numpy().astype(np.float64)
    worst = float(np.max(np.abs(got - exact) / np.maximum(tol, 1e-300)))
    print("n = %d shifts %s: %d blocks, up to %d terms per thread, worst slot error / bound %.3f" % (n, shifts, B, int(terms.max()), worst))
    assert (np.abs(got - exact) <= tol).all()
    assert (exact[count == 0] == 0).all() and (got[count == 0] == 0).all()
    m2 = int(m.max()) + (-(-B // T)) + 6 + 4
    total = float(exact.sum())
    err = abs(float(out[0]) - total)
    print("    total: error / bound %.3f" % (err / (m2 * U / (1.0 - m2 * U) * total)))
    assert err <= m2 * U / (1.0 - m2 * U) * total + n * 2.0 ** -149
    assert _guards_intact(sg, B) and _guards_intact(ag, n, shifts[1]) and _guards_intact(gg, n, shifts[0])
    # a non-finite input makes the total non-finite
    if n >= 257:
        for bad in (np.inf, np.nan):
            _put(gv, g)
            gv[n // 2] = bad
            hip.grad_accum_close(n, gv, av, c, sv)
            hip.sqnorm_final(sv, out)
            torch.cuda.synchronize()
            assert not np.isfinite(float(out[0])), bad
            assert int((~torch.isfinite(sv)).sum()) == 1                     # and only the slot of the block that stored it


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
STATE = ("flat_w", "flat_v", "flat_g", "loss_buf", "flat_stats")


def _engine(k=None, dtype="float32", optimizer="SGD", seed=3, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM)
    cfg.OPTIMIZER = optimizer
    if k is not None:
        cfg.GRAD_ACCUM_STEPS = k
    for key, v in cfgkw.items():
        setattr(cfg, key, v)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(seed):
    if seed not in _batches:
        img, loc, ori, _ = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)
        _batches[seed] = (img, loc, ori)
    return _batches[seed]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _steps(eng, k, first=11, eager=False):
    for s in range(k):
        eng.load_batch(*_batch(first + s))
        eng.step_eager() if eager else eng.step()
    torch.cuda.synchronize()


def _gradients(ref, seeds):
    """g_j of the batches `seeds` at the reference engine's weights, without ever running its optimizer."""
    out = []
    for s in seeds:
        ref.load_batch(*_batch(s))
        ref.run_prep(); ref.run_forward(); ref.run_backward()
        torch.cuda.synchronize()
        out.append(ref.flat_g.cpu().numpy().copy())
    return out


def test_default_plan_is_the_parents_and_the_key_adds_two_launches(monkeypatch):
    unset, cfg0 = _engine(None)
    one, _ = _engine(1)
    assert "GRAD_ACCUM_STEPS" not in vars(cfg0)
    assert unset.labels == one.labels and "accum" not in one.labels and one.labels["opt"] == ["sqnorm", "sgd"]
    for eng in (unset, one):
        assert eng.flat_acc is None and eng.grad_accum() is None and eng.accum_ops == []
    _steps(unset, 5)
    _steps(one, 5)
    assert float(one.flat_g.abs().max()) > 0 and bool(torch.isfinite(one.flat_w).all())
    for name in STATE:
        assert _same(getattr(unset, name), getattr(one, name)), name
    monkeypatch.setenv("URSO_WGRAD_STREAM", "2")                             # the forked capture is not supported under accumulation
    on, _ = _engine(3)
    assert on.labels["accum"] == ["grad_accum"] and on.labels["opt"] == ["grad_close", "sqnorm", "sgd"]
    assert {p: l for p, l in on.labels.items() if p in ("prep", "fwd", "loss")} == {p: l for p, l in one.labels.items() if p in ("prep", "fwd", "loss")}
    assert on.forked is False and on.wgrad_stream is None and not on.fused_sqnorm
    assert on.flat_acc is not None and on.flat_acc.shape == on.flat_w.shape and on.grad_accum() == {"steps": 3, "micro": 0}
    assert on.sqpart.numel() == _hip().grad_accum_parts(on.n_flat) == 4096   # 11.3 M parameters: the grid-stride loop
    _steps(on, 3)
    assert on.forked is False and on.grad_accum() == {"steps": 3, "micro": 0}
    monkeypatch.delenv("URSO_WGRAD_STREAM")
    every, _ = _engine(2, dtype="float16", optimizer="ADAM", LOSS_SCALE=1024.0, WEIGHT_EMA=0.9)
    assert every.labels["opt"] == ["grad_close", "sqnorm", "adam", "loss_scale", "ema"] and every.labels["accum"] == ["grad_accum"]
    from ursonet_amd.engine import Engine
    _, cfg = _engine(None)
    cfg.GRAD_ACCUM_STEPS = "nonsense"
    inf = Engine(cfg, "inference", seed=3)
    assert inf.flat_acc is None and inf.grad_accum() is None                 # inference ignores the key


@pytest.mark.parametrize("variant", ["SGD", "ADAM", "SGD+loss_weights"])
def test_the_accumulated_gradient_is_the_recurrence(variant, monkeypatch):
    """flat_g in front of the optimizer of the closing micro-step = close32(add32(first32(g_1), g_2), g_3, inv32(3)) of the gradients a
    reference engine (same seed, k = 1, the plan without the fused norm) computes for the same batches at the same weights, and the update
    is the one that engine's optimizer makes of that gradient.
    GRADIENT_CLIP_NORM: the clip factor is a function of the norm, which the two engines sum in different orders (4096 slots of the close
    launch here, 1024 partials of urso_sqnorm there), so the two updates are the same bits exactly where the clip is idle; the threshold is
    set out of reach, and the two norms are compared within the summation bound of the slots test."""
    GA = _GA()
    optimizer = variant.split("+")[0]
    kw = dict(optimizer=optimizer, GRADIENT_CLIP_NORM=1e9)
    if "+" in variant:
        kw["LEARNABLE_LOSS_WEIGHTS"] = True
    monkeypatch.setenv("URSO_FUSE_SQNORM", "0")
    ref, _ = _engine(1, **kw)
    monkeypatch.delenv("URSO_FUSE_SQNORM")
    eng, _ = _engine(3, **kw)
    assert not ref.fused_sqnorm and _same(ref.flat_w, eng.flat_w)
    w0 = eng.flat_w.clone()
    gs = _gradients(ref, (11, 12, 13))
    assert not np.array_equal(gs[0], gs[1]) and np.isfinite(gs[0]).all() and float(np.abs(gs[2]).max()) > 0
    want = GA.close32(GA.add32(GA.first32(gs[0]), gs[1]), gs[2], GA.inv32(3))
    assert np.array_equal(want.view(np.int32), GA.accumulate32(gs).view(np.int32))
    _steps(eng, 3)
    assert np.array_equal(_bits(eng.flat_g), want.view(np.int32))
    if "+" in variant:
        from ursonet_amd import loss_weights
        o = eng.slices[(loss_weights.LAYER, "ori_weight")][0]
        assert want[o] != 0 and want[o + 4] != 0                             # the two slots are part of it
    ref.flat_g.copy_(torch.from_numpy(want))
    ref.run_optimizer()
    torch.cuda.synchronize()
    assert _same(eng.flat_w, ref.flat_w) and _same(eng.flat_v, ref.flat_v)
    assert not _same(eng.flat_w, w0)                                         # (the step was performed)
    total = float(np.sum(want.astype(np.float64) ** 2))
    m = 12 + 6 + 4 + 16 + 6 + 4                                              # 11.3 M / 2^20 threads: up to 12 terms; 4096 / 256 = 16 slots per thread
    assert abs(float(eng.normsq[0]) - total) <= m * U / (1.0 - m * U) * total
    if optimizer == "ADAM":
        assert float(eng.hyper[5]) == 1.0 and float(ref.hyper[5]) == 1.0 and _same(eng.flat_v2, ref.flat_v2) and _same(eng.flat_vhat, ref.flat_vhat)


def test_nothing_moves_before_the_close():
    eng, _ = _engine(3, dtype="float16", optimizer="ADAM", LOSS_SCALE=1.0, WEIGHT_EMA=0.9)
    names = ("flat_w", "flat_v", "flat_v2", "flat_vhat", "hyper", "ema_state", "flat_ema", "ls_state")
    before = {nm: getattr(eng, nm).clone() for nm in names}
    assert eng.grad_accum() == {"steps": 3, "micro": 0}
    for micro in (1, 2):
        _steps(eng, 1, first=10 + micro)
        assert eng.grad_accum()["micro"] == micro
        for nm in names:
            assert _same(before[nm], getattr(eng, nm)), (micro, nm)
    _steps(eng, 1, first=13)
    assert eng.grad_accum()["micro"] == 0
    assert float(eng.hyper[5]) == 1.0 and eng.weight_ema()["updates"] == 1 and not eng.loss_scale()["last_step_skipped"]
    for nm in ("flat_w", "flat_v", "flat_v2", "flat_ema"):
        assert not _same(before[nm], getattr(eng, nm)), nm
    # reset_optimizer and a re-plan drop a begun optimizer step
    _steps(eng, 1, first=14)
    assert eng.grad_accum()["micro"] == 1
    eng.reset_optimizer()
    assert eng.grad_accum()["micro"] == 0
    _steps(eng, 2, first=15)
    from ursonet_amd.graph import layer_regex
    eng.set_trainable(layer_regex("heads"))
    assert eng.grad_accum() == {"steps": 3, "micro": 0} and eng._graphs is None and eng.labels["opt"][0] == "grad_close"


@pytest.mark.parametrize("k", [2, 3])
def test_graph_replay_equals_the_eager_step(k):
    a, _ = _engine(k)
    b, _ = _engine(k)
    a.load_batch(*_batch(11))
    for role in _GA().roles(k):                                              # the warm-up step of every capture is undone, the index too
        a.capture(role)
        torch.cuda.synchronize()
        assert a.grad_accum()["micro"] == 0 and _same(a.flat_w, b.flat_w) and _same(a.flat_v, b.flat_v) and _same(a.flat_acc, b.flat_acc)
    a._graphs = None
    _steps(a, 2 * k)
    _steps(b, 2 * k, eager=True)
    assert sorted(a._graphs) == sorted(set(_GA().roles(k))) and b._graphs is None
    for name in STATE + ("flat_acc", "normsq"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert a.grad_accum() == b.grad_accum() == {"steps": k, "micro": 0}
    one, _ = _engine(1)
    assert not _same(a.flat_w, one.flat_w)


def test_a_poisoned_micro_step_costs_one_optimizer_step(monkeypatch):
    """fp16 under LOSS_SCALE = 1.0 and k = 3.  An inf in flat_acc after micro-step 1 (a numerical overflow: nothing else is provoked) reaches the
    closed gradient and the norm; the optimizer skips, loss scaling counts ONE skipped step, the average does not count it.  The next
    optimizer step begins with a bit copy: its gradient is the recurrence of its own three gradients, with no leftovers."""
    GA = _GA()
    kw = dict(dtype="float16", LOSS_SCALE=1.0, WEIGHT_EMA=0.9)
    eng, _ = _engine(3, **kw)
    w0 = eng.flat_w.clone()
    _steps(eng, 1, first=11)
    o = eng.slices[("loc_final", "kernel")][0]
    eng.flat_acc[o + 1] = float("inf")
    _steps(eng, 2, first=12)
    assert not np.isfinite(float(eng.normsq[0]))
    assert eng.loss_scale()["skipped_total"] == 1 and eng.loss_scale()["last_step_skipped"]
    assert _same(eng.flat_w, w0) and eng.weight_ema()["updates"] == 0 and eng.grad_accum()["micro"] == 0
    monkeypatch.setenv("URSO_FUSE_SQNORM", "0")
    ref, _ = _engine(1, **kw)
    monkeypatch.delenv("URSO_FUSE_SQNORM")
    assert _same(ref.flat_w, w0)
    gs = _gradients(ref, (14, 15, 16))
    _steps(eng, 3, first=14)
    assert np.isfinite(gs[0]).all() and np.array_equal(_bits(eng.flat_g), GA.accumulate32(gs).view(np.int32))
    assert np.isfinite(float(eng.normsq[0])) and bool(torch.isfinite(eng.flat_acc).all())
    assert eng.loss_scale()["skipped_total"] == 1 and not eng.loss_scale()["last_step_skipped"]
    assert not _same(eng.flat_w, w0) and eng.weight_ema()["updates"] == 1


def test_weight_ema_counts_optimizer_steps():
    from ursonet_amd import weight_ema as WE
    eng, cfg = _engine(2, WEIGHT_EMA=0.9)
    state = WE.initial_state(cfg)
    ema = eng.flat_ema.cpu().numpy().copy()
    for s in range(2):
        _steps(eng, 1, first=11 + 2 * s)
        assert eng.weight_ema()["updates"] == s and np.array_equal(_bits(eng.flat_ema), ema.view(np.int32))
        _steps(eng, 1, first=12 + 2 * s)
        ema = WE.update32(ema, eng.flat_w.cpu().numpy(), state[WE.NEXT_DECAY])
        state = WE.next_state(state)
        assert eng.ema_state.tolist() == state and np.array_equal(_bits(eng.flat_ema), ema.view(np.int32))
    assert eng.weight_ema()["updates"] == 2


def test_batch_statistics_bn_advances_per_micro_batch(monkeypatch):
    GA = _GA()
    monkeypatch.setenv("URSO_FUSE_SQNORM", "0")
    ref, _ = _engine(1, TRAIN_BN=None)
    monkeypatch.delenv("URSO_FUSE_SQNORM")
    eng, _ = _engine(3, TRAIN_BN=None)
    assert eng.train_bn and _same(ref.flat_stats, eng.flat_stats)
    s0 = eng.flat_stats.clone()
    gs = _gradients(ref, (11, 12, 13))
    _steps(eng, 3)
    assert _same(eng.flat_stats, ref.flat_stats) and not _same(eng.flat_stats, s0)
    assert np.array_equal(_bits(eng.flat_g), GA.accumulate32(gs).view(np.int32))       # the BN gamma / beta gradients accumulate like the rest


@pytest.mark.parametrize("bad", [True, 2.0, "2", 0, -3])
def test_refusals_at_engine_build(bad):
    with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS"):
        _engine(bad)


def test_train_draws_k_batches_per_optimizer_step(tmp_path, capsys, monkeypatch):
    from ursonet_amd import feeder, net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config(dtype="float32", lr=0.01, **GEOM)
    cfg.NAME = "accum"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 1
    cfg.GRAD_ACCUM_STEPS = 2
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    eng = model._engine
    asked, rows = {}, []
    next_into = feeder.DeviceFeeder.next_into

    def counted(self, *a, **kw):
        asked[id(self)] = asked.get(id(self), 0) + 1
        return next_into(self, *a, **kw)
    monkeypatch.setattr(feeder.DeviceFeeder, "next_into", counted)
    step = eng.step

    def recorded():
        step()
        rows.append(eng.loss_buf.detach().cpu().numpy().copy())
    eng.step = recorded
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all")
    out = capsys.readouterr().out
    assert list(asked.values()) == [4, 1]                                    # the training feeder (asked first), then the validation feeder
    assert "Gradient accumulation: 2 micro-batches x 2 images per optimizer step (effective batch 4)" in out
    assert len(rows) == 4 and len(hist.loc_loss_acc) == 2 and len(hist.ori_loss_acc) == 2
    for i in range(2):
        mean = ((rows[2 * i].astype(np.float64) + rows[2 * i + 1]) / 2).astype(np.float32)
        assert hist.loc_loss_acc[i] == float(mean[0]) and hist.ori_loss_acc[i] == float(mean[1]) and np.isfinite(mean[:2]).all()
    assert rows[0][0] != rows[1][0]
    assert re.search(r"^epoch 1  loc_loss \d+\.\d{5}  val_loc_loss", out, re.M)
    assert eng.grad_accum() == {"steps": 2, "micro": 0}
    ddir, ck = model.find_last()
    assert os.path.basename(ck) in ("weights_accum_0001.npz", "weights_accum_0001.h5") and os.path.exists(ck)
