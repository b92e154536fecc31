"""Stochastic weight averaging and SWAG-diagonal on the GPU (Config.SWA).

Kernel level, through the C ABI: urso_swa_update bit for bit against ursonet_amd.swa.collect32 / next_state in guarded buffers (every
ragged-tail case of a 16-byte access, one block, many blocks, buffers off the 16-byte boundary, with and without the mean of squares,
models 0 -> 1 -> 2 -> 3), the shut gate, the loss-scale skip, twelve steps of the state; urso_swag_sample's normals against the float64
reference, its output bit for bit against sample32 of its own normals, the independence of how a range is cut and aligned, its fixed
points; the refusals.
Engine level (resnet18, 64 x 64, batch 2, the engine of the WEIGHT_EMA tests): the plan, the untouched trajectory, the recurrence over the
weights read after steps p and 2p, graph replay, the detours, frozen layers, accumulation, a skipped fp16 step, checkpoints, train()."""
import os
import re

import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats in front of and behind every buffer under test (256 bytes: the buffer itself stays 16-byte aligned)
GUARD_BITS = 0x7FA5A5A5          # a NaN with a payload: an arithmetic pass over it would show, and so would a copy
SIZES = [1, 3, 4, 5, 255, 256, 257, 4097, 2 ** 20 + 3]
SHIFTS = [(1, 1), (3, 3), (2, 0), (0, 1)]


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _S():
    from ursonet_amd import swa
    return swa


def _values(n, seed):
    """Finite random fp32 values over six decades whose squares stay finite and normal."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)


def _guarded(values, shift=0):
    """(whole device buffer, the view under test): GUARD words, `shift` more, the values, GUARD words."""
    n = values.size
    whole = torch.full((GUARD + shift + n + GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    view = whole[GUARD + shift:GUARD + shift + n]
    view.copy_(torch.from_numpy(values.view(np.int32)))
    return whole, view.view(torch.float32)


def _guards_intact(whole, n, shift=0):
    g = whole.cpu().numpy()
    return bool((g[:GUARD + shift] == GUARD_BITS).all() and (g[GUARD + shift + n:] == GUARD_BITS).all())


def _bits(t):
    if isinstance(t, np.ndarray):
        return t.view(np.int32)
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _state(period=1, start=0, ticks=0, models=0, variance=False):
    return [period, start, ticks, models, 0, 1 if variance else 0, 0, 0]


def _dev_state(s):
    return torch.tensor(s, dtype=torch.int32, device="cuda")


def _fdev(s):
    return torch.tensor(s, dtype=torch.float32, device="cuda")


# ===================================================================================================================== urso_swa_update
def _three_models(n, shifts, with_sq):
    """models 0 -> 1 -> 2 -> 3 at period 1: the copy, then two folds, bit for bit; w only read; guards and state as specified."""
    hip, S = _hip(), _S()
    sw, sm = shifts
    junk = _values(n, 900 + n)                                               # what the buffers hold before the first model: it must not matter
    mg, mv = _guarded(junk, sm)
    qg, qv = _guarded(junk[::-1].copy(), sw) if with_sq else (None, None)
    st = _state(variance=with_sq)
    sd = _dev_state(st)
    mean = sq = None
    for m in (1, 2, 3):
        w = _values(n, 100 * m + n)
        if m > 1:
            w[::3] = mean[::3]                                               # a third of the elements stand still
        wg, wv = _guarded(w, sw)
        assert wv.data_ptr() % 16 == 4 * sw and mv.data_ptr() % 16 == 4 * sm
        hip.swa_update(n, wv, mv, qv, sd)
        torch.cuda.synchronize()
        mean, sq = S.collect32(mean, sq if with_sq else None, w, m) if m > 1 else S.collect32(None, junk if with_sq else None, w, 1)
        st = S.next_state(st)
        what = "n = %d shifts %s model %d" % (n, shifts, m)
        assert np.array_equal(_bits(mv), _bits(mean)), what
        if with_sq:
            assert np.array_equal(_bits(qv), _bits(sq)), what
            assert _guards_intact(qg, n, sw), what
        assert np.array_equal(_bits(wv), _bits(w)) and _guards_intact(wg, n, sw) and _guards_intact(mg, n, sm), what
        assert sd.tolist() == st and st[S.MODELS] == m and st[S.COLLECTED] == 1, what
        if m > 1:                                                            # where w stands still the mean keeps its bits
            assert np.array_equal(_bits(mv)[::3], _bits(w)[::3]), what
    assert np.isfinite(mean).all()


@pytest.mark.parametrize("with_sq", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_update_is_collect32_bit_for_bit(n, with_sq):
    _three_models(n, (0, 0), with_sq)


@pytest.mark.parametrize("with_sq", [False, True])
@pytest.mark.parametrize("shifts", SHIFTS)
@pytest.mark.parametrize("n", [1, 3, 5, 257, 4097])
def test_update_off_the_16_byte_boundary(n, shifts, with_sq):
    _three_models(n, shifts, with_sq)


def test_a_shut_gate_moves_only_ticks_and_collected():
    hip, S = _hip(), _S()
    n = 4097
    m0, q0, w = _values(n, 1), _values(n, 2), _values(n, 3)
    mg, mv = _guarded(m0)
    qg, qv = _guarded(q0)
    st = _state(period=4, start=3, ticks=7, models=1, variance=True)        # the step before was a collection; this one (tick 8) is none
    st[S.COLLECTED] = 1
    sd = _dev_state(st)
    hip.swa_update(n, _fdev(w), mv, qv, sd)
    torch.cuda.synchronize()
    want = S.next_state(st)
    assert sd.tolist() == want and want[S.TICKS] == 8 and want[S.COLLECTED] == 0 and want[S.MODELS] == 1
    assert np.array_equal(_bits(mv), _bits(m0)) and np.array_equal(_bits(qv), _bits(q0)) and _guards_intact(mg, n) and _guards_intact(qg, n)
    # the model cap: the gate of a collecting tick stays shut at 2^24 models
    cap = _state(period=1, models=2 ** 24, variance=True)
    sd = _dev_state(cap)
    hip.swa_update(n, _fdev(w), mv, qv, sd)
    torch.cuda.synchronize()
    assert sd.tolist() == S.next_state(cap) and sd.tolist()[S.MODELS] == 2 ** 24 and sd.tolist()[S.TICKS] == 1
    assert np.array_equal(_bits(mv), _bits(m0)) and np.array_equal(_bits(qv), _bits(q0))
    # saturated ticks stay where they are
    sat = _state(period=5, ticks=2 ** 31 - 1, models=3)
    sd = _dev_state(sat)
    hip.swa_update(n, _fdev(w), mv, None, sd)
    torch.cuda.synchronize()
    assert sd.tolist() == S.next_state(sat) and sd.tolist()[S.TICKS] == 2 ** 31 - 1


def test_a_skipped_loss_scale_step_moves_nothing():
    from ursonet_amd import loss_scale as LS
    hip, S = _hip(), _S()
    n = 4097
    m0, q0, w = _values(n, 4), _values(n, 5), _values(n, 6)
    mg, mv = _guarded(m0)
    qg, qv = _guarded(q0)
    st = _state(period=1, ticks=4, models=4, variance=True)
    st[S.COLLECTED] = 1
    ls = [1024.0, 1.0 / 1024, 0.0, 0.0, 1024.0, 1024.0, 3.0, 1.0]
    assert ls[LS.LAST_SKIPPED] == 1.0
    sd, lsd, wd = _dev_state(st), _fdev(ls), _fdev(w)
    hip.swa_update(n, wd, mv, qv, sd, ls=lsd)
    torch.cuda.synchronize()
    assert sd.tolist() == st == S.next_state(st, skipped=True) and lsd.tolist() == ls
    assert np.array_equal(_bits(mv), _bits(m0)) and np.array_equal(_bits(qv), _bits(q0))
    ls[LS.LAST_SKIPPED] = 0.0
    lsd = _fdev(ls)
    hip.swa_update(n, wd, mv, qv, sd, ls=lsd)
    torch.cuda.synchronize()
    mean, sq = S.collect32(m0, q0, w, 5)
    assert sd.tolist() == S.next_state(st) and lsd.tolist() == ls
    assert np.array_equal(_bits(mv), _bits(mean)) and np.array_equal(_bits(qv), _bits(sq)) and _guards_intact(mg, n) and _guards_intact(qg, n)
    assert not np.array_equal(_bits(mv), _bits(m0))


def test_twelve_steps_follow_the_emulation_field_for_field():
    hip, S = _hip(), _S()
    n = 4097
    st = _state(period=4, start=3, variance=True)
    mg, mv = _guarded(_values(n, 7))
    qg, qv = _guarded(_values(n, 8))
    sd = _dev_state(st)
    mean, sq = _bits(mv).copy().view(np.float32), _bits(qv).copy().view(np.float32)
    collected = []
    for k in range(12):
        w = _values(n, 20 + k)
        st = S.next_state(st)
        if st[S.COLLECTED]:
            mean, sq = S.collect32(mean, sq, w, st[S.MODELS])
            collected.append(k + 1)
        hip.swa_update(n, _fdev(w), mv, qv, sd)
        torch.cuda.synchronize()
        assert sd.tolist() == st, (k, sd.tolist(), st)
        assert np.array_equal(_bits(mv), _bits(mean)) and np.array_equal(_bits(qv), _bits(sq)), "step %d" % (k + 1)
    assert collected == [7, 11] and st[S.TICKS] == 12 and st[S.MODELS] == 2 and _guards_intact(mg, n) and _guards_intact(qg, n)


def test_a_sq_buffer_that_contradicts_the_state_is_refused_on_the_device():
    hip, S = _hip(), _S()
    n = 257
    m0, q0, w = _values(n, 9), _values(n, 10), _values(n, 11)
    _mg, mv = _guarded(m0)
    _qg, qv = _guarded(q0)
    for st, sqbuf in ((_state(variance=True), None), (_state(variance=False), qv)):
        sd = _dev_state(st)
        hip.swa_update(n, _fdev(w), mv, sqbuf, sd)
        torch.cuda.synchronize()
        want = list(st)
        want[S.COLLECTED] = S.REFUSED
        assert sd.tolist() == want and np.array_equal(_bits(mv), _bits(m0)) and np.array_equal(_bits(qv), _bits(q0))
        assert S.as_dict(sd.tolist())["collected"] is False


# ===================================================================================================================== urso_swag_sample
_refs = {}


def _ref_normals(seed, sample):
    """float64 reference normals of the longest buffer, computed once per (seed, sample) and shared"""
    if (seed, sample) not in _refs:
        z = _S().normals64(max(SIZES), seed, sample)
        z.setflags(write=False)
        _refs[(seed, sample)] = z
    return _refs[(seed, sample)]


def _moments(n, seed):
    rng = np.random.default_rng(seed)
    mean = _values(n, seed)
    sq = ((mean * mean).astype(np.float32) * (1.0 + rng.uniform(0.0, 0.5, size=n)).astype(np.float32)).astype(np.float32)
    sq[::5] = ((mean * mean).astype(np.float32) * np.float32(0.999))[::5]    # a fifth has a (slightly) negative difference: sd = 0
    return mean, sq


@pytest.mark.parametrize("seed", [5, 2 ** 32 + 9])
@pytest.mark.parametrize("sample", [0, 1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_sample_normals_and_rule(n, sample, seed):
    hip, S = _hip(), _S()
    mean, sq = _moments(n, 40 + n)
    mg, mv = _guarded(mean)
    qg, qv = _guarded(sq)
    og, ov = _guarded(np.zeros(n, np.float32))
    zg, zv = _guarded(np.zeros(n, np.float32))
    s = S.scale32(0.5)
    hip.swag_sample(n, mv, qv, ov, s, seed, sample, z_out=zv)
    torch.cuda.synchronize()
    z = zv.cpu().numpy()
    ref = _ref_normals(seed, sample)[:n]
    err = np.abs(z.astype(np.float64) - ref)
    tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 2.0 ** -44
    assert np.all(err <= tol), "max excess %g" % float((err - tol).max())
    out = ov.cpu().numpy()
    assert np.array_equal(_bits(out), _bits(S.sample32(mean, sq, z, s)))     # the second half: the device's own z through the written rule
    assert np.array_equal(_bits(out)[::5], _bits(mean)[::5])
    assert n < 255 or not np.array_equal(out, mean)
    assert np.array_equal(_bits(mv), _bits(mean)) and np.array_equal(_bits(qv), _bits(sq))
    assert all(_guards_intact(g, n) for g in (mg, qg, og, zg))
    # without z_out: the same sample
    o2g, o2v = _guarded(np.zeros(n, np.float32))
    hip.swag_sample(n, mv, qv, o2v, s, seed, sample)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(o2v), _bits(out)) and _guards_intact(o2g, n)


@pytest.mark.parametrize("n", SIZES)
def test_sample_depends_on_the_absolute_index_not_on_the_cut_or_the_alignment(n):
    hip, S = _hip(), _S()
    seed, sample, s = 2 ** 32 + 9, 7, S.scale32(0.5)
    mean, sq = _moments(n, 60 + n)
    md, qd = _fdev(mean), _fdev(sq)
    full, zfull = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    hip.swag_sample(n, md, qd, full, s, seed, sample, z_out=zfull)
    # two launches: [0, h) and [h, n), h a multiple of 4 (0 for the smallest sizes: an empty first launch)
    h = (n // 2) // 4 * 4
    og, ov = _guarded(np.zeros(n, np.float32))
    zg, zv = _guarded(np.zeros(n, np.float32))
    hip.swag_sample(h, md, qd, ov, s, seed, sample, z_out=zv)
    hip.swag_sample(n - h, md[h:], qd[h:], ov[h:], s, seed, sample, z_out=zv[h:], first=h)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ov), _bits(full)) and np.array_equal(_bits(zv), _bits(zfull))
    assert _guards_intact(og, n) and _guards_intact(zg, n)
    if n > 4097:
        return
    # buffers off the 16-byte boundary, alike (vectors that take the end of one Philox block and the beginning of the next) and not
    for sm, sq_, so, sz in ((1, 1, 1, 1), (3, 3, 3, 3), (2, 2, 2, 2), (2, 0, 0, 0), (0, 0, 0, 1), (1, 1, 1, None)):
        _mg, mv = _guarded(mean, sm)
        _qg, qv = _guarded(sq, sq_)
        og, ov = _guarded(np.zeros(n, np.float32), so)
        zg, zv = _guarded(np.zeros(n, np.float32), sz) if sz is not None else (None, None)
        hip.swag_sample(n, mv, qv, ov, s, seed, sample, z_out=zv)
        torch.cuda.synchronize()
        what = "n = %d shifts %s" % (n, (sm, sq_, so, sz))
        assert np.array_equal(_bits(ov), _bits(full)) and _guards_intact(og, n, so), what
        if zv is not None:
            assert np.array_equal(_bits(zv), _bits(zfull)) and _guards_intact(zg, n, sz), what


@pytest.mark.parametrize("n", [5, 4097])
def test_sample_fixed_points(n):
    hip, S = _hip(), _S()
    mean, sq = _moments(n, 80 + n)
    md = _fdev(mean)
    out = torch.zeros(n, device="cuda")
    hip.swag_sample(n, md, _fdev((mean * mean).astype(np.float32)), out, S.scale32(0.5), 3, 1)        # sq = fl(mean * mean)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(mean))
    out.zero_()
    hip.swag_sample(n, md, _fdev(sq), out, 0.0, 3, 1)                        # s = 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(mean))
    hip.swag_sample(0, md, _fdev(sq), out, 0.5, 3, 1)                        # n = 0 touches nothing
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(mean))


def test_bad_arguments_are_refused_and_launch_nothing():
    hip = _hip()
    n = 257
    vals = _values(n, 12)
    bufs = [_guarded(vals) for _ in range(4)]
    (_, a), (_, b), (_, c), (_, d) = bufs
    st = _dev_state(_state(variance=True))
    E = hip.UrsoHipError
    for call in (lambda: hip.swa_update(n, a, a, c, st), lambda: hip.swa_update(n, a, b, b, st), lambda: hip.swa_update(n - 4, a, b, a[4:], st),
                 lambda: hip.swag_sample(n, a, b, a, 0.5, 0, 0), lambda: hip.swag_sample(n, a, b, b, 0.5, 0, 0),
                 lambda: hip.swag_sample(n, a, b, c, 0.5, 0, 0, z_out=c), lambda: hip.swag_sample(n, a, b, c, -1.0, 0, 0),
                 lambda: hip.swag_sample(n, a, b, c, float("nan"), 0, 0), lambda: hip.swag_sample(n, a, b, c, float("inf"), 0, 0),
                 lambda: hip.swag_sample(n, a, b, c, 0.5, 0, -1), lambda: hip.swag_sample(n, a, b, c, 0.5, 0, 0, first=2),
                 lambda: hip.swag_sample(n, a, b, c, 0.5, 0, 0, first=-4), lambda: hip.swag_sample(n - 4, a, b, a[4:], 0.5, 0, 0)):
        with pytest.raises(E, match=r"urso_sw\w+ failed \(-1\)"):
            call()
    torch.cuda.synchronize()
    assert st.tolist() == _state(variance=True)
    for whole, view in bufs:
        assert np.array_equal(_bits(view), _bits(vals)) and _guards_intact(whole, n)


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(swa=None, dtype="float32", optimizer="SGD", seed=3, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM)
    cfg.OPTIMIZER = optimizer
    cfg.SWA = swa
    for k, v in cfgkw.items():
        setattr(cfg, k, v)
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


def test_default_plan_is_the_parents_and_the_key_appends_one_launch():
    off, _ = _engine(None)
    assert off.labels["opt"] == ["sqnorm", "sgd"] and off.swa() is None
    assert off.flat_swa is None and off.flat_swa_sq is None and off.swa_state is None and off._swag_hold is None
    assert not any("swa" in l for ls in off.labels.values() for l in ls)
    on, _ = _engine(4, SWA_START=3)
    assert on.labels["opt"] == ["sqnorm", "sgd", "swa"]
    assert {k: v for k, v in on.labels.items() if k != "opt"} == {k: v for k, v in off.labels.items() if k != "opt"}
    assert on.flat_swa is not None and on.flat_swa_sq is None and on.swa_state.dtype == torch.int32
    assert on.swa() == {"period": 4, "start": 3, "ticks": 0, "models": 0, "collected": False, "variance": False}
    var, _ = _engine(4, SWA_VARIANCE=True)
    assert var.flat_swa_sq is not None and var.flat_swa_sq.data_ptr() != var.flat_swa.data_ptr() and var.swa()["variance"]
    every, _ = _engine(2, optimizer="ADAM", LOSS_SCALE=1024.0, WEIGHT_EMA=0.9)
    assert every.labels["opt"] == ["sqnorm", "adam", "loss_scale", "ema", "swa"]       # the last: behind ema, and so behind loss_scale
    sam, _ = _engine(2, SAM=0.05)
    assert sam.labels["opt"].count("swa") == 1 and sam.labels["opt"][-1] == "swa" and not any("swa" in l for l in sam.labels.get("sam", []))
    with pytest.raises(ValueError, match="^SWA must be"):
        _engine(0)
    with pytest.raises(ValueError, match="SWA_RECAL_BATCHES = 1 needs SWA"):
        _engine(None, SWA_RECAL_BATCHES=1, TRAIN_BN=None)
    from ursonet_amd.engine import Engine
    _, cfg = _engine(None)
    cfg.SWA = 2
    inf = Engine(cfg, "inference", seed=3)
    assert inf.flat_swa is None and inf.swa_state is None                    # inference ignores the key


def test_the_feature_does_not_perturb_training():
    a, _ = _engine(None)
    b, _ = _engine(2, SWA_VARIANCE=True)
    _steps(a, 5)
    _steps(b, 5)
    assert float(a.flat_g.abs().max()) > 0 and bool(torch.isfinite(a.flat_w).all())
    for name in ("flat_w", "flat_v", "flat_g", "loss_buf", "flat_stats"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert b.swa()["models"] == 2 and b.swa()["ticks"] == 5 and not _same(b.flat_swa, b.flat_w)


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_the_average_is_the_recurrence_over_the_collected_weights(optimizer):
    """2p + 1 steps at period p = 2: mean and sq are collect32 over the weights read after steps p and 2p; the state is next_state's."""
    S = _S()
    p = 2
    eng, cfg = _engine(p, optimizer=optimizer, SWA_VARIANCE=True)
    state = S.initial_state(cfg)
    assert eng.swa_state.tolist() == state
    read = {}
    for s in range(1, 2 * p + 2):
        _steps(eng, 1, first=10 + s)
        state = S.next_state(state)
        assert eng.swa_state.tolist() == state, s
        read[s] = eng.flat_w.cpu().numpy().copy()
    assert not np.array_equal(read[p], read[2 * p])
    mean, sq = S.collect32(None, np.zeros_like(read[p]), read[p], 1)
    mean, sq = S.collect32(mean, sq, read[2 * p], 2)
    assert state[S.MODELS] == 2 and state[S.TICKS] == 2 * p + 1 and state[S.COLLECTED] == 0
    assert np.array_equal(_bits(eng.flat_swa), _bits(mean)) and np.array_equal(_bits(eng.flat_swa_sq), _bits(sq))
    v = eng.flat_v.clone()
    eng.reset_optimizer()                                                    # the average is no optimizer state: staged training keeps it
    assert float(eng.flat_v.abs().max()) == 0 and float(v.abs().max()) > 0
    assert eng.swa_state.tolist() == state and np.array_equal(_bits(eng.flat_swa), _bits(mean))
    eng.reset_swa()                                                          # by hand
    assert eng.swa_state.tolist() == S.initial_state(cfg)
    _steps(eng, p, first=30)                                                 # the next model is number 1 again: a copy
    assert eng.swa()["models"] == 1 and _same(eng.flat_swa, eng.flat_w)


def test_graph_replay_equals_the_eager_step():
    a, _ = _engine(2, SWA_VARIANCE=True)
    b, _ = _engine(2, SWA_VARIANCE=True)
    a.load_batch(*_batch(11))
    a.capture()
    torch.cuda.synchronize()
    assert a.swa()["ticks"] == 0 and _same(a.flat_w, b.flat_w) and _same(a.flat_swa, b.flat_swa)      # the warm-up step is undone
    _steps(a, 5)
    _steps(b, 5, eager=True)
    for name in ("flat_w", "flat_v", "flat_g", "flat_swa", "flat_swa_sq", "swa_state", "loss_buf"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert a.swa()["models"] == 2


def test_the_detours_leave_no_trace():
    """evaluate() inside swa_weights() = evaluate() of a second engine loaded with get_weights(swa=True); swag_weights() puts
    sample32(mean, sq, normals) into flat_w; after either, also when the body raises, every bit of the training state is back."""
    S = _S()
    a, cfg = _engine(1, WEIGHT_EMA=0.9, SWA_VARIANCE=True)
    c, _ = _engine(1, WEIGHT_EMA=0.9, SWA_VARIANCE=True)
    _steps(a, 3)
    _steps(c, 3)
    names = ("flat_w", "flat_swa", "flat_swa_sq", "flat_ema", "flat_v", "swa_state", "ema_state", "flat_stats")
    before = [getattr(a, nm).clone() for nm in names]
    back = lambda: all(_same(x, getattr(a, nm)) for nm, x in zip(names, before))
    val = _batch(40)
    a.load_batch(*val)
    raw = a.evaluate()
    saved, saved_sq, saved_raw = a.get_weights(swa=True), a.get_weights(swa="sq"), a.get_weights()
    with a.swa_weights() as inside:
        assert inside is a and a.swa_swapped and _same(a.flat_w, before[1]) and _same(a.flat_swa, before[0])
        got, got_raw = a.get_weights(swa=True), a.get_weights()             # either set is found wherever it lies
        assert all(np.array_equal(_bits(got[l][w]), _bits(saved[l][w])) for l in saved for w in saved[l])
        assert all(np.array_equal(_bits(got_raw[l][w]), _bits(saved_raw[l][w])) for l in saved for w in saved[l])
        avg = a.evaluate()
        avg_bits = a.loss_buf.clone()
        with pytest.raises(AssertionError, match="stands in"):
            a.step()
        with pytest.raises(AssertionError):
            a.swap_ema()
        with pytest.raises(AssertionError):
            with a.swa_weights():
                pass
        with pytest.raises(AssertionError):
            with a.swag_weights(0):
                pass
    assert not a.swa_swapped and back()
    with a.ema_weights():
        with pytest.raises(AssertionError):
            a.swap_swa()
        with pytest.raises(AssertionError):
            with a.swag_weights(0):
                pass
    assert back()
    b, _ = _engine(None, seed=99)
    b.set_weights(saved)
    b.load_batch(*val)
    assert b.evaluate() == avg and _same(b.loss_buf, avg_bits) and raw != avg
    with pytest.raises(RuntimeError, match="boom"):
        with a.swa_weights():
            raise RuntimeError("boom")
    assert not a.swa_swapped and back()
    # a sample: the written rule over the device buffers, under the shared statistics
    s = S.scale32(0.25)
    want = S.sample32(before[1].cpu().numpy()[:a.n_flat], before[2].cpu().numpy()[:a.n_flat], S.normals(a.n_flat, 77, 3), s)
    with a.swag_weights(3, seed=77, var_scale=0.25):
        assert a._swag_active and np.array_equal(_bits(a.flat_w[:a.n_flat]), _bits(want)) and not _same(a.flat_w, before[0])
        got = a.get_weights()                                                # the sample is the model: what save_weights() writes
        assert all(np.array_equal(_bits(got[l][w]), _bits(a.wview(l, w).cpu().numpy())) for l in saved for w in saved[l])
        assert not np.array_equal(got["loc_final"]["kernel"], saved_raw["loc_final"]["kernel"])
        sampled = a.evaluate()
        with pytest.raises(AssertionError, match="stands in"):
            a.step()
        with pytest.raises(AssertionError):
            a.swap_swa()
    assert not a._swag_active and back() and sampled != raw
    with pytest.raises(RuntimeError, match="boom"):
        with a.swag_weights(1):
            raise RuntimeError("boom")
    assert not a._swag_active and back()
    with a.swag_weights(3, seed=77, var_scale=0.0):                          # var_scale = 0: the mean itself
        assert np.array_equal(_bits(a.flat_w[:a.n_flat]), _bits(before[1][:a.n_flat]))
    assert back()
    for bad in (dict(sample=-1), dict(sample=True), dict(sample=0, seed=-1), dict(sample=0, seed=2 ** 64), dict(sample=0, var_scale=-1.0)):
        with pytest.raises(ValueError):
            a.swag_weights(**bad)
    # the next step ends where the same engine ends without the detours
    _steps(a, 1, first=14)
    _steps(c, 1, first=14)
    for name in ("flat_w", "flat_v", "flat_swa", "flat_swa_sq", "swa_state", "flat_ema"):
        assert _same(getattr(a, name), getattr(c, name)), name
    # fewer than two models: no variance to sample from; no SWA_VARIANCE: no sampling at all
    one, _ = _engine(2, SWA_VARIANCE=True)
    _steps(one, 2)
    w = one.flat_w.clone()
    with pytest.raises(ValueError, match="at least 2 collected models"):
        with one.swag_weights(0):
            pass
    assert _same(one.flat_w, w) and not one._swag_active and one._swag_hold is None
    plain, _ = _engine(2)
    with pytest.raises(AssertionError, match="SWA_VARIANCE"):
        plain.swag_weights(0)


def test_frozen_layers_are_sampled_at_exactly_their_weights():
    from ursonet_amd.graph import layer_regex
    eng, _ = _engine(1, SWA_VARIANCE=True)
    w0 = eng.flat_w.clone()
    eng.set_trainable(layer_regex("heads"))                                  # a re-plan: the buffers and the state survive it
    assert eng.labels["opt"][-1] == "swa"
    _steps(eng, 3)
    assert eng.swa()["models"] == 3
    w3 = eng.flat_w.clone()
    with eng.swag_weights(5, seed=2 ** 40 + 1):
        frozen = moved = 0
        for (ln, wn), (o, n, _) in eng.slices.items():
            same = _same(eng.flat_w[o:o + n], w0[o:o + n])
            if eng.layer_trainable[ln]:
                moved += not same and not _same(eng.flat_w[o:o + n], w3[o:o + n])
            else:
                assert same, (ln, wn)
                frozen += 1
    assert frozen > 20 and moved >= 4 and _same(eng.flat_w, w3)


def test_under_accumulation_only_closing_steps_tick():
    eng, _ = _engine(1, GRAD_ACCUM_STEPS=2)
    assert eng.labels["opt"][-1] == "swa" and "swa" not in eng.labels["accum"]
    _steps(eng, 1)
    assert eng.swa()["ticks"] == 0 and eng.swa()["models"] == 0              # an open micro-step
    _steps(eng, 1, first=12)
    assert eng.swa()["ticks"] == 1 and eng.swa()["models"] == 1 and _same(eng.flat_swa, eng.flat_w)
    _steps(eng, 3, first=13)
    assert eng.swa()["ticks"] == 2 and eng.grad_accum()["micro"] == 1


def test_a_skipped_fp16_step_does_not_tick():
    """fp16 under a static loss scale of 2**24: every step overflows and is skipped (as in the WEIGHT_EMA tests)."""
    eng, _ = _engine(1, dtype="float16", LOSS_SCALE=2.0 ** 24, SWA_VARIANCE=True)
    eng.flat_swa.fill_(3.0)
    st0, w0 = eng.swa_state.tolist(), eng.flat_w.clone()
    _steps(eng, 2)
    assert not bool(torch.isfinite(eng.normsq).all()) and eng.loss_scale()["skipped_total"] == 2
    assert eng.swa_state.tolist() == st0 and _same(eng.flat_w, w0) and float(eng.flat_swa.min()) == 3.0 == float(eng.flat_swa.max())
    ok, _ = _engine(1, dtype="float16", LOSS_SCALE=1.0, SWA_VARIANCE=True)
    _steps(ok, 1)
    assert not ok.loss_scale()["last_step_skipped"] and ok.swa()["models"] == 1 and _same(ok.flat_swa, ok.flat_w)


def test_checkpoints_restart_and_training_state():
    S = _S()
    eng, cfg = _engine(2, SWA_VARIANCE=True)
    _steps(eng, 4)
    assert eng.swa()["models"] == 2
    mean, sq, st = eng.flat_swa.clone(), eng.flat_swa_sq.clone(), eng.swa_state.tolist()
    saved = eng.save_train_state()
    _steps(eng, 2, first=20)
    assert eng.swa()["models"] == 3 and not _same(eng.flat_swa, mean)
    eng.restore_train_state(saved)
    assert _same(eng.flat_swa, mean) and _same(eng.flat_swa_sq, sq) and eng.swa_state.tolist() == st
    pm, ps, pw = eng.get_weights(swa=True), eng.get_weights(swa="sq"), eng.get_weights()
    eng.set_weights(pw)                                                      # loading weights restarts the collection
    assert eng.swa()["ticks"] == 0 and eng.swa()["models"] == 0
    other, _ = _engine(2, SWA_VARIANCE=True, seed=8)
    other.set_swa_weights(pm, ps, models=2)
    assert _same(other.flat_swa[:eng.n_flat], mean[:eng.n_flat]) and _same(other.flat_swa_sq[:eng.n_flat], sq[:eng.n_flat])
    want = list(st)
    want[S.COLLECTED] = 0
    assert st[S.TICKS] == 4 and other.swa_state.tolist() == want             # ticks = start + models * period: the collection goes on from there
    for bad in (dict(models=0), dict(models=True), dict(models=None), dict(models=2.0)):
        with pytest.raises(ValueError, match="models must be an int"):
            other.set_swa_weights(pm, ps, **bad)
    with pytest.raises(ValueError, match="SWA_VARIANCE"):
        other.set_swa_weights(pm, None, models=2)


def test_train_validates_logs_saves_and_recalibrates_the_average(tmp_path, capsys):
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config(dtype="float32", lr=0.01, **GEOM)
    cfg.NAME = "swa"
    cfg.TRAIN_BN = None
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 3, 1
    cfg.SWA, cfg.SWA_START, cfg.SWA_VARIANCE, cfg.SWA_RECAL_BATCHES = 2, 2, True, 1
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    eng = model._engine
    adds = []
    orig_add = eng.bn_recal_add
    eng.bn_recal_add = lambda: (adds.append(eng.swa_swapped), orig_add())[1]
    capsys.readouterr()
    model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=3, layers="all")
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if re.match(r"epoch \d  loc_loss", l)]
    num = r"\d+\.\d{5}"
    assert len(lines) == 3
    # models are collected at steps 4, 6, 8: none in epoch 1 (no line about the average, no file), one in epoch 2, three after epoch 3
    assert re.fullmatch(r"epoch 1  loc_loss %s  val_loc_loss %s  val_ori_loss %s" % (num, num, num), lines[0]), lines[0]
    for k, models in ((2, 2), (3, 3)):
        assert re.fullmatch(r"epoch %d  loc_loss %s  val_loc_loss %s  val_ori_loss %s  val_swa_loc_loss %s  val_swa_ori_loss %s  swa models %d"
                            % (k, num, num, num, num, num, models), lines[k - 1]), lines[k - 1]
    recal = re.findall(r"^epoch (\d)  bn recal  1 batches x 2 images under the averaged weights", out, re.M)
    assert recal == ["2", "3"] and adds == [True, True] and not eng.swa_swapped
    assert eng.swa() == {"period": 2, "start": 2, "ticks": 9, "models": 3, "collected": False, "variance": True}
    ddir, ck = model.find_last()
    assert os.path.basename(ck) in ("weights_swa_0003.npz", "weights_swa_0003.h5")          # the raw file, not its averaged twins
    files = sorted(f for f in os.listdir(ddir) if f.endswith(".npz"))
    assert files == sorted(["weights_swa_%04d.npz" % e for e in (1, 2, 3)] + ["swa_weights_swa_%04d.npz" % e for e in (2, 3)] +
                           ["swa_sqmean_swa_%04d.npz" % e for e in (2, 3)])
    raw3 = net.read_weights_file(os.path.join(ddir, "weights_swa_0003.npz"))
    avg3 = net.read_weights_file(os.path.join(ddir, "swa_weights_swa_0003.npz"))
    sqm3 = net.read_weights_file(os.path.join(ddir, "swa_sqmean_swa_0003.npz"))
    now_avg, now_sq, now_raw = eng.get_weights(swa=True), eng.get_weights(swa="sq"), eng.get_weights()
    assert list(avg3) == list(now_avg) == list(sqm3)
    bn_stats = set(eng.stat_slices)
    for l in now_avg:
        for w in now_avg[l]:
            assert np.array_equal(_bits(raw3[l][w]), _bits(now_raw[l][w])), (l, w)         # the raw statistics included: back bit for bit
            if (l, w) in bn_stats:                                           # the averaged file has statistics of its own
                assert not np.array_equal(avg3[l][w], raw3[l][w]) and np.isfinite(avg3[l][w]).all(), (l, w)
            else:
                assert np.array_equal(_bits(avg3[l][w]), _bits(now_avg[l][w])) and np.array_equal(_bits(sqm3[l][w]), _bits(now_sq[l][w])), (l, w)
    assert not np.array_equal(avg3["loc_final"]["kernel"], raw3["loc_final"]["kernel"])
    # the files load back into the device buffers bit for bit, and the sampled model is an ordinary weights file
    m1 = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    p3 = os.path.join(ddir, "weights_swa_0003.npz")
    m1.load_weights(p3, p3, by_name=True)
    assert m1._engine.swa()["models"] == 0
    m1.load_swa(os.path.join(ddir, "swa_weights_swa_0003.npz"), os.path.join(ddir, "swa_sqmean_swa_0003.npz"), models=3)
    e1 = m1._engine
    assert _same(e1.flat_swa[:e1.n_flat], eng.flat_swa[:e1.n_flat]) and _same(e1.flat_swa_sq[:e1.n_flat], eng.flat_swa_sq[:e1.n_flat])
    assert _same(e1.flat_w[:e1.n_flat], eng.flat_w[:e1.n_flat]) and e1.swa()["models"] == 3 and e1.swa()["ticks"] == 8
    with m1.swag_weights(0, seed=11):
        written = m1.save_weights(os.path.join(str(tmp_path), "sampled_0.npz"))
        inside = e1.flat_w.clone()
    sampled = net.read_weights_file(written[0])
    assert np.array_equal(_bits(sampled["loc_final"]["kernel"]), _bits(e1.wview("loc_final", "kernel", inside).cpu().numpy()))
    assert not np.array_equal(sampled["loc_final"]["kernel"], raw3["loc_final"]["kernel"]) and _same(e1.flat_w[:e1.n_flat], eng.flat_w[:e1.n_flat])
