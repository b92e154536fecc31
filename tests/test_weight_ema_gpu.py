"""The weights' moving average on the GPU (Config.WEIGHT_EMA).

Kernel level: urso_ema_update bit for bit against ursonet_amd.weight_ema.update32 and next_state in guarded buffers (every ragged-tail
case of a 16-byte access, one block, many blocks, the grid-stride loop, buffers off the 16-byte boundary), the loss-scale skip, and
urso_ema_swap on int32 views.
Engine level (resnet18, 64 x 64, batch 2: 11.3 M parameters, so the step's own launch walks its grid-stride loop): the feature leaves the
training trajectory bit for bit, the average is the written recurrence of the weights after every step, graph replay equals the eager
step, a swap evaluates what a second engine evaluates on the saved average, frozen layers keep the weights' bits, a skipped fp16 step
does not count, the plan is the parent's with the key off, and UrsoNet.train() validates, logs and saves the average.

NaN results: IEEE 754 leaves the payload and sign of a NaN result to the implementation (x86 gives inf - inf a negative quiet NaN, gfx950 a
positive one), so the update is compared bit for bit wherever the emulation's result is not a NaN, and NaN for NaN where it is.  The swap
moves integers: every bit, NaN payloads included."""
import os
import re

import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats in front of and behind every buffer under test (256 bytes: the buffer itself stays 16-byte aligned)
GUARD_BITS = 0x7FA5A5A5          # a NaN with a payload: an arithmetic pass over it would show, and so would a copy
# the issue's sizes: the ragged tail on each side of a 16-byte access, one block, more than one block; + one size past 4096 blocks x 256
# threads x 4 elements, the only one at which the grid-stride loop takes a second turn
SIZES = [1, 3, 4, 5, 255, 256, 257, 4096 + 1, 2 ** 20 + 3, 2 ** 22 + 2 ** 12 + 1]


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _WE():
    from ursonet_amd import weight_ema
    return weight_ema


def _values(n, seed):
    """Normal-range random fp32 values over twelve decades, with +inf, -inf and NaNs (two payloads) sprinkled in where n allows."""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32)
    x[np.abs(x) < 1e-30] = 1.0
    if n >= 255:
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


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _assert_update_bits(got, want, what):
    """got: fp32 device tensor; want: the emulation's float32 array.  Bit for bit off the NaNs, NaN for NaN on them."""
    got = got.detach().cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaNs in other places"
    bad = got.view(np.int32)[~nan] != want.view(np.int32)[~nan]
    assert not bad.any(), "%s: %d of %d elements differ from update32" % (what, int(bad.sum()), got.size)


def _ema_state(decay, warmup=True, updates=0.0):
    WE = _WE()
    s = [float(np.float32(decay)), float(warmup), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    s[WE.UPDATES] = float(updates)
    s[WE.NEXT_DECAY] = float(WE._schedule(s[WE.DECAY], warmup, updates))
    return s


def _dev_state(s):
    return torch.tensor(s, dtype=torch.float32, device="cuda")


# ===================================================================================================================== kernel level
@pytest.mark.parametrize("n", SIZES)
def test_update_is_update32_bit_for_bit(n):
    """One update at decay 0.9 without warm-up (c = fl32(1 - fl32(0.9)) has a full mantissa) in guarded buffers; the state advances as
    next_state says, w is only read, the guard words on both sides of both buffers keep their bits."""
    hip, WE = _hip(), _WE()
    w, e = _values(n, 100 + n), _values(n, 200 + n)
    e[::3] = w[::3]                                                          # a third of the elements are "frozen": w == ema
    st = _ema_state(0.9, warmup=False)
    wg, wv = _guarded(w)
    eg, ev = _guarded(e)
    sd = _dev_state(st)
    hip.ema_update(n, wv, ev, sd)
    torch.cuda.synchronize()
    want = WE.update32(e, w, st[WE.NEXT_DECAY])
    _assert_update_bits(ev, want, "n = %d" % n)
    same = (w == e) & np.isfinite(w)
    assert np.array_equal(_bits(ev)[same], e.view(np.int32)[same])           # equal operands (infinities are not: inf - inf) keep ema's bits
    assert np.array_equal(_bits(wv), w.view(np.int32)) and _guards_intact(wg, n) and _guards_intact(eg, n)
    assert sd.tolist() == WE.next_state(st)


@pytest.mark.parametrize("n", [1, 3, 5, 257, 4096 + 1])
@pytest.mark.parametrize("shifts", [(1, 1), (3, 3), (2, 0), (0, 1)])
def test_update_and_swap_off_the_16_byte_boundary(n, shifts):
    """4-byte alignment is all the entry points ask for: both buffers off the boundary alike (a scalar head, then vectors) and differently
    (scalars alone) give the same bits and leave the guards alone."""
    hip, WE = _hip(), _WE()
    w, e = _values(n, 300 + n), _values(n, 400 + n)
    wg, wv = _guarded(w, shifts[0])
    eg, ev = _guarded(e, shifts[1])
    assert wv.data_ptr() % 16 == 4 * shifts[0] and ev.data_ptr() % 16 == 4 * shifts[1]
    st = _ema_state(0.9, warmup=False)
    hip.ema_update(n, wv, ev, _dev_state(st))
    torch.cuda.synchronize()
    want = WE.update32(e, w, st[WE.NEXT_DECAY])
    _assert_update_bits(ev, want, "n = %d shifts %s" % (n, shifts))
    assert np.array_equal(_bits(wv), w.view(np.int32)) and _guards_intact(wg, n, shifts[0]) and _guards_intact(eg, n, shifts[1])
    after = _bits(ev).copy()
    hip.ema_swap(n, wv, ev)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(wv), after) and np.array_equal(_bits(ev), w.view(np.int32))
    assert _guards_intact(wg, n, shifts[0]) and _guards_intact(eg, n, shifts[1])


def test_twelve_updates_with_warmup_follow_the_emulation():
    """Decay 0.5 with warm-up: the ramp (1 + t) / (10 + t) up to the knee at t = 8 and the configured decay behind it.  ema is the
    emulation bit for bit and the state is next_state field for field after every one of 12 updates of fresh weights."""
    hip, WE = _hip(), _WE()
    n = 4096 + 1
    st = _ema_state(0.5)
    e = _values(n, 7)
    e[np.isnan(e) | np.isinf(e)] = 1.0
    eg, ev = _guarded(e)
    sd = _dev_state(st)
    used = []
    for k in range(12):
        w = _values(n, 20 + k)
        w[np.isnan(w) | np.isinf(w)] = -2.0                                  # finite throughout: twelve steps of bit-for-bit, no NaN rule
        used.append(st[WE.NEXT_DECAY])
        e = WE.update32(e, w, st[WE.NEXT_DECAY])
        st = WE.next_state(st)
        hip.ema_update(n, torch.from_numpy(w).cuda(), ev, sd)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ev), e.view(np.int32)), "update %d" % (k + 1)
        assert sd.tolist() == st, (k, sd.tolist(), st)
    assert _guards_intact(eg, n)
    assert used[0] == float(np.float32(1.0) / np.float32(10.0)) and sum(d < 0.5 for d in used) == 8 and used[8:] == [0.5] * 4     # both branches
    assert st[WE.UPDATES] == 12.0
    # saturation: an update from t = 2**24 leaves t there
    sat = _ema_state(0.5, updates=2.0 ** 24)
    sd = _dev_state(sat)
    hip.ema_update(n, torch.from_numpy(_values(n, 1)).cuda(), ev, sd)
    torch.cuda.synchronize()
    assert sd.tolist() == WE.next_state(sat) == sat


def test_loss_scale_state_gates_the_update():
    """ls_state with LAST_SKIPPED = 1: ema and the state keep their bits.  LAST_SKIPPED = 0: the update happens, as without a state."""
    from ursonet_amd import loss_scale as LS
    hip, WE = _hip(), _WE()
    n = 4096 + 1
    w, e = _values(n, 31), _values(n, 32)
    st = _ema_state(0.5)
    ls = [1024.0, 1.0 / 1024, 0.0, 0.0, 1024.0, 1024.0, 3.0, 1.0]
    assert ls[LS.LAST_SKIPPED] == 1.0
    eg, ev = _guarded(e)
    sd, lsd, wd = _dev_state(st), _dev_state(ls), torch.from_numpy(w).cuda()
    hip.ema_update(n, wd, ev, sd, ls=lsd)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ev), e.view(np.int32)) and sd.tolist() == st and lsd.tolist() == ls
    ls[LS.LAST_SKIPPED] = 0.0
    lsd = _dev_state(ls)
    hip.ema_update(n, wd, ev, sd, ls=lsd)
    torch.cuda.synchronize()
    _assert_update_bits(ev, WE.update32(e, w, st[WE.NEXT_DECAY]), "LAST_SKIPPED = 0")
    assert sd.tolist() == WE.next_state(st) and lsd.tolist() == ls and _guards_intact(eg, n)
    assert not np.array_equal(_bits(ev), e.view(np.int32))


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_every_bit(n):
    hip = _hip()
    a, b = _values(n, 500 + n), _values(n, 600 + n)
    ag, av = _guarded(a)
    bg, bv = _guarded(b)
    ai, bi = av.view(torch.int32), bv.view(torch.int32)
    hip.ema_swap(n, ai, bi)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(av), b.view(np.int32)) and np.array_equal(_bits(bv), a.view(np.int32))
    assert _guards_intact(ag, n) and _guards_intact(bg, n)
    hip.ema_swap(n, ai, bi)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(av), a.view(np.int32)) and np.array_equal(_bits(bv), b.view(np.int32))      # NaN payloads included
    assert _guards_intact(ag, n) and _guards_intact(bg, n)
    hip.ema_swap(0, ai, bi)                                                  # n = 0 touches nothing
    hip.ema_update(0, av, bv, _dev_state(_ema_state(0.5)))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(av), a.view(np.int32)) and np.array_equal(_bits(bv), b.view(np.int32))


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(ema=None, dtype="float32", optimizer="SGD", seed=3, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM)
    cfg.OPTIMIZER = optimizer
    cfg.WEIGHT_EMA = ema
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
    assert off.labels["opt"] == ["sqnorm", "sgd"] and off.flat_ema is None and off.ema_state is None and off.weight_ema() is None
    assert not any("ema" in l for ls in off.labels.values() for l in ls)
    on, _ = _engine(0.9)
    assert on.labels["opt"] == ["sqnorm", "sgd", "ema"] and {k: v for k, v in on.labels.items() if k != "opt"} == {k: v for k, v in off.labels.items() if k != "opt"}
    assert _same(on.flat_ema, on.flat_w) and on.flat_ema.data_ptr() != on.flat_w.data_ptr()
    assert on.weight_ema() == {"decay": float(np.float32(0.9)), "warmup": True, "updates": 0, "next_decay": float(np.float32(1.0) / np.float32(10.0))}
    both, _ = _engine(0.9, LOSS_SCALE=1024.0, optimizer="ADAM")
    assert both.labels["opt"] == ["sqnorm", "adam", "loss_scale", "ema"]       # behind loss_scale: LAST_SKIPPED is this step's
    with pytest.raises(ValueError, match="WEIGHT_EMA"):
        _engine(1.0)
    from ursonet_amd.engine import Engine
    _, cfg = _engine(None)
    cfg.WEIGHT_EMA = 0.9
    inf = Engine(cfg, "inference", seed=3)
    assert inf.flat_ema is None and inf.ema_state is None                    # inference ignores the key


def test_the_feature_does_not_perturb_training():
    a, _ = _engine(None)
    b, _ = _engine(0.9)
    _steps(a, 5)
    _steps(b, 5)
    assert float(a.flat_g.abs().max()) > 0 and bool(torch.isfinite(a.flat_w).all())
    for name in ("flat_w", "flat_v", "flat_g", "loss_buf", "flat_stats"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert b.weight_ema()["updates"] == 5 and not _same(b.flat_ema, b.flat_w)


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_the_average_is_the_recurrence_of_the_weights(optimizer):
    WE = _WE()
    eng, cfg = _engine(0.9, optimizer=optimizer)
    state = WE.initial_state(cfg)
    assert eng.ema_state.tolist() == state
    ema = eng.flat_ema.cpu().numpy().copy()
    decays = []
    for s in range(6):
        _steps(eng, 1, first=11 + s)
        w = eng.flat_w.cpu().numpy()
        decays.append(state[WE.NEXT_DECAY])
        ema = WE.update32(ema, w, state[WE.NEXT_DECAY])
        state = WE.next_state(state)
        assert np.array_equal(eng.flat_ema.cpu().numpy().view(np.int32), ema.view(np.int32)), "step %d" % (s + 1)
        assert eng.ema_state.tolist() == state
    assert np.isfinite(ema).all() and decays == [float(min(np.float32(0.9), np.float32(1 + t) / np.float32(10 + t))) for t in range(6)]
    v = eng.flat_v.clone()
    eng.reset_optimizer()                                                    # the average is no optimizer state
    assert float(eng.flat_v.abs().max()) == 0 and float(v.abs().max()) > 0
    assert eng.ema_state.tolist() == state and np.array_equal(eng.flat_ema.cpu().numpy().view(np.int32), ema.view(np.int32))


def test_graph_replay_equals_the_eager_step():
    a, _ = _engine(0.9)
    b, _ = _engine(0.9)
    a.load_batch(*_batch(11))
    a.capture()
    torch.cuda.synchronize()
    assert a.weight_ema()["updates"] == 0 and _same(a.flat_ema, a.flat_w) and _same(a.flat_w, b.flat_w)      # the warm-up step is undone
    _steps(a, 3)
    _steps(b, 3, eager=True)
    for name in ("flat_w", "flat_v", "flat_g", "flat_ema", "ema_state", "loss_buf"):
        assert _same(getattr(a, name), getattr(b, name)), name
    assert a.weight_ema()["updates"] == 3


def test_validation_on_the_average_is_a_detour_without_trace():
    """evaluate() inside ema_weights() = evaluate() of a second engine loaded with get_weights(ema=True); after the context every bit of the
    training state is back, and the next step ends where the same engine ends without the detour."""
    a, cfg = _engine(0.9)
    c, _ = _engine(0.9)
    _steps(a, 3)
    _steps(c, 3)
    before = [t.clone() for t in (a.flat_w, a.flat_ema, a.flat_v, a.ema_state, a.flat_stats)]
    val = _batch(40)
    a.load_batch(*val)
    raw = a.evaluate()
    raw_bits = a.loss_buf.clone()
    saved = a.get_weights(ema=True)
    with a.ema_weights() as inside:
        assert inside is a and a.ema_swapped
        assert _same(a.flat_w, before[1]) and _same(a.flat_ema, before[0])
        inside_weights = a.get_weights(ema=True)
        assert all(np.array_equal(inside_weights[l][w].view(np.int32), saved[l][w].view(np.int32)) for l in saved for w in saved[l])
        avg = a.evaluate()
        avg_bits = a.loss_buf.clone()
        with pytest.raises(AssertionError, match="swapped"):
            a.step()
    assert not a.ema_swapped
    torch.cuda.synchronize()
    for name, x, y in zip(("flat_w", "flat_ema", "flat_v", "ema_state", "flat_stats"), before, (a.flat_w, a.flat_ema, a.flat_v, a.ema_state, a.flat_stats)):
        assert _same(x, y), name
    b, _ = _engine(None, seed=99)
    b.set_weights(saved)
    b.load_batch(*val)
    ref = b.evaluate()
    assert _same(b.loss_buf, avg_bits) and ref == avg
    assert not _same(raw_bits, avg_bits) and raw != avg                      # the two sets differ after three steps, and so do their losses
    _steps(a, 1, first=14)
    _steps(c, 1, first=14)
    for name in ("flat_w", "flat_v", "flat_ema", "ema_state"):
        assert _same(getattr(a, name), getattr(c, name)), name


def test_frozen_layers_keep_the_weights_bits():
    from ursonet_amd.graph import layer_regex
    eng, _ = _engine(0.9)
    w0 = eng.flat_w.clone()
    eng.set_trainable(layer_regex("heads"))                                  # a re-plan: flat_ema and ema_state survive it
    assert eng.labels["opt"][-1] == "ema" and _same(eng.flat_ema, w0)
    _steps(eng, 3)
    assert eng.weight_ema()["updates"] == 3
    frozen = moved = 0
    for (ln, wn), (o, n, _) in eng.slices.items():
        same = _same(eng.flat_ema[o:o + n], eng.flat_w[o:o + n])
        if eng.layer_trainable[ln]:
            assert not same, (ln, wn)
            moved += 1
        else:
            assert same and _same(eng.flat_w[o:o + n], w0[o:o + n]), (ln, wn)
            frozen += 1
    assert frozen > 20 and moved >= 4


def test_a_skipped_fp16_step_does_not_count():
    """fp16 under a static loss scale of 2**24: the scaled head gradients are far past 65504, every step overflows and is skipped.  The
    average is moved off the weights first, so an update that ran anyway would show."""
    eng, _ = _engine(0.9, dtype="float16", LOSS_SCALE=2.0 ** 24)
    eng.flat_ema.mul_(0.5)
    ema0, w0, st0 = eng.flat_ema.clone(), eng.flat_w.clone(), eng.ema_state.tolist()
    _steps(eng, 2)
    assert not bool(torch.isfinite(eng.normsq).all())
    assert eng.loss_scale()["skipped_total"] == 2 and eng.loss_scale()["last_step_skipped"]
    assert eng.weight_ema()["updates"] == 0 and eng.ema_state.tolist() == st0
    assert _same(eng.flat_ema, ema0) and _same(eng.flat_w, w0)
    # the same engine's launch does move it once the step is performed: a finite norm under a scale of 1
    ok, _ = _engine(0.9, dtype="float16", LOSS_SCALE=1.0)
    ok.flat_ema.mul_(0.5)
    ema0 = ok.flat_ema.clone()
    _steps(ok, 1)
    assert not ok.loss_scale()["last_step_skipped"] and ok.weight_ema()["updates"] == 1 and not _same(ok.flat_ema, ema0)


def test_train_validates_logs_and_saves_the_average(tmp_path, capsys):
    import copy
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    WE = _WE()
    cfg = make_config(dtype="float32", lr=0.01, **GEOM)
    cfg.NAME = "ema"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 3, 1
    cfg.WEIGHT_EMA = 0.9
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    lines = [l for l in capsys.readouterr().out.splitlines() if re.match(r"epoch \d", l)]
    num = r"\d+\.\d{5}"
    assert len(lines) == 2
    for k, line in enumerate(lines):
        assert re.fullmatch(r"epoch %d  loc_loss %s  val_ema_loc_loss %s  val_ema_ori_loss %s  val_loc_loss %s  val_ori_loss %s  ema_decay \S+"
                            % (k + 1, num, num, num, num, num), line), line
    sched = [float(min(np.float32(0.9), np.float32(1 + t) / np.float32(10 + t))) for t in range(6)]
    assert hist.ema_decay_acc == sched and len(hist.loc_loss_acc) == 6
    assert lines[0].endswith("ema_decay %g" % sched[2]) and lines[1].endswith("ema_decay %g" % sched[5])
    eng = model._engine
    assert eng.weight_ema()["updates"] == 6 and not eng.ema_swapped
    ddir, ck = model.find_last()
    assert os.path.basename(ck) in ("weights_ema_0002.npz", "weights_ema_0002.h5")          # the raw file, not its averaged twin
    for epoch in (1, 2):
        for stem in ("weights_ema_%04d.npz" % epoch, "ema_weights_ema_%04d.npz" % epoch):
            assert os.path.exists(os.path.join(ddir, stem)), stem
    raw2 = net.read_weights_file(os.path.join(ddir, "weights_ema_0002.npz"))
    avg2 = net.read_weights_file(os.path.join(ddir, "ema_weights_ema_0002.npz"))
    avg1 = net.read_weights_file(os.path.join(ddir, "ema_weights_ema_0001.npz"))
    now_avg, now_raw = eng.get_weights(ema=True), eng.get_weights()
    assert list(avg2) == list(now_avg)
    assert all(np.array_equal(avg2[l][w], now_avg[l][w]) for l in now_avg for w in now_avg[l])
    assert all(np.array_equal(raw2[l][w], now_raw[l][w]) for l in now_raw for w in now_raw[l])
    assert not np.array_equal(avg2["loc_final"]["kernel"], raw2["loc_final"]["kernel"])
    assert not np.array_equal(avg2["loc_final"]["kernel"], avg1["loc_final"]["kernel"])
    # a training model that loads the raw checkpoint of epoch 1 finds the averaged twin beside it
    m1 = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    p1 = os.path.join(ddir, "weights_ema_0001.npz")
    m1.load_weights(p1, p1, by_name=True)
    got_avg, got_raw, raw1 = m1._engine.get_weights(ema=True), m1._engine.get_weights(), net.read_weights_file(p1)
    assert all(np.array_equal(got_avg[l][w], avg1[l][w]) for l in avg1 for w in avg1[l])
    assert all(np.array_equal(got_raw[l][w], raw1[l][w]) for l in raw1 for w in raw1[l])
    # the averaged file is an ordinary weights file: an inference model loads it and detect() runs on it
    icfg = copy.copy(cfg)
    icfg.IMAGES_PER_GPU = 1
    icfg.update()
    m2 = net.UrsoNet(mode="inference", config=icfg, model_dir=str(tmp_path))
    assert m2._engine.flat_ema is None
    pa = os.path.join(ddir, "ema_weights_ema_0002.npz")
    m2.load_weights(pa, pa, by_name=True)
    loaded = m2._engine.get_weights()
    assert all(np.array_equal(loaded[l][w], avg2[l][w]) for l in avg2 for w in avg2[l]) and m2.epoch == 2
    res = m2.detect([ds_val.load_image(0)], verbose=0)
    assert set(res[0]) == {"loc", "ori"} and np.isfinite(res[0]["loc"]).all() and np.isfinite(res[0]["ori"]).all()
