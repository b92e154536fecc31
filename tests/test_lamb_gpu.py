"""LAMB on the GPU (Config.LAMB).

Kernel level: urso_lamb_moments, urso_lamb_trust and urso_lamb_apply bit for bit against ursonet_amd.lamb.step32 over the layout of
tests/lamb_layout.py -- ten tensors in one flat buffer at the sizes where the kernels take another path (a single element, the ragged end
on each side of a 16-byte access, less than a wave, less than a chunk, a chunk, a chunk and one, several chunks with a short and with a
whole last one), a NaN-payload sentinel in all padding and guards of all five buffers, a tensor with g = 0 and zero moments, one with
w = 0, two that do not adapt, non-trivial m, v, vhat and t = 3; clip factor 1 and below 1, LAMB_CLIP off and on, two consecutive steps,
T = 0, and the skipped step of the loss-scaled form.  tests/test_lamb_cpu.py checks, on the NumPy rule alone, that every stored
intermediate of that layout is zero or a normal float32 and that its adapting tensors lie on both sides of LAMB_CLIP's min.
Engine level (resnet18, 64 x 64, batch 2, the engine of the LARS tests, OPTIMIZER = Adam): after every step() the weights, both moments,
vhat, t and the state are lamb.step32 of the previous ones, this step's gradient and the engine's norm, bit for bit, and lamb_report() is
that step's table; the same under GRAD_ACCUM_STEPS = 2 and WEIGHT_EMA, and under fp16 with a dynamic LOSS_SCALE whose first replays
overflow; graph replay equals eager launches; frozen layers keep trust 1 and do not move; with the key off the plan and the weights are
plain Adam's; UrsoNet.train() prints the trust summary once per epoch."""
import numpy as np
import pytest
import torch

import lamb_layout as LAY
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

SIZES, ZERO_G, ZERO_W, PLAIN, SENTINEL = LAY.SIZES, LAY.ZERO_G, LAY.ZERO_W, LAY.PLAIN, LAY.SENTINEL
BUFS = ("w", "m", "v", "vhat")


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _B():
    from ursonet_amd import lamb
    return lamb


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_refs = {}


def _ref(clip, clip_mode):
    """The two consecutive reference steps of one case, computed once and shared."""
    if (clip, clip_mode) not in _refs:
        _refs[(clip, clip_mode)] = LAY.reference(clip, clip_mode, steps=2)
    return _refs[(clip, clip_mode)]


class _Case(object):
    """The layout on the device with a fresh plan whose outputs hold a marker."""

    def __init__(self, clip, normsq=None, ls=False):
        hip, lay = _hip(), LAY.layout()
        self.d = {k: _dev(lay[k]) for k in LAY.NAMES}
        hyper_h, state_h = LAY.hyper_state(clip)
        self.hyper, self.normsq = _dev(hyper_h), _dev(np.array([lay["normsq"] if normsq is None else normsq], dtype=np.float32))
        self.plan = hip.LambPlan(lay["tensors"], "cuda")
        self.plan.state.copy_(_dev(state_h))
        self.plan.part.fill_(-1.0); self.plan.trust.fill_(-1.0); self.plan.stat.fill_(-1.0)
        self.ls = _dev(np.array([1024.0, 1.0 / 1024.0, 0, 2000, 1, 65536, 0, 0], dtype=np.float32)) if ls else None

    def run(self, clip_mode):
        d, p = self.d, self.plan
        p.moments(d["w"], d["g"], d["m"], d["v"], d["vhat"], self.hyper, self.normsq, ls=self.ls)
        p.trust_ratios(self.normsq, LAY.ETA, LAY.EPS, clip_mode, ls=self.ls)
        p.apply(d["w"], d["m"], d["vhat"], self.hyper, self.normsq, ls=self.ls)
        torch.cuda.synchronize()

    def host(self, name):
        return self.d[name].cpu().numpy()


# ===================================================================================================================== kernel level
def test_plan_shares_the_block_map_and_owns_its_outputs():
    hip, lay = _hip(), LAY.layout()
    from ursonet_amd import lars as L
    plan = hip.LambPlan(lay["tensors"], "cuda")
    assert plan.T == 10 and plan.nblocks == sum(L.chunks(n) for n in SIZES) == 6 + 1 + 2 + 3 + 3
    assert isinstance(plan.tables, hip.LarsPlan)
    assert plan.blockmap.cpu().tolist() == [[t, c] for t, n in enumerate(SIZES) for c in range(L.chunks(n))]
    assert plan.first.cpu().tolist() == list(np.cumsum([0] + [L.chunks(n) for n in SIZES]))
    assert plan.tab.cpu().tolist() == [[o, n] for o, n, _ in lay["tensors"]] and plan.adapt.cpu().tolist() == [int(a) for _, _, a in lay["tensors"]]
    assert plan.state.tolist() == [1.0, 1.0, 0.0] and plan.part.shape == (plan.nblocks, 2) and plan.stat.shape == (10, 3)
    assert plan.trust.dtype == torch.float32 and plan.stat.dtype == torch.float64


@pytest.mark.parametrize("clip_mode", [False, True])
@pytest.mark.parametrize("clip", LAY.CLIPS)
def test_three_launches_bit_for_bit(clip, clip_mode):
    """clip = 0 and 1e9: c = 1 (no clip, and one out of reach); clip = 1e4: c < 1 (the gradient's norm is about 3e4)."""
    from ursonet_amd import lars as L
    lay = LAY.layout()
    tensors, used = lay["tensors"], lay["used"]
    assert (L.clip_factor32(lay["normsq"], clip) < 1) == (clip == 1e4)
    case = _Case(clip)
    prev = {k: lay[k] for k in BUFS}
    for step, (ew, em, ev, eh, ehyper, estate, etrust, estat) in enumerate(_ref(clip, clip_mode)):
        case.run(clip_mode)
        exp = dict(w=ew, m=em, v=ev, vhat=eh)
        part = case.plan.part.cpu().numpy()
        r = _B().direction32(em, eh, estate[2], ehyper[3])                   # the direction of this step, from the stored moments
        for t, (o, n, _a) in enumerate(tensors):                             # the slots
            s0, s1 = int(case.plan.first_h[t]), int(case.plan.first_h[t + 1])
            assert _same_bits(part[s0:s1, 0], L.slot_sums32(prev["w"][o:o + n])), ("w slots", step, t)
            assert _same_bits(part[s0:s1, 1], L.slot_sums32(r[o:o + n])), ("r slots", step, t)
        trust, stat = case.plan.trust.cpu().numpy(), case.plan.stat.cpu().numpy()
        assert _same_bits(stat, estat) and _same_bits(trust, etrust), step
        for name in BUFS:
            got = case.host(name)
            assert _same_bits(got[used], exp[name][used]), (name, step)
            assert (_bits(got[~used]) == SENTINEL).all(), (name, step)       # padding and guards keep the sentinel
        assert _same_bits(case.host("g"), lay["g"])                          # g is only read
        assert _same_bits(case.hyper.cpu().numpy(), ehyper) and _same_bits(case.plan.state.cpu().numpy(), estate)
        assert ehyper[5] == 4 + step
        # what the cases are there for
        assert trust[ZERO_G] == 1 and stat[ZERO_G, 1] == 0 and stat[ZERO_G, 0] > 0
        if step == 0:                                                        # (the first step moves it off zero at trust 1)
            assert trust[ZERO_W] == 1 and stat[ZERO_W, 0] == 0 and stat[ZERO_W, 1] > 0
        else:
            assert trust[ZERO_W] != 1 and stat[ZERO_W, 0] > 0
        o, n, _a = tensors[ZERO_G]
        assert _same_bits(case.host("w")[o:o + n], lay["w"][o:o + n])        # r = 0: it does not move
        for t in PLAIN:
            assert trust[t] == 1 and stat[t, 2] == 1 and stat[t, 0] > 0 and stat[t, 1] > 0
        adapting = [t for t in range(len(SIZES)) if t not in PLAIN + (ZERO_G, ZERO_W)]
        assert all(trust[t] != 1 for t in adapting if not clip_mode) and all(0 < trust[t] <= 1 for t in adapting if clip_mode)
        if clip_mode and step == 0:
            assert any(trust[t] == 1 for t in adapting) and any(trust[t] < 1 for t in adapting)      # both sides of the min
        assert not _same_bits(exp["w"][used], prev["w"][used])
        prev = exp
    # a second run from the same inputs gives the same bits
    again = _Case(clip)
    again.run(clip_mode); again.run(clip_mode)
    for name in BUFS:
        assert torch.equal(again.d[name].view(torch.int32), case.d[name].view(torch.int32)), name
    for name, it in (("part", torch.int32), ("trust", torch.int32), ("stat", torch.int64), ("state", torch.int32)):
        assert torch.equal(getattr(again.plan, name).view(it), getattr(case.plan, name).view(it)), name


def test_no_tensors_launch_nothing():
    hip, lay = _hip(), LAY.layout()
    for tensors in ([], [(0, 0, True), (64, 0, False)]):
        case = _Case(5.0)
        hyper0, state0 = case.hyper.cpu().numpy().copy(), case.plan.state.cpu().numpy().copy()
        case.plan = hip.LambPlan(tensors, "cuda")
        case.plan.state.copy_(_dev(state0))
        assert case.plan.nblocks == 0
        case.plan.part.fill_(-1.0)
        case.run(False)
        for name in LAY.NAMES:
            assert _same_bits(case.host(name), lay[name]), name
        assert bool((case.plan.part == -1.0).all())
        assert _same_bits(case.hyper.cpu().numpy(), hyper0) and _same_bits(case.plan.state.cpu().numpy(), state0)     # not even the tick


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_skipped_step_keeps_every_bit(bad):
    """The loss-scaled form with a non-finite squared norm: w, m, v, vhat, t, the state, the slots, trust and stat keep their bits.  With
    a finite one it is the plain form."""
    lay = LAY.layout()
    case = _Case(5.0, normsq=bad, ls=True)
    case.plan.trust.copy_(_dev(np.arange(10, dtype=np.float32) + 2)); case.plan.stat.copy_(_dev(np.arange(30, dtype=np.float64).reshape(10, 3) - 7))
    keep = {k: getattr(case.plan, k).cpu().numpy().copy() for k in ("part", "trust", "stat", "state")}
    hyper0 = case.hyper.cpu().numpy().copy()
    case.run(False)
    for name in LAY.NAMES:
        assert _same_bits(case.host(name), lay[name]), name
    for k, a in keep.items():
        assert _same_bits(getattr(case.plan, k).cpu().numpy(), a), k
    assert _same_bits(case.hyper.cpu().numpy(), hyper0) and hyper0[5] == 3
    # the same launches with a finite norm perform the step: the guard looks at the norm alone
    case.normsq.copy_(_dev(np.array([lay["normsq"]], dtype=np.float32)))
    case.run(False)
    ew, em, ev, eh, ehyper, estate, etrust, estat = LAY.reference(5.0, False, guard=True)[0]
    used = lay["used"]
    for name, e in (("w", ew), ("m", em), ("v", ev), ("vhat", eh)):
        assert _same_bits(case.host(name)[used], e[used]), name
    assert _same_bits(case.plan.trust.cpu().numpy(), etrust) and _same_bits(case.plan.stat.cpu().numpy(), estat)
    assert _same_bits(case.hyper.cpu().numpy(), ehyper) and _same_bits(case.plan.state.cpu().numpy(), estate)


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(seed=3, dtype="float32", optimizer="Adam", **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM)
    cfg.OPTIMIZER = optimizer
    for key, val in cfgkw.items():
        setattr(cfg, key, val)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(seed):
    if seed not in _batches:
        img, loc, ori, _ = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)
        _batches[seed] = (img, loc, ori)
    return _batches[seed]


def _tensors(eng):
    B = _B()
    return [(o, n, B.adapts(shape)) for (o, n, shape) in eng.slices.values()]


class _Host(object):
    """The host's copy of everything the three launches write, advanced by lamb.step32."""
    NAMES = (("w", "flat_w"), ("m", "flat_v"), ("v", "flat_v2"), ("vhat", "flat_vhat"), ("hyper", "hyper"), ("state", "lamb_state"))

    def __init__(self, eng):
        for k, attr in self.NAMES:
            setattr(self, k, getattr(eng, attr).cpu().numpy().copy())

    def unchanged(self, eng):
        return all(_same_bits(getattr(eng, attr).cpu().numpy(), getattr(self, k)) for k, attr in self.NAMES)

    def advance(self, eng, eta, eps=1e-8, clip_mode=False, guard=False):
        """step32 with the engine's gradient and norm; asserts the engine holds its bits.  Returns (trust, stat)."""
        g, normsq = eng.flat_g.cpu().numpy(), np.float32(eng.normsq.cpu().numpy()[0])
        assert np.isfinite(normsq) and normsq > 0
        res = _B().step32(self.w, g, self.m, self.v, self.vhat, _tensors(eng), self.hyper, self.state, normsq, eta, eps, clip_mode, guard)
        w0 = self.w
        self.w, self.m, self.v, self.vhat, self.hyper, self.state = res[:6]
        for k, attr in self.NAMES:
            assert _same_bits(getattr(eng, attr).cpu().numpy(), getattr(self, k)), attr
        assert not _same_bits(self.w, w0)
        return res[6], res[7]


def _check_report(eng, trust, stat):
    rep = eng.lamb_report()
    assert list(rep) == list(eng.slices) and eng.lars_report() is None
    for t, key in enumerate(eng.slices):
        nw, nr, tr = rep[key]
        assert (nw, nr) == (float(stat[t, 0]), float(stat[t, 1])) and np.float32(tr) == trust[t], key
    kernels = eng.lamb_report(adapting_only=True)
    assert set(kernels) == {key for key, (_o, _n, shape) in eng.slices.items() if len(shape) >= 2} and 0 < len(kernels) < len(rep)
    return rep


@pytest.mark.parametrize("variant", ["plain", "accum", "ema", "clip"])
def test_engine_steps_are_step32_bit_for_bit(variant):
    B = _B()
    from ursonet_amd import lars as L
    kw = dict(LAMB=1.0, GRADIENT_CLIP_NORM=5.0)
    if variant == "accum":
        kw["GRAD_ACCUM_STEPS"] = 2
    if variant == "ema":
        kw["WEIGHT_EMA"] = 0.9
    if variant == "clip":
        kw.update(LAMB=0.05, LAMB_CLIP=True, LAMB_EPS=0.0)
    eng, cfg = _engine(**kw)
    eta, eps, clip_mode = B.validate(cfg)
    k = 2 if variant == "accum" else 1
    want_opt = (["grad_close"] if k > 1 else []) + ["sqnorm", "lamb_moments", "lamb_trust", "lamb_apply"] + (["ema"] if variant == "ema" else [])
    assert eng.labels["opt"] == want_opt
    assert eng.lamb_plan.nblocks == sum(L.chunks(n) for _o, n, _s in eng.slices.values()) and eng.lars_plan is None
    assert eng.lamb_state.tolist() == [1.0, 1.0, 0.0] and eng.hyper.numel() == 8 and eng.lamb_plan.state is eng.lamb_state
    host = _Host(eng)
    ema = eng.flat_ema.cpu().numpy().copy() if variant == "ema" else None
    if variant == "ema":
        from ursonet_amd import weight_ema as WE
        state = WE.initial_state(cfg)
    seed = 11
    for step in range(3):
        for micro in range(k):
            eng.load_batch(*_batch(seed)); seed += 1
            eng.step()
            torch.cuda.synchronize()
            if micro < k - 1:                                                # weights, moments and the tick move only at the close
                assert host.unchanged(eng)
        trust, stat = host.advance(eng, eta, eps, clip_mode)
        assert host.hyper[5] == step + 1
        rep = _check_report(eng, trust, stat)
        tr = [r[2] for key, r in rep.items() if len(eng.slices[key][2]) >= 2]
        if step == 0 and variant != "clip":                                  # the layers really differ: that is what the rule is for
            assert max(tr) > min(tr) > 0
            s = B.summary(eng.lamb_report(adapting_only=True))
            assert s["min"] == min(tr) and s["max"] == max(tr) and s["tensors"] == len(tr)
        if variant == "clip":
            assert 0 < min(tr) and max(tr) <= 1
        if variant == "ema":                                                 # the average follows the LAMB-updated weights
            ema = WE.update32(ema, host.w, state[WE.NEXT_DECAY])
            state = WE.next_state(state)
            assert _same_bits(eng.flat_ema.cpu().numpy(), ema)
    # reset_optimizer: the moments, t and the state are as before the first step
    eng.reset_optimizer()
    assert eng.lamb_state.tolist() == [1.0, 1.0, 0.0] and float(eng.hyper[5]) == 0 and not bool(eng.flat_v.any()) and not bool(eng.flat_vhat.any())


def test_fp16_steps_that_overflow_move_nothing_then_the_next_one_does():
    """fp16 under a dynamic LOSS_SCALE that begins at 2^24: the scaled head gradients are past 65504, the first replays overflow and are
    skipped -- nothing moves, the tick included -- while the scale halves; the first finite step is step32 of the untouched state."""
    B = _B()
    eng, cfg = _engine(dtype="float16", LAMB=1.0, GRADIENT_CLIP_NORM=5.0, LOSS_SCALE="dynamic", LOSS_SCALE_INIT=2.0 ** 24)
    assert eng.labels["opt"] == ["sqnorm", "lamb_moments", "lamb_trust", "lamb_apply", "loss_scale"]
    host = _Host(eng)
    trust0, stat0 = eng.lamb_plan.trust.cpu().numpy().copy(), eng.lamb_plan.stat.cpu().numpy().copy()
    skipped = 0
    for s in range(26):                                                      # 2^24 halves to 1 in 24 steps: the loop ends long before
        eng.load_batch(*_batch(11 + s))
        eng.step()
        torch.cuda.synchronize()
        if not eng.loss_scale()["last_step_skipped"]:
            break
        skipped += 1
        assert not bool(torch.isfinite(eng.normsq).all()) and host.unchanged(eng)
        assert _same_bits(eng.lamb_plan.trust.cpu().numpy(), trust0) and _same_bits(eng.lamb_plan.stat.cpu().numpy(), stat0)
    assert 1 <= skipped < 25 and eng.loss_scale()["skipped_total"] == skipped
    trust, stat = host.advance(eng, 1.0, guard=True)
    assert host.hyper[5] == 1 and host.state[0] == host.hyper[1]              # the first tick: the skipped steps did not count
    _check_report(eng, trust, stat)


def test_graph_replay_equals_the_eager_step():
    a, _ = _engine(LAMB=1.0, GRADIENT_CLIP_NORM=5.0)
    b, _ = _engine(LAMB=1.0, GRADIENT_CLIP_NORM=5.0)
    a.load_batch(*_batch(11))
    a.capture()
    torch.cuda.synchronize()
    assert a.lamb_state.tolist() == [1.0, 1.0, 0.0] and float(a.hyper[5]) == 0          # the warm-up step is undone, the tick included
    assert torch.equal(a.flat_w.view(torch.int32), b.flat_w.view(torch.int32)) and not bool(a.flat_v.any())
    for s in range(3):
        for eng in (a, b):
            eng.load_batch(*_batch(11 + s))
        a.step()
        b.step_eager()
    torch.cuda.synchronize()
    for name in ("flat_w", "flat_v", "flat_v2", "flat_vhat", "flat_g", "hyper", "lamb_state", "loss_buf"):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert torch.equal(a.lamb_plan.stat.view(torch.int64), b.lamb_plan.stat.view(torch.int64)) and float(a.hyper[5]) == 3
    # save / restore carry the state
    st = a.save_train_state()
    a.load_batch(*_batch(20)); a.step(); torch.cuda.synchronize()
    assert float(a.hyper[5]) == 4 and not torch.equal(a.lamb_state, b.lamb_state)
    a.restore_train_state(st)
    assert torch.equal(a.lamb_state.view(torch.int32), b.lamb_state.view(torch.int32)) and float(a.hyper[5]) == 3
    assert torch.equal(a.flat_w.view(torch.int32), b.flat_w.view(torch.int32))


def test_frozen_layers_keep_trust_one_and_do_not_move():
    eng, _ = _engine(LAMB=1.0)
    state = eng.lamb_state
    eng.set_trainable(r"(bottleneck_layer|loc_.*|ori_.*)")
    assert eng.labels["opt"][-3:] == ["lamb_moments", "lamb_trust", "lamb_apply"]
    assert eng.lamb_state is state and eng.lamb_plan.state is state           # a rebuilt plan keeps the tick's state
    frozen = [key for key in eng.slices if not eng.layer_trainable[key[0]]]
    assert frozen and len(frozen) < len(eng.slices)
    w0 = eng.flat_w.cpu().numpy().copy()
    eng.load_batch(*_batch(11))
    eng.step()
    torch.cuda.synchronize()
    rep = eng.lamb_report()
    w1, m1, h1 = eng.flat_w.cpu().numpy(), eng.flat_v.cpu().numpy(), eng.flat_vhat.cpu().numpy()
    for key in frozen:
        o, n, _shape = eng.slices[key]
        assert rep[key][1] == 0 and rep[key][2] == 1 and _same_bits(w1[o:o + n], w0[o:o + n]) and not m1[o:o + n].any() and not h1[o:o + n].any(), key
    assert not _same_bits(w1, w0)


def test_off_is_off():
    """With LAMB = None the plan is launch for launch that of a config without the key -- plain Adam -- and so are the weights after three
    steps, against the plain launch driven by hand from the same gradients."""
    from ursonet_amd.config import Config
    hip = _hip()
    unset, cfg0 = _engine()
    for key in ("LAMB", "LAMB_EPS", "LAMB_CLIP"):
        assert key not in vars(cfg0) and hasattr(Config, key)
    off, _ = _engine(LAMB=None, LAMB_EPS=0.5, LAMB_CLIP=True)               # the other two keys alone change nothing
    assert off.labels == unset.labels and off.labels["opt"] == ["sqnorm", "adam"]
    assert off.lamb_plan is None and off.lamb_state is None and off.lamb_report() is None and off.lars_report() is None
    assert len(off.save_train_state()) == len(unset.save_train_state()) == 6
    # the parent's Adam bits: urso_adam_amsgrad_clip on copies, from each step's gradient and norm
    w, m, v, vhat, hyper = (x.clone() for x in (off.flat_w, off.flat_v, off.flat_v2, off.flat_vhat, off.hyper))
    for s in (11, 12, 13):
        for eng in (unset, off):
            eng.load_batch(*_batch(s))
            eng.step()
        torch.cuda.synchronize()
        hip.adam_amsgrad_clip(off.n_flat, w, off.flat_g, m, v, vhat, hyper, off.normsq)
        torch.cuda.synchronize()
        assert torch.equal(w.view(torch.int32), off.flat_w.view(torch.int32)), s
    for name in ("flat_w", "flat_v", "flat_v2", "flat_vhat", "flat_g", "loss_buf", "flat_stats", "hyper"):
        a, b = getattr(unset, name), getattr(off, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    sgd, _ = _engine(optimizer="SGD")
    assert sgd.labels["opt"] == ["sqnorm", "sgd"] and sgd.lamb_plan is None
    on, _ = _engine(LAMB=1.0, LOSS_SCALE=1024.0)
    assert on.labels["opt"] == ["sqnorm", "lamb_moments", "lamb_trust", "lamb_apply", "loss_scale"]
    assert {p: l for p, l in on.labels.items() if p != "opt"} == {p: l for p, l in unset.labels.items() if p != "opt"}
    from ursonet_amd.engine import Engine
    cfg0.LAMB = "nonsense"
    inf = Engine(cfg0, "inference", seed=3)
    assert inf.lamb_plan is None and inf.lamb_report() is None               # inference ignores the key


def test_sgd_lars_and_a_launcher_raise():
    from ursonet_amd.engine import Engine
    for kw, world in ((dict(OPTIMIZER="SGD"), 1), (dict(LARS=0.001), 1), (dict(LARS=0.001, OPTIMIZER="SGD"), 1), (dict(), 2)):
        cfg = make_config(dtype="float32", **GEOM)
        cfg.OPTIMIZER, cfg.LAMB = "Adam", 1.0
        for key, val in kw.items():
            setattr(cfg, key, val)
        with pytest.raises(ValueError, match="LAMB"):
            if world == 1:
                Engine(cfg, "training", seed=3)
            else:
                _B().validate(cfg, world=world)
    import types
    from ursonet_amd import dp
    eng, _ = _engine(LAMB=1.0)
    orig = dp.dist.get_world_size
    dp.dist.get_world_size = lambda group=None: 2
    try:
        with pytest.raises(ValueError, match="LAMB.*data parallelism.*world size 2"):
            dp.DataParallelEngine(eng, comm_cus=0)
    finally:
        dp.dist.get_world_size = orig


def test_train_logs_the_trust_ratios_once_per_epoch(tmp_path, capsys):
    import re
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    B = _B()
    cfg = make_config(dtype="float32", lr=0.001, **GEOM)
    cfg.NAME = "lamb"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 1
    cfg.OPTIMIZER, cfg.LAMB = "Adam", 1.0
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    eng = model._engine
    w0 = eng.flat_w.clone()
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    out = capsys.readouterr().out
    lines = re.findall(r"^epoch (\d)  lamb trust  min (\S+)  median (\S+)  max (\S+)  \((\d+) kernels\)$", out, re.M)
    assert [l[0] for l in lines] == ["1", "2"], out
    assert "lars trust" not in out
    s = B.summary(eng.lamb_report(adapting_only=True))                       # the last step's table is the second line's
    assert (float(lines[1][1]), float(lines[1][2]), float(lines[1][3])) == tuple(float("%.3e" % s[k]) for k in ("min", "median", "max"))
    assert int(lines[1][4]) == s["tensors"] and 0 < s["min"] <= s["median"] <= s["max"]
    assert len(hist.loc_loss_acc) == 4 and np.isfinite(hist.loc_loss_acc).all()
    assert bool(torch.isfinite(eng.flat_w).all()) and not torch.equal(eng.flat_w, w0)
    assert eng.labels["opt"][-3:] == ["lamb_moments", "lamb_trust", "lamb_apply"]      # set_trainable("all") rebuilt the plan with the launches
    assert float(eng.hyper[5]) == 4                                          # ... and kept the tick: four steps
