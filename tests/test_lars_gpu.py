"""Layer-wise adaptive rate scaling on the GPU (Config.LARS).

Kernel level: urso_lars_norms, urso_lars_trust and urso_lars_sgd bit for bit against ursonet_amd.lars (slot_sums32, norms64, trust32,
update32, step32) over one flat buffer of ten tensors at the sizes where the kernels take another path -- a single element, the ragged
end on each side of a 16-byte access, less than a wave, less than a chunk, a chunk, a chunk and one, several chunks with a whole and
with a short last one -- with a sentinel in the padding between them, a tensor whose gradient is zero, one whose weights are zero, two
that do not adapt; clip factor 1 and below 1, LARS_CLIP on and off, T = 0, and the skipped step of the loss-scaled form.
Engine level (resnet18, 64 x 64, batch 2, the engine of the WEIGHT_EMA and GRAD_ACCUM_STEPS tests): after every step() the weights and
the momentum are lars.step32 of the previous ones, this step's gradient and the engine's norm, bit for bit, and lars_report() is that
step's table; the same under GRAD_ACCUM_STEPS = 2 and WEIGHT_EMA; frozen layers keep trust 1 and do not move; with the key off the plan
and the weights are the parent's; UrsoNet.train() prints the trust summary once per epoch."""
import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 1023, 4096, 4097, 2 * 4096 + 4, 3 * 4096]
ZERO_G, ZERO_W, PLAIN = 5, 6, (2, 7)           # tensor indices: g == 0 | w == 0 | the two that do not adapt
SENTINEL = 0x7FA5A5A5                          # a NaN with a payload: an arithmetic pass over the padding would show, and so would a store
GUARD = 64                                     # floats in front of and behind the tensors (the buffers stay 16-byte aligned)


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _L():
    from ursonet_amd import lars
    return lars


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


_layout_cache = {}


def _layout():
    """The ten tensors in one flat buffer, padded offsets (a multiple of 4 floats, as the engine lays its slices), the host's random w, g
    and v with the sentinel everywhere else.  Computed once and shared; the tests copy what they change."""
    if not _layout_cache:
        rng = np.random.default_rng(19)
        tensors, off = [], GUARD
        for t, n in enumerate(SIZES):
            tensors.append((off, n, t not in PLAIN))
            off += -(-n // 4) * 4 + (8 if t == 3 else 0)                     # (one wider gap: offsets need not be dense)
        total = off + GUARD
        used = np.zeros(total, dtype=bool)
        bufs = []
        for _ in range(3):
            x = np.full(total, SENTINEL, dtype=np.uint32).view(np.float32).copy()
            for o, n, _a in tensors:
                x[o:o + n] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
                used[o:o + n] = True
            bufs.append(x)
        w, g, v = bufs
        for t, (o, n, _a) in enumerate(tensors):                             # gradient scales over four decades: LARS_CLIP sees both sides of its min
            g[o:o + n] *= np.float32(10.0 ** ((t % 5) - 2))
        o, n, _a = tensors[ZERO_G]
        g[o:o + n] = 0
        o, n, _a = tensors[ZERO_W]
        w[o:o + n] = 0
        _layout_cache.update(tensors=tensors, total=total, used=used, w=w, g=g, v=v,
                             normsq=np.float32(np.square(g[used].astype(np.float64)).sum()))
    return _layout_cache


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(plan, w, g, v, hyper, normsq, eta, eps, clip_mode, ls=None):
    plan.norms(w, g)
    plan.trust_ratios(hyper, normsq, eta, eps, clip_mode, ls=ls)
    plan.sgd(w, g, v, hyper, normsq, ls=ls)
    torch.cuda.synchronize()


# ===================================================================================================================== kernel level
def test_plan_is_the_documented_block_map():
    hip, L, lay = _hip(), _L(), _layout()
    plan = hip.LarsPlan(lay["tensors"], "cuda")
    assert plan.T == 10 and plan.nblocks == sum(L.chunks(n) for n in SIZES) == 6 + 1 + 2 + 3 + 3
    assert plan.blockmap.cpu().tolist() == [[t, c] for t, n in enumerate(SIZES) for c in range(L.chunks(n))]
    assert plan.first.cpu().tolist() == list(np.cumsum([0] + [L.chunks(n) for n in SIZES]))
    assert plan.tab.cpu().tolist() == [[o, n] for o, n, _ in lay["tensors"]] and plan.adapt.cpu().tolist() == [int(a) for _, _, a in lay["tensors"]]
    assert all(o % 4 == 0 for o, _, _ in lay["tensors"])


@pytest.mark.parametrize("clip_mode", [False, True])
@pytest.mark.parametrize("clip", [0.0, 1e9, 1e4])
def test_three_launches_bit_for_bit(clip, clip_mode):
    """clip = 0 and 1e9: c = 1 (no clip, and one out of reach); clip = 1e4: c < 1 (the gradient's norm is about 3e4)."""
    hip, L, lay = _hip(), _L(), _layout()
    tensors, used = lay["tensors"], lay["used"]
    eta, eps = (0.001, 1e-8) if not clip_mode else (0.02, 0.0)
    hyper_h = np.array([0.01, 0.9, clip], dtype=np.float32)
    c = L.clip_factor32(lay["normsq"], hyper_h[2])
    assert (c < 1) == (clip == 1e4)
    w, g, v = _dev(lay["w"]), _dev(lay["g"]), _dev(lay["v"])
    hyper, normsq = _dev(hyper_h), _dev(np.array([lay["normsq"]], dtype=np.float32))
    plan = hip.LarsPlan(tensors, "cuda")
    plan.part.fill_(-1.0); plan.trust.fill_(-1.0); plan.stat.fill_(-1.0)
    _run(plan, w, g, v, hyper, normsq, eta, eps, clip_mode)
    # the slots
    part = plan.part.cpu().numpy()
    for t, (o, n, _a) in enumerate(tensors):
        s0, s1 = int(plan.first_h[t]), int(plan.first_h[t + 1])
        assert _same_bits(part[s0:s1, 0], L.slot_sums32(lay["w"][o:o + n])), ("w slots", t)
        assert _same_bits(part[s0:s1, 1], L.slot_sums32(lay["g"][o:o + n])), ("g slots", t)
    # trust, stat, w and v
    ew, ev, etrust, estat = L.step32(lay["w"], lay["g"], lay["v"], tensors, hyper_h, lay["normsq"], eta, eps, clip_mode)
    trust, stat = plan.trust.cpu().numpy(), plan.stat.cpu().numpy()
    assert _same_bits(stat, estat) and _same_bits(trust, etrust)
    gw, gv = w.cpu().numpy(), v.cpu().numpy()
    assert _same_bits(gw[used], ew[used]) and _same_bits(gv[used], ev[used])
    assert (_bits(gw[~used]) == SENTINEL).all() and (_bits(gv[~used]) == SENTINEL).all()        # padding and guards keep the sentinel
    assert _same_bits(g.cpu().numpy(), lay["g"])                              # g is only read
    # what the cases are there for
    assert trust[ZERO_G] == 1 and stat[ZERO_G, 1] == 0 and stat[ZERO_G, 0] > 0 and trust[ZERO_W] == 1 and stat[ZERO_W, 0] == 0
    for t in PLAIN:
        assert trust[t] == 1 and stat[t, 2] == 1 and stat[t, 0] > 0 and stat[t, 1] > 0
        o, n, _a = tensors[t]
        pw, pv = L.update32(lay["w"][o:o + n], lay["g"][o:o + n], lay["v"][o:o + n], hyper_h[0], hyper_h[1], c, np.float32(1))
        assert _same_bits(gw[o:o + n], pw) and _same_bits(gv[o:o + n], pv)    # the plain SGD update
    adapting = [t for t in range(len(SIZES)) if t not in PLAIN + (ZERO_G, ZERO_W)]
    assert all(trust[t] != 1 for t in adapting if not clip_mode) and all(0 < trust[t] <= 1 for t in adapting if clip_mode)
    if clip_mode:
        assert any(trust[t] == 1 for t in adapting) and any(trust[t] < 1 for t in adapting)      # both sides of the min
    # a second run from the same inputs gives the same bits
    w2, v2 = _dev(lay["w"]), _dev(lay["v"])
    plan2 = hip.LarsPlan(tensors, "cuda")
    _run(plan2, w2, g, v2, hyper, normsq, eta, eps, clip_mode)
    assert torch.equal(w2.view(torch.int32), w.view(torch.int32)) and torch.equal(v2.view(torch.int32), v.view(torch.int32))
    assert torch.equal(plan2.part.view(torch.int32), plan.part.view(torch.int32))
    assert torch.equal(plan2.stat.view(torch.int64), plan.stat.view(torch.int64)) and torch.equal(plan2.trust.view(torch.int32), plan.trust.view(torch.int32))


def test_no_tensors_launch_nothing():
    hip, lay = _hip(), _layout()
    w, g, v = _dev(lay["w"]), _dev(lay["g"]), _dev(lay["v"])
    hyper, normsq = _dev(np.array([0.01, 0.9, 5.0], dtype=np.float32)), _dev(np.array([lay["normsq"]], dtype=np.float32))
    for tensors in ([], [(0, 0, True), (64, 0, False)]):
        plan = hip.LarsPlan(tensors, "cuda")
        assert plan.nblocks == 0
        plan.part.fill_(-1.0)
        _run(plan, w, g, v, hyper, normsq, 0.001, 1e-8, False)
        assert _same_bits(w.cpu().numpy(), lay["w"]) and _same_bits(v.cpu().numpy(), lay["v"]) and bool((plan.part == -1.0).all())


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_skipped_step_keeps_every_bit(bad):
    """The loss-scaled form with a non-finite squared norm: w, v, trust and stat keep their bits.  With a finite one it is the plain form."""
    hip, L, lay = _hip(), _L(), _layout()
    tensors = lay["tensors"]
    hyper_h = np.array([0.01, 0.9, 5.0], dtype=np.float32)
    w, g, v = _dev(lay["w"]), _dev(lay["g"]), _dev(lay["v"])
    hyper = _dev(hyper_h)
    ls = _dev(np.array([1024.0, 1.0 / 1024.0, 0, 2000, 1, 65536, 0, 0], dtype=np.float32))
    plan = hip.LarsPlan(tensors, "cuda")
    plan.trust.copy_(_dev(np.arange(10, dtype=np.float32) + 2)); plan.stat.copy_(_dev(np.arange(30, dtype=np.float64).reshape(10, 3) - 7))
    trust0, stat0 = plan.trust.cpu().numpy().copy(), plan.stat.cpu().numpy().copy()
    _run(plan, w, g, v, hyper, _dev(np.array([bad], dtype=np.float32)), 0.001, 1e-8, False, ls=ls)
    assert _same_bits(w.cpu().numpy(), lay["w"]) and _same_bits(v.cpu().numpy(), lay["v"])
    assert _same_bits(plan.trust.cpu().numpy(), trust0) and _same_bits(plan.stat.cpu().numpy(), stat0)
    # the same launches with a finite norm perform the step: the guard looks at the norm alone
    _run(plan, w, g, v, hyper, _dev(np.array([lay["normsq"]], dtype=np.float32)), 0.001, 1e-8, False, ls=ls)
    ew, ev, etrust, estat = L.step32(lay["w"], lay["g"], lay["v"], tensors, hyper_h, lay["normsq"], 0.001, 1e-8, False, guard=True)
    used = lay["used"]
    assert _same_bits(w.cpu().numpy()[used], ew[used]) and _same_bits(v.cpu().numpy()[used], ev[used])
    assert _same_bits(plan.trust.cpu().numpy(), etrust) and _same_bits(plan.stat.cpu().numpy(), estat)


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(seed=3, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype="float32", **GEOM)
    for key, val in cfgkw.items():
        setattr(cfg, key, val)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(seed):
    if seed not in _batches:
        img, loc, ori, _ = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)
        _batches[seed] = (img, loc, ori)
    return _batches[seed]


def _flat_grads(eng):
    """This step's gradient as get_grads() returns it, laid back into the flat buffer's slices (zeros in the padding, as flat_g has)."""
    g = np.zeros(eng.flat_g.numel(), dtype=np.float32)
    grads = eng.get_grads()
    for (ln, wn), (o, n, _shape) in eng.slices.items():
        g[o:o + n] = grads[ln][wn].reshape(-1)
    assert _same_bits(g, eng.flat_g.cpu().numpy())
    return g


def _tensors(eng):
    L = _L()
    return [(o, n, L.adapts(shape)) for (o, n, shape) in eng.slices.values()]


def _check_report(eng, trust, stat):
    rep = eng.lars_report()
    assert list(rep) == list(eng.slices)
    for t, key in enumerate(eng.slices):
        nw, ng, tr = rep[key]
        assert (nw, ng) == (float(stat[t, 0]), float(stat[t, 1])) and np.float32(tr) == trust[t], key
    kernels = eng.lars_report(adapting_only=True)
    assert set(kernels) == {key for key, (_o, _n, shape) in eng.slices.items() if len(shape) >= 2} and 0 < len(kernels) < len(rep)
    return rep


@pytest.mark.parametrize("variant", ["plain", "accum", "ema"])
def test_engine_steps_are_step32_bit_for_bit(variant):
    L = _L()
    kw = dict(LARS=0.001, GRADIENT_CLIP_NORM=5.0)
    if variant == "accum":
        kw["GRAD_ACCUM_STEPS"] = 2
    if variant == "ema":
        kw["WEIGHT_EMA"] = 0.9
    eng, cfg = _engine(**kw)
    k = 2 if variant == "accum" else 1
    want_opt = (["grad_close"] if k > 1 else []) + ["sqnorm", "lars_norms", "lars_trust", "lars_sgd"] + (["ema"] if variant == "ema" else [])
    assert eng.labels["opt"] == want_opt
    assert eng.lars_plan.nblocks == sum(L.chunks(n) for _o, n, _s in eng.slices.values())
    tensors = _tensors(eng)
    hyper = eng.hyper.cpu().numpy()
    w, v = eng.flat_w.cpu().numpy().copy(), eng.flat_v.cpu().numpy().copy()
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
            if micro < k - 1:                                                # weights move only at the close
                assert _same_bits(eng.flat_w.cpu().numpy(), w) and _same_bits(eng.flat_v.cpu().numpy(), v)
        g = _flat_grads(eng)
        normsq = np.float32(eng.normsq.cpu().numpy()[0])
        assert np.isfinite(normsq) and normsq > 0
        w2, v2, trust, stat = L.step32(w, g, v, tensors, hyper, normsq, 0.001, 1e-8, False)
        assert _same_bits(eng.flat_w.cpu().numpy(), w2), "flat_w after step %d" % step
        assert _same_bits(eng.flat_v.cpu().numpy(), v2), "flat_v after step %d" % step
        assert not _same_bits(w2, w)
        rep = _check_report(eng, trust, stat)
        if step == 0:                                                        # the layers really differ: that is what the rule is for
            tr = [r[2] for key, r in rep.items() if len(eng.slices[key][2]) >= 2]
            assert max(tr) > min(tr) > 0
            s = L.summary(eng.lars_report(adapting_only=True))
            assert s["min"] == min(tr) and s["max"] == max(tr) and s["tensors"] == len(tr)
        if variant == "ema":                                                 # the average follows the LARS-updated weights
            ema = WE.update32(ema, w2, state[WE.NEXT_DECAY])
            state = WE.next_state(state)
            assert _same_bits(eng.flat_ema.cpu().numpy(), ema)
        w, v = w2, v2


def test_frozen_layers_keep_trust_one_and_do_not_move():
    L = _L()
    eng, _ = _engine(LARS=0.001)
    eng.set_trainable(r"(bottleneck_layer|loc_.*|ori_.*)")
    assert eng.labels["opt"][-3:] == ["lars_norms", "lars_trust", "lars_sgd"]
    frozen = [key for key in eng.slices if not eng.layer_trainable[key[0]]]
    assert frozen and len(frozen) < len(eng.slices)
    w0 = eng.flat_w.cpu().numpy().copy()
    eng.load_batch(*_batch(11))
    eng.step()
    torch.cuda.synchronize()
    rep = eng.lars_report()
    w1, v1 = eng.flat_w.cpu().numpy(), eng.flat_v.cpu().numpy()
    for key in frozen:
        o, n, _shape = eng.slices[key]
        assert rep[key][1] == 0 and rep[key][2] == 1 and _same_bits(w1[o:o + n], w0[o:o + n]) and not v1[o:o + n].any(), key
    assert not _same_bits(w1, w0)


def test_off_is_off():
    """With LARS = None the plan is launch for launch that of a config without the key, and so are the weights after two steps."""
    from ursonet_amd.config import Config
    unset, cfg0 = _engine()
    for key in ("LARS", "LARS_EPS", "LARS_CLIP"):
        assert key not in vars(cfg0) and hasattr(Config, key)
    off, _ = _engine(LARS=None, LARS_EPS=0.5, LARS_CLIP=True)               # the other two keys alone change nothing
    assert off.labels == unset.labels and off.labels["opt"] == ["sqnorm", "sgd"]
    assert off.lars_plan is None and off.lars_report() is None
    for eng in (unset, off):
        for s in (11, 12):
            eng.load_batch(*_batch(s))
            eng.step()
    torch.cuda.synchronize()
    for name in ("flat_w", "flat_v", "flat_g", "loss_buf", "flat_stats"):
        a, b = getattr(unset, name), getattr(off, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    on, _ = _engine(LARS=0.001, LOSS_SCALE=1024.0)
    assert on.labels["opt"] == ["sqnorm", "lars_norms", "lars_trust", "lars_sgd", "loss_scale"]
    assert {p: l for p, l in on.labels.items() if p != "opt"} == {p: l for p, l in unset.labels.items() if p != "opt"}
    from ursonet_amd.engine import Engine
    cfg0.LARS = "nonsense"
    inf = Engine(cfg0, "inference", seed=3)
    assert inf.lars_plan is None and inf.lars_report() is None               # inference ignores the key
    cfg0.LARS, cfg0.OPTIMIZER = 0.001, "ADAM"
    with pytest.raises(ValueError, match="LAMB"):
        Engine(cfg0, "training", seed=3)


def test_train_logs_the_trust_ratios_once_per_epoch(tmp_path, capsys):
    import re
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    L = _L()
    cfg = make_config(dtype="float32", lr=0.01, **GEOM)
    cfg.NAME = "lars"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 1
    cfg.LARS = 0.001
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    eng = model._engine
    w0 = eng.flat_w.clone()
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    out = capsys.readouterr().out
    lines = re.findall(r"^epoch (\d)  lars trust  min (\S+)  median (\S+)  max (\S+)  \((\d+) kernels\)$", out, re.M)
    assert [l[0] for l in lines] == ["1", "2"], out
    s = L.summary(eng.lars_report(adapting_only=True))                       # the last step's table is the second line's
    assert (float(lines[1][1]), float(lines[1][2]), float(lines[1][3])) == tuple(float("%.3e" % s[k]) for k in ("min", "median", "max"))
    assert int(lines[1][4]) == s["tensors"] and 0 < s["min"] <= s["median"] <= s["max"]
    assert len(hist.loc_loss_acc) == 4 and np.isfinite(hist.loc_loss_acc).all()
    assert bool(torch.isfinite(eng.flat_w).all()) and not torch.equal(eng.flat_w, w0)
    assert eng.labels["opt"][-3:] == ["lars_norms", "lars_trust", "lars_sgd"]      # set_trainable("all") rebuilt the plan with the launches
