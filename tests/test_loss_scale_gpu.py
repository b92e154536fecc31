"""Loss scaling on the GPU (Config.LOSS_SCALE).

Kernel level: the scaled loss entry points against the plain ones bit for bit (scale 1, scale 2**10), the scaled cross-entropy
at the model's own size against a float64 reference (the rounded-once bound of tests/exactprobe.py), the update rule against
ursonet_amd.loss_scale.next_state, the guarded optimizers.
Engine level (resnet18, 64 x 128, batch 3): a static scale of 1024 leaves every weight and momentum bit where the unscaled step
leaves it (fp32, bf16: a missed unscale or a scale applied after the rounding fails here), an overflowed fp16 step is skipped and
the dynamic scale recovers, and an orientation gradient that unscaled fp16 loses entirely comes back as exact as fp16 gets."""
import numpy as np
import pytest
import torch

import exactprobe as X
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _LS():
    from ursonet_amd import loss_scale
    return loss_scale


def dev(t):
    return t.contiguous().to(torch.float32).cuda()


def _state(scale, interval=0.0, lo=None, hi=None):
    lo = scale if lo is None else lo
    hi = scale if hi is None else hi
    return torch.tensor([scale, 1.0 / scale, 0.0, interval, lo, hi, 0.0, 0.0], dtype=torch.float32, device="cuda")


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ===================================================================================================================== kernel level
def _loss_cases():
    """(name, run(ls) -> (dz fp32 tensor, loss fp32[1])) for every scaled loss entry point: B = 3; cross-entropy K = 64 / 4096, once
    with relu_mask; the regression losses D = 3 and 4 in rows padded to 8."""
    hip = _hip()
    B = 3
    cases = []
    for K, relu in ((64, 0), (4096, 1), (64, 1), (4096, 0)):
        z, p = X.xent_inputs(B, K, 1.0, seed=K + relu)
        zd, pd = dev(z), dev(p)

        def run(ls, K=K, relu=relu, zd=zd, pd=pd):
            dz = torch.full((B, K), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
            hip.softmax_xent(B, K, zd, pd, 0.7, relu, F32, loss, dz, torch.empty(B, device="cuda"), ls=ls)
            return dz, loss
        cases.append(("xent K=%d relu=%d" % (K, relu), run))
    g = torch.Generator().manual_seed(5)
    for D in (3, 4):
        gt = torch.randn(B, D, generator=g)
        pred = torch.zeros(B, 8); pred[:, :D] = gt + 0.3 * torch.randn(B, D, generator=g)
        gtd, pd = dev(gt), dev(pred)

        def rel(ls, D=D, gtd=gtd, pd=pd):
            d = torch.full((B, 8), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
            hip.rel_l2(B, D, 8, gtd, pd, 1.3, F32, loss, d, torch.empty(2, device="cuda"), ls=ls)
            return d, loss

        def mse(ls, D=D, gtd=gtd, pd=pd):
            d = torch.full((B, 8), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
            hip.mse(B, D, 8, gtd, pd, 1.3, F32, loss, d, ls=ls)
            return d, loss

        def absdot(ls, D=D, gtd=gtd, pd=pd):
            d = torch.full((B, 8), float("nan"), device="cuda"); loss = torch.full((1,), float("nan"), device="cuda")
            hip.absdot(B, D, 8, 1 if D == 4 else 0, gtd, pd, 1.3, F32, torch.empty(B, D, device="cuda"), loss, d, ls=ls)
            return d, loss
        cases += [("rel_l2 D=%d" % D, rel), ("mse D=%d" % D, mse), ("absdot D=%d" % D, absdot)]
    return cases


def test_scaled_losses_are_the_plain_ones_times_a_power_of_two():
    """fp32 output: state scale 1 reproduces the plain entry point's dz and loss bits; scale 2**10 gives dz bits equal to 2**10 x the plain
    fp32 dz (a power of two commutes with the rounding; nothing here is near fp32's range limits) and the same loss bits."""
    one, big = _state(1.0), _state(1024.0)
    for name, run in _loss_cases():
        dz0, l0 = run(None)
        assert bool(torch.isfinite(dz0).all()) and bool(torch.isfinite(l0).all()), name
        assert float(dz0.abs().max()) > 0, name
        dz1, l1 = run(one)
        assert _same_bits(dz1, dz0) and _same_bits(l1, l0), name + ": scale 1"
        dzk, lk = run(big)
        assert _same_bits(dzk, dz0 * 1024.0), name + ": scale 2**10"
        assert _same_bits(lk, l0), name + ": the loss scalar must stay unscaled"
    torch.cuda.synchronize()
    assert one.tolist() == [1.0, 1.0, 0, 0, 1.0, 1.0, 0, 0] and big.tolist()[:2] == [1024.0, 1.0 / 1024]      # the losses only read the state


def test_scaled_cross_entropy_keeps_what_fp16_loses():
    """B = 32, K = 24**3, near-uniform PMF, fp16 gradient.  Premise (derived: (1 / K) / B = 2.3e-6 against fp16's smallest normal
    6.1e-5): more than half of the plain entry point's dz are below 2**-14.  With scale 2**15 every dz is the fp16 rounding of the float64
    gradient x 2**15 within the rounded-once bound (scale 2**15 on the gradient = weight x 2**15: the same fp32 factor, a power of two)."""
    hip = _hip()
    B, K, S = 32, 13824, 2.0 ** 15
    g = torch.Generator().manual_seed(24)
    z = torch.relu(0.05 * torch.randn(B, K, generator=g)).contiguous()                      # post-ReLU logits, softmax within a few % of uniform
    p = torch.softmax(0.05 * torch.randn(B, K, generator=g), 1).to(torch.float32).contiguous()
    zd, pd = dev(z), dev(p)
    row = torch.empty(B, device="cuda"); loss = torch.zeros(2, device="cuda")
    plain = torch.empty(B, K, dtype=torch.float16, device="cuda")
    hip.softmax_xent(B, K, zd, pd, 1.0, 0, F16, loss[0:1], plain, row)
    scaled = torch.empty(B, K, dtype=torch.float16, device="cuda")
    hip.softmax_xent(B, K, zd, pd, 1.0, 0, F16, loss[1:2], scaled, row, ls=_state(S))
    torch.cuda.synchronize()
    ref = X.softmax_xent64(z, p, 1.0, 0)[2]
    below = float((plain.float().abs() < 2.0 ** -14).sum()) / plain.numel()
    ref_sub = float((ref.abs() < 2.0 ** -14).sum()) / ref.numel()
    print("plain fp16 dz below 2**-14: %.4f of %d (float64 reference: %.4f); max |dz| %.3e" % (below, plain.numel(), ref_sub, float(ref.abs().max())))
    assert below > 0.5
    ref_s = X.softmax_xent64(z, p, S, 0)[2]
    assert bool(torch.equal(ref_s, ref * S))
    ratio = X.assert_within(scaled, ref_s, X.softmax_xent_bounds(z, p, S, 0, F16)[2], "scaled fp16 dz")
    print("scaled fp16 dz: largest ratio to the rounded-once bound %.3f; share below 2**-14: %.4f"
          % (ratio, float((scaled.float().abs() < 2.0 ** -14).sum()) / scaled.numel()))
    assert _same_bits(loss[0:1], loss[1:2])


def test_update_rule_on_the_device_follows_next_state():
    """urso_loss_scale_update over 12 hand-written norms (growth_interval 3) and a static state: every field equals next_state's."""
    hip, LS = _hip(), _LS()
    inf, nan = float("inf"), float("nan")
    norms = [1.0, 0.0, 3.0e38, 2.5, 7.0, 1e-30, inf, nan, -inf, inf, 4.0, 9.0]
    st = _state(8.0, interval=3.0, lo=2.0, hi=16.0)
    want = st.tolist()
    normsq = torch.zeros(1, device="cuda")
    scales = []
    for v in norms:
        normsq.fill_(v)
        hip.loss_scale_update(st, normsq)
        want = LS.next_state(want, bool(np.isfinite(v)))
        assert st.tolist() == want, (v, st.tolist(), want)
        scales.append(want[LS.SCALE])
    assert scales == [8, 8, 16, 16, 16, 16, 8, 4, 2, 2, 2, 2] and want[LS.SKIPPED_TOTAL] == 4          # growth, cap, halving, floor all occurred
    st = _state(1024.0)
    want = st.tolist()
    for v in (1.0, inf, nan, 2.0, 3.0, 4.0):
        normsq.fill_(v)
        hip.loss_scale_update(st, normsq)
        want = LS.next_state(want, bool(np.isfinite(v)))
        assert st.tolist() == want and want[LS.SCALE] == 1024.0


@pytest.mark.parametrize("n", [1027])
def test_guarded_optimizers_skip_a_non_finite_norm(n):
    """urso_sgd_momentum_clip_ls / urso_adam_amsgrad_clip_ls: a finite norm gives the plain entry point's bits; inf or NaN leaves w, v, m,
    vhat and Adam's t untouched (n = 1027: the 16-byte body and the ragged tail)."""
    hip = _hip()
    g0 = torch.Generator().manual_seed(3)
    w, g, v = (torch.randn(n, generator=g0).cuda() for _ in range(3))
    g[5] = float("inf")
    st = _state(1024.0)
    hyper = torch.tensor([0.01, 0.9, 5.0], device="cuda")
    for bad in (float("inf"), float("nan")):
        w1, v1 = w.clone(), v.clone()
        hip.sgd_momentum_clip(n, w1, g, v1, hyper, torch.tensor([bad], device="cuda"), ls=st)
        assert _same_bits(w1, w) and _same_bits(v1, v)
    g[5] = 0.5
    nsq = (g * g).sum().reshape(1)
    wa, va, wb, vb = w.clone(), v.clone(), w.clone(), v.clone()
    hip.sgd_momentum_clip(n, wa, g, va, hyper, nsq)
    hip.sgd_momentum_clip(n, wb, g, vb, hyper, nsq, ls=st)
    assert _same_bits(wa, wb) and _same_bits(va, vb) and not _same_bits(wa, w)
    ah = torch.tensor([0.01, 0.9, 0.999, 1e-7, 5.0, 3.0, 0.1, 0.001], device="cuda")
    m, v2, vh = torch.zeros(n, device="cuda"), torch.rand(n, generator=g0).cuda(), torch.rand(n, generator=g0).cuda()
    for bad in (float("inf"), float("nan")):
        w1, m1, v1, h1, a1 = w.clone(), m.clone(), v2.clone(), vh.clone(), ah.clone()
        hip.adam_amsgrad_clip(n, w1, g, m1, v1, h1, a1, torch.tensor([bad], device="cuda"), ls=st)
        assert _same_bits(w1, w) and _same_bits(m1, m) and _same_bits(v1, v2) and _same_bits(h1, vh) and _same_bits(a1, ah)
    outs = []
    for ls in (None, st):
        w1, m1, v1, h1, a1 = w.clone(), m.clone(), v2.clone(), vh.clone(), ah.clone()
        hip.adam_amsgrad_clip(n, w1, g, m1, v1, h1, a1, nsq, ls=ls)
        outs.append((w1, m1, v1, h1, a1))
    assert all(_same_bits(a, b) for a, b in zip(*outs)) and float(outs[1][4][5]) == 4.0 and not _same_bits(outs[1][0], w)


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=128, batch=3)
HEADS = {
    "quat_regloc": dict(regress_ori=True, regress_loc=True),                                  # abs-dot + rel-l2
    "softclass": dict(regress_ori=False, regress_loc=False, ori_bins=8, loc_bins=4),          # cross-entropy on both heads
    "keypoints": dict(keypoints=True),                                                        # three MSE heads
    "softclass_ori": dict(regress_ori=False, regress_loc=True, ori_bins=8),                   # rel-l2 + cross-entropy over 8**3 bins
}


def _engine(heads, dtype, loss_scale=None, optimizer="SGD", train_bn=False, seed=3, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM, **HEADS[heads])
    cfg.OPTIMIZER = optimizer
    cfg.TRAIN_BN = train_bn
    cfg.LOSS_SCALE = loss_scale
    for k, v in cfgkw.items():
        setattr(cfg, k, v)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(heads, seed):
    """The same synthetic batches for every engine of a head set (computed once)."""
    if (heads, seed) not in _batches:
        cfg = make_config(dtype="float32", **GEOM, **HEADS[heads])
        img, loc, ori, _ = synthetic_batch(cfg, 3, seed=seed)
        if heads == "keypoints":
            rng = np.random.default_rng(seed)
            k2, k3 = (loc + rng.normal(0, 0.5, loc.shape)).astype(np.float32), (loc + rng.normal(0, 0.5, loc.shape)).astype(np.float32)
            _batches[(heads, seed)] = (img, loc, k2, k3)
        else:
            _batches[(heads, seed)] = (img, loc, ori)
    return _batches[(heads, seed)]


def _opt_state(eng):
    t = [eng.flat_w, eng.flat_v, eng.flat_g, eng.loss_buf]
    if eng.adam:
        t += [eng.flat_v2, eng.flat_vhat, eng.hyper]
    return t


@pytest.mark.parametrize("heads,dtype,optimizer,train_bn", [
    ("quat_regloc", "float32", "SGD", False), ("quat_regloc", "bfloat16", "SGD", False),
    ("softclass", "float32", "SGD", False), ("softclass", "bfloat16", "SGD", False),
    ("keypoints", "float32", "SGD", False), ("keypoints", "bfloat16", "SGD", False),
    ("quat_regloc", "float32", "ADAM", False),
    ("quat_regloc", "bfloat16", "SGD", None)])
def test_static_scale_leaves_every_bit_of_the_step(heads, dtype, optimizer, train_bn):
    """Two engines from the same weights over the same three batches, LOSS_SCALE None and 1024 (SGD with clip 5 and weight decay 1e-4, the
    Config defaults; Adam once; batch-statistics BN once): weights, momentum (Adam: both moments, vhat, t), the gradient buffer and the
    reported losses are bit-identical after every step.  The backward pass is linear in dz and 2**10 commutes with every rounding while
    nothing leaves the normal range, so a finalisation path without its unscale, or a scale applied after the rounding, shows here."""
    a, cfg = _engine(heads, dtype, None, optimizer, train_bn)
    b, _ = _engine(heads, dtype, 1024.0, optimizer, train_bn)
    assert float(cfg.GRADIENT_CLIP_NORM) == 5.0 and float(cfg.WEIGHT_DECAY) == 1e-4
    assert a.ls_state is None and a.loss_scale() is None and b.ls_state is not None
    assert _same_bits(a.flat_w, b.flat_w)
    for step in range(3):
        bt = _batch(heads, 11 + step)
        for e in (a, b):
            e.load_batch(*bt)
            e.step()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a.flat_g).all()) and float(a.flat_g.abs().max()) > 0
        for name, x, y in zip(("weights", "momentum", "gradient", "losses", "m", "vhat", "hyper"), _opt_state(a), _opt_state(b)):
            assert _same_bits(x, y), "%s differ after step %d (%d of %d elements)" % (name, step + 1, int((_bits(x) != _bits(y)).sum()), x.numel())
        assert _same_bits(a.flat_stats, b.flat_stats)
    assert b.loss_scale() == {"scale": 1024.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 3}


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_overflowed_step_is_skipped_and_the_scale_recovers(optimizer):
    """fp16, dynamic, scale 2**24 = its maximum, growth_interval 2.  The abs-dot gradient is ~|gt| / 3 ~ 0.1 per component, x 2**24 it is far
    past fp16's 65504: the first replay overflows by construction.  It leaves weights, momentum (and Adam's moments and t) bit for bit,
    halves the scale and counts one skip; replaying on (deterministic, at most 30 replays), every state is next_state of the one before, the
    first finite step moves the weights, the second finite step in a row doubles the scale, and no weight is ever non-finite."""
    LS = _LS()
    eng, _ = _engine("quat_regloc", "float16", "dynamic", optimizer, LOSS_SCALE_INIT=2.0 ** 24, LOSS_SCALE_MAX=2.0 ** 24, LOSS_SCALE_GROWTH_INTERVAL=2)
    eng.load_batch(*_batch("quat_regloc", 11))
    eng.capture()                                                   # (its warm-up step is undone, loss-scale state included)
    assert eng.loss_scale() == {"scale": 2.0 ** 24, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}
    before = [t.clone() for t in _opt_state(eng)[:2] + _opt_state(eng)[4:]]
    state = eng.ls_state.tolist()
    eng.step(); torch.cuda.synchronize()
    now = _opt_state(eng)[:2] + _opt_state(eng)[4:]
    assert all(_same_bits(x, y) for x, y in zip(before, now)), "a skipped step changed the training state"
    if optimizer == "ADAM":
        assert float(eng.hyper[5]) == 0.0
    assert not bool(torch.isfinite(eng.normsq).all())
    state = LS.next_state(state, False)
    assert eng.ls_state.tolist() == state
    assert eng.loss_scale() == {"scale": 2.0 ** 23, "skipped_total": 1, "last_step_skipped": True, "good_steps": 0}
    moved_at = doubled_at = None
    for replay in range(2, 31):
        w_prev, scale_prev, good_prev = eng.flat_w.clone(), state[LS.SCALE], state[LS.GOOD_STEPS]
        eng.step(); torch.cuda.synchronize()
        finite = bool(torch.isfinite(eng.normsq).all())
        state = LS.next_state(state, finite)
        assert eng.ls_state.tolist() == state, replay
        assert bool(torch.isfinite(eng.flat_w).all()), replay
        if not finite:
            assert _same_bits(eng.flat_w, w_prev), replay
        elif moved_at is None:
            moved_at = replay
            assert not _same_bits(eng.flat_w, w_prev), "the first finite step must move the weights"
            assert good_prev == 0
        if finite and state[LS.SCALE] == 2 * scale_prev:
            doubled_at = replay
            assert good_prev == 1, "the scale doubles on the second finite step in a row"
            break
    print("%s: first finite step at replay %s (scale 2**%d), doubled at replay %s, %d skipped"
          % (optimizer, moved_at, int(np.log2(state[LS.SCALE])) - (1 if doubled_at else 0), doubled_at, int(state[LS.SKIPPED_TOTAL])))
    assert moved_at is not None and doubled_at is not None
    eng.reset_optimizer()
    assert eng.loss_scale() == {"scale": 2.0 ** 24, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}


def _ori_update(eng):
    """The momentum slice of ori_final's kernel after ONE applied step from zero momentum: v = -lr c g, the step's update of that kernel."""
    o, n, _ = eng.slices[("ori_final", "kernel")]
    return eng.flat_v[o:o + n].double().cpu(), eng.flat_g[o:o + n].clone(), eng.flat_w[o:o + n]


def _rel_err(a, b):
    return float((a - b).norm() / b.norm())


ORI_W = 2.0 ** -17


def test_dynamic_scale_recovers_the_orientation_gradient_fp16_loses():
    """Soft-classification orientation head, 8**3 bins, near-uniform labels and near-uniform logits (ori_final's initial kernel x 0.1 in
    every engine), orientation loss weight W = 2**-17.
    Premise (asserted on the float64 gradient at the fp32 engine's logits): every |dz| = W / 3 |softmax - p| is below 2**-26, a quarter of
    the smallest fp16 subnormal, so the unscaled fp16 store rounds all of it to zero (a factor 2 of margin for the fp16 forward pass).
    A weight of 1e-4 puts the largest of these gradients at 1.1e-7, above the rounding point 2**-25 = 3e-8: some survive as one or two
    subnormal steps, and the gfx950 MFMA keeps fp16 subnormal operands (measured: DESIGN.md section 14), so at 1e-4 the unscaled gradient
    is 46 % wrong, not zero; the zero claim needs the smaller weight.
      - unscaled fp16: ori_final's kernel gradient is the weight-decay term alone, bit for bit;
      - "dynamic" (from 2**24 down to the first scale that does not overflow): the update of the first applied step differs from the fp32
        engine's by at most twice what the unscaled fp16 engine differs by at orientation weight 1 (Frobenius-relative, same batch, same
        weights; the factor 2 covers the different rounding points)."""
    W = ORI_W
    heads = "softclass_ori"
    img, loc, _ = _batch(heads, 11)
    g = torch.Generator().manual_seed(7)
    p = torch.softmax(0.1 * torch.randn(3, 512, generator=g), 1).to(torch.float32).numpy()

    def one_step(dtype, w_ori, loss_scale=None, **kw):
        eng, cfg = _engine(heads, dtype, loss_scale, LOSS_WEIGHTS={"loc_loss": 1.0, "ori_loss": w_ori, "k2_loss": 1.0, "k3_loss": 1.0}, **kw)
        o, n, _ = eng.slices[("ori_final", "kernel")]
        eng.flat_w[o:o + n] *= 0.1
        w0 = eng.flat_w.clone()
        eng.load_batch(img, loc, p)
        for _ in range(30):
            eng.step(); torch.cuda.synchronize()
            if not _same_bits(eng.flat_w, w0):
                break
        return eng, cfg, w0

    f32_w, cfg, w0 = one_step("float32", W)
    logits = f32_w.outputs()[1].double().cpu()
    dz64 = X.softmax_xent64(logits, torch.as_tensor(p), W, 1)[2]
    print("float64 |dz| max %.3e (2**-25 = %.3e)" % (float(dz64.abs().max()), 2.0 ** -25))
    assert 0 < float(dz64.abs().max()) < 2.0 ** -26
    ref_v, _, _ = _ori_update(f32_w)

    f16_w, _, _ = one_step("float16", W)
    _, g16, _ = _ori_update(f16_w)
    o, n, shape = f16_w.slices[("ori_final", "kernel")]
    K, N = int(np.prod(shape[:-1])), int(shape[-1])
    regc = np.float32(2.0) * np.float32(cfg.WEIGHT_DECAY) / (np.float32(K) * np.float32(N))
    decay_only = w0[o:o + n] * torch.tensor(regc, device="cuda")
    assert _same_bits(g16, decay_only), "unscaled fp16 must lose the whole orientation gradient at this weight"
    assert not _same_bits(f32_w.flat_g[o:o + n], decay_only)

    dyn, _, _ = one_step("float16", W, "dynamic", LOSS_SCALE_INIT=2.0 ** 24)
    st = dyn.loss_scale()
    assert not st["last_step_skipped"] and st["good_steps"] == 1
    err_dyn = _rel_err(_ori_update(dyn)[0], ref_v)

    f32_1, _, _ = one_step("float32", 1.0)
    f16_1, _, _ = one_step("float16", 1.0)
    yard = _rel_err(_ori_update(f16_1)[0], _ori_update(f32_1)[0])
    print("ori_final update vs fp32: dynamic fp16 at W = 2**-17 (scale 2**%d, %d skipped) %.3e; unscaled fp16 at W = 1 (yardstick) %.3e"
          % (int(np.log2(st["scale"])), st["skipped_total"], err_dyn, yard))
    assert err_dyn <= 2.0 * yard


def test_changed_keys_take_effect_on_the_next_plan():
    """The LOSS_SCALE keys are read whenever the plan is built: static 1024 -> "dynamic" from 8 with growth_interval 2 -> None, each
    followed by set_trainable (a re-plan).  The state restarts from the new settings, reset_optimizer() restores the NEW settings, and
    with None the engine is back to the plain step (no state)."""
    eng, cfg = _engine("quat_regloc", "float32", 1024.0)
    assert eng.config is cfg
    eng.load_batch(*_batch("quat_regloc", 11))
    eng.step(); torch.cuda.synchronize()
    assert eng.loss_scale() == {"scale": 1024.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 1}
    cfg.LOSS_SCALE, cfg.LOSS_SCALE_INIT, cfg.LOSS_SCALE_GROWTH_INTERVAL = "dynamic", 8.0, 2
    eng.set_trainable(".*")
    eng.load_batch(*_batch("quat_regloc", 11))                      # (a re-plan allocates new input buffers)
    assert eng.loss_scale() == {"scale": 8.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}
    for _ in range(2):
        eng.step()
    torch.cuda.synchronize()
    assert eng.loss_scale() == {"scale": 16.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}
    eng.reset_optimizer()
    assert eng.loss_scale() == {"scale": 8.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}
    assert eng.ls_state.tolist()[_LS().GROWTH_INTERVAL] == 2.0
    cfg.LOSS_SCALE = None
    eng.set_trainable(".*")
    eng.load_batch(*_batch("quat_regloc", 11))                      # (a re-plan allocates new input buffers)
    assert eng.ls_state is None and eng.loss_scale() is None
    w = eng.flat_w.clone()
    eng.step(); torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.flat_w).all()) and not _same_bits(eng.flat_w, w)


EPOCH_LINE = r"epoch 1  loc_loss \d+\.\d{5}  val_loc_loss \d+\.\d{5}  val_ori_loss \d+\.\d{5}"


def _train_once(tmp_path, capsys, **cfgkw):
    import re
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=False, ori_bins=4, dtype="float32", lr=0.01)
    cfg.NAME = "ls"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 4, 1
    for k, v in cfgkw.items():
        setattr(cfg, k, v)
    ds_train, ds_val = SyntheticPoses(16, 64, 128, cfg, seed=1), SyntheticPoses(8, 64, 128, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all")
    lines = [l for l in capsys.readouterr().out.splitlines() if re.match(r"epoch \d", l)]
    assert len(lines) == 1 and len(hist.loc_loss_acc) == 4 and np.isfinite(hist.loc_loss_acc).all()
    return model, hist, lines[0]


def test_train_records_and_prints_the_loss_scale(tmp_path, capsys):
    """UrsoNet.train() with "dynamic" from 8, growth_interval 2, maximum 32, fp32 (nothing overflows): the per-step history beside the
    losses is what next_state gives over four finite steps (8, 16, 16, 32; nothing skipped), and the epoch line is the plain one followed
    by the last scale and the epoch's skipped steps."""
    import re
    LS = _LS()
    model, hist, line = _train_once(tmp_path, capsys, LOSS_SCALE="dynamic", LOSS_SCALE_INIT=8.0, LOSS_SCALE_GROWTH_INTERVAL=2, LOSS_SCALE_MAX=32.0)
    state, want = LS.initial_state(model.config), []
    for _ in range(4):
        state = LS.next_state(state, True)
        want.append(state[LS.SCALE])
    assert want == [8.0, 16.0, 16.0, 32.0]
    assert hist.loss_scale_acc == want and hist.skipped_acc == [False] * 4
    assert re.fullmatch(EPOCH_LINE + r"  loss_scale 32  skipped 0", line), line
    assert model._engine.loss_scale() == {"scale": 32.0, "skipped_total": 0, "last_step_skipped": False, "good_steps": 0}


def test_train_epoch_line_is_the_plain_one_when_off(tmp_path, capsys):
    """LOSS_SCALE = None: the epoch line ends after the validation losses, as it did before the key existed, and the history has no
    loss-scale lists."""
    import re
    model, hist, line = _train_once(tmp_path, capsys)
    assert re.fullmatch(EPOCH_LINE, line), line
    assert not hasattr(hist, "loss_scale_acc") and not hasattr(hist, "skipped_acc")
    assert model._engine.ls_state is None
