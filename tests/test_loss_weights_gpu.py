"""Learnable loss weights on the GPU (Config.LEARNABLE_LOSS_WEIGHTS).

Kernel level: urso_softmax_xent_fwd_bwd_lw, urso_rel_l2_fwd_bwd_lw and urso_absdot_fwd_bwd_lw (include/ursonet_ext.h) against the float64
NumPy statement of tests/test_loss_weights_cpu.py, element by element, with bounds counted from the operations (tests/exactprobe.py), and
bit for bit against the plain / loss-scaled entry points at s = 0.

Whole step: the engine with the key on against the unchanged oracle run with LOSS_WEIGHTS = w exp(-s), the update of the two scalars by
SGD and Adam under a clip, both norm plans, a frozen layer, validation, graph replay against eager launches, 16-bit steps under loss
scaling and UrsoNet.train().

Bound of the weighted quantities: the device forms w_eff = fl(w expf(-s)) (expf 1 ulp = 2 U, product 1 U) where the helpers of
exactprobe.py take an exact fp32 weight, and the cross-entropy divides it by B once more on the device (1 U) where the helper's quotient
is the host's (1 U), the reference's own weight being unrounded (1 U): LW_SLACK = 6 U relative on everything proportional to the weight,
on top of the plain kernel's own count."""
import copy
import math
import re

import numpy as np
import pytest
import torch

import exactprobe as X
import test_loss_weights_cpu as R
from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

SLACK = 64
NAN = float("nan")
LW_SLACK = 6
S_VALUES = (0.0, -2.3, 3.0)
SCALE = 2.0 ** 15
W_PLAIN, W_SCALED = 0.7, 0.7 / 64       # under the scale 2^15 the weight is smaller, so that no fp16 gradient overflows (checked per case)


def _hip():
    import ursonet_amd.hip as hip
    return hip


def dev(t):
    return t.contiguous().to(torch.float32).cuda()


def guarded(n, dt=0):
    buf = torch.full((int(n) + SLACK,), NAN, dtype=X.tdtype(dt), device="cuda")
    return buf, buf[:int(n)]


def assert_guard(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[int(n):]).all()), "%s: wrote past its extent of %d elements" % (what, n)
    assert not bool(torch.isnan(buf[:int(n)]).any()), "%s: elements of its extent were not written" % what


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


_worst = {}


def check(name, got, ref, bound, what=None):
    ref = X.d64(ref) if not isinstance(ref, torch.Tensor) else ref.to(torch.float64)
    bound = X.d64(bound) if not isinstance(bound, torch.Tensor) else bound.to(torch.float64)
    r = X.assert_within(got, ref, bound, what or name)
    _worst[name] = max(_worst.get(name, 0.0), float(r))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_worst):
        print("RATIO %-28s %.3f" % (k, _worst[k]))


def _state():
    return torch.tensor([SCALE, 1.0 / SCALE, 0.0, 0.0, SCALE, SCALE, 0.0, 0.0], device="cuda")


def _s_dev(s):
    return torch.tensor([s], dtype=torch.float32, device="cuda")


def _f32(x):
    return float(np.float32(x))


def _check_scalars(name, tag, loss_got, ds_got, rep, ds, w, s, plain_loss_bound):
    """reported = P + w s and ds = w - P, P the plain loss under w_eff: P's error is the plain fp32 bound + LW_SLACK U |P|; the report adds
    the product w s (1 U) and its sum (the store's half ulp), ds the difference (the store's half ulp)."""
    P = torch.tensor(w - ds, dtype=torch.float64)
    err_p = X.d64(plain_loss_bound) + LW_SLACK * X.U32 * P.abs()
    rep, ds = torch.tensor(rep, dtype=torch.float64), torch.tensor(ds, dtype=torch.float64)
    check(name + " loss", loss_got, rep, X.store_bound(rep, err_p + X.U32 * abs(w * s), 0), "loss " + tag)
    check(name + " ds", ds_got, ds, X.store_bound(ds, err_p, 0), "ds " + tag)


def _grad_bound(g64, plain_bound32, scale, dt):
    """The head gradient: the plain fp32 bound (its own half ulp of fp32 included) + LW_SLACK U |g|, times the (power-of-two, exact) loss
    scale, then ONE rounding to the storage type."""
    err = (plain_bound32 + LW_SLACK * X.U32 * g64.abs()) * scale
    assert float((g64.abs() * scale + err).max()) < (6.0e4 if dt == 2 else 1e38), "the case overflows its storage type"
    return X.store_bound(g64 * scale, err, dt)


# ===================================================================================================================== kernels
@pytest.mark.parametrize("K", [8, 4096])
def test_softmax_xent_lw_elementwise(K):
    hip = _hip()
    for B in (1, 3, 33):
        z, p = X.xent_inputs(B, K, 1.0)
        zd, pd = dev(z), dev(p)
        for relu in (0, 1):
            for s in S_VALUES:
                for state in (None, _state()):
                    w, s32 = _f32(W_PLAIN if state is None else W_SCALED), _f32(s)
                    rep, ds, g, _ = R.softmax_xent(z.numpy(), p.numpy(), w, s32, relu)
                    g = torch.from_numpy(g)
                    bl, _, bz = X.softmax_xent_bounds(z, p, R.w_eff(w, s32), relu, 0)
                    for dt in (0, 1, 2):
                        tag = "K=%d B=%d relu=%d s=%g scaled=%d dt=%d" % (K, B, relu, s, state is not None, dt)
                        loss4 = torch.tensor([7.0, NAN, 9.0, 11.0], device="cuda")
                        rowb, row = guarded(B); dzb, dz = guarded(B * K, dt); dsb, dsv = guarded(1)
                        hip.softmax_xent(B, K, zd, pd, w, relu, dt, loss4[1:2], dz, row, ls=state, lw=(_s_dev(s32), dsv))
                        assert_guard(dzb, B * K, "dz"); assert_guard(rowb, B, "row_ws"); assert_guard(dsb, 1, "ds")
                        assert loss4.tolist()[0::2] == [7.0, 9.0] and float(loss4[3]) == 11.0, "neighbouring loss slots touched"
                        _check_scalars("xent", tag, loss4[1], dsv[0], rep, ds, w, s32, bl)
                        check("xent dz %s" % ("fp32", "bf16", "fp16")[dt], dz.reshape(B, K), g * (SCALE if state is not None else 1.0),
                              _grad_bound(g, bz, SCALE if state is not None else 1.0, dt), "dz " + tag)
                        if relu:
                            assert float(dz.reshape(B, K).float()[zd <= 0].abs().sum()) == 0.0


def _head(B, D, ld, seed, unit):
    g = torch.Generator().manual_seed(seed)
    gt, x = torch.randn(B, D, generator=g), torch.randn(B, ld, generator=g)
    if unit:
        gt = gt / gt.norm(dim=1, keepdim=True)
    return gt, x


@pytest.mark.parametrize("D", [3, 4])
def test_rel_l2_lw_elementwise(D):
    hip = _hip()
    ld = 8
    for B in (1, 3, 33):
        gt, x = _head(B, D, ld, 400 + 10 * B + D, False)
        gtd, xd = dev(gt), dev(x)
        nplain = torch.empty(2, device="cuda")
        hip.rel_l2(B, D, ld, gtd, xd, 1.0, 0, torch.empty(1, device="cuda"), torch.empty(B * ld, device="cuda"), nplain)
        for s in S_VALUES:
            for state in (None, _state()):
                w, s32 = _f32(W_PLAIN if state is None else W_SCALED), _f32(s)
                rep, ds, g, _ = R.rel_l2(gt.numpy(), x.numpy(), w, s32)
                g = torch.from_numpy(g)
                bl, bg, _ = X.rel_l2_bounds(gt, x, R.w_eff(w, s32), 0)
                for dt in (0, 1, 2):
                    tag = "D=%d B=%d s=%g scaled=%d dt=%d" % (D, B, s, state is not None, dt)
                    lb, l1 = guarded(1); gb, g1 = guarded(B * ld, dt); nb, n1 = guarded(2); dsb, dsv = guarded(1)
                    hip.rel_l2(B, D, ld, gtd, xd, w, dt, l1, g1, n1, ls=state, lw=(_s_dev(s32), dsv))
                    for b_, n_, nm in ((lb, 1, "loss"), (gb, B * ld, "gradient"), (nb, 2, "norms"), (dsb, 1, "ds")):
                        assert_guard(b_, n_, "rel_l2_lw " + nm)
                    _check_scalars("rel_l2", tag, l1[0], dsv[0], rep, ds, w, s32, bl)
                    sc = SCALE if state is not None else 1.0
                    check("rel_l2 gradient", g1.reshape(B, ld), g * sc, _grad_bound(g, bg, sc, dt), "gradient " + tag)
                    X.assert_zero_columns(g1.reshape(B, ld), D, "rel_l2_lw gradient")
                    assert same_bits(n1, nplain), "the squared norms do not depend on the weight"


@pytest.mark.parametrize("D", [3, 4])
def test_absdot_lw_elementwise(D):
    hip = _hip()
    ld = 8
    for B in (1, 3, 33):
        gt, x = _head(B, D, ld, 700 + 10 * B + D, True)
        if B >= 3:
            gt[0], x[0] = 0, 0
            gt[0, 0], x[0, 1] = 1, 1                      # dot == 0 exactly: no gradient
            x[2] = 0                                      # zeros: the clamp branch
        gtd, xd = dev(gt), dev(x)
        for normalize in (0, 1):
            qplain = torch.empty(B * D, device="cuda")
            hip.absdot(B, D, ld, normalize, gtd, xd, 1.0, 0, qplain, torch.empty(1, device="cuda"), torch.empty(B * ld, device="cuda"))
            for s in S_VALUES:
                for state in (None, _state()):
                    w, s32 = _f32(W_PLAIN if state is None else W_SCALED), _f32(s)
                    rep, ds, g, _ = R.absdot(gt.numpy(), x.numpy(), w, s32, normalize)
                    g = torch.from_numpy(g)
                    _, bl, bdx = X.absdot_bounds(gt, x, R.w_eff(w, s32), normalize, 0)
                    for dt in (0, 1, 2):
                        tag = "D=%d B=%d normalize=%d s=%g scaled=%d dt=%d" % (D, B, normalize, s, state is not None, dt)
                        qb, q1 = guarded(B * D); lb, l1 = guarded(1); gb, g1 = guarded(B * ld, dt); dsb, dsv = guarded(1)
                        hip.absdot(B, D, ld, normalize, gtd, xd, w, dt, q1, l1, g1, ls=state, lw=(_s_dev(s32), dsv))
                        for b_, n_, nm in ((qb, B * D, "q"), (lb, 1, "loss"), (gb, B * ld, "gradient"), (dsb, 1, "ds")):
                            assert_guard(b_, n_, "absdot_lw " + nm)
                        _check_scalars("absdot", tag, l1[0], dsv[0], rep, ds, w, s32, bl)
                        sc = SCALE if state is not None else 1.0
                        check("absdot gradient", g1.reshape(B, ld), g * sc, _grad_bound(g, bdx, sc, dt), "gradient " + tag)
                        X.assert_zero_columns(g1.reshape(B, ld), D, "absdot_lw gradient")
                        assert same_bits(q1, qplain), "q does not depend on the weight"


def test_at_s_zero_the_bits_are_those_of_the_plain_and_the_scaled_kernels():
    """s = 0: w_eff = w exactly, so head gradient, norms, q and loss carry the bits of urso_*_fwd_bwd (no state) or urso_*_fwd_bwd_ls (a
    state), for every storage type; ds = w - loss.  A frozen s (ds = None) writes the same and touches no gradient slot."""
    hip = _hip()
    w, ld = _f32(0.7), 8
    s0 = _s_dev(0.0)
    for state in (None, _state()):
        for dt in (0, 1, 2):
            for B in (1, 3, 33):
                for K in (8, 4096):
                    z, p = X.xent_inputs(B, K, 1.0)
                    zd, pd = dev(z), dev(p)
                    for relu in (0, 1):
                        out = []
                        for lw in (None, (s0, torch.full((1,), NAN, device="cuda")), (s0, None)):
                            l1 = torch.full((1,), NAN, device="cuda"); dz = torch.empty(B * K, dtype=X.tdtype(dt), device="cuda")
                            row = torch.empty(B, device="cuda")
                            hip.softmax_xent(B, K, zd, pd, w, relu, dt, l1, dz, row, ls=state, lw=lw)
                            out.append((l1, dz, row))
                            if lw is not None and lw[1] is not None:
                                assert float(lw[1]) == float(np.float32(w) - np.float32(float(l1)))
                        for o in out[1:]:
                            assert all(same_bits(a, b) for a, b in zip(out[0], o)), ("xent", state is not None, dt, B, K, relu)
                for D in (3, 4):
                    gt, x = _head(B, D, ld, 900 + 10 * B + D, True)
                    gtd, xd = dev(gt), dev(x)
                    out = []
                    for lw in (None, (s0, torch.full((1,), NAN, device="cuda")), (s0, None)):
                        l1 = torch.full((1,), NAN, device="cuda"); g1 = torch.empty(B * ld, dtype=X.tdtype(dt), device="cuda")
                        n1 = torch.empty(2, device="cuda")
                        hip.rel_l2(B, D, ld, gtd, xd, w, dt, l1, g1, n1, ls=state, lw=lw)
                        out.append((l1, g1, n1))
                        if lw is not None and lw[1] is not None:
                            assert float(lw[1]) == float(np.float32(w) - np.float32(float(l1)))
                    for o in out[1:]:
                        assert all(same_bits(a, b) for a, b in zip(out[0], o)), ("rel_l2", state is not None, dt, B, D)
                    for normalize in (0, 1):
                        out = []
                        for lw in (None, (s0, torch.full((1,), NAN, device="cuda")), (s0, None)):
                            l1 = torch.full((1,), NAN, device="cuda"); g1 = torch.empty(B * ld, dtype=X.tdtype(dt), device="cuda")
                            q1 = torch.empty(B * D, device="cuda")
                            hip.absdot(B, D, ld, normalize, gtd, xd, w, dt, q1, l1, g1, ls=state, lw=lw)
                            out.append((l1, g1, q1))
                        for o in out[1:]:
                            assert all(same_bits(a, b) for a, b in zip(out[0], o)), ("absdot", state is not None, dt, B, D, normalize)


# ===================================================================================================================== whole step
HEADS = {"regress_regress": dict(regress_loc=True, regress_ori=True),
         "classify_classify": dict(regress_loc=False, regress_ori=False, loc_bins=8, ori_bins=8),
         "regress_classify": dict(regress_loc=True, regress_ori=False, ori_bins=8)}
W = {"loc_loss": 0.8, "ori_loss": 1.25}
LAYER = "loss_weights"


def _cfg(heads="regress_regress", dtype="float32", **kw):
    cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64, dtype=dtype, **HEADS[heads])
    cfg.LEARNABLE_LOSS_WEIGHTS = True
    cfg.LOSS_WEIGHTS = dict(W, k2_loss=1., k3_loss=1.)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _engine(cfg, seed=3, batch_seed=1):
    from ursonet_amd.engine import Engine
    img, loc, ori, _ = synthetic_batch(cfg, cfg.BATCH_SIZE, seed=batch_seed)
    eng = Engine(cfg, "training", seed=seed, randomize_bn=True)
    eng.load_batch(img, loc, ori)
    return eng, (img, loc, ori)


def _slots(eng):
    """indices of (ori_weight, loc_weight) in the flat buffers"""
    return [eng.slices[(LAYER, "ori_weight")][0], eng.slices[(LAYER, "loc_weight")][0]]


@pytest.mark.parametrize("heads", sorted(HEADS))
def test_training_step_against_the_oracle_with_reweighted_losses(heads):
    """The unchanged oracle, run with LOSS_WEIGHTS = {name: w exp(-s)} on the same weights and batch, gives O_name = its weighted loss and
    its gradients: the engine reports O + w s, writes ds = w - O and every network gradient is the oracle's.  Tolerances: those of
    tests/test_model_gpu.py::test_training_step_parity_fp32 for the same quantities (losses 1e-3 |O| + 1e-6, lines 184-185; every
    gradient 1e-3 of its tensor's maximum, line 193; ReLU decisions as there, lines 180-182)."""
    from test_model_gpu import ReluDecisions, _oracle_step, _rel
    cfg = _cfg(heads)
    eng, (img, loc, ori) = _engine(cfg)
    w0 = eng.get_weights()
    s = {wn: float(w0[LAYER][wn][0]) for wn in ("ori_weight", "loc_weight")}
    assert s == {"ori_weight": _f32(-2.3), "loc_weight": 0.0}
    eng.step(); torch.cuda.synchronize()
    ocfg = copy.copy(cfg)
    ocfg.LEARNABLE_LOSS_WEIGHTS = False
    ocfg.LOSS_WEIGHTS = dict(cfg.LOSS_WEIGHTS, loc_loss=W["loc_loss"] * math.exp(-s["loc_weight"]), ori_loss=W["ori_loss"] * math.exp(-s["ori_weight"]))
    w0o = {ln: ws for ln, ws in w0.items() if ln != LAYER}
    dec = ReluDecisions(eng, tol=1e-5)
    ref, _ = _oracle_step(ocfg, w0o, img, loc, ori, cfg.LEARNING_RATE, relu_hook=dec)
    assert dec.flips <= max(4, 2e-6 * dec.total), "too many ReLU decision flips: %d of %d" % (dec.flips, dec.total)
    ls, grads = eng.losses(), eng.get_grads()
    for name, wn in (("loc_loss", "loc_weight"), ("ori_loss", "ori_weight")):
        O = ocfg.LOSS_WEIGHTS[name] * ref[name]
        tol = 1e-3 * abs(O) + 1e-6
        print("LW %s %s: reported %.6f expected %.6f  ds %.6f expected %.6f" % (heads, name, ls[name], O + W[name] * s[wn],
                                                                              float(grads[LAYER][wn][0]), W[name] - O))
        assert abs(ls[name] - (O + W[name] * s[wn])) < tol, name
        assert abs(float(grads[LAYER][wn][0]) - (W[name] - O)) < tol, wn
    worst = ("", 0.0)
    for ln, ws in ref["grads"].items():
        for wn, gref in ws.items():
            e = _rel(grads[ln][wn], gref.numpy())
            if e > worst[1]:
                worst = (ln + "/" + wn, e)
    assert worst[1] < 1e-3, "worst gradient mismatch %s: %.3e" % worst


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_the_scalars_are_clipped_and_updated_with_the_rest(optimizer):
    """Two steps under a GRADIENT_CLIP_NORM far below the gradient norm (SGD: momentum 0, then 0.9): s, and its optimizer state, move by
    the update rule applied in float64 to the ds and normsq read back from the device, within the rule's own fp32 roundings
    (exactprobe.sgd64 / adam64 count them)."""
    cfg = _cfg(OPTIMIZER=optimizer, GRADIENT_CLIP_NORM=0.05, LEARNING_RATE=0.01)
    eng, _ = _engine(cfg)
    idx = _slots(eng)
    assert eng.adam == (optimizer == "ADAM")
    for k in range(2):
        if not eng.adam:
            eng.hyper[1] = 0.0 if k == 0 else 0.9
        w, v = eng.flat_w[idx].clone(), eng.flat_v[idx].clone()
        if eng.adam:
            v2, vh = eng.flat_v2[idx].clone(), eng.flat_vhat[idx].clone()
        eng.step(); torch.cuda.synchronize()
        g, normsq = eng.flat_g[idx].clone(), float(eng.normsq)
        clip = float(eng.hyper[4 if eng.adam else 2])
        assert math.sqrt(normsq) > 4 * clip and float(g.abs().min()) > 0, "the step is not clipped, or a scalar has no gradient"
        if eng.adam:
            assert float(eng.hyper[5]) == k + 1
            out = X.adam64(w, g, v, v2, vh, eng.hyper, normsq)
            for name, got in (("w", eng.flat_w[idx]), ("m", eng.flat_v[idx]), ("v", eng.flat_v2[idx]), ("vhat", eng.flat_vhat[idx])):
                check("adam " + name, got, out[name][0], out[name][1], "adam %s step %d" % (name, k))
        else:
            w2, vn, bw, bv, _ = X.sgd64(w, g, v, float(eng.hyper[0]), float(eng.hyper[1]), clip, normsq)
            check("sgd v", eng.flat_v[idx], vn, bv, "v step %d" % k)
            check("sgd s", eng.flat_w[idx], w2, bw, "s step %d" % k)
        assert not same_bits(eng.flat_w[idx], w), "s did not move"


def _fused_depth(eng):
    """Longest chain of fp32 additions into normsq in the fused plan (exactprobe.finalize_sq_depth, with one row slab: the most rows a
    thread can own) over the trainable layers, or the loss weights' own slot (urso_sqnorm over 8 floats), + urso_sqnorm_final."""
    per = X.sqnorm_depth(8)
    for n in eng.graph.nodes:
        if n.op != "conv":
            continue
        K = n.kh * n.kw * n.cin
        per = max(per, ((4 + -(-K // 16)) if n.cout % 4 == 0 else (1 + -(-K // 4))) + X.block_sum_depth())
    return per + X.sqnorm_final_depth(int(eng.sqpart.numel()))


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_both_norm_plans_count_the_two_scalars(fuse, monkeypatch):
    """normsq against the float64 sum of squares of the device's gradient buffer, the two ds included, within the rounding of the sum (its
    longest chain of additions); dropping the two would miss the bound tenfold at the least."""
    monkeypatch.setenv("URSO_FUSE_SQNORM", fuse)
    eng, _ = _engine(_cfg())
    assert eng.fused_sqnorm == (fuse == "1")
    labels = eng.labels["opt"]
    assert ("sqnorm_lw" in labels) == (fuse == "1") and labels.index("sqnorm") == (1 if fuse == "1" else 0)
    eng.step(); torch.cuda.synchronize()
    g = eng.flat_g.double().cpu()
    ref = (g * g).sum()
    ds2 = float((g[_slots(eng)] ** 2).sum())
    depth = _fused_depth(eng) if fuse == "1" else X.sqnorm_depth(eng.n_flat)
    bound = X.store_bound(ref, X.tree_sum_bound(ref, depth), 0)
    print("LW normsq fuse=%s: device %.6f float64 %.6f bound %.2e (depth %d), the scalars' share %.4f" % (fuse, float(eng.normsq), float(ref), float(bound), depth, ds2))
    assert ds2 > 10 * float(bound), "the case cannot tell whether the scalars are counted"
    check("normsq fuse=" + fuse, eng.normsq[0], ref, bound)


def test_a_frozen_layer_is_a_fixed_reweighting():
    """set_trainable on a regex that does not match loss_weights: s and its optimizer state keep their bits, its gradient slots stay
    zero, the norm does not count them -- and the network's gradients are bit for bit those of the all-trainable plan, i.e. weighted by
    exp(-s) (which the oracle case above checks)."""
    cfg = _cfg()
    ref, _ = _engine(cfg)
    ref.step(); torch.cuda.synchronize()
    eng, _ = _engine(cfg)
    eng.set_trainable(r"(?!loss_weights).*")
    eng.load_batch(*synthetic_batch(cfg, cfg.BATCH_SIZE, seed=1)[:3])        # (a re-plan allocates new input buffers)
    assert not eng.layer_trainable[LAYER] and "sqnorm_lw" not in eng.labels["opt"] and "sqnorm_lw" in ref.labels["opt"]
    idx = _slots(eng)
    w0 = eng.flat_w.clone()
    eng.step(); torch.cuda.synchronize()
    assert same_bits(eng.flat_w[idx], w0[idx]) and eng.flat_w[idx].tolist() == [_f32(-2.3), 0.0]
    assert eng.flat_g[idx].tolist() == [0.0, 0.0] and eng.flat_v[idx].tolist() == [0.0, 0.0]
    assert float(ref.flat_g[idx].abs().min()) > 0
    keep = torch.ones(eng.n_flat, dtype=torch.bool, device="cuda"); keep[idx] = False
    assert same_bits(eng.flat_g[:eng.n_flat][keep], ref.flat_g[:ref.n_flat][keep]), "the network's gradients changed"
    assert same_bits(eng.loss_buf, ref.loss_buf)
    g = eng.flat_g.double()
    assert abs(float(eng.normsq) - float((g * g).sum())) <= 1e-5 * float(eng.normsq) < 0.1 * float((ref.flat_g[idx].double() ** 2).sum())
    assert not same_bits(eng.flat_w[:eng.n_flat][keep], w0[:eng.n_flat][keep])


def test_validation_between_two_steps_changes_nothing():
    """evaluate(read=False) on another batch between two steps: flat_w and the optimizer state keep their bits across the call, it
    reports the transformed loss at the current s, and the second step ends bit for bit where it ends without the call."""
    cfg = _cfg()
    a, batch = _engine(cfg)
    b, _ = _engine(cfg)
    other = synthetic_batch(cfg, cfg.BATCH_SIZE, seed=7)[:3]
    for eng in (a, b):
        eng.step()
    torch.cuda.synchronize()
    before = (a.flat_w.clone(), a.flat_v.clone())
    a.load_batch(*other)
    assert a.evaluate(read=False) is None
    torch.cuda.synchronize()
    assert same_bits(a.flat_w, before[0]) and same_bits(a.flat_v, before[1])
    val = a.loss_buf.clone()
    a.load_batch(*batch)
    # the validation loss is the transformed one: the same batch through a training step of the second engine's weights reports it
    a.evaluate(read=False); torch.cuda.synchronize()
    at_s = a.loss_buf.clone()
    assert not same_bits(val, at_s)
    for eng in (a, b):
        eng.step()
    torch.cuda.synchronize()
    assert same_bits(b.loss_buf, at_s), "evaluate() reports another loss than the step on the same weights and batch"
    assert same_bits(a.flat_w, b.flat_w) and same_bits(a.flat_v, b.flat_v) and same_bits(a.flat_g, b.flat_g) and same_bits(a.normsq, b.normsq)


def test_graph_replay_equals_eager_launches_over_three_steps():
    cfg = _cfg("regress_classify")
    a, _ = _engine(cfg)
    b, _ = _engine(cfg)
    for _ in range(3):
        a.step()
        b.step_eager()
    torch.cuda.synchronize()
    assert same_bits(a.flat_w, b.flat_w) and same_bits(a.flat_g, b.flat_g) and same_bits(a.flat_v, b.flat_v) and same_bits(a.loss_buf, b.loss_buf)
    assert a.flat_w[_slots(a)].tolist() != [_f32(-2.3), 0.0]


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16_bit_step_under_loss_scaling_moves_s_by_the_unscaled_rule(dtype):
    """LOSS_SCALE = 2^10: the step runs and is finite; ds is w - P of the reported loss (not 2^10 times it), and s moves by the SGD
    rule on that ds and the device's normsq."""
    cfg = _cfg(dtype=dtype, LOSS_SCALE=2.0 ** 10)
    eng, _ = _engine(cfg)
    assert eng.ls_state is not None
    idx = _slots(eng)
    w, v = eng.flat_w[idx].clone(), eng.flat_v[idx].clone()
    eng.step(); torch.cuda.synchronize()
    assert eng.loss_scale()["skipped_total"] == 0 and bool(torch.isfinite(eng.flat_w).all()) and bool(torch.isfinite(eng.flat_g).all())
    g, normsq = eng.flat_g[idx].clone(), float(eng.normsq)
    rep = eng.loss_buf.double().cpu()
    for j, (name, slot) in enumerate((("ori_loss", 1), ("loc_loss", 0))):
        s = float(w[j])
        P = float(rep[slot]) - W[name] * s                  # |P| to half an ulp of the report and of the product
        assert abs(float(g[j]) - (W[name] - P)) <= 4 * X.U32 * (abs(float(rep[slot])) + abs(W[name] * s) + W[name]), name
    w2, vn, bw, bv, _ = X.sgd64(w, g, v, float(eng.hyper[0]), float(eng.hyper[1]), float(eng.hyper[2]), normsq)
    check("sgd v 16-bit", eng.flat_v[idx], vn, bv)
    check("sgd s 16-bit", eng.flat_w[idx], w2, bw)
    assert not same_bits(eng.flat_w[idx], w)


def test_train_records_prints_and_checkpoints_the_scalars(tmp_path, capsys):
    """UrsoNet.train(), 2 epochs x 3 steps + 1 validation step: six history entries per scalar, the entry of each epoch's last step is the
    value its checkpoint holds, the last one is the device's, and the epoch line ends with exp(s) of both."""
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = _cfg(LEARNING_RATE=0.01)
    cfg.NAME = "lw"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 3, 1
    ds_train, ds_val = SyntheticPoses(12, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    assert model.keras_model.get_layer(LAYER).weights == ["loss_weights/ori_weight:0", "loss_weights/loc_weight:0"]
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    lines = [l for l in capsys.readouterr().out.splitlines() if re.match(r"epoch \d", l)]
    assert len(lines) == 2
    for lst in (hist.ori_weight_acc, hist.loc_weight_acc, hist.ori_loss_acc, hist.loc_loss_acc):
        assert len(lst) == 6 and np.isfinite(lst).all()
    assert len(set(hist.ori_weight_acc)) == 6 and hist.ori_weight_acc[0] != _f32(-2.3)        # it moves with every step
    eng = model._engine
    dev_s = eng.loss_weight_values().tolist()
    assert [hist.ori_weight_acc[5], hist.loc_weight_acc[5]] == dev_s == [float(x[0]) for x in model.keras_model.get_layer(LAYER).get_weights()]
    for epoch, k in ((1, 2), (2, 5)):
        path = model.checkpoint_path.format(epoch=epoch)
        ck = net.read_weights_file(path[:-3] + ".npz")
        assert [float(ck[LAYER]["ori_weight"][0]), float(ck[LAYER]["loc_weight"][0])] == [hist.ori_weight_acc[k], hist.loc_weight_acc[k]], epoch
        m = re.search(r"  ori var (\d+\.\d{5})  loc var (\d+\.\d{5})$", lines[epoch - 1])
        assert m, lines[epoch - 1]
        assert abs(float(m.group(1)) - math.exp(hist.ori_weight_acc[k])) < 1e-5 and abs(float(m.group(2)) - math.exp(hist.loc_weight_acc[k])) < 1e-5
    # the checkpoint loads into an inference model, which has no such layer
    icfg = copy.copy(cfg)
    inf = net.UrsoNet(mode="inference", config=icfg, model_dir=str(tmp_path))
    inf.load_weights(model.checkpoint_path.format(epoch=2)[:-3] + ".npz", model.checkpoint_path.format(epoch=2))
    assert LAYER not in inf._engine.get_weights() and not hasattr(inf._engine, "flat_g")
    probe = "bottleneck_layer"
    assert np.array_equal(inf._engine.get_weights()[probe]["kernel"], eng.get_weights()[probe]["kernel"])


def test_the_default_plan_has_no_trace_of_the_feature():
    cfg = _cfg(LEARNABLE_LOSS_WEIGHTS=False)
    eng, _ = _engine(cfg)
    assert not eng.learn_lw and LAYER not in eng.graph.params and "sqnorm_lw" not in eng.labels["opt"]
    assert eng.labels["opt"] == ["sqnorm", "sgd"] and eng.labels["loss"] == ["loss", "loss"]
    on, _ = _engine(_cfg())
    assert on.n_flat == eng.n_flat + 8 and on.labels["loss"] == ["loss", "loss"] and on.labels["opt"] == ["sqnorm_lw", "sqnorm", "sgd"]
    with pytest.raises(ValueError, match="LEARNABLE_LOSS_WEIGHTS"):
        _engine(_cfg(DP_EXACT_REL_LOSS=True))
