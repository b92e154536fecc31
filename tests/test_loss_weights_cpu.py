"""Learnable loss weights without a GPU (Config.LEARNABLE_LOSS_WEIGHTS, ursonet_amd/loss_weights.py): what the key
refuses, the parameter layer and its checkpoints across feature on / off and training / inference, and the float64 NumPy statement
of the three losses under a learnable weight, checked against finite differences (tests/test_loss_weights_gpu.py imports it).

With w = LOSS_WEIGHTS[name], L the batch-mean loss without its weight and s the trainable scalar:
    w_eff = w exp(-s);  reported = w (L exp(-s) + s);  d reported / ds = w (1 - L exp(-s));  head gradient = w_eff dL / d(head)."""
import os
from collections import OrderedDict

import numpy as np
import pytest

from ursonet_amd import loss_weights as LW
from ursonet_amd.config import Config
from util import make_config

ABSDOT_CLAMP = float(np.float32(1e-12))


# ------------------------------------------------------------------ the float64 statement of the formulas
def w_eff(w, s):
    return float(w) * np.exp(-float(s))


def reported(L, w, s):
    """The loss the step reports: w (L exp(-s) + s)."""
    return float(w) * (L * np.exp(-float(s)) + float(s))


def d_reported_ds(L, w, s):
    return float(w) * (1.0 - L * np.exp(-float(s)))


def softmax_xent(z, p, w, s, relu_mask):
    """Soft-label cross-entropy of [B][K] logits: L = mean_b (lse_b sum_k p - sum_k p z); dz = (softmax - p) w_eff / B, zero where
    relu_mask and z <= 0.  -> (reported, ds, dz, L)."""
    z, p = np.asarray(z, np.float64), np.asarray(p, np.float64)
    B = z.shape[0]
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(1, keepdims=True)
    lse = (m + np.log(S))[:, 0]
    L = float((lse * p.sum(1) - (p * z).sum(1)).sum() / B)
    dz = (e / S - p) * (w_eff(w, s) / B)
    if relu_mask:
        dz = np.where(z > 0, dz, 0.0)
    return reported(L, w, s), d_reported_ds(L, w, s), dz, L


def rel_l2(gt, pred, w, s):
    """L = ||gt - pred||_F / ||gt||_F over the batch; pred is [B][ld], its columns D.. are ignored and get a zero gradient.
    -> (reported, ds, dpred [B][ld], L)."""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    D = gt.shape[1]
    e = gt - pred[:, :D]
    nd, ng = np.sqrt((e * e).sum()), np.sqrt((gt * gt).sum())
    L = float(nd / ng)
    g = np.zeros_like(pred)
    g[:, :D] = -w_eff(w, s) / (nd * ng) * e
    return reported(L, w, s), d_reported_ds(L, w, s), g, L


def absdot(gt, x, w, s, normalize):
    """L = mean_b (1 - |gt_b . q_b|), q = x / sqrt(max(|x|^2, 1e-12)) (normalize) or x; dq = -sign(dot) gt w_eff / B (sign(0) = 0);
    dx = rinv (dq - q (q . dq)), and rinv dq on a clamped row.  -> (reported, ds, dx [B][ld], L)."""
    gt, x = np.asarray(gt, np.float64), np.asarray(x, np.float64)
    B, D = gt.shape
    xv = x[:, :D]
    ss = (xv * xv).sum(1, keepdims=True)
    clamped = ~(ss > ABSDOT_CLAMP)
    rinv = 1.0 / np.sqrt(np.maximum(ss, ABSDOT_CLAMP)) if normalize else np.ones_like(ss)
    q = xv * rinv
    dot = (gt * q).sum(1, keepdims=True)
    L = float((1.0 - np.abs(dot)).mean())
    dq = -np.sign(dot) * gt * (w_eff(w, s) / B)
    proj = np.where(clamped, 0.0, q * (q * dq).sum(1, keepdims=True))
    g = np.zeros_like(x)
    g[:, :D] = rinv * (dq - proj) if normalize else dq
    return reported(L, w, s), d_reported_ds(L, w, s), g, L


# ------------------------------------------------------------------ the formulas against finite differences
def _fd(f, x, h=1e-6):
    """Central differences of the scalar f over every element of the array x."""
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        xp, xm = x.copy(), x.copy()
        xp[i] += h; xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("s", [0.0, -2.3, 3.0])
def test_formulas_agree_with_finite_differences(s):
    rng = np.random.default_rng(5)
    w, B = 0.7, 3
    z = np.abs(rng.normal(size=(B, 8))) + 0.1
    p = rng.dirichlet(np.ones(8), size=B)
    gt3, x3 = rng.normal(size=(B, 3)), rng.normal(size=(B, 8))
    gt4 = rng.normal(size=(B, 4)); gt4 /= np.linalg.norm(gt4, axis=1, keepdims=True)
    x4 = rng.normal(size=(B, 8))
    cases = [("xent", lambda a, s_: softmax_xent(a, p, w, s_, 0), z),
             ("rel_l2", lambda a, s_: rel_l2(gt3, a, w, s_), x3),
             ("absdot", lambda a, s_: absdot(gt4, a, w, s_, 0), x4),
             ("absdot normalized", lambda a, s_: absdot(gt4, a, w, s_, 1), x4)]
    for name, f, a in cases:
        rep, ds, g, L = f(a, s)
        assert rep == pytest.approx(w * (L * np.exp(-s) + s), rel=1e-14, abs=1e-14), name
        assert ds == pytest.approx(w * (1 - L * np.exp(-s)), rel=1e-14, abs=1e-14), name
        fd_s = (f(a, s + 1e-6)[0] - f(a, s - 1e-6)[0]) / 2e-6
        assert abs(fd_s - ds) <= 1e-7 * (1 + abs(ds)), (name, fd_s, ds)
        fd_a = _fd(lambda v: f(v, s)[0], a)
        assert np.abs(fd_a - g).max() <= 1e-6 * (1 + np.abs(g).max()), (name, np.abs(fd_a - g).max())
        if name != "xent":
            assert np.abs(g[:, gt3.shape[1] if name == "rel_l2" else 4:]).max() == 0.0      # the padding columns get no gradient
    # at s = 0 the reported loss is the plain weighted loss and the gradient the plain gradient
    assert softmax_xent(z, p, w, 0.0, 0)[0] == pytest.approx(w * softmax_xent(z, p, 1.0, 0.0, 0)[3], rel=1e-15)
    # the ReLU mask only zeroes the gradient where the logit is not positive
    zz = z.copy(); zz[0, :3] = 0.0
    g0, g1 = softmax_xent(zz, p, w, s, 0)[2], softmax_xent(zz, p, w, s, 1)[2]
    assert (g1[0, :3] == 0).all() and (g1[0, 3:] == g0[0, 3:]).all() and (g0[0, :3] != 0).all()


# ------------------------------------------------------------------ what the key refuses
def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_keypoints_exact_rel_loss_and_data_parallel_runs_are_refused(tmp_path):
    from ursonet_amd.net import UrsoNet
    LW.validate(_cfg(LEARNABLE_LOSS_WEIGHTS=True))                            # one GPU, the loc / ori pair: accepted
    with pytest.raises(ValueError, match="LEARNABLE_LOSS_WEIGHTS.*REGRESS_KEYPOINTS"):
        LW.validate(_cfg(LEARNABLE_LOSS_WEIGHTS=True, REGRESS_KEYPOINTS=True))
    with pytest.raises(ValueError, match="LEARNABLE_LOSS_WEIGHTS.*DP_EXACT_REL_LOSS"):
        LW.validate(_cfg(LEARNABLE_LOSS_WEIGHTS=True, DP_EXACT_REL_LOSS=True))
    with pytest.raises(ValueError, match="LEARNABLE_LOSS_WEIGHTS.*data parallelism.*world size 2"):
        LW.validate(_cfg(LEARNABLE_LOSS_WEIGHTS=True), world=2)
    # off: nothing to refuse
    for kw in (dict(REGRESS_KEYPOINTS=True), dict(DP_EXACT_REL_LOSS=True)):
        LW.validate(_cfg(**kw), world=8)
    # at build, through the model
    for kw in (dict(keypoints=True), dict()):
        cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, regress_ori=True, **kw)
        cfg.LEARNABLE_LOSS_WEIGHTS = True
        if not kw:
            cfg.DP_EXACT_REL_LOSS = True
        with pytest.raises(ValueError, match="LEARNABLE_LOSS_WEIGHTS"):
            UrsoNet("training", cfg, str(tmp_path), build_engine=False)


# ------------------------------------------------------------------ the parameter layer
def _model(mode, on, tmp_path):
    from ursonet_amd.net import UrsoNet
    cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, regress_ori=True, bottleneck=16, branch=64)
    cfg.LEARNABLE_LOSS_WEIGHTS = on
    return UrsoNet(mode, cfg, str(tmp_path), build_engine=False)


def test_layer_exists_only_in_training_mode_with_the_key_on(tmp_path):
    assert Config().LEARNABLE_LOSS_WEIGHTS is False
    off = _model("training", False, tmp_path)
    assert LW.LAYER not in off._graph.params and all(l.name != LW.LAYER for l in off.keras_model.layers)
    inf = _model("inference", True, tmp_path)
    assert LW.LAYER not in inf._graph.params and [l.name for l in inf.keras_model.layers] == [l.name for l in off.keras_model.layers]
    on = _model("training", True, tmp_path)
    assert list(on._graph.params)[:-1] == list(off._graph.params) and list(on._graph.params)[-1] == LW.LAYER == "loss_weights"
    layer = on.keras_model.get_layer("loss_weights")
    assert layer.weights == ["loss_weights/ori_weight:0", "loss_weights/loc_weight:0"] and layer.trainable
    assert on._graph.params[LW.LAYER] == OrderedDict((("ori_weight", (1,)), ("loc_weight", (1,))))
    from ursonet_amd.engine import initial_weights
    init = initial_weights(on._graph, seed=7)
    assert init[LW.LAYER]["ori_weight"].tolist() == [np.float32(-2.3)] and init[LW.LAYER]["loc_weight"].tolist() == [0.0]
    assert init[LW.LAYER]["ori_weight"].dtype == np.float32
    # the other layers draw what they draw without the layer
    ref = initial_weights(off._graph, seed=7)
    assert all(np.array_equal(init[ln][wn], a) for ln, ws in ref.items() for wn, a in ws.items())
    assert LW.WEIGHT_OF_LOSS == {"ori_loss": "ori_weight", "loc_loss": "loc_weight"}


class _HostEngine(object):
    """Engine.set_weights / get_weights over host arrays: what UrsoNet.load_weights and save_weights go through."""

    def __init__(self, graph, seed):
        import torch
        from ursonet_amd.engine import Engine, initial_weights
        self.graph = graph
        self._t = {(ln, wn): torch.from_numpy(a.copy()) for ln, ws in initial_weights(graph, seed).items() for wn, a in ws.items()}
        self.set_weights = lambda params, strict=True: Engine.set_weights(self, params, strict)
        self.get_weights = lambda: OrderedDict((ln, OrderedDict((wn, self._t[(ln, wn)].numpy().copy()) for wn in ws)) for ln, ws in graph.params.items())

    def wview(self, ln, wn):
        return self._t[(ln, wn)]


def _with_engine(mode, on, tmp_path, seed):
    m = _model(mode, on, tmp_path)
    m._engine = _HostEngine(m._graph, seed)
    return m


def test_checkpoint_round_trip_and_loading_across_modes(tmp_path):
    from ursonet_amd.net import read_weights_file, write_weights_file
    src = _with_engine("training", True, tmp_path, seed=1)
    w = src._engine.get_weights()
    w[LW.LAYER]["ori_weight"][:] = -1.25
    w[LW.LAYER]["loc_weight"][:] = 0.5
    src._engine.set_weights(w)
    path = str(tmp_path / "run" / "weights_synthetic_0002.npz")
    os.makedirs(os.path.dirname(path))
    written = src.save_weights(path)
    assert path in written
    back = read_weights_file(path)
    assert list(back[LW.LAYER]) == ["ori_weight", "loc_weight"]
    assert back[LW.LAYER]["ori_weight"].tolist() == [-1.25] and back[LW.LAYER]["loc_weight"].tolist() == [0.5]
    assert back[LW.LAYER]["ori_weight"].dtype == np.float32 and back[LW.LAYER]["ori_weight"].shape == (1,)
    assert list(back) == list(w) and all(np.array_equal(back[ln][wn], a) for ln, ws in w.items() for wn, a in ws.items())
    probe = "bottleneck_layer"

    # written with the feature -> a training model that has it: the scalars arrive
    dst = _with_engine("training", True, tmp_path, seed=2)
    dst.load_weights(path, path)
    got = dst._engine.get_weights()
    assert got[LW.LAYER]["ori_weight"].tolist() == [-1.25] and got[LW.LAYER]["loc_weight"].tolist() == [0.5]
    assert np.array_equal(got[probe]["kernel"], w[probe]["kernel"])
    # -> an inference model, and a training model with the feature off: the layer is skipped, everything else arrives (by_name or not)
    for mode, on in (("inference", True), ("training", False)):
        for by_name in (False, True):
            dst = _with_engine(mode, on, tmp_path, seed=2)
            dst.load_weights(path, path, by_name=by_name)
            got = dst._engine.get_weights()
            assert LW.LAYER not in got and np.array_equal(got[probe]["kernel"], w[probe]["kernel"])
    # written without the feature -> a model that has it on: by name, the scalars keep their initial values
    plain = _with_engine("training", False, tmp_path, seed=3)
    ppath = str(tmp_path / "run" / "weights_synthetic_0003.npz")
    plain.save_weights(ppath)
    assert LW.LAYER not in read_weights_file(ppath)
    dst = _with_engine("training", True, tmp_path, seed=2)
    dst.load_weights(ppath, ppath, by_name=True)
    got = dst._engine.get_weights()
    assert got[LW.LAYER]["ori_weight"].tolist() == [np.float32(-2.3)] and got[LW.LAYER]["loc_weight"].tolist() == [0.0]
    assert np.array_equal(got[probe]["kernel"], plain._engine.get_weights()[probe]["kernel"])
    with pytest.raises(ValueError, match="loss_weights"):                     # not by name: the missing layer is named, as any other
        dst.load_weights(ppath, ppath, by_name=False)
    assert write_weights_file(str(tmp_path / "again.npz"), back) == [str(tmp_path / "again.npz")]


def test_extension_surface_lists_the_three_entry_points():
    import ursonet_amd.hip as hip
    names = {"urso_softmax_xent_fwd_bwd_lw", "urso_rel_l2_fwd_bwd_lw", "urso_absdot_fwd_bwd_lw"}
    assert names <= set(hip.SIDE_SYMBOLS["ext"]) and not names & set(hip.EXPORTED_SYMBOLS) and not names & set(hip.LOSS_SCALE_SYMBOLS)
    lib = hip.side_lib("ext")
    # argument checks run before any launch: a null s is refused by name
    assert lib.urso_rel_l2_fwd_bwd_lw(2, 3, 8, None, None, 1.0, 0, None, None, None, None, None, None, None) != 0
    assert "urso_rel_l2_fwd_bwd_lw" in hip.last_error()
    assert lib.urso_softmax_xent_fwd_bwd_lw(2, 8, None, None, 1.0, 0, 0, None, None, None, None, None, None, None) != 0
    assert lib.urso_absdot_fwd_bwd_lw(2, 4, 8, 1, None, None, 1.0, 0, None, None, None, None, None, None, None) != 0
