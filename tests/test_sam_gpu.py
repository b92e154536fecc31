"""SAM on the GPU (Config.SAM).

Kernel level: urso_sam_ascend and urso_sam_descend bit for bit against ursonet_amd.sam.ascend32 and a bit copy, at the sizes where the walk
takes another path (a single element, each ragged end around a 16-byte access, a block's worth of vectors and one either side, and one
vector more than 4096 blocks of 256 threads cover, where the grid stride takes over), with the three buffers 0 .. 3 floats off a 16-byte
boundary -- all alike (vectors) and differing (scalars) --, NaN-payload guards on both sides of every buffer, values with both zeros,
subnormals and magnitudes across 2^-60 .. 2^60; a zero or non-finite norm leaves w alone and still writes w0; the state is ascend_state32's
and settle32's.
Engine level (resnet18, 64 x 64, batch 2, the engine of the LAMB tests): the SAM step is the composition -- a plain engine B, driven by
hand through pass 1, the host's ascend32, pass 2, the way back and the optimizer, holds the bits of engine A's one step(); for SGD with
clip, Adam, LARS, LAMB, WEIGHT_EMA, batch-statistics BN, learnable loss weights, keypoints and GRAD_ACCUM_STEPS = 2.  N is taken by
hip.sqnorm over B's flat_g: the engine's own normsq comes from the fused slots, which add in another order, and the ascent is specified
with the unfused launch.  Graph replay equals eager launches; fp16 steps that overflow move nothing; frozen layers are not perturbed; off
is off; the refusals; UrsoNet.train() prints the SAM line once per epoch and set_sam_rho() needs no re-capture."""
import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                            # a NaN with a payload: never the result of an operation
GUARD = 8                                        # floats on either side (32 bytes: the data keeps its place against the 16-byte boundary)
SIZES = (1, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 4096 + 5)
RHO, EPS = 0.05, 1e-12


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _S():
    from ursonet_amd import sam
    return sam


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _teq(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ===================================================================================================================== kernel level
_values = {}


def _vals(n, seed):
    """n float32 values: normals scaled across 2^-60 .. 2^60, with both zeros, subnormals and the smallest normal sprinkled in.  Shared."""
    if (n, seed) not in _values:
        rng = np.random.default_rng(1000 * seed + n % 997)
        v = (rng.standard_normal(n) * np.exp2(rng.integers(-60, 61, n))).astype(np.float32)
        special = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -140, 2.0 ** -127, 2.0 ** -126, -1.5 * 2.0 ** 60, 2.0 ** -60], dtype=np.float32)
        idx = rng.permutation(n)[:max(1, min(n // 3, 64 * len(special)))]
        v[idx] = special[(np.arange(len(idx)) + seed) % len(special)]
        _values[(n, seed)] = v
    return _values[(n, seed)]


class _Buf(object):
    """n floats on the device, `off` floats behind a 16-byte boundary, between two guards that hold the sentinel."""

    def __init__(self, data, off):
        n = len(data)
        host = np.full(GUARD + off + n + GUARD, SENTINEL, dtype=np.uint32)
        host[GUARD + off:GUARD + off + n] = _bits(data)
        self.n, self.lo = n, GUARD + off
        self.t = torch.from_numpy(host.view(np.float32)).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[self.lo:self.lo + n]
        assert self.view.data_ptr() % 16 == 4 * off

    def host(self):
        return self.t.cpu().numpy()[self.lo:self.lo + self.n]

    def guards_intact(self):
        h = _bits(self.t.cpu().numpy())
        return bool((h[:self.lo] == SENTINEL).all() and (h[self.lo + self.n:] == SENTINEL).all())


def _state(normsq, total=3.0, pending=1.0):
    S = _S()
    st = np.array(S.initial_state(RHO, EPS), dtype=np.float32)
    st[S.NORMSQ], st[S.SCALE], st[S.APPLIED], st[S.APPLIED_TOTAL], st[S.PENDING] = normsq, 123.0, 7.0, total, pending
    return st


ALIGN = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (1, 1, 3), (2, 0, 0), (3, 3, 0)]


@pytest.mark.parametrize("offs", ALIGN, ids=lambda o: "w%d_g%d_w0%d" % o)
def test_ascend_and_descend_bit_for_bit(offs):
    """All three buffers alike against the 16-byte boundary: the vector walk with its scalar head and tail; any other: scalars alone."""
    hip, S = _hip(), _S()
    for n in SIZES:
        w_h, g_h = _vals(n, 1), _vals(n, 2)
        normsq = np.float32(7.5e3) if n % 2 else np.float32(3.0e-7)
        w, g, w0 = _Buf(w_h, offs[0]), _Buf(g_h, offs[1]), _Buf(np.full(n, 5.0, dtype=np.float32), offs[2])
        st_h = _state(normsq)
        st = torch.from_numpy(st_h).cuda()
        hip.sam_ascend(n, w.view, g.view, w0.view, st)
        torch.cuda.synchronize()
        ew, ew0, s, applied = S.ascend32(w_h, g_h, normsq, RHO, EPS)
        assert applied and _same_bits(w.host(), ew) and _same_bits(w0.host(), w_h) and _same_bits(g.host(), g_h), (n, offs)
        assert w.guards_intact() and g.guards_intact() and w0.guards_intact(), (n, offs)
        est = S.ascend_state32(st_h)
        assert _same_bits(st.cpu().numpy(), est) and _same_bits(est[S.SCALE], S.scale32(normsq, RHO, EPS)[0]) and est[S.APPLIED] == 1
        assert est[S.APPLIED_TOTAL] == 4 and est[S.PENDING] == 2
        if n > 64:
            assert not _same_bits(ew, w_h)
        # the way back: w and w0 alike or not, as this case has them
        hip.sam_descend(n, w.view, w0.view)
        torch.cuda.synchronize()
        assert _same_bits(w.host(), w_h) and _same_bits(w0.host(), w_h) and w.guards_intact() and w0.guards_intact(), (n, offs)


@pytest.mark.parametrize("normsq", [0.0, float("inf"), float("nan")])
def test_a_zero_or_non_finite_norm_leaves_w_alone_and_still_writes_w0(normsq):
    hip, S = _hip(), _S()
    for n, offs in ((1025, (1, 1, 1)), (1025, (0, 2, 1)), (5, (3, 3, 3))):
        w_h, g_h = _vals(n, 1), _vals(n, 2)
        w, g, w0 = _Buf(w_h, offs[0]), _Buf(g_h, offs[1]), _Buf(np.full(n, 5.0, dtype=np.float32), offs[2])
        st_h = _state(np.float32(normsq))
        st = torch.from_numpy(st_h).cuda()
        hip.sam_ascend(n, w.view, g.view, w0.view, st)
        torch.cuda.synchronize()
        assert _same_bits(w.host(), w_h) and _same_bits(w0.host(), w_h) and _same_bits(g.host(), g_h)
        assert w.guards_intact() and g.guards_intact() and w0.guards_intact()
        got = st.cpu().numpy()
        assert _same_bits(got, S.ascend_state32(st_h))
        assert got[S.SCALE] == 0 and got[S.APPLIED] == 0 and got[S.APPLIED_TOTAL] == 3 and got[S.PENDING] == 1


def test_descend_moves_any_bits():
    """The way back is an integer copy: NaN payloads, both zeros and subnormals arrive as they are; n = 0 launches nothing."""
    hip = _hip()
    for n, offs in ((1029, (0, 0)), (1029, (2, 3)), (7, (1, 1))):
        src = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
        w, w0 = _Buf(_vals(n, 3), offs[0]), _Buf(src, offs[1])
        hip.sam_descend(n, w.view, w0.view)
        torch.cuda.synchronize()
        assert _same_bits(w.host(), src) and _same_bits(w0.host(), src) and w.guards_intact() and w0.guards_intact()
        hip.sam_descend(0, w.view, w0.view)
        hip.sam_ascend(0, w.view, w0.view, _Buf(src, 0).view, torch.zeros(8, device="cuda"))
        torch.cuda.synchronize()
        assert _same_bits(w.host(), src)


@pytest.mark.parametrize("normsq,guard", [(2.5, True), (float("inf"), True), (float("nan"), True), (float("inf"), False)])
def test_settle_is_settle32(normsq, guard):
    hip, S = _hip(), _S()
    st_h = _state(np.float32(4.0), total=9.0, pending=2.0)
    st, nsq = torch.from_numpy(st_h).cuda(), torch.tensor([normsq], dtype=torch.float32, device="cuda")
    hip.sam_settle(st, nsq, guard)
    torch.cuda.synchronize()
    want = S.settle32(st_h, normsq, guard)
    assert _same_bits(st.cpu().numpy(), want) and want[S.PENDING] == 0
    assert want[S.APPLIED_TOTAL] == (7 if guard and not np.isfinite(normsq) else 9)


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(seed=3, dtype="float32", keypoints=False, **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, keypoints=keypoints, **GEOM)
    for key, val in cfgkw.items():
        setattr(cfg, key, val)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(seed, keypoints=False):
    if (seed, keypoints) not in _batches:
        img, loc, ori, _ = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)
        if keypoints:
            rng = np.random.default_rng(seed)
            _batches[(seed, keypoints)] = (img, loc, rng.uniform(-1, 1, (2, 3)).astype(np.float32), rng.uniform(-1, 1, (2, 3)).astype(np.float32))
        else:
            _batches[(seed, keypoints)] = (img, loc, ori)
    return _batches[(seed, keypoints)]


def _state_buffers(eng):
    """The engine's own table of persistent state (Engine.train_state) and what a step leaves beside it."""
    return [name for name, _ in eng.train_state()] + ["flat_g", "normsq"]


def _unfused_normsq(eng):
    hip = _hip()
    out = torch.zeros(1, dtype=torch.float32, device=eng.device)
    hip.sqnorm(eng.n_flat, eng.flat_g, torch.empty_like(eng.sq_ws), out)
    torch.cuda.synchronize()
    return np.float32(out.cpu().numpy()[0])


def _two_passes_by_hand(B, rho=RHO, eps=EPS):
    """On the plain engine B, whose batch is loaded: pass 1, the host's ascent, pass 2 and the way back -- everything in front of the optimizer
    (or the accumulation launch).  Returns (N, s, applied, L(w), L(w + e), g2) and leaves g2 in flat_g, w in flat_w and pass 1's statistics
    in flat_stats."""
    S = _S()
    B.run_prep(); B.run_forward(); B.run_backward()
    torch.cuda.synchronize()
    N = _unfused_normsq(B)
    loss1, stats1 = B.loss_buf.clone(), B.flat_stats.clone()
    w = B.flat_w.cpu().numpy()
    w1, w0, s, applied = S.ascend32(w, B.flat_g.cpu().numpy(), N, rho, eps)
    B.flat_w.copy_(torch.from_numpy(w1))
    B.run_prep(); B.run_forward(); B.run_backward()
    torch.cuda.synchronize()
    loss2 = B.loss_buf.clone()
    B.flat_w.copy_(torch.from_numpy(w0))
    B.flat_stats.copy_(stats1)
    return N, s, applied, loss1, loss2, B.flat_g.cpu().numpy().copy()


def _check_against(A, B, N, s, loss1, loss2, total):
    """A after its step() against B after the hand-driven one."""
    S = _S()
    for name in _state_buffers(B):
        assert _teq(getattr(A, name), getattr(B, name)), name
    assert _teq(A.loss_buf, loss1) and _teq(A.sam_loss, loss2)
    st = A.sam_state.cpu().numpy()
    assert _same_bits(st[S.NORMSQ], N) and _same_bits(st[S.SCALE], s) and st[S.APPLIED] == 1 and st[S.APPLIED_TOTAL] == total
    rep = A.sam_report()
    l1, l2 = loss1.cpu().numpy(), loss2.cpu().numpy()
    slot = {"loc_loss": 0, "ori_loss": 1, "k2_loss": 2, "k3_loss": 3}
    assert set(rep) == {"rho", "grad_norm", "scale", "applied", "applied_total", "loss", "loss_perturbed"}
    assert rep["loss"] == A.losses() and rep["loss"] == {k: float(l1[slot[k]]) for k in rep["loss"]}
    assert rep["loss_perturbed"] == {k: float(l2[slot[k]]) for k in rep["loss"]} and rep["loss_perturbed"] != rep["loss"]
    assert rep["applied"] is True and rep["applied_total"] == total and rep["scale"] == float(s) and rep["rho"] == float(np.float32(RHO))
    assert rep["grad_norm"] == float(np.sqrt(N))


VARIANTS = {
    "sgd_clip": dict(GRADIENT_CLIP_NORM=5.0),
    "adam": dict(OPTIMIZER="Adam", GRADIENT_CLIP_NORM=5.0),
    "lars": dict(LARS=0.001),
    "lamb": dict(OPTIMIZER="Adam", LAMB=1.0),
    "ema": dict(WEIGHT_EMA=0.9),
    "train_bn": dict(TRAIN_BN=None),
    "learn_lw": dict(LEARNABLE_LOSS_WEIGHTS=True),
    "keypoints": dict(),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_step_is_the_composition(variant):
    kw, kp = VARIANTS[variant], variant == "keypoints"
    A, _ = _engine(keypoints=kp, SAM=RHO, **kw)
    B, _ = _engine(keypoints=kp, **kw)
    assert A.labels["sam"] == ["sam_norm", "sam_ascend", "sam_descend"] and "sam" not in B.labels
    assert {p: l for p, l in A.labels.items() if p != "sam"} == B.labels             # every other launch is the plain step's
    assert A.flat_w0 is not None and A.sam_state.cpu().tolist() == list(np.array(_S().initial_state(RHO, EPS), dtype=np.float32))
    assert A.sam_report()["applied_total"] == 0 and not A.forked
    for step in range(3):
        batch = _batch(11 + step, kp)
        A.load_batch(*batch); B.load_batch(*batch)
        stats0 = B.flat_stats.clone()
        N, s, applied, loss1, loss2, _g2 = _two_passes_by_hand(B)
        assert applied and np.isfinite(N) and N > 0
        if variant == "train_bn":                                            # the moving statistics moved in pass 1, and pass 2 did not move them again
            assert not _teq(B.flat_stats, stats0)
        w_before = B.flat_w.clone()
        B.run_optimizer()
        A.step()
        torch.cuda.synchronize()
        assert not _teq(B.flat_w, w_before)
        _check_against(A, B, N, s, loss1, loss2, step + 1)
    if variant == "learn_lw":                                                # the two scalars are parameters like any other: perturbed with the rest
        from ursonet_amd import loss_weights as LW
        o = A.slices[(LW.LAYER, "ori_weight")][0]
        A.load_batch(*_batch(20)); A.run_prep(); A.run_forward(); A.run_backward(); A.sam_ops[0](); A.sam_ops[1]()
        torch.cuda.synchronize()
        assert not _teq(A.flat_w[o:o + 8], A.flat_w0[o:o + 8]) and bool(A.flat_g[o:o + 8:4].abs().min() > 0)
        A.sam_ops[2]()
        torch.cuda.synchronize()
        assert _teq(A.flat_w, A.flat_w0)
    # reset_optimizer clears the record and the counts, not rho and eps
    A.reset_optimizer()
    assert A.sam_state.cpu().tolist() == list(np.array(_S().initial_state(RHO, EPS), dtype=np.float32))


def test_accumulation_ascends_every_micro_batch_and_moves_only_at_the_close():
    from ursonet_amd import grad_accum as GA
    A, _ = _engine(SAM=RHO, GRAD_ACCUM_STEPS=2, GRADIENT_CLIP_NORM=5.0)
    B, _ = _engine(GRAD_ACCUM_STEPS=2, GRADIENT_CLIP_NORM=5.0)
    assert A.labels["sam"] == ["sam_norm", "sam_ascend", "sam_descend"] and A.labels["accum"] == ["grad_accum"] == B.labels["accum"]
    assert A.labels["opt"] == B.labels["opt"] == ["grad_close", "sqnorm", "sgd"]
    seed, total = 11, 0
    for step in range(3):
        before = {name: getattr(A, name).clone() for name in ("flat_w", "flat_v", "flat_stats")}
        g2s = []
        for micro, role in enumerate(GA.roles(2)):
            batch = _batch(seed); seed += 1
            A.load_batch(*batch); B.load_batch(*batch)
            N, s, applied, loss1, loss2, g2 = _two_passes_by_hand(B)
            g2s.append(g2)
            B._accum_role = role
            for op in (B.opt_ops if role == "close" else B.accum_ops):
                op()
            A.step()
            torch.cuda.synchronize()
            total += 1
            if role != "close":                                              # nothing but flat_acc (and the scratch) has moved
                for name, t in before.items():
                    assert _teq(getattr(A, name), t), name
                assert _teq(A.flat_acc, B.flat_acc) and _same_bits(A.flat_acc.cpu().numpy(), GA.first32(g2))
                assert _teq(A.loss_buf, loss1) and _teq(A.sam_loss, loss2) and A.sam_report()["applied_total"] == total
        assert _same_bits(A.flat_g.cpu().numpy(), GA.accumulate32(g2s))
        _check_against(A, B, N, s, loss1, loss2, total)
        assert not _teq(A.flat_w, before["flat_w"])
    assert A.grad_accum() == {"steps": 2, "micro": 0}


def test_graph_replay_equals_the_eager_step():
    S = _S()
    a, _ = _engine(SAM=RHO, GRADIENT_CLIP_NORM=5.0, TRAIN_BN=None)
    b, _ = _engine(SAM=RHO, GRADIENT_CLIP_NORM=5.0, TRAIN_BN=None)
    init = a.sam_state.clone()
    a.load_batch(*_batch(11))
    a.capture()
    torch.cuda.synchronize()
    assert _teq(a.sam_state, init) and float(a.sam_state[S.APPLIED_TOTAL]) == 0      # the warm-up step is undone, the count included
    assert _teq(a.flat_w, b.flat_w) and _teq(a.flat_stats, b.flat_stats) and not bool(a.flat_v.any())
    names = ("flat_w", "flat_v", "flat_g", "normsq", "flat_stats", "loss_buf", "sam_loss", "sam_state", "flat_w0", "sam_stats")
    for s in range(3):
        for eng in (a, b):
            eng.load_batch(*_batch(11 + s))
        a.step()
        b.step_eager()
        torch.cuda.synchronize()
        for name in names:
            assert _teq(getattr(a, name), getattr(b, name)), (name, s)
    assert float(a.sam_state[S.APPLIED_TOTAL]) == 3 and float(a.sam_state[S.PENDING]) == 3      # (no loss scale: nothing settles)
    # profile_step: one record per launch of the doubled chain
    lab = b.labels
    one = lab["prep"] + lab["fwd"] + lab["loss"] + lab["bwd"]
    b.load_batch(*_batch(14))
    recs = b.profile_step()
    assert [r[0] for r in recs] == one + ["sam_norm", "sam_ascend"] + one + ["sam_descend"] + lab["opt"]
    a.load_batch(*_batch(14)); a.step(); torch.cuda.synchronize()            # (b took its fourth step inside profile_step)
    for name in names:
        assert _teq(getattr(a, name), getattr(b, name)), name
    # save / restore carry the state
    st = a.save_train_state()
    assert len(st) == 4
    a.load_batch(*_batch(20)); a.step(); torch.cuda.synchronize()
    assert float(a.sam_state[S.APPLIED_TOTAL]) == 5 and not _teq(a.sam_state, b.sam_state)
    a.restore_train_state(st)
    assert _teq(a.sam_state, b.sam_state) and _teq(a.flat_w, b.flat_w) and _teq(a.flat_stats, b.flat_stats)


def test_fp16_steps_that_overflow_move_nothing_then_the_next_one_is_the_composition():
    """fp16 under a dynamic LOSS_SCALE that begins at 2^24: pass 1 overflows, nothing is perturbed, pass 2 repeats it, the optimizer skips
    and the scale halves -- weights, momentum, the average and applied_total keep their bits; the first finite step is the composition."""
    S = _S()
    kw = dict(dtype="float16", GRADIENT_CLIP_NORM=5.0, WEIGHT_EMA=0.9, LOSS_SCALE="dynamic", LOSS_SCALE_INIT=2.0 ** 24)
    A, _ = _engine(SAM=RHO, **kw)
    B, _ = _engine(**kw)
    assert A.labels["opt"] == ["sqnorm", "sam_settle", "sgd", "loss_scale", "ema"] and B.labels["opt"] == ["sqnorm", "sgd", "loss_scale", "ema"]
    keep = ("flat_w", "flat_v", "flat_ema", "ema_state", "flat_stats")
    before = {name: getattr(A, name).clone() for name in keep}
    skipped = 0
    for i in range(26):                                                      # 2^24 halves to 1 in 24 steps: the loop ends long before
        batch = _batch(11 + i)
        A.load_batch(*batch)
        ls = A.ls_state.clone()
        A.step()
        torch.cuda.synchronize()
        if not A.loss_scale()["last_step_skipped"]:
            break
        skipped += 1
        st = A.sam_state.cpu().numpy()
        assert not bool(torch.isfinite(A.normsq).all()) and all(_teq(getattr(A, name), before[name]) for name in keep)
        assert st[S.APPLIED_TOTAL] == 0 and st[S.PENDING] == 0 and A.sam_report()["applied_total"] == 0
    assert 1 <= skipped < 25 and A.loss_scale()["skipped_total"] == skipped
    B.ls_state.copy_(ls)                                                     # B has not stepped: it holds A's weights of before, and now its scale
    B.load_batch(*batch)
    N, s, applied, loss1, loss2, _g2 = _two_passes_by_hand(B)
    assert applied
    B.run_optimizer()
    torch.cuda.synchronize()
    _check_against(A, B, N, s, loss1, loss2, 1)
    assert not _teq(A.flat_w, before["flat_w"]) and float(A.sam_state[S.PENDING]) == 0


def test_a_step_whose_second_pass_alone_overflows_is_settled():
    """The launches of a loss-scaled step by hand, with an infinity put into g2: w is back, the optimizer skips, and the ascent that was
    applied leaves applied_total again."""
    S = _S()
    A, _ = _engine(SAM=RHO, LOSS_SCALE=1024.0)
    A.load_batch(*_batch(11))
    w = A.flat_w.clone()
    A.run_prep(); A.run_forward(); A.run_backward()
    A.sam_ops[0](); A.sam_ops[1]()
    torch.cuda.synchronize()
    assert float(A.sam_state[S.APPLIED_TOTAL]) == 1 and float(A.sam_state[S.PENDING]) == 1 and not _teq(A.flat_w, w)
    A.run_prep(); A.run_forward(); A.run_backward()
    A.sam_ops[2]()
    A.flat_g[5] = float("inf")
    if A.sqpart is not None:                                                 # (the optimizer's norm adds the slots the finalisations left)
        A.sqpart[0] = float("inf")
    A.run_optimizer()
    torch.cuda.synchronize()
    st = A.sam_state.cpu().numpy()
    assert _teq(A.flat_w, w) and not bool(A.flat_v.any()) and A.loss_scale()["last_step_skipped"]
    assert st[S.APPLIED] == 1 and st[S.APPLIED_TOTAL] == 0 and st[S.PENDING] == 0


def test_frozen_layers_are_not_perturbed_and_do_not_move():
    A, _ = _engine(SAM=RHO)
    state = A.sam_state
    A.set_trainable(r"(bottleneck_layer|loc_.*|ori_.*)")
    assert A.sam_state is state and A.labels["sam"] == ["sam_norm", "sam_ascend", "sam_descend"]      # a rebuilt plan keeps the state
    frozen = [key for key in A.slices if not A.layer_trainable[key[0]]]
    assert frozen and len(frozen) < len(A.slices)
    A.load_batch(*_batch(11))
    start = A.flat_w.cpu().numpy().copy()
    # the middle of a hand-driven eager step
    A.run_prep(); A.run_forward(); A.run_backward()
    A.sam_ops[0](); A.sam_ops[1]()
    torch.cuda.synchronize()
    w, w0, g = A.flat_w.cpu().numpy(), A.flat_w0.cpu().numpy(), A.flat_g.cpu().numpy()
    assert _same_bits(w0, start) and A.sam_report()["applied"]
    moved = 0
    for key, (o, n, _shape) in A.slices.items():
        if key in frozen:
            assert not g[o:o + n].any() and np.array_equal(w[o:o + n], w0[o:o + n]), key
        else:
            moved += int(not _same_bits(w[o:o + n], w0[o:o + n]))
    assert moved > 0
    A.run_prep(); A.run_forward(); A.run_backward()
    A.sam_ops[2]()
    A.run_optimizer()
    torch.cuda.synchronize()
    w1 = A.flat_w.cpu().numpy()
    for key in frozen:
        o, n, _shape = A.slices[key]
        assert _same_bits(w1[o:o + n], start[o:o + n]), key
    assert not _same_bits(w1, start)


def test_off_is_off():
    from ursonet_amd.config import Config
    from ursonet_amd.engine import Engine
    unset, cfg0 = _engine(GRADIENT_CLIP_NORM=5.0)
    for key in ("SAM", "SAM_EPS"):
        assert key not in vars(cfg0) and hasattr(Config, key)
    off, _ = _engine(GRADIENT_CLIP_NORM=5.0, SAM=None, SAM_EPS=0.5)         # the other key alone changes nothing
    assert off.labels == unset.labels and "sam" not in off.labels and off.labels["opt"] == ["sqnorm", "sgd"]
    assert off.sam_report() is None and off.sam_state is None and off.flat_w0 is None and off.sam_ops == []
    assert len(off.save_train_state()) == len(unset.save_train_state()) == 3
    for s in (11, 12, 13):
        for eng in (unset, off):
            eng.load_batch(*_batch(s))
            eng.step()
    torch.cuda.synchronize()
    for name in ("flat_w", "flat_v", "flat_g", "loss_buf", "flat_stats", "hyper", "normsq"):
        assert _teq(getattr(unset, name), getattr(off, name)), name
    on, _ = _engine(GRADIENT_CLIP_NORM=5.0, SAM=RHO)
    assert {p: l for p, l in on.labels.items() if p != "sam"} == unset.labels and len(on.save_train_state()) == 4
    with pytest.raises(AssertionError, match="SAM is off"):
        off.set_sam_rho(0.1)
    cfg0.SAM, cfg0.SAM_EPS = "nonsense", "too"
    inf = Engine(cfg0, "inference", seed=3)
    assert inf.sam_report() is None and inf.sam_state is None and "sam" not in inf.labels      # inference ignores the keys


def test_bad_keys_a_launcher_and_the_wrapper_raise():
    from ursonet_amd.engine import Engine
    for kw, world in ((dict(SAM=True), 1), (dict(SAM=1), 1), (dict(SAM=-0.05), 1), (dict(SAM="0.05"), 1), (dict(SAM=float("inf")), 1),
                      (dict(SAM=RHO, SAM_EPS=-1.0), 1), (dict(SAM=RHO, SAM_EPS=float("nan")), 1), (dict(SAM=RHO), 2)):
        cfg = make_config(dtype="float32", **GEOM)
        for key, val in kw.items():
            setattr(cfg, key, val)
        with pytest.raises(ValueError, match="SAM"):
            if world == 1:
                Engine(cfg, "training", seed=3)
            else:
                _S().validate(cfg, world=world)
    from ursonet_amd import dp
    cfg = make_config(dtype="float32", **GEOM)
    cfg.SAM = RHO
    orig = dp.launcher_world
    dp.launcher_world = lambda: (0, 0, 2)                                    # a launcher's environment: refused before anything is allocated
    try:
        with pytest.raises(ValueError, match="SAM.*data parallelism.*world size 2"):
            Engine(cfg, "training", seed=3)
    finally:
        dp.launcher_world = orig
    eng, _ = _engine(SAM=RHO)
    orig = dp.dist.get_world_size
    dp.dist.get_world_size = lambda group=None: 2
    try:
        with pytest.raises(ValueError, match="SAM.*data parallelism.*world size 2"):
            dp.DataParallelEngine(eng, comm_cus=0)
    finally:
        dp.dist.get_world_size = orig
    with pytest.raises(ValueError, match="SAM"):
        eng.set_sam_rho(0)


def test_train_logs_sam_once_per_epoch_and_rho_moves_without_a_new_capture(tmp_path, capsys):
    import re
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    S = _S()
    cfg = make_config(dtype="float32", lr=0.001, **GEOM)
    cfg.NAME = "sam"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 3, 1
    cfg.SAM = RHO
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    eng = model._engine
    w0 = eng.flat_w.clone()
    capsys.readouterr()
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all")
    out = capsys.readouterr().out
    lines = re.findall(r"^epoch (\d)  sam rho (\S+)  median \|g\| (\S+)  d_loc_loss (\S+)  d_ori_loss (\S+)  \((\d+) of (\d+) ascents applied\)$", out, re.M)
    assert len(lines) == 1 and lines[0][0] == "1" and float(lines[0][1]) == float("%g" % np.float32(RHO)), out
    assert (lines[0][5], lines[0][6]) == ("3", "3")
    assert len(hist.loc_loss_acc) == 3 and len(hist.sam_grad_norm_acc) == 3 and hist.sam_applied_acc == [True] * 3
    assert float(lines[0][2]) == float("%.4e" % np.median(hist.sam_grad_norm_acc)) and min(hist.sam_grad_norm_acc) > 0
    assert [sorted(d) for d in hist.sam_sharpness_acc] == [["loc_loss", "ori_loss"]] * 3
    assert float(lines[0][3]) == float("%+.3e" % np.mean([d["loc_loss"] for d in hist.sam_sharpness_acc]))
    rep = eng.sam_report()
    assert rep["applied_total"] == 3 and hist.sam_grad_norm_acc[-1] == rep["grad_norm"]
    assert bool(torch.isfinite(eng.flat_w).all()) and not torch.equal(eng.flat_w, w0)
    # rho is a device field: the captured graph takes the new one at its next replay
    graph = eng._graphs
    assert graph is not None
    eng.set_sam_rho(0.125)
    eng.step()
    torch.cuda.synchronize()
    st = eng.sam_state.cpu().numpy()
    assert eng._graphs is graph and st[S.RHO] == 0.125 and st[S.APPLIED_TOTAL] == 4
    assert _same_bits(st[S.SCALE], S.scale32(st[S.NORMSQ], 0.125, EPS)[0]) and eng.sam_report()["rho"] == 0.125
