"""BN recalibration on the GPU (recalibrate_bn, Config.BN_RECAL_BATCHES).

Kernel level: urso_bn_recal_add and urso_bn_recal_settle bit for bit against ursonet_amd.bn_recal.pool_add64 / pool_settle32 on ONE
table of 32 layers -- every N of {1, 3, 4, 5, 255, 256, 257, 2048} with every M of {1, 2, 8, 2621440} --, four adds from the zero state
and the settlement, means scaled across 2^-20 .. 2^20 with both zeros and subnormals, variances >= 0 with zeros and subnormals, NaN-payload
sentinels around every accumulator and statistics slice and in the padding between them, one channel fed a NaN mean (compared by class),
and the refusals of the plan call.
Engine level (resnet18, 64 x 64, batch 2, TRAIN_BN = None: the engine of the LAMB / SAM tests; float32 and bfloat16): three batches and
one batch against the NumPy fold of the (bmean, bvar) read after every add; the stem layer against float64 statistics of its
concatenated z; an inference engine that comes closer to the training-mode output; no other state moves and a following step equals a
twin's; abort; the public call on an unlabelled dataset, its refusals; train() with BN_RECAL_BATCHES = 2; off is off."""
import os
import re

import numpy as np
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC0BEEF                              # NaNs with a payload: never the result of an operation
SENT64 = 0x7FF80000DEADBEEF
GUARD = 8
NS = (1, 3, 4, 5, 255, 256, 257, 2048)
MS = (1, 2, 8, 2621440)
ADDS = 4
NAN_LAYER, NAN_CH, NAN_ADD = 26, 100, 1          # layer 26 of _table: N = 257, M = 8


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _R():
    from ursonet_amd import bn_recal
    return bn_recal


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _teq(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ===================================================================================================================== kernel level
def _stat_values(N, seed):
    """ADDS batches of N float32 (mu_b, v_b)."""
    rng = np.random.default_rng(seed)
    scale = np.exp2(rng.integers(-20, 21, size=N))
    mu = (scale * (rng.normal(size=N) + rng.normal(size=(ADDS, N)))).astype(np.float32)
    v = (scale ** 2 * rng.uniform(0.0, 2.0, size=(ADDS, N))).astype(np.float32)
    special_mu = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -140, 2.0 ** -127, 2.0 ** 20, -2.0 ** -20], dtype=np.float32)
    special_v = np.array([0.0, 2.0 ** -149, 2.0 ** -130, 2.0 ** -126, 0.0, 2.0 ** 40, 2.0 ** -40], dtype=np.float32)
    for k in range(ADDS):
        idx = rng.permutation(N)[:max(1, N // 4)]
        mu[k, idx] = special_mu[(np.arange(len(idx)) + k) % len(special_mu)]
        idx = rng.permutation(N)[:max(1, N // 4)]
        v[k, idx] = special_v[(np.arange(len(idx)) + k) % len(special_v)]
    return mu, v


def _table():
    """[(N, M, off_mean, off_var)] for every (N, M), and n_stats: a guard in front, slices rounded up to 4 as Engine lays flat_stats out
    (so N = 1, 3, 5, 255, 257 leave padding), one more padding gap of 4 between a layer's two slices, a guard behind."""
    rows, off = [], GUARD
    for N in NS:
        for M in MS:
            pad = (N + 3) // 4 * 4
            rows.append((N, M, off, off + pad + 4))
            off += 2 * pad + 4
    return rows, off + GUARD


def test_add_and_settle_bit_for_bit_on_one_table():
    hip, R = _hip(), _R()
    rows, n_stats = _table()
    assert rows[NAN_LAYER][:2] == (257, 8)
    vals = [_stat_values(N, 10 * i + 1) for i, (N, _M, _om, _ov) in enumerate(rows)]
    vals[NAN_LAYER][0][NAN_ADD, NAN_CH] = np.nan
    inside = np.zeros(n_stats, dtype=bool)
    for N, _M, om, ov in rows:
        assert not inside[om:om + N].any() and not inside[ov:ov + N].any()
        inside[om:om + N] = inside[ov:ov + N] = True
    assert (~inside).sum() > 2 * GUARD + 4 * len(rows)                       # guards, gaps and rounding padding
    acc_h = np.full(n_stats, SENT64, dtype=np.uint64)
    acc_h[inside] = 0                                                        # the zero state
    stats_h = np.full(n_stats, SENT32, dtype=np.uint32)
    acc = torch.from_numpy(acc_h.view(np.float64)).cuda()
    stats = torch.from_numpy(stats_h.view(np.float32)).cuda()
    # the batch statistics of all layers in one guarded buffer each
    src_off, o = [], GUARD
    for N, _M, _om, _ov in rows:
        src_off.append(o)
        o += N + GUARD
    bm_h = np.full((ADDS, o), SENT32, dtype=np.uint32)
    bv_h = np.full((ADDS, o), SENT32, dtype=np.uint32)
    for (N, _M, _om, _ov), so, (mu, v) in zip(rows, src_off, vals):
        bm_h[:, so:so + N], bv_h[:, so:so + N] = _b32(mu), _b32(v)
    bm_d = torch.from_numpy(bm_h.view(np.float32)).cuda()
    bv_d = torch.from_numpy(bv_h.view(np.float32)).cuda()
    bm, bv = torch.empty(o, dtype=torch.float32, device="cuda"), torch.empty(o, dtype=torch.float32, device="cuda")
    plan = hip.BnRecalPlan([(bm[so:so + N], bv[so:so + N], M, om, ov) for (N, M, om, ov), so in zip(rows, src_off)], n_stats, "cuda")
    assert plan.L == 32 and plan.acc.numel() == n_stats and not bool(plan.acc.any())
    plan.acc = acc                                                           # the guarded accumulator in place of the plan's own
    for k in range(ADDS):
        bm.view(torch.int32).copy_(bm_d[k].view(torch.int32))
        bv.view(torch.int32).copy_(bv_d[k].view(torch.int32))
        assert plan.t == k
        plan.add()
    plan.settle(stats)
    torch.cuda.synchronize()
    got_acc, got_stats = acc.cpu().numpy(), stats.cpu().numpy()
    assert (_b64(got_acc)[~inside] == SENT64).all() and (_b32(got_stats)[~inside] == SENT32).all()
    assert _teq(bm, bm_d[ADDS - 1]) and _teq(bv, bv_d[ADDS - 1])             # the inputs are read only
    for li, ((N, M, om, ov), (mu, v)) in enumerate(zip(rows, vals)):
        ref = R.pool_zero(N)
        for k in range(ADDS):
            ref = R.pool_add64(ref, mu[k], v[k], M, k)
        mm, mv = R.pool_settle32(ref, M, ADDS)
        ok = np.ones(N, dtype=bool)
        if li == NAN_LAYER:
            ok[NAN_CH] = False
            for a in (got_acc[om + NAN_CH], got_acc[ov + NAN_CH], got_stats[om + NAN_CH], got_stats[ov + NAN_CH]):
                assert not np.isfinite(a)
            assert np.isnan(mm[NAN_CH]) and np.isnan(mv[NAN_CH])
        assert np.array_equal(_b64(got_acc[om:om + N])[ok], _b64(ref[0])[ok]), (N, M, "mean")
        assert np.array_equal(_b64(got_acc[ov:ov + N])[ok], _b64(ref[1])[ok]), (N, M, "m2")
        assert np.array_equal(_b32(got_stats[om:om + N])[ok], _b32(mm)[ok]), (N, M, "moving_mean")
        assert np.array_equal(_b32(got_stats[ov:ov + N])[ok], _b32(mv)[ok]), (N, M, "moving_variance")
        assert np.isfinite(mm[ok]).all() and np.isfinite(mv[ok]).all() and (mv[ok] >= 0).all()


def test_the_plan_call_refuses_before_any_launch():
    hip = _hip()
    m, v = torch.zeros(8, dtype=torch.float32, device="cuda"), torch.ones(8, dtype=torch.float32, device="cuda")
    m2, v2 = torch.zeros(4, dtype=torch.float32, device="cuda"), torch.ones(4, dtype=torch.float32, device="cuda")
    good = [(m, v, 16, 0, 8), (m2, v2, 4, 16, 20)]
    plan = hip.BnRecalPlan(good, 24, "cuda")
    stats = torch.full((24,), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(hip.UrsoHipError, match="urso_bn_recal_settle: nothing was added"):
        plan.settle(stats)                                                   # t == 0: refused on the host
    plan.add()
    plan.settle(stats)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [0.0] * 8 + [1.0] * 8 + [0.0] * 4 + [1.0] * 4
    bad = [([(m, v, 0, 0, 8)], 24, "M must be > 0"), ([(m, v, -2, 0, 8)], 24, "M must be > 0"), ([(m, v, 16, -1, 8)], 24, "negative offset"),
           ([(m, v, 16, 0, -8)], 24, "negative offset"), ([(m, v, 16, 0, 4)], 24, "overlap"), ([(m, v, 16, 0, 8), (m2, v2, 4, 6, 20)], 24, "overlap"),
           ([(m, v, 16, 0, 8), (m2, v2, 4, 16, 16)], 24, "overlap"), ([(m, v, 16, 0, 8), (m2, v2, 4, 16, 21)], 24, "ends behind n_stats"),
           ([(m, v, 16, 0, 8)], 15, "ends behind n_stats"), ([(m[1:], v[1:], 16, 0, 8)], 0, "n_stats must be > 0"), ([], 24, "L must be")]
    for layers, n, msg in bad:
        with pytest.raises(hip.UrsoHipError, match="urso_bn_recal_plan: .*" + msg):
            hip.BnRecalPlan(layers, n, "cuda")
    # null and misaligned pointers, N <= 0: the raw call (a tensor cannot express them)
    lib = hip.side_lib("train")
    tab = torch.zeros(6, dtype=torch.int64, device="cuda")
    for fields, msg in ((dict(bmean=None), "null"), (dict(bvar=None), "null"), (dict(bmean=m.data_ptr() + 2), "4-byte aligned"),
                        (dict(bvar=v.data_ptr() + 1), "4-byte aligned"), (dict(N=0), "N must be > 0"), (dict(N=-1), "N must be > 0")):
        row = (hip.BnRecalLayer * 1)()
        row[0].bmean, row[0].bvar, row[0].N, row[0].M, row[0].off_mean, row[0].off_var = m.data_ptr(), v.data_ptr(), 8, 16, 0, 8
        for k, val in fields.items():
            setattr(row[0], k, val)
        assert lib.urso_bn_recal_plan(1, row, 24, tab.data_ptr()) == -1 and msg in hip.last_error(), fields
    assert lib.urso_bn_recal_plan(1, row, 24, None) == -1 and lib.urso_bn_recal_plan(1, None, 24, tab.data_ptr()) == -1
    assert lib.urso_bn_recal_plan(1, row, 24, tab.data_ptr() + 4) == -1 and "8-byte aligned" in hip.last_error()
    torch.cuda.synchronize()
    assert not bool(tab.any())                                               # nothing was copied by a refused call


# ===================================================================================================================== engine level
GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)


def _engine(seed=3, dtype="float32", **cfgkw):
    from ursonet_amd.engine import Engine
    cfg = make_config(dtype=dtype, **GEOM)
    cfg.TRAIN_BN = None
    for key, val in cfgkw.items():
        setattr(cfg, key, val)
    return Engine(cfg, "training", seed=seed, randomize_bn=True), cfg


_batches = {}


def _batch(seed):
    if seed not in _batches:
        _batches[seed] = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)[:3]
    return _batches[seed]


def _bn_convs(eng):
    return [c for c in eng.convs.values() if c.batch_bn]


def _slice_mask(eng):
    inside = np.zeros(eng.flat_stats.numel(), dtype=bool)
    for o, n, _s in eng.stat_slices.values():
        inside[o:o + n] = True
    return inside


def _pool(eng, seeds, read_z=None):
    """begin, one add per batch seed, end.  Returns per BN conv the list of (bmean, bvar) read after every add (and, with read_z, that
    conv's z after every add as float64 [Mpix, N])."""
    seen, zs = [[] for _ in _bn_convs(eng)], []
    eng.bn_recal_begin()
    for s in seeds:
        eng.load_batch(*_batch(s))
        eng.bn_recal_add()
        torch.cuda.synchronize()
        for rec, c in zip(seen, _bn_convs(eng)):
            rec.append((c.bmean.cpu().numpy().copy(), c.bvar.cpu().numpy().copy()))
        if read_z is not None:
            zs.append(read_z.z.double().cpu().numpy().reshape(read_z.Mpix, read_z.N))
    eng.bn_recal_end()
    torch.cuda.synchronize()
    return seen, zs


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_three_batches_one_batch_and_the_stem(dtype):
    R = _R()
    eng, _ = _engine(dtype=dtype)
    convs = _bn_convs(eng)
    assert len(convs) > 1 and {c.node.bn for c in convs} == {ln for ln, _ in eng.stat_slices}
    inside = _slice_mask(eng)
    assert (~inside).any() or all(n % 4 == 0 for _o, n, _s in eng.stat_slices.values())
    before = eng.flat_stats.cpu().numpy().copy()
    stem = convs[0]
    assert stem.node.stem
    # ---- three batches: every slice is the NumPy fold of what the forward passes left; padding untouched
    seen, zs = _pool(eng, (11, 12, 13), read_z=stem)
    after = eng.flat_stats.cpu().numpy()
    assert np.array_equal(_b32(after[~inside]), _b32(before[~inside]))
    for c, rec in zip(convs, seen):
        acc = R.pool_zero(c.N)
        for t, (mu, v) in enumerate(rec):
            acc = R.pool_add64(acc, mu, v, c.Mpix, t)
        mm, mv = R.pool_settle32(acc, c.Mpix, 3)
        assert np.array_equal(_b32(eng.wview(c.node.bn, "moving_mean").cpu().numpy()), _b32(mm)), c.name
        assert np.array_equal(_b32(eng.wview(c.node.bn, "moving_variance").cpu().numpy()), _b32(mv)), c.name
        assert not np.array_equal(rec[0][0], rec[1][0])                      # the batches differ
    # ---- the stem's input depends on no other BN: pooled statistics against float64 mean / var of the three z concatenated.
    # Each batch's mean and variance were formed in float64 over M values and rounded ONCE to float32 (relative 2^-24 =: u32); the
    # float64 sums over M values add at most M 2^-53 of E[z^2] each.  With A = max |mu_b|, V = max v_b:
    #   mean:  the average of T means each off by u32 A, the fold's own error (a few 2^-53 A) and the float32 store of the result
    #   var :  the average of T variances each off by u32 V; the between term (mu_b - mean)^2 with both off by u32 A and |mu_b - mean|
    #          <= 2 A moves by at most 2 (2 A) (2 u32 A) + (2 u32 A)^2; the float32 store of the result
    z = np.concatenate(zs, axis=0)
    T, M = 3, stem.Mpix
    assert z.shape == (T * M, stem.N)
    u32, u64 = 2.0 ** -24, 2.0 ** -53
    A = np.max(np.abs(np.stack([r[0] for r in seen[0]]).astype(np.float64)), axis=0)
    V = np.max(np.stack([r[1] for r in seen[0]]).astype(np.float64), axis=0)
    Ez2 = np.mean(z * z, axis=0)
    mean64, var64 = z.mean(axis=0), z.var(axis=0)
    slack64 = 4 * T * M * u64
    b_mean = u32 * A + u32 * np.abs(mean64) + slack64 * (A + np.sqrt(Ez2)) + 2.0 ** -150
    b_var = u32 * V + (8 * u32 + 4 * u32 * u32) * A * A + u32 * var64 + slack64 * (Ez2 + A * A) + 2.0 ** -150
    got_m = eng.wview(stem.node.bn, "moving_mean").cpu().numpy().astype(np.float64)
    got_v = eng.wview(stem.node.bn, "moving_variance").cpu().numpy().astype(np.float64)
    print("stem %s: max mean error / bound %.3f, max var error / bound %.3f" % (
        dtype, float(np.max(np.abs(got_m - mean64) / b_mean)), float(np.max(np.abs(got_v - var64) / b_var))))
    assert np.all(np.abs(got_m - mean64) <= b_mean) and np.all(np.abs(got_v - var64) <= b_var)
    assert float(np.max(var64)) > 0
    # ---- one batch: the moving statistics are that batch's, bit for bit
    seen, _ = _pool(eng, (14,))
    for c, rec in zip(convs, seen):
        assert np.array_equal(_b32(eng.wview(c.node.bn, "moving_mean").cpu().numpy()), _b32(rec[0][0])), c.name
        assert np.array_equal(_b32(eng.wview(c.node.bn, "moving_variance").cpu().numpy()), _b32(rec[0][1])), c.name
    assert np.array_equal(_b32(eng.flat_stats.cpu().numpy()[~inside]), _b32(before[~inside]))


def test_an_inference_engine_comes_closer_to_the_training_mode_output():
    """Random initial statistics; after one batch the folded statistics are that batch's, so the inference engine reproduces the
    training-mode forward output up to the rounding of the folded filters.  An ordering, not a tolerance."""
    from ursonet_amd.engine import Engine
    eng, cfg = _engine()
    img = _batch(21)[0]
    old = eng.get_weights()
    eng.load_batch(*_batch(21))
    eng.bn_recal_begin(); eng.bn_recal_add(); eng.bn_recal_end()
    target = torch.cat([o.reshape(2, -1).double() for o in eng.outputs()], dim=1).cpu().numpy()
    new = eng.get_weights()
    inf = Engine(cfg, "inference", seed=3)
    dist = []
    for params in (old, new):
        inf.set_weights(params)
        inf.load_batch(img)
        inf.forward()
        torch.cuda.synchronize()
        out = torch.cat([o.reshape(2, -1).double() for o in inf.outputs()], dim=1).cpu().numpy()
        dist.append(float(np.linalg.norm(out - target)))
    print("distance to the training-mode output: old statistics %.4e, recalibrated %.4e" % tuple(dist))
    assert np.isfinite(dist).all() and dist[1] < dist[0]


FULL = dict(dtype="bfloat16", OPTIMIZER="Adam", LAMB=1.0, SAM=0.05, WEIGHT_EMA=0.9, LOSS_SCALE="dynamic")


def _state_names(eng):
    names = ["flat_w", "flat_g", "flat_v", "hyper", "flat_stats", "normsq", "loss_buf"]
    for name in ("flat_v2", "flat_vhat", "flat_ema", "ema_state", "ls_state", "lamb_state", "sam_state", "flat_w0", "flat_acc"):
        if getattr(eng, name, None) is not None:
            names.append(name)
    return names


def test_no_other_state_moves_and_the_next_step_is_a_twins():
    A, _ = _engine(**FULL)
    B, _ = _engine(**FULL)
    names = _state_names(A)
    assert {"flat_ema", "ema_state", "ls_state", "lamb_state", "sam_state", "flat_v2", "flat_vhat"} <= set(names)
    for s in (31, 32):
        for eng in (A, B):
            eng.load_batch(*_batch(s))
            eng.step()
    torch.cuda.synchronize()
    graph = A._graphs
    assert graph is not None and all(_teq(getattr(A, n), getattr(B, n)) for n in names)
    keep = {n: getattr(A, n).clone() for n in names}
    ptrs = {n: getattr(A, n).data_ptr() for n in names}
    labels = dict(A.labels)
    A.bn_recal_begin()
    for s in (33, 34):
        A.load_batch(*_batch(s))
        A.bn_recal_add()
    A.bn_recal_end()
    torch.cuda.synchronize()
    for n in names:
        if n not in ("flat_stats", "loss_buf"):
            assert _teq(getattr(A, n), keep[n]), n
        assert getattr(A, n).data_ptr() == ptrs[n], n
    assert not _teq(A.flat_stats, keep["flat_stats"]) and A.labels == labels and A._graphs is graph and not A.ema_swapped
    # the twin is handed the same statistics through set_weights (which also starts the average at the layer's weights: the twin's
    # average is put back) and both step on the same batch
    ema = B.flat_ema.clone()
    got = A.get_weights()
    B.set_weights({ln: got[ln] for ln in {l for l, _ in A.stat_slices}}, strict=False)
    B.flat_ema.copy_(ema)
    assert _teq(A.flat_stats, B.flat_stats) and _teq(A.flat_w, B.flat_w) and _teq(A.flat_ema, B.flat_ema)
    for eng in (A, B):
        eng.load_batch(*_batch(35))
        eng.step()
    torch.cuda.synchronize()
    assert A._graphs is graph                                                # the captured graph is still the one
    for n in names:
        assert _teq(getattr(A, n), getattr(B, n)), n
    assert not _teq(A.flat_w, keep["flat_w"])


def test_abort_restores_the_statistics_bit_for_bit():
    eng, _ = _engine(dtype="bfloat16")
    before = eng.flat_stats.clone()
    eng.bn_recal_abort()                                                     # without a begin: nothing
    eng.bn_recal_begin()
    eng.load_batch(*_batch(41))
    eng.bn_recal_add()
    torch.cuda.synchronize()
    assert not _teq(eng.flat_stats, before)                                  # the forward kernels' momentum updates
    eng.bn_recal_abort()
    assert _teq(eng.flat_stats, before)
    with pytest.raises(AssertionError, match="without bn_recal_begin"):
        eng.bn_recal_add()
    eng.bn_recal_begin()
    with pytest.raises(_hip().UrsoHipError, match="nothing was added"):
        eng.bn_recal_end()                                                   # settle with t == 0
    eng.bn_recal_abort()
    assert _teq(eng.flat_stats, before)
    frozen, _ = _engine(TRAIN_BN=False)
    with pytest.raises(ValueError, match="TRAIN_BN = None"):
        frozen.bn_recal_begin()


# ------------------------------------------------------------------ the public call
def _unlabelled(n, cfg, seed=5, fail_at=None):
    from ursonet_amd.dataset import SyntheticPoses

    class Unlabelled(SyntheticPoses):
        loads = 0

        def load_image(self, image_id):
            type(self).loads += 1
            if fail_at is not None and int(image_id) == fail_at:
                raise IOError("frame %d is unreadable" % image_id)
            return super(Unlabelled, self).load_image(image_id)

    def no_label(self, image_id):
        raise AssertionError("a label loader was called")
    for name in ("load_location", "load_quaternion", "load_keypoints", "load_euler_angles", "load_angle_axis", "load_location_encoded",
                 "load_orientation_encoded"):
        setattr(Unlabelled, name, no_label)
    return Unlabelled(n, 64, 64, cfg, seed=seed)


def _model(tmp_path, mode="training", **cfgkw):
    from ursonet_amd import net
    cfg = make_config(dtype="float32", **GEOM)
    cfg.TRAIN_BN = None
    for key, val in cfgkw.items():
        setattr(cfg, key, val)
    return net.UrsoNet(mode=mode, config=cfg, model_dir=str(tmp_path)), cfg


def test_recalibrate_bn_on_an_unlabelled_dataset_and_its_refusals(tmp_path):
    R = _R()
    model, cfg = _model(tmp_path, WEIGHT_EMA=0.9)
    eng = model._engine
    eng.load_batch(*_batch(51))
    eng.step()                                                               # the average leaves the weights
    eng.step()
    torch.cuda.synchronize()
    ds = _unlabelled(5, cfg)
    w, ema, stats0 = eng.flat_w.clone(), eng.flat_ema.clone(), eng.flat_stats.clone()
    res = R.recalibrate_bn(model, ds, workers=2)
    assert (res.images_used, res.images_dropped, res.batches) == (4, 1, 2) and type(ds).loads == 4
    assert list(res.layers) == [ln for ln, wn in eng.stat_slices if wn == "moving_mean"]
    assert all(np.isfinite(v).all() and v[0] > 0 and v[1] > 0 for v in res.layers.values())
    assert "4 images in 2 batches (1 dropped" in res.lines()[0]
    raw_stats = eng.flat_stats.clone()
    assert _teq(eng.flat_w, w) and _teq(eng.flat_ema, ema) and not _teq(raw_stats, stats0) and not eng.ema_swapped
    from ursonet_amd.graph import BN_EPS
    host = R.shift_report(eng.stat_slices, stats0.cpu().numpy(), raw_stats.cpu().numpy(), BN_EPS)
    assert host == dict(res.layers)
    # under the averaged weights: other statistics, the same weights afterwards
    res_e = R.recalibrate_bn(model, ds, nr_images=4, ema=True)
    assert (res_e.images_used, res_e.images_dropped, res_e.batches) == (4, 0, 2)
    assert _teq(eng.flat_w, w) and _teq(eng.flat_ema, ema) and not eng.ema_swapped and not _teq(eng.flat_stats, raw_stats)
    # ---- refusals
    now = eng.flat_stats.clone()
    with pytest.raises(ValueError, match="at least one whole batch of 2 images, got 1"):
        R.recalibrate_bn(model, ds, nr_images=1)
    with pytest.raises(ValueError, match="at least one whole batch"):
        R.recalibrate_bn(model, _unlabelled(0, cfg))
    from ursonet_amd import dp
    orig = dp.launcher_world
    dp.launcher_world = lambda: (0, 0, 2)
    try:
        with pytest.raises(ValueError, match="data-parallel launcher"):
            R.recalibrate_bn(model, ds)
    finally:
        dp.launcher_world = orig
    howto = r"UrsoNet\('training', cfg\).*TRAIN_BN = None.*load_weights.*recalibrate_bn.*save_weights"
    frozen, _ = _model(tmp_path, TRAIN_BN=False)
    with pytest.raises(ValueError, match=howto):
        R.recalibrate_bn(frozen, ds)
    inference, _ = _model(tmp_path, mode="inference")
    with pytest.raises(ValueError, match=howto):
        R.recalibrate_bn(inference, ds)
    plain, _ = _model(tmp_path)
    with pytest.raises(ValueError, match="ema=True.*WEIGHT_EMA"):
        R.recalibrate_bn(plain, ds, ema=True)
    # ---- an exception out of the feeder in mid-pass, and statistics that are not finite: the statistics are back bit for bit
    with pytest.raises(IOError, match="frame 5 is unreadable"):                # (the third batch: at least one was added before)
        R.recalibrate_bn(model, _unlabelled(7, cfg, fail_at=5), workers=1)
    assert _teq(eng.flat_stats, now) and not eng.ema_swapped
    with pytest.raises(IOError, match="frame 4 is unreadable"):
        R.recalibrate_bn(model, _unlabelled(7, cfg, fail_at=4), workers=1, ema=True)
    assert _teq(eng.flat_stats, now) and not eng.ema_swapped and _teq(eng.flat_w, w)
    o = next(v for (_ln, wn), v in eng.slices.items() if wn == "kernel")[0]      # the stem's filter: every statistic behind it
    eng.flat_w[o] = float("nan")
    with pytest.raises(FloatingPointError, match="not finite"):
        R.recalibrate_bn(model, ds)
    assert _teq(eng.flat_stats, now)
    assert _teq(eng.flat_w[o + 1:], w[o + 1:])


# ------------------------------------------------------------------ train()
def test_train_recalibrates_the_averaged_checkpoint(tmp_path, capsys):
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    model, cfg = _model(tmp_path, WEIGHT_EMA=0.9, BN_RECAL_BATCHES=2)
    cfg.NAME = "recal"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 1
    model.set_log_dir()
    ds_train, ds_val = SyntheticPoses(8, 64, 64, cfg, seed=1), SyntheticPoses(4, 64, 64, cfg, seed=2)
    eng = model._engine
    adds = []
    orig_add = eng.bn_recal_add
    eng.bn_recal_add = lambda: (adds.append(eng.ema_swapped), orig_add())[1]
    capsys.readouterr()
    model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    out = capsys.readouterr().out
    lines = re.findall(r"^epoch (\d)  bn recal  2 batches x 2 images under the averaged weights  max mean shift / sigma (\S+)  "
                       r"max var ratio (\S+)  \((\d+) BN layers\)$", out, re.M)
    assert [l[0] for l in lines] == ["1", "2"], out
    assert adds == [True] * 4 and not eng.ema_swapped                        # twice per checkpoint, under the average
    ddir, _ck = model.find_last()
    bn_layers = [ln for ln, wn in eng.stat_slices if wn == "moving_mean"]
    assert int(lines[0][3]) == len(bn_layers)
    for epoch in (1, 2):
        raw = net.read_weights_file(os.path.join(ddir, "weights_recal_%04d.npz" % epoch))
        avg = net.read_weights_file(os.path.join(ddir, "ema_weights_recal_%04d.npz" % epoch))
        for ln in bn_layers:
            assert not np.array_equal(avg[ln]["moving_mean"], raw[ln]["moving_mean"]), ln
            assert not np.array_equal(avg[ln]["moving_variance"], raw[ln]["moving_variance"]), ln
            assert np.isfinite(avg[ln]["moving_mean"]).all() and (avg[ln]["moving_variance"] >= 0).all()
    now = eng.get_weights()
    for ln in bn_layers:                                                     # the raw statistics are back, bit for bit
        for wn in ("moving_mean", "moving_variance"):
            assert np.array_equal(_b32(now[ln][wn]), _b32(raw[ln][wn])), (ln, wn)
    now_avg = eng.get_weights(ema=True)
    assert np.array_equal(avg["loc_final"]["kernel"], now_avg["loc_final"]["kernel"])


def test_off_is_off_and_bad_keys_raise(tmp_path):
    from ursonet_amd.config import Config
    from ursonet_amd.engine import Engine
    unset, cfg0 = _engine(WEIGHT_EMA=0.9)
    assert "BN_RECAL_BATCHES" not in vars(cfg0) and Config.BN_RECAL_BATCHES == 0
    off, _ = _engine(WEIGHT_EMA=0.9, BN_RECAL_BATCHES=0)
    on, _ = _engine(WEIGHT_EMA=0.9, BN_RECAL_BATCHES=2)
    assert off.labels == unset.labels == on.labels and len(off.save_train_state()) == len(unset.save_train_state())
    for s in (61, 62):
        for eng in (unset, off):
            eng.load_batch(*_batch(s))
            eng.step()
    torch.cuda.synchronize()
    for name in ("flat_w", "flat_v", "flat_g", "flat_stats", "flat_ema", "loss_buf"):
        assert _teq(getattr(unset, name), getattr(off, name)), name
    a, b = unset.get_weights(ema=True), off.get_weights(ema=True)
    assert all(np.array_equal(_b32(a[l][w]), _b32(b[l][w])) for l in a for w in a[l])
    for kw, msg in ((dict(BN_RECAL_BATCHES=True), "must be an int"), (dict(BN_RECAL_BATCHES=-1), "must be an int"),
                    (dict(BN_RECAL_BATCHES=1.5), "must be an int"), (dict(BN_RECAL_BATCHES=2), "needs WEIGHT_EMA"),
                    (dict(BN_RECAL_BATCHES=2, WEIGHT_EMA=0.9, TRAIN_BN=False), "TRAIN_BN = None")):
        with pytest.raises(ValueError, match="BN_RECAL_BATCHES.*" + msg):
            _engine(**kw)
        with pytest.raises(ValueError, match="BN_RECAL_BATCHES.*" + msg):
            _model(tmp_path, **kw)
    cfg = make_config(dtype="float32", **GEOM)
    cfg.TRAIN_BN, cfg.WEIGHT_EMA, cfg.BN_RECAL_BATCHES = None, 0.9, 2
    with pytest.raises(ValueError, match="BN_RECAL_BATCHES.*data parallelism.*world size 2"):
        _R().validate(cfg, world=2)                                          # (under a launcher the engine refuses WEIGHT_EMA first)
    cfg0.BN_RECAL_BATCHES = "nonsense"
    Engine(cfg0, "inference", seed=3)                                        # inference ignores the key
