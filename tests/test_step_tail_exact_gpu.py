"""Elementwise float64 probes of what follows the last conv of a training step (helpers: tests/exactprobe.py): the five loss
kernels, the global norm, SGD / Adam / scale, the parameter-gradient finalisation and the batch-statistics BatchNorm kernels.

Every kernel is called through the C ABI and compared ELEMENT BY ELEMENT, over its whole extent, with a float64 reference of the
operation's definition; the bound of each element is half an ulp of the storage type plus the fp32 roundings counted from the
operation (each helper's docstring states the count; tests/test_exactprobe_cpu.py shows that the bounds accept a plain fp32
restatement and reject the faults a kernel can have).  Outputs live in buffers with slack filled with NaN: inside the extent no
NaN may remain (every element written), past it every bit must be unchanged.  Where an entry point chooses a kernel, ran()
asserts which one ran.  Each test prints the largest ratio to its bound."""
import math

import numpy as np
import pytest
import torch

import exactprobe as X

pytestmark = pytest.mark.gpu

SLACK = 64
NAN = float("nan")


def _hip():
    import ursonet_amd.hip as hip
    return hip


def dev(t, dt=0):
    return t.contiguous().to(X.tdtype(dt)).cuda()


def guarded(n, dt=0):
    """(whole buffer, its first n elements): n + SLACK elements of NaN."""
    buf = torch.full((int(n) + SLACK,), NAN, dtype=X.tdtype(dt), device="cuda")
    return buf, buf[:int(n)]


def with_slack(t, dt=0):
    """An in / out operand followed by NaN slack: (whole buffer, view of the data)."""
    buf, v = guarded(t.numel(), dt)
    v.copy_(t.reshape(-1).to(X.tdtype(dt)))
    return buf, v


def assert_guard(buf, n, what):
    """Nothing past element n was written (the slack is still NaN) and no NaN is left before it."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[int(n):]).all()), "%s: wrote past its extent of %d elements" % (what, n)
    assert not bool(torch.isnan(buf[:int(n)]).any()), "%s: elements of its extent were not written" % what


_worst = {}


def note(name, ratio):
    _worst[name] = max(_worst.get(name, 0.0), float(ratio))


def check(name, got, ref, bound, what=None):
    note(name, X.assert_within(got, ref, bound, what or name))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_worst):
        print("RATIO %-28s %.3f" % (k, _worst[k]))


# ===================================================================================================================== losses
XENT_K = [1, 63, 64, 65, 257, 512, 4095, 4096, 4097, 13824, 16383, 16384, 16385, 32768]


def _xent_sym(K):
    return ("softmax_xent_reg_kernel", "ILi4E") if K <= 4096 else (("softmax_xent_reg_kernel", "ILi16E") if K <= 16384 else "softmax_xent_kernel")


def _run_xent(z, p, weight, relu, dt, loss4, slot, row_buf):
    hip = _hip()
    B, K = z.shape
    dzb, dz = guarded(B * K, dt)
    with X.ran(_xent_sym(K)):
        hip.softmax_xent(B, K, z, p, weight, relu, dt, loss4[slot:slot + 1], dz, row_buf[:B])
    assert_guard(dzb, B * K, "softmax_xent dz")
    return dz.reshape(B, K)


@pytest.mark.parametrize("K", XENT_K)
def test_softmax_xent_elementwise(K):
    """dz, the per-row losses and the scalar loss of urso_softmax_xent_fwd_bwd at both edges of each kernel's range; B 1 / 32,
    relu_mask 0 / 1, label mass 1 / 0.6, gradient stored as fp32 / bf16 / fp16; the other three floats of the engine's 4-float
    loss buffer stay untouched."""
    for B in (1, 32):
        for psum in (1.0, 0.6):
            z, p = X.xent_inputs(B, K, psum)
            zd, pd = dev(z), dev(p)
            for relu in (0, 1):
                ref = X.softmax_xent64(z, p, 1.0, relu)
                if K >= 63 and not relu:
                    X.assert_sensitive(ref[2], what="softmax_xent dz")
                for dt in (0, 1, 2):
                    bl, br, bz = X.softmax_xent_bounds(z, p, 1.0, relu, dt)
                    loss4 = torch.tensor([7.0, NAN, 9.0, 11.0], device="cuda")
                    rowb, _ = guarded(B)
                    dz = _run_xent(zd, pd, 1.0, relu, dt, loss4, 1, rowb)
                    assert_guard(rowb, B, "softmax_xent row_ws")
                    tag = "K=%d B=%d psum=%g relu=%d dt=%d" % (K, B, psum, relu, dt)
                    check("xent dz %s" % ("fp32", "bf16", "fp16")[dt], dz, ref[2], bz, "dz " + tag)
                    check("xent row loss", rowb[:B], ref[1], br, "row loss " + tag)
                    check("xent loss", loss4[1], ref[0], bl, "loss " + tag)
                    assert loss4.tolist()[0::2] == [7.0, 9.0] and float(loss4[3]) == 11.0, "neighbouring loss slots touched"
                    if relu:
                        assert float(dz.float()[zd <= 0].abs().sum()) == 0.0


def test_softmax_xent_two_heads_share_row_ws():
    """The location call and then the orientation call with the SAME row workspace, as the engine issues them: both losses right."""
    hip = _hip()
    B = 32
    zl, pl = X.xent_inputs(B, 512, 1.0, seed=1)
    zo, po = X.xent_inputs(B, 13824, 1.0, seed=2)
    loss4 = torch.full((4,), NAN, device="cuda")
    rowb, row = guarded(B)
    gl = torch.empty(B, 512, dtype=torch.bfloat16, device="cuda"); go = torch.empty(B, 13824, dtype=torch.bfloat16, device="cuda")
    hip.softmax_xent(B, 512, dev(zl), dev(pl), 1.0, 1, 1, loss4[0:1], gl, row)
    hip.softmax_xent(B, 13824, dev(zo), dev(po), 0.5, 1, 1, loss4[1:2], go, row)
    assert_guard(rowb, B, "row_ws")
    rl, ro = X.softmax_xent64(zl, pl, 1.0, 1), X.softmax_xent64(zo, po, 0.5, 1)
    check("xent loss", loss4[0], rl[0], X.softmax_xent_bounds(zl, pl, 1.0, 1, 1)[0], "location loss")
    bo = X.softmax_xent_bounds(zo, po, 0.5, 1, 1)
    check("xent loss", loss4[1], ro[0], bo[0], "orientation loss")
    check("xent row loss", row, ro[1], bo[1])
    check("xent dz bf16", go, ro[2], bo[2])
    assert bool(torch.isnan(loss4[2:]).all())


def test_softmax_xent_fp16_subnormal_shares():
    """B = 32, K = 24^3, fp16 gradient store: nearly all nonzero gradients are fp16 subnormals.  The kernel must keep them: the bound
    near 0 is half a subnormal spacing, so a flushed value that should round to a nonzero one fails it.  The shares are printed for the
    record (a measurement, not a gate of its own)."""
    B, K = 32, 13824
    z, p = X.xent_inputs(B, K, 1.0)
    ref = X.softmax_xent64(z, p, 1.0, 0)[2]
    loss4 = torch.zeros(4, device="cuda"); rowb, _ = guarded(B)
    dz = _run_xent(dev(z), dev(p), 1.0, 0, 2, loss4, 0, rowb)
    check("xent dz fp16", dz, ref, X.softmax_xent_bounds(z, p, 1.0, 0, 2)[2])
    nz = ref != 0
    n = float(nz.sum())
    sub = float((nz & (ref.abs() < 2.0 ** -14)).sum()) / n
    ref0 = float((X.round_to(ref, 2)[nz] == 0).sum()) / n
    got0 = float((dz.cpu().double()[nz] == 0).sum()) / n
    print("FP16SHARE subnormal %.4f  reference rounds to zero %.4f  kernel stores zero %.4f" % (sub, ref0, got0))
    assert sub > 0.9


def _head(B, D, ld, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g), torch.randn(B, ld, generator=g)


@pytest.mark.parametrize("B", [1, 5, 32, 300])
def test_regression_losses_elementwise(B):
    """urso_rel_l2_fwd_bwd, the two-phase urso_rel_l2_norms + urso_rel_l2_from_norms and urso_mse_fwd_bwd at D = 3, ld = 8."""
    hip = _hip()
    D, ld, w = 3, 8, 0.7
    gt, x = _head(B, D, ld, 40 + B)
    gtd, xd = dev(gt), dev(x)
    for dt in (0, 1, 2):
        loss, g, norms = X.rel_l2_64(gt, x, w)
        bl, bg, bn = X.rel_l2_bounds(gt, x, w, dt)
        X.assert_sensitive(g[:, :D], what="rel_l2 gradient")
        lb, l1 = guarded(1); gb, g1 = guarded(B * ld, dt); nb, n1 = guarded(2)
        hip.rel_l2(B, D, ld, gtd, xd, w, dt, l1, g1, n1)
        for b_, n_, nm in ((lb, 1, "loss"), (gb, B * ld, "gradient"), (nb, 2, "norms")):
            assert_guard(b_, n_, "rel_l2 " + nm)
        check("rel_l2 gradient", g1.reshape(B, ld), g, bg); check("rel_l2 loss", l1[0], loss, bl); check("rel_l2 norms", n1, norms, bn)
        X.assert_zero_columns(g1.reshape(B, ld), D, "rel_l2 gradient")
        # two phases with gscale 1: bit for bit the one-launch form; with gscale 4: four times it, within the bound
        nb2, n2 = guarded(2)
        hip.rel_l2_norms(B, D, ld, gtd, xd, n2)
        assert_guard(nb2, 2, "rel_l2_norms")
        assert torch.equal(n1, n2)
        for gscale in (1.0, 4.0):
            lb2, l2 = guarded(1); gb2, g2 = guarded(B * ld, dt)
            hip.rel_l2_from_norms(B, D, ld, gtd, xd, w, torch.tensor([gscale], device="cuda"), dt, n2, l2, g2)
            assert_guard(lb2, 1, "rel_l2_from_norms loss"); assert_guard(gb2, B * ld, "rel_l2_from_norms gradient")
            X.assert_zero_columns(g2.reshape(B, ld), D, "rel_l2_from_norms gradient")
            if gscale == 1.0:
                assert torch.equal(l1, l2) and torch.equal(g1, g2)
            else:
                assert torch.equal(l1, l2)
                check("rel_l2 gradient", g2.reshape(B, ld), X.rel_l2_64(gt, x, w, 4.0)[1], X.rel_l2_bounds(gt, x, w, dt, 4.0)[1], "gscale 4")
        loss, g = X.mse64(gt, x, w)
        bl, bg = X.mse_bounds(gt, x, w, dt)
        lb, l1 = guarded(1); gb, g1 = guarded(B * ld, dt)
        hip.mse(B, D, ld, gtd, xd, w, dt, l1, g1)
        assert_guard(lb, 1, "mse loss"); assert_guard(gb, B * ld, "mse gradient")
        check("mse gradient", g1.reshape(B, ld), g, bg); check("mse loss", l1[0], loss, bl)
        X.assert_zero_columns(g1.reshape(B, ld), D, "mse gradient")


@pytest.mark.parametrize("D", [3, 4])
@pytest.mark.parametrize("B", [1, 5, 32, 300])
def test_absdot_elementwise(B, D):
    """urso_absdot_fwd_bwd with and without normalisation: rows with dot < 0, dot == 0 exactly, a row of zeros and a tiny row (both take
    the clamp branch); B = 300 makes the one block loop over samples.  The inference form (gt = None) writes q alone."""
    hip = _hip()
    ld, w = 8, 0.9
    gt, x = _head(B, D, ld, 70 + B + D)
    if B >= 5:
        gt[0], x[0] = 0, 0
        gt[0, 0], x[0, 1] = 1, 1                          # dot == 0 exactly
        x[2] = 0                                          # zeros: clamped, q = 0
        x[3] *= 1e-7                                      # |x|^2 <= 1e-12: clamped with a nonzero dot
        gt[3] *= 0.01                                     # ... whose gradient 1e6 dq stays inside fp16's range
    gtd, xd = dev(gt), dev(x)
    for normalize in (0, 1):
        q, loss, dx, dot, _ = X.absdot64(gt, x, w, normalize)
        gtq = (gt.double() * q).abs().sum(1)
        assert bool(((dot.abs() > 1e3 * X.U32 * gtq) | (dot == 0)).all()), "a dot product cancels too far for its sign to be certain in fp32"
        if B >= 5:
            assert float(dot[0]) == 0 and bool((dot < 0).any())
            X.assert_sensitive(dx[:, :D], what="absdot gradient")
        for dt in (0, 1, 2):
            bq, bl, bdx = X.absdot_bounds(gt, x, w, normalize, dt)
            qb, q1 = guarded(B * D); lb, l1 = guarded(1); gb, g1 = guarded(B * ld, dt)
            hip.absdot(B, D, ld, normalize, gtd, xd, w, dt, q1, l1, g1)
            assert_guard(qb, B * D, "absdot q"); assert_guard(lb, 1, "absdot loss"); assert_guard(gb, B * ld, "absdot gradient")
            check("absdot q", q1.reshape(B, D), q, bq); check("absdot loss", l1[0], loss, bl)
            check("absdot gradient", g1.reshape(B, ld), dx, bdx, "dx normalize=%d dt=%d" % (normalize, dt))
            X.assert_zero_columns(g1.reshape(B, ld), D, "absdot gradient")
            if B >= 5:
                assert float(g1.reshape(B, ld)[0].float().abs().max()) == 0.0 and float(g1.reshape(B, ld)[2].float().abs().max()) == 0.0
        qb, q1 = guarded(B * D)
        hip.absdot(B, D, ld, normalize, None, xd, w, 0, q1, None, None)
        assert_guard(qb, B * D, "absdot q (inference)")
        check("absdot q", q1.reshape(B, D), X.absdot_q64(x, D, normalize), X.absdot_bounds(gt, x, w, normalize, 0)[0], "inference q")


# ===================================================================================================================== norm, optimizers
def _sqnorm(hip, g, n):
    ws = torch.empty(hip.sqnorm_ws_bytes(n) // 4, device="cuda")
    ob, out = guarded(1)
    hip.sqnorm(n, g, ws, out)
    assert_guard(ob, 1, "sqnorm")
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1048576, 1048577, 8388919])
def test_sqnorm_elementwise(n):
    hip = _hip()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.1
    gb, gd = with_slack(g)
    gb[n:] = 1e30                                         # anything read past n would show
    out = _sqnorm(hip, gd, n)
    ref = (g.double() ** 2).sum()
    check("sqnorm", out[0], ref, X.store_bound(ref, X.tree_sum_bound(ref, X.sqnorm_depth(n)), 0), "sqnorm n=%d" % n)


def test_sqnorm_refuses_unaligned_pointer():
    hip = _hip()
    buf = torch.randn(1028, device="cuda")
    ws = torch.empty(hip.sqnorm_ws_bytes(1024) // 4, device="cuda")
    ob, out = guarded(1)
    with pytest.raises(hip.UrsoHipError):
        hip.sqnorm(1024, buf[1:1025], ws, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ob).all())


@pytest.mark.parametrize("case", ["unclipped", "clipped", "noclip", "mom0"])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 1000003, 8388919])
def test_sgd_momentum_clip_elementwise(n, case):
    """urso_sgd_momentum_clip: v and w element by element against sgd64 with the norm THE DEVICE wrote (checked on its own first).
    n = 8388919 = 2 x 4194304 + 311: two full sweeps of the capped grid, a ragged third and a 3-element tail."""
    hip = _hip()
    w, g, v, lr, mom, clip = X.sgd_data(n, case)
    gb, gd = with_slack(g); wb, wd_ = with_slack(w); vb, vd = with_slack(v)
    nsq = _sqnorm(hip, gd, n)
    ref = (g.double() ** 2).sum()
    check("sqnorm", nsq[0], ref, X.store_bound(ref, X.tree_sum_bound(ref, X.sqnorm_depth(n)), 0))
    nsq_dev = float(nsq[0])
    assert clip == 0 or abs(math.sqrt(nsq_dev) - clip) > 0.01 * clip
    hyper = torch.tensor([lr, mom, clip], device="cuda")
    with X.ran("sgd_kernel"):
        hip.sgd_momentum_clip(n, wd_, gd, vd, hyper, nsq)
    assert_guard(wb, n, "sgd w"); assert_guard(vb, n, "sgd v"); assert_guard(gb, n, "sgd g")
    w64, v64, bw, bv, ratio = X.sgd64(w, g, v, lr, mom, clip, nsq_dev)
    if n > 100:
        assert ratio >= 0.1, "median |step g| / |mom v| = %g: a wrong step size would hide in v" % ratio
    assert (X.clip_factor64(nsq_dev, clip) < 1) == (case == "clipped")
    check("sgd v", vd, v64, bv, "v n=%d %s" % (n, case)); check("sgd w", wd_, w64, bw, "w n=%d %s" % (n, case))
    assert torch.equal(gd.cpu(), g), "the gradient was modified"


@pytest.mark.parametrize("n", [5, 10007, 2098179])
def test_adam_amsgrad_clip_elementwise(n):
    """Three steps, the second clipped: w, m, v, vhat element by element against adam64 applied to the state the device held before
    the step, with the device's norm; hyper[5] counts 1, 2, 3.  n = 2098179 = 2 x 1048576 + 1027: the grid-stride loop turns."""
    hip = _hip()
    gen = torch.Generator().manual_seed(n)
    f = np.float32
    hyper = torch.tensor([1e-3, 0.9, 0.999, 1e-7, 5.0, 0.0, float(f(1) - f(0.9)), float(f(1) - f(0.999))], device="cuda")
    bufs = {k: with_slack(t) for k, t in (("w", torch.randn(n, generator=gen)), ("m", torch.zeros(n)), ("v", torch.zeros(n)), ("vhat", torch.zeros(n)))}
    for t in (1, 2, 3):
        g = torch.randn(n, generator=gen) * ((3.0 if t == 2 else 0.001) * (10007.0 / n) ** 0.5 if n > 5 else (9.0 if t == 2 else 0.5))
        gb, gd = with_slack(g)
        before = {k: b[1].cpu().clone() for k, b in bufs.items()}
        nsq = _sqnorm(hip, gd, n)
        nsq_dev = float(nsq[0])
        assert abs(math.sqrt(nsq_dev) - 5.0) > 0.05 and (math.sqrt(nsq_dev) >= 5.0) == (t == 2)
        with X.ran("adam_tick_kernel"):
            hip.adam_amsgrad_clip(n, bufs["w"][1], gd, bufs["m"][1], bufs["v"][1], bufs["vhat"][1], hyper, nsq)
        torch.cuda.synchronize()
        assert float(hyper[5]) == t
        ref = X.adam64(before["w"], g, before["m"], before["v"], before["vhat"], hyper.cpu(), nsq_dev)
        for k, (buf, view) in bufs.items():
            assert_guard(buf, n, "adam " + k)
            check("adam " + k, view, ref[k][0], ref[k][1], "adam %s step %d n=%d" % (k, t, n))
        X.assert_sensitive(ref["m"][0], what="adam m")


def test_scale_f32_elementwise():
    hip = _hip()
    n = 2098179
    x = torch.randn(n, generator=torch.Generator().manual_seed(9))
    xb, xd = with_slack(x)
    with X.ran("scale_kernel"):
        hip.scale_f32(n, xd, 0.3)
    assert_guard(xb, n, "scale_f32")
    ref = x.double() * X.f32v(0.3)
    check("scale_f32", xd, ref, X.store_bound(ref, torch.zeros_like(ref), 0))


# ===================================================================================================================== gradient finalisation
FIN_SHAPES = [(144, 24, 24), (2048, 3, 8), (1024, 4, 8), (1024, 13, 16), (64, 64, 64), (147, 64, 64), (4608, 512, 512), (2560, 1024, 1024),
              (1024, 4096, 4096), (576, 64, 72)]
PAD_SENTINEL = 3.0e7                                      # in the padded columns of dw_raw: must not leak into any output


def _fin_case(K, N, ldn, seed):
    g = torch.Generator().manual_seed(seed)
    dwp = torch.full((K, ldn), PAD_SENTINEL)
    dwp[:, :N] = torch.randn(K, N, generator=g)
    return dict(dwp=dwp, cs=torch.randn(N, generator=g) * 5, W=torch.randn(K, N, generator=g) / K ** 0.5, b=torch.randn(N, generator=g),
                gamma=torch.rand(N, generator=g) + 0.5, mean=torch.randn(N, generator=g), var=torch.rand(N, generator=g) + 0.5)


def _finalize(c, K, N, ldn, bias, bn, trainable, bn_trainable, sq):
    """One launch of urso_param_grad_finalize(_sq) on guarded outputs -> dict of output views (+ 'slots')."""
    hip = _hip()
    eps, wd = 1e-3, 1e-2
    d = lambda k: dev(c[k])
    out = {"gw": guarded(K * N)}
    if bias:
        out["gb"] = guarded(N)
    if bn:
        out["ggamma"], out["gbeta"] = guarded(N), guarded(N)
    ws = torch.empty(hip.param_grad_finalize_ws_bytes(K, N) // 4 + 4, device="cuda")
    o = lambda k: out[k][1] if k in out else None
    args = (K, N, ldn, d("dwp"), d("cs"), d("W"), d("b") if bias else None, d("gamma") if bn else None, d("mean") if bn else None,
            d("var") if bn else None, eps, wd, trainable, bn_trainable, o("gw"), o("gb"), o("ggamma"), o("gbeta"), ws)
    nslots = hip.param_grad_finalize_sq_slots(K, N)
    with X.ran("finalize_mat_kernel"):
        if sq:
            out["slots"] = guarded(nslots)
            hip.param_grad_finalize_sq(*args, out["slots"][1])
        else:
            hip.param_grad_finalize(*args)
    for k, (buf, view) in out.items():
        assert_guard(buf, view.numel(), "finalize " + k)
    return {k: v[1] for k, v in out.items()}


@pytest.mark.parametrize("KNl", FIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_param_grad_finalize_elementwise(KNl):
    """urso_param_grad_finalize and its _sq form against the closed form finalize64 (random dw_raw / colsum, no conv needed): the 16-byte
    vector body, the scalar body of the real heads (N = 3 / 4 / 13 in a padded row), several row slabs, a padded row stride on the vector
    path; with and without bias and BN, frozen layers, and a sentinel in dw_raw's padded columns.  The _sq slots: exactly
    urso_param_grad_finalize_sq_slots are written, and urso_sqnorm_final over them -- as urso_sqnorm over the stored gradients laid
    out flat -- is the sum of squares of what was stored.  A layer with neither bias nor BN has its ceil(N / 256) channel slots
    cleared to 0 by the entry point."""
    hip = _hip()
    K, N, ldn = KNl
    ks = (hip.param_grad_finalize_ws_bytes(K, N) - 256) // (4 * N)
    c = _fin_case(K, N, ldn, K + N)
    big = K * N > 2 ** 21
    variants = [(True, True, 1, 1), (False, True, 1, 1), (True, False, 1, 1), (False, False, 1, 1), (True, True, 0, 1), (True, True, 1, 0)]
    if big:
        variants = [variants[0], variants[3]]
    for bias, bn, trainable, bn_trainable in variants:
        ref = X.finalize64(c["dwp"][:, :N], c["cs"], c["W"], c["b"] if bias else None, c["gamma"] if bn else None, c["mean"], c["var"], 1e-3, 1e-2)
        bnd = X.finalize_bounds(ref, K, N, ldn, ks)
        for name in ref:
            X.assert_sensitive(ref[name][0], what="finalize " + name)
        zero = lambda t: torch.zeros_like(t)
        for sq in (0, 1):
            got = _finalize(c, K, N, ldn, bias, bn, trainable, bn_trainable, sq)
            assert set(got) - {"slots"} == set(ref)
            tag = "%s bias=%d bn=%d trainable=%d bn_trainable=%d sq=%d" % (KNl, bias, bn, trainable, bn_trainable, sq)
            for name in ref:
                frozen = (name in ("gw", "gb") and not trainable) or (name in ("ggamma", "gbeta") and not bn_trainable)
                if frozen:
                    X.assert_exact(got[name].reshape(ref[name][0].shape), zero(ref[name][0]), "%s %s (frozen)" % (name, tag))
                else:
                    check("finalize " + name, got[name], ref[name][0], bnd[name], "%s %s" % (name, tag))
            if sq:
                slots = got["slots"]
                nslots = slots.numel()
                stored = torch.cat([got[k].reshape(-1) for k in ("gw", "gb", "ggamma", "gbeta") if k in got])
                want = (stored.double().cpu() ** 2).sum()
                depth = X.finalize_sq_depth(K, N, ldn, ks, nslots)
                ob, o1 = guarded(1)
                hip.sqnorm_final(slots, o1)
                assert_guard(ob, 1, "sqnorm_final")
                check("finalize sq slots", o1[0], want, X.store_bound(want, X.tree_sum_bound(want, depth), 0), "slots " + tag)
                flat = _sqnorm(hip, stored.contiguous(), stored.numel())
                check("sqnorm", flat[0], want, X.store_bound(want, X.tree_sum_bound(want, X.sqnorm_depth(stored.numel())), 0), "flat " + tag)
                if not bias and not bn:
                    assert float(slots[nslots - -(-N // 256):].abs().max()) == 0.0, "channel slots of a layer without bias / BN are cleared"


# ===================================================================================================================== batch-statistics BatchNorm
BN_SHAPES = [(2, 8), (130, 40), (257, 24), (600, 264), (3000, 2048), (20000, 256), (100003, 64), (5000, 24), (130, 20), (130, 6)]


def _bn_fixed(M, N, dt):
    """Which template variant urso_bn_apply / urso_bn_backward choose: FIXED when the grid's stride is a multiple of the row's vectors."""
    ve = 4 if dt == 0 else 8
    nvec = M * N // ve
    blocks = min(-(-nvec // 256), 4096)
    return (blocks * 256) % (N // ve) == 0


def test_bn_shapes_reach_both_template_variants():
    seen = {(dt, _bn_fixed(M, N, dt)) for M, N in BN_SHAPES for dt in (0, 1, 2) if N % (4 if dt == 0 else 8) == 0}
    assert seen == {(dt, f) for dt in (0, 1, 2) for f in (True, False)}


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("MN", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_stat_bn_elementwise(MN, dt):
    """urso_bn_batch_stats / urso_bn_apply / urso_bn_backward: statistics and moving statistics per channel, y and dz element by element
    (rounded once), dbeta / dgamma per channel; a constant channel (variance clamps at 0) and a channel of mean 1000 with unit spread;
    relu 0 / 1, with and without residual, bn_trainable 0 / 1.  N that is not a multiple of the 16-byte vector ((130, 20) in 16 bits,
    (130, 6) in every type) is refused with an error, nothing launched."""
    hip = _hip()
    M, N = MN
    ve = 4 if dt == 0 else 8
    t = X.tdtype(dt)
    eps, mom = 1e-3, 0.99
    ws = torch.empty(hip.bn_ws_bytes(M, max(N, ve)) // 8 + 8, dtype=torch.float64, device="cuda")
    if N % ve:
        z = torch.zeros(M, N, dtype=t, device="cuda"); f = lambda: torch.zeros(N, device="cuda")
        mb, m1 = guarded(N)
        with pytest.raises(hip.UrsoHipError):
            hip.bn_batch_stats(M, N, dt, z, ws, m1, f(), None, None, mom, eps)
        with pytest.raises(hip.UrsoHipError):
            hip.bn_apply(M, N, dt, z, f(), f(), f(), f(), eps, None, 0, torch.empty_like(z))
        with pytest.raises(hip.UrsoHipError):
            hip.bn_backward(M, N, dt, z, z, f(), f(), f(), eps, ws, f(), f(), 1, f(), f(), torch.empty_like(z))
        torch.cuda.synchronize()
        assert bool(torch.isnan(mb).all())
        return
    g = torch.Generator().manual_seed(M + N + dt)
    z = torch.randn(M, N, generator=g) * 2 + torch.randn(N, generator=g)
    z[:, 0] = 0.75
    z[:, 1] = torch.randn(M, generator=g) + 1000.0
    z = z.to(t); res = torch.randn(M, N, generator=g).to(t); gy = torch.randn(M, N, generator=g).to(t)
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    mm, mv = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    Z, R, G_ = dev(z, dt), dev(res, dt), dev(gy, dt)
    meanb, mean_d = guarded(N); varb, var_d = guarded(N); mmb, mmd = with_slack(mm); mvb, mvd = with_slack(mv)
    with X.ran("bn_colreduce_kernel"):
        hip.bn_batch_stats(M, N, dt, Z, ws, mean_d, var_d, mmd, mvd, mom, eps)
    for b_, nm in ((meanb, "mean"), (varb, "var"), (mmb, "moving mean"), (mvb, "moving variance")):
        assert_guard(b_, N, "bn " + nm)
    st = X.bn_stats64(z, mm, mv, mom, eps)
    for nm, got in (("mean", mean_d), ("var", var_d), ("mmean", mmd), ("mvar", mvd)):
        check("bn " + nm, got, st[nm][0], st[nm][1], "%s %s dt=%d" % (nm, MN, dt))
    fixed = _bn_fixed(M, N, dt)
    sym = ("bn_apply_kernel", "Lb1E" if fixed else "Lb0E")
    mean_h, var_h = mean_d.cpu(), var_d.cpu()
    for relu in (0, 1):
        for r_ in (R, None):
            yb, y = guarded(M * N, dt)
            with X.ran(sym):
                hip.bn_apply(M, N, dt, Z, mean_d, var_d, dev(gamma), dev(beta), eps, r_, relu, y)
            assert_guard(yb, M * N, "bn_apply y")
            y64, by = X.bn_apply64(z, mean_h, var_h, gamma, beta, eps, res if r_ is not None else None, relu, dt)
            check("bn y", y.reshape(M, N), y64, by, "y %s dt=%d relu=%d res=%d" % (MN, dt, relu, r_ is not None))
    for bn_trainable in (1, 0):
        dbb, db = guarded(N); dgb, dg = guarded(N); gbb, gbe = guarded(N); ggb, gga = guarded(N); dzb, dz = guarded(M * N, dt)
        with X.ran("bn_colreduce_kernel"):
            hip.bn_backward(M, N, dt, G_, Z, mean_d, var_d, dev(gamma), eps, ws, db, dg, bn_trainable, gbe, gga, dz)
        for b_, n_, nm in ((dbb, N, "dbeta"), (dgb, N, "dgamma"), (gbb, N, "gbeta"), (ggb, N, "ggamma"), (dzb, M * N, "dz")):
            assert_guard(b_, n_, "bn_backward " + nm)
        bw = X.bn_backward64(gy, z, mean_h, var_h, gamma, eps, dt, db.cpu(), dg.cpu())
        check("bn dbeta", db, *bw["dbeta"]); check("bn dgamma", dg, *bw["dgamma"])
        check("bn dz", dz.reshape(M, N), bw["dz"][0], bw["dz"][1], "dz %s dt=%d" % (MN, dt))
        if bn_trainable:
            assert torch.equal(gbe, db) and torch.equal(gga, dg)
        else:
            assert float(gbe.abs().max()) == 0.0 and float(gga.abs().max()) == 0.0
