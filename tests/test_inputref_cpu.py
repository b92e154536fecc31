"""tests/inputref.py proven on the CPU before it judges a kernel (the pattern of tests/test_exactprobe_cpu.py): a NumPy float32 simulation
of every input-side kernel -- the device's arithmetic: float32 sums in the kernel's tap order, the 2-D blur weights as products of two
float32 exponentials -- must be ACCEPTED by assert_equal_off_ties / byte equality against the float64 / integer references, and the same
simulation with one defect injected must be REJECTED, one defect at a time.  Also: the blur against scipy.ndimage.correlate1d(mode="mirror"),
the two warp references against each other on the edge maps of the GPU tests, and the judge's own edges.

No golden file under tests/golden/ covers the warp, the grey conversion or the sim2real stages (they are "parity unpinned": neither OpenCV nor
imgaug exists where the goldens were made), so there is no overlap to re-check through these helpers."""
import numpy as np
import pytest

import inputref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------ float32 simulation of urso_sim2real_op
def _sat32(v, half_up=False):
    v = np.asarray(v, dtype=F32)
    r = np.floor(v + F32(0.5)) if half_up else np.rint(v)
    return np.clip(r, 0, 255).astype(np.uint8)


def sim_stage32(img, code, par, seed=0, mask=None, defect=None):
    """One stage as the kernel computes it (float32), with an optional injected defect."""
    H, W = img.shape[:2]
    f = img.astype(F32)
    half_up = defect == "half_up"
    code = int(code)
    if code == 0:
        if defect == "noise_x_only":
            n = np.tile(R.noise_field(seed, W, par[0], dtype=F32), H)
        else:
            n = R.noise_field(0 if defect == "noise_no_seed" else seed, H * W, par[0], dtype=F32)
        return _sat32(f + n.reshape(H, W, 1), half_up)
    if code == 1:
        s = F32(par[0])
        if s < F32(1e-3):
            return img.copy()
        r = int(np.floor(F32(3) * s)) if defect == "blur_floor" else int(np.ceil(F32(3) * s))
        d = np.arange(-r, r + 1).astype(F32)
        k = np.exp(F32(-0.5) * d * d / (s * s)).astype(F32)
        pad = np.pad(f, ((r, r), (r, r), (0, 0)), mode="symmetric" if defect == "blur_reflect" else "reflect")
        acc = np.zeros_like(f); wsum = F32(0)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                w = F32(k[dy] * k[dx])
                acc = acc + w * pad[dy:dy + H, dx:dx + W]; wsum = F32(wsum + w)
        if defect == "blur_unnormalised":
            wsum = F32(2 * np.pi) * s * s                      # the continuous Gaussian's norm instead of the sum of the taps
        v = acc / wsum
        if defect == "blur_bias":
            v = v + F32(0.4)
        return _sat32(v, half_up)
    if code == 2:
        return _sat32(f + F32(par[0]), half_up)
    if code == 3:
        return _sat32(f * F32(par[0]), half_up)
    if code == 4:
        dh, dw = int(par[0]), int(par[1])
        m = np.asarray(mask).reshape(-1)[:dh * dw].reshape(dh, dw).astype(bool)
        return np.where(m[R.dropout_index(H, dh)][:, R.dropout_index(W, dw)][:, :, None], 0, img).astype(np.uint8)
    return img.copy()


def sim_batch32(frames, draw, defect=None):
    """augment.sim2real_batch as the device runs it: grey, then five launches over the batch with the per-sample op code of the slot and the
    dropout flags in one [B, stride] buffer.  Returns (grey, [batch after launch 1 .. 5])."""
    B = len(frames)
    a = R.grey3(frames)
    grey = a.copy()
    stride = max(m.size for m in draw["masks"])
    drop = np.zeros((B, stride), dtype=np.uint8)
    for i, m in enumerate(draw["masks"]):
        drop[i, :m.size] = m.reshape(-1)
    flat = drop.reshape(-1)
    outs = []
    for slot in range(5):
        nxt = np.empty_like(a)
        for b in range(B):
            op = slot if defect == "default_order" else draw["order"][b, slot]
            code = int(op) if draw["apply"][b] else -1
            par = draw["par"][b, op]
            dh, dw = int(draw["par"][b, 4, 0]), int(draw["par"][b, 4, 1])
            row = flat[b * dh * dw:b * dh * dw + dh * dw] if defect == "drop_stride" else drop[b]
            nxt[b] = sim_stage32(a[b], code, par, int(draw["seeds"][b]), row)
        a = nxt
        outs.append(a.copy())
    return grey, outs


def _frame(h=72, w=96, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    g[0, :4] = (0, 255, 1, 254)
    return np.repeat(g[..., None], 3, -1)


def _judge(img, code, par, seed=0, mask=None, defect=None, delta=None):
    ref, un = R.sim2real_stage(img, code, par, seed, mask)
    delta = R.stage_delta(code, par) if delta is None else delta
    got = sim_stage32(img, code, par, seed, mask, defect)
    return R.assert_equal_off_ties(got, ref, un, delta, 4 * delta, "code %d %s" % (code, defect))


PAR = lambda *v: np.array(list(v) + [0] * (4 - len(v)), dtype=F32)


# ------------------------------------------------------------------------------------------------ the judge itself
def test_judge_edges():
    un = np.array([10.49995, 10.2, 254.50001, 3.5])
    ref = R.sat_u8(un)
    assert list(ref) == [10, 10, 255, 4] and list(R.near_tie(un, 1e-4)) == [True, False, True, True]
    got = ref.copy(); got[0] = 11
    assert R.assert_equal_off_ties(got, ref, un, 1e-4, 0.25)["excused"] == 1
    with pytest.raises(AssertionError, match="more than the cap"):
        R.assert_equal_off_ties(got, ref, un, 1e-4, 0.2)
    with pytest.raises(AssertionError, match="not at a tie"):
        R.assert_equal_off_ties(got, ref, un, 1e-5, 1.0)                      # 10.49995 is 5e-5 from the tie
    got = ref.copy(); got[1] = 11
    with pytest.raises(AssertionError, match="not at a tie"):
        R.assert_equal_off_ties(got, ref, un, 1e-4, 1.0)                      # not near a tie at all
    got = ref.copy(); got[0] = 12
    with pytest.raises(AssertionError, match="not at a tie"):
        R.assert_equal_off_ties(got, ref, un, 1e-4, 1.0)                      # two levels away
    got = ref.copy(); got[0] = 9
    with pytest.raises(AssertionError, match="not at a tie"):
        R.assert_equal_off_ties(got, ref, un, 1e-4, 1.0)                      # one level away, on the wrong side of the tie
    got = ref.copy(); got[3] = 3
    with pytest.raises(AssertionError):
        R.assert_equal_off_ties(got, ref, un, 0.0, 0.0)                       # delta 0: the half-even rule is part of the reference


def test_derived_deltas():
    """The figures docs/LAB_NOTEBOOK.md quotes; a uniformly distributed fraction stays under cap = 4 delta with room (2 delta expected)."""
    assert 2.0e-5 < R.delta_noise(2.55) < 3.0e-5
    assert R.delta_blur(0.0005) == 0.0 and [R.blur_radius(s) for s in (0.34, 1.0, 1.5)] == [2, 3, 5]
    assert all(1.0e-3 < R.delta_blur(s) < 6.0e-3 for s in (0.34, 1.0, 1.5))
    assert R.delta_multiply(0.5) == 0.0 and R.delta_multiply(2.0) == 0.0 and 0 < R.delta_multiply(1.7) < 4e-5
    un = np.random.default_rng(0).random(1 << 20) * 255
    for d in (R.delta_noise(2.55), R.delta_blur(1.5)):
        assert R.tie_share(un, d) < 3 * d


# ------------------------------------------------------------------------------------------------ noise
def test_noise_field_float32_against_float64():
    """The float32 evaluation of the restatement against the float64 one on a 1200 x 1920 frame: inside delta_noise's function part, and the
    rounded grey levels differ at near-ties only."""
    npix = 1200 * 1920
    n64 = R.noise_field(0x1234567, npix, 2.55)
    n32 = R.noise_field(0x1234567, npix, 2.55, dtype=F32)
    assert n32.dtype == F32 and np.abs(n32 - n64).max() < 1.2e-5
    assert abs(n64.mean()) < 0.01 and abs(n64.std() - 2.55) < 0.01
    un = 128.0 + n64
    d = R.delta_noise(2.55)
    assert R.tie_share(un, d) < 4 * d
    st = R.assert_equal_off_ties(_sat32(F32(128) + n32), R.sat_u8(un), un, d, 4 * d, "noise 2.3 M")
    print(R.report(st))
    u1, u2, _ = R.noise_uniforms(7, 1 << 16)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert float(F32(1.0) / F32(16777217.0)) == 2.0 ** -24


@pytest.mark.parametrize("defect", ["noise_x_only", "noise_no_seed"])
def test_noise_defects_rejected(defect):
    img = _frame()
    _judge(img, 0, PAR(2.55), seed=0x80000001)
    for seed in (0x80000001, 1):
        with pytest.raises(AssertionError):
            _judge(img, 0, PAR(2.55), seed=seed, defect=defect)
    # seeds that differ in one bit (bit 0, bit 31) give different fields
    a = R.noise_field(0x1000, 4096, 2.55)
    assert np.abs(a - R.noise_field(0x1001, 4096, 2.55)).max() > 1 and np.abs(a - R.noise_field(0x80001000, 4096, 2.55)).max() > 1


# ------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize("sigma", [0.34, 1.0, 1.2, 1.5])
def test_blur_reference_against_scipy(sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    img = _frame(40, 56, 3)
    k = R.blur_taps(sigma)
    assert len(k) == 2 * R.blur_radius(sigma) + 1 and abs(k.sum() - 1) < 1e-15 and np.array_equal(k, k[::-1])
    sp = ndi.correlate1d(ndi.correlate1d(img.astype(np.float64), k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
    assert np.abs(sp - R.blur_reference(img, sigma)).max() < 1e-11


@pytest.mark.parametrize("sigma", [0.0005, 0.34, 1.0, 1.5])
def test_blur_clean_simulation_accepted(sigma):
    img = _frame()
    _, un = R.sim2real_stage(img, 1, PAR(sigma))
    d = R.delta_blur(sigma)
    assert R.tie_share(un, d) <= 4 * d
    print(R.report(_judge(img, 1, PAR(sigma))))


@pytest.mark.parametrize("defect", ["blur_floor", "blur_reflect", "blur_unnormalised", "blur_bias"])
def test_blur_defects_rejected(defect):
    img = _frame()
    sigma = 1.2                                                # 3 sigma = 3.6: floor and ceil differ
    _judge(img, 1, PAR(sigma))
    with pytest.raises(AssertionError):
        _judge(img, 1, PAR(sigma), defect=defect)


def test_uniform_one_level_offset_is_no_longer_accepted():
    """What `d <= 1` let through: the + 0.4 bias moves ~40 % of the pixels by one level, none of them further."""
    img = _frame()
    ref, _ = R.sim2real_stage(img, 1, PAR(1.2))
    got = sim_stage32(img, 1, PAR(1.2), defect="blur_bias")
    d = np.abs(got.astype(int) - ref.astype(int))
    assert d.max() == 1 and 0.3 < (d == 1).mean() < 0.5        # the old assertion passes ...
    with pytest.raises(AssertionError, match="not at a tie"):
        _judge(img, 1, PAR(1.2), defect="blur_bias")           # ... the new one does not


# ------------------------------------------------------------------------------------------------ add / multiply / dropout / rounding rule
def test_exact_stages_and_the_half_even_rule():
    img = _frame()
    for code, par in ((2, PAR(-20)), (2, PAR(20)), (3, PAR(0.5)), (3, PAR(2.0)), (-1, PAR(0))):
        st = _judge(img, code, par)
        assert st["delta"] == 0.0 and st["excused"] == 0
    ref, un = R.sim2real_stage(img, 3, PAR(0.5))
    assert ref[0, 0, 0] == 0 and ref[0, 1, 0] == 128 and ref[0, 2, 0] == 0 and ref[0, 3, 0] == 127     # 0, 127.5 -> 128, 0.5 -> 0, 127
    assert (R.near_tie(un, 0.0)).mean() > 0.3
    with pytest.raises(AssertionError):
        _judge(img, 3, PAR(0.5), defect="half_up")
    assert R.multiply_tie_free(1.7183) and not R.multiply_tie_free(1.7) and R.multiply_tie_free(0.5)
    _judge(img, 3, PAR(1.7183))
    ref, _ = R.sim2real_stage(img, 2, PAR(20))
    assert ref[0, 1, 0] == 255 and ref[0, 0, 0] == 20
    ref, _ = R.sim2real_stage(img, 2, PAR(-20))
    assert ref[0, 0, 0] == 0 and ref[0, 1, 0] == 235


def test_pipeline_clean_accepted_defects_rejected():
    B, H, W = 8, 60, 80
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    draw = R.handmade_draw(B, H, W)
    assert draw["apply"].sum() >= 5 and not draw["apply"].all()
    assert all(R.multiply_tie_free(p[3, 0]) for p, a in zip(draw["par"], draw["apply"]) if a)
    assert len({tuple(o) for o, a in zip(draw["order"], draw["apply"]) if a}) == 5
    assert len({m.size for m in draw["masks"]}) >= 4 and max(m.size for m in draw["masks"]) > 15
    grey, outs = sim_batch32(frames, draw)
    stats, excused = R.judge_pipeline_teacher_forced(grey, outs, draw, check_share=False)
    assert sum(s["n"] for s in stats) == 5 * B * H * W * 3
    ref = R.sim2real_pipeline(frames, draw)
    clean = excused == 0                                       # no tie excused in any stage: free-running reference = simulation, by induction
    assert clean.sum() >= 4 and np.array_equal(outs[-1][clean], ref[clean])
    skipped = ~draw["apply"]
    assert np.array_equal(outs[-1][skipped], grey[skipped]) and np.array_equal(ref[skipped], grey[skipped])
    assert (np.abs(outs[-1].astype(int) - ref.astype(int)) > 1).mean() < 0.01          # free-running: a tie in one stage feeds the next
    for defect in ("drop_stride", "default_order"):
        g2, o2 = sim_batch32(frames, draw, defect)
        with pytest.raises(AssertionError):
            R.judge_pipeline_teacher_forced(g2, o2, draw, check_share=False)


# ------------------------------------------------------------------------------------------------ warp
def _sim_warp(img, Minv, interp, defect=None):
    """The kernel's arithmetic per pixel in plain Python (double coordinates, llrint, 64-bit integers), with an optional defect."""
    H, W, C = img.shape
    M = np.asarray(Minv, dtype=np.float64).reshape(9)
    out = np.zeros_like(img)
    rnd = (lambda v: int(np.trunc(v))) if defect == "trunc" else (lambda v: int(np.rint(v)))
    for y in range(H):
        for x in range(W):
            X, Y, Wd = M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5], M[6] * x + M[7] * y + M[8]
            iw = ((32.0 if interp == "linear" else 1.0) / Wd) if Wd != 0.0 else 0.0
            qx = rnd(max(min(X * iw, 2147483647.0), -2147483648.0)); qy = rnd(max(min(Y * iw, 2147483647.0), -2147483648.0))
            if interp != "linear":
                if 0 <= qx < W and 0 <= qy < H:
                    out[y, x] = img[qy, qx]
                continue
            sx, sy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
            ws = ((32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32)
            v = np.zeros(C, dtype=np.int64)
            for wgt, (yy, xx) in zip(ws, ((sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1))):
                if 0 <= yy < H and 0 <= xx < W:
                    v += wgt * img[yy, xx].astype(np.int64)
            out[y, x] = (((v + (0 if defect == "no_round" else 1 << 14)) >> 15) & 255).astype(np.uint8)
    return out


def _rot_map(H, W, deg, pitch=0.0, yaw=0.0):
    from oracle import pose_math as P
    f = 1.2 * W
    K = np.array([[f, 0, W / 2.0], [0, -f, H / 2.0], [0, 0, 1.0]])
    return P.invert3x3(K @ P.euler2SO3_left(pitch, yaw, deg) @ np.linalg.inv(K))


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_warp_references_agree_and_reject_defects(interp):
    from oracle import pose_math as P
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(30, 41, 3), dtype=np.uint8)
    for M in (_rot_map(30, 41, 85.0), _rot_map(30, 41, -33.0, 4.0, -6.0)):
        a, b = R.warp_reference(img, M, interp)
        assert np.array_equal(a, b) and (a != 0).any(-1).mean() > 0.2
        assert np.array_equal(_sim_warp(img, M, interp), b)
        assert not np.array_equal(_sim_warp(img, M, interp, "trunc"), b)
        if interp == "linear":
            assert not np.array_equal(_sim_warp(img, M, interp, "no_round"), b)
    rows = [0, 7, 29]
    part = P.warp_perspective(img, M, inverse_map=True, interp=interp, rows=rows)
    assert np.array_equal(part[rows], b[rows]) and not part[[1, 8]].any()


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("name", sorted(R.warp_edge_maps(24, 40)))
def test_warp_references_agree_on_edge_maps(name, interp):
    """The hand-built inverse maps of the GPU edge test: W == 0 on a column, W < 0 on half the frame, coordinates past +-2^31, taps at -1, W - 1,
    32767 and 32768, half-pixel shifts -- the oracle's per-pixel loop and the integer statement agree byte for byte."""
    H, W = 24, 40
    img = np.random.default_rng(2).integers(1, 256, size=(H, W, 3), dtype=np.uint8)
    M, check = R.warp_edge_maps(H, W)[name]
    a, b = R.warp_reference(img, M, interp)
    assert np.array_equal(a, b), name
    assert np.array_equal(_sim_warp(img, M, interp), b), name
    if check is not None:
        check(img, b, interp)


def test_mold_bits_against_torch():
    torch = pytest.importorskip("torch")
    img = np.random.default_rng(3).integers(0, 256, size=(2, 9, 16, 3), dtype=np.uint8)
    mean = np.array([123.7, 116.8, 103.9], dtype=F32)
    for dt, tdt in ((1, torch.bfloat16), (2, torch.float16)):
        for m in (None, mean):
            f = torch.as_tensor(img).float() - (0 if m is None else torch.as_tensor(m))
            want = f.to(tdt).view(torch.int16).numpy().view(np.uint16)
            got = R.mold_bits(img, m, dt)
            assert np.array_equal(got[..., :3], want) and not got[..., 3].any()
