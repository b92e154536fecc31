"""The input-side kernels at real frame sizes against exact references (tests/inputref.py; proven in tests/test_inputref_cpu.py):
urso_warp_perspective, urso_rgb_to_grey3, urso_sim2real_op, urso_mold_images, augment.sim2real_batch and the 32-bit guard of
urso_maxpool3x3s2_fwd.  A bug here raises no error and trips no parity gate: the network just learns from slightly wrong pixels.

Every shape that claims to drive a grid-stride loop through a second iteration asserts so from the launch arithmetic, restated next to the
line of the .hip file it mirrors.  Comparisons are byte equality, or equality off ties (assert_equal_off_ties: delta and cap are derived
in tests/inputref.py, not measured).  Run with -s to see, per kernel, the elements compared, those excused as ties, delta and cap.

Parity with the real OpenCV / imgaug stays unpinned (neither library is available): the references restate the documented arithmetic.
The per-pixel Python loop of oracle.pose_math.warp_perspective judges a sample of 16 rows of a full-size frame by default and every
row with URSO_FULL_SIZE_ORACLE=1 (minutes); the vectorised integer statement judges every pixel always."""
import os

import numpy as np
import pytest
import torch

import inputref as R

pytestmark = pytest.mark.gpu

FULL = os.environ.get("URSO_FULL_SIZE_ORACLE", "0") == "1"


def _hip():
    import ursonet_amd.hip as hip
    return hip


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _par(*v):
    return np.array(list(v) + [0] * (4 - len(v)), dtype=np.float32)


# ------------------------------------------------------------------------------------------------ warp, real frames
def _strided_warp(npix):
    """augment.hip, urso_warp_perspective: `int blocks = (int)((npix + 255) / 256); if (blocks > 8192) blocks = 8192;` and warp_kernel's
    `i += (size_t)gridDim.x * blockDim.x` (grey3_kernel: the same two lines in urso_rgb_to_grey3): iterations of the first thread."""
    blocks = min((npix + 255) // 256, 8192)
    return -(-npix // (blocks * 256))


@pytest.mark.parametrize("interp", ["linear", "nearest"])
@pytest.mark.parametrize("shape", [(2, 960, 1280, 3), (2, 1200, 1920, 1), (2, 1200, 1920, 3)], ids=["urso", "speed_grey", "speed_rgb"])
def test_warp_real_frame_sizes(shape, interp):
    """A rotate_cam-style perturbation (frame 0) and an in-plane rotation of 85 degrees (frame 1; -85 for the one-channel case), where most of
    the border lies outside the source, at URSO and SPEED frame sizes: byte equality with the integer statement on every pixel and with the
    oracle's loop on the sampled rows."""
    from ursonet_amd import augment as A
    from ursonet_amd.dataset import Camera
    B, H, W, C = shape
    assert _strided_warp(B * H * W) >= 2
    rng = np.random.default_rng(H + C)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    cam = Camera(W, H)
    pyr = np.array([[6.5, -8.25, 9.0], [0.0, 0.0, -85.0 if C == 1 else 85.0]])
    Ms = np.stack([A.rotation_homography(cam.K, A.euler2SO3_left(*p)) for p in pyr])
    out = A.warp_images(img, Ms, interp=interp).cpu().numpy()
    rows = None if FULL else sorted(set(np.linspace(0, H - 1, 16).astype(int)))
    for b in range(B):
        Mi = A.invert_homography(Ms[b])
        loop, full = R.warp_reference(img[b], Mi, interp, rows=rows)
        outside = (full == 0).all(-1).mean()
        assert 0.15 < outside < 0.9                                          # the case really samples the image, and really leaves it (corners, border)
        bad = (out[b] != full).any(-1)
        assert not bad.any(), "sample %d: %d pixels differ from the integer statement (first at %s)" % (b, bad.sum(), np.argwhere(bad)[0])
        sel = slice(None) if rows is None else rows
        assert np.array_equal(out[b][sel], loop[sel]), "sample %d differs from oracle.pose_math.warp_perspective" % b
    print("input-side warp %s %s: %d pixels compared byte for byte (oracle loop on %s rows)" % (shape, interp, B * H * W, "all" if FULL else 16))


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_warp_edges(interp):
    """Hand-built inverse maps against both references: W exactly zero on a destination column (-> coordinates (0, 0)), W negative on half the
    frame, coordinates clamped at +-2^31, taps at -1, W - 1, 32767 and 32768 (the last two on a frame 32800 pixels wide, where they read real
    pixels: the 1/32-pixel fixed-point path beyond 2^15), half-pixel translations in x, in y and in both against shifted integer averages.
    Every load of warp_kernel is bounds-checked (x0 / x1 / y0 / y1 select index 0 for a tap outside, and the tap's value is not used), so
    none of these maps can make it read outside the frame."""
    hip = _hip()
    for H, W, C, names in ((24, 40, 3, None), (2, 32800, 1, ("tap_at_32767", "tap_at_32768_half", "tap_at_32768", "half_xy", "tap_at_w_minus_1_half"))):
        img = np.random.default_rng(W).integers(1, 256, size=(H, W, C), dtype=np.uint8)
        maps = R.warp_edge_maps(H, W)
        names = sorted(maps) if names is None else names
        src = _dev(np.repeat(img[None], len(names), 0))
        m = _dev(np.stack([maps[n][0].reshape(9) for n in names]))
        dst = torch.full_like(src, 0xA5)
        hip.warp_perspective(len(names), H, W, C, 1 if interp == "linear" else 0, src, m, dst)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        for k, n in enumerate(names):
            loop, full = R.warp_reference(img, maps[n][0], interp)
            assert np.array_equal(loop, full), n
            assert np.array_equal(out[k], full), "%s (%d x %d): %d bytes differ" % (n, H, W, (out[k] != full).sum())
            if maps[n][1] is not None:
                maps[n][1](img, out[k], interp)
        if W > 32768:
            k = names.index("tap_at_32767")
            assert np.array_equal(out[k][:, :W - 32767], img[:, 32767:]) and not out[k][:, W - 32767:].any()


# ------------------------------------------------------------------------------------------------ grey
def test_grey3_every_rgb_triple():
    """One 4096 x 4096 frame holding all 2^24 RGB triples against the float64 sum truncated by the uint8 assignment: every .999... case at once,
    and eight iterations of grey3_kernel's stride loop."""
    hip = _hip()
    n = 1 << 24
    assert _strided_warp(n) == 8
    idx = np.arange(n, dtype=np.uint32)
    rgb = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    x = _dev(rgb)
    g = torch.full_like(x, 0xA5)
    hip.rgb_to_grey3(1, 4096, 4096, x, g)
    torch.cuda.synchronize()
    got, ref = g.cpu().numpy(), R.grey3(rgb)
    assert np.array_equal(got, ref), "%d of 2^24 triples differ" % (got != ref).any(-1).sum()
    print("input-side grey3: %d triples compared byte for byte" % n)


# ------------------------------------------------------------------------------------------------ urso_sim2real_op
def _strided_s2r(H, W):
    """augment.hip, urso_sim2real_op: `int bx = (H * W + 255) / 256; if (bx > 1024) bx = 1024;` per image (grid dim3(bx, B)) and
    sim2real_op_kernel's `i += gridDim.x * blockDim.x`."""
    bx = min((H * W + 255) // 256, 1024)
    return -(-(H * W) // (bx * 256))


def _run_stage(frames, codes, pars, seeds, masks):
    """One urso_sim2real_op launch over a batch; masks: per-sample flag arrays, laid out at a stride LARGER than the largest mask."""
    hip = _hip()
    B, H, W, _ = frames.shape
    stride = max(m.size for m in masks) + 7
    drop = np.zeros((B, stride), dtype=np.uint8)
    for i, m in enumerate(masks):
        drop[i, :m.size] = m.reshape(-1)
    src = _dev(frames)
    dst = torch.full_like(src, 0xA5)
    hip.sim2real_op(B, H, W, src, dst, _dev(np.asarray(codes, dtype=np.int32)), _dev(np.stack(pars).astype(np.float32)),
                    _dev(np.asarray(seeds, dtype=np.uint32).view(np.int32)), _dev(drop), stride)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _frames(B, H, W, seed):
    f = np.random.default_rng(seed).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)      # three independent channels
    f[:, 0, :2] = 0; f[:, 0, 2:4] = 255; f[:, -1, -1] = 255; f[:, -1, -2] = 0
    return f


@pytest.mark.parametrize("shape", [(4, 512, 640), (2, 1200, 1920)], ids=["b4_512x640", "b2_1200x1920"])
def test_sim2real_op_every_code_at_frame_size(shape):
    """Blur at sigma 0.0005 / 0.34 / 1.0 / 1.5 (radius 0 / 2 / 3 / 5), add at +-20 on frames holding 0 and 255, multiply at 0.5 and 2.0 (exact .5
    products: the half-even rule), dropout with the smallest (1 x 1) and the largest (int(0.1 H) x int(0.1 W)) mask sim2real_draw can produce at a
    drop_stride larger than the mask, and copy; two iterations or more of the kernel's stride loop.  Blur is judged off ties with its derived
    delta; everything else byte for byte (delta = 0)."""
    B, H, W = shape
    assert _strided_s2r(H, W) >= 2
    rng = np.random.default_rng(H)
    big = rng.random((int(0.1 * H), int(0.1 * W))) < 0.3
    cases = [(1, _par(0.0005), None), (1, _par(0.34), None), (1, _par(1.0), None), (1, _par(1.5), None),
             (2, _par(-20), None), (2, _par(20), None), (3, _par(0.5), None), (3, _par(2.0), None),
             (4, _par(1, 1), np.ones((1, 1), dtype=bool)), (4, _par(*big.shape), big), (4, _par(1, 1), np.zeros((1, 1), dtype=bool)), (-1, _par(0), None)]
    assert [R.blur_radius(c[1][0]) for c in cases[1:4]] == [2, 3, 5]
    totals = {}
    for k in range(0, len(cases), B):
        chunk = cases[k:k + B]
        chunk = chunk + [cases[-1]] * (B - len(chunk))
        frames = _frames(B, H, W, 100 + k)
        masks = [c[2] if c[2] is not None else np.zeros((1, 1), dtype=bool) for c in chunk]
        refs = []
        for b, (code, par, mask) in enumerate(chunk):                        # the reference first: its own near-tie share must be under the cap
            ref, un = R.sim2real_stage(frames[b], code, par, 0, masks[b])
            delta = R.stage_delta(code, par)
            assert (code == 1 and par[0] >= 1e-3) == (delta > 0)
            if delta > 0:
                share = R.tie_share(un, delta)
                assert share <= 4 * delta, (code, par, share, delta)
                print("input-side reference alone: blur sigma %.4g near-tie share %.3g (delta %.3g)" % (par[0], share, delta))
            refs.append((ref, un, delta))
        out = _run_stage(frames, [c[0] for c in chunk], [c[1] for c in chunk], np.zeros(B, dtype=np.uint32), masks)
        for b, (code, par, mask) in enumerate(chunk):
            ref, un, delta = refs[b]
            st = R.assert_equal_off_ties(out[b], ref, un, delta, 4 * delta, "op %d par %s %dx%d" % (code, list(par[:2]), H, W))
            if code == 4:
                assert (out[b] == 0).all() == bool(mask.all()) and (mask.any() or np.array_equal(out[b], frames[b]))
            key = "sim2real_op code %d" % code
            t = totals.setdefault(key, {"what": key, "n": 0, "excused": 0, "delta": 0.0, "cap": 0.0})
            t["n"] += st["n"]; t["excused"] += st["excused"]; t["delta"] = max(t["delta"], delta); t["cap"] = max(t["cap"], 4 * delta)
    for key in sorted(totals):
        R.report(totals[key])


@pytest.mark.parametrize("shape", [(4, 512, 640), (2, 1200, 1920)], ids=["b4_512x640", "b2_1200x1920"])
def test_noise_elementwise_against_the_generator(shape):
    """The additive-noise stage on a flat and on a random frame, seeds that differ only in bit 0 and only in bit 31, element by element against
    noise_field (lowbias32 twice, Box-Muller in float64), off ties with delta_noise; the three channels receive the same sample; and the
    statistical assertions the small test makes."""
    B, H, W = shape
    assert _strided_s2r(H, W) >= 2
    s0 = 0x12345678
    seeds = np.array([s0, s0 ^ 1, s0 ^ 0x80000000, s0] if B == 4 else [s0 ^ 1, s0 ^ 0x80000000], dtype=np.uint32)
    frames = np.full((B, H, W, 3), 128, dtype=np.uint8)
    frames[-1] = np.repeat(np.random.default_rng(9).integers(0, 256, size=(H, W, 1), dtype=np.uint8), 3, -1)
    sigma = 0.01 * 255
    delta = R.delta_noise(sigma)
    refs = []
    for b in range(B):
        ref, un = R.sim2real_stage(frames[b], 0, _par(sigma), int(seeds[b]))
        share = R.tie_share(un, delta)
        assert share <= 4 * delta, (b, share, delta)
        print("input-side reference alone: noise near-tie share %.3g (delta %.3g)" % (share, delta))
        refs.append((ref, un))
    out = _run_stage(frames, [0] * B, [_par(sigma)] * B, seeds, [np.zeros((1, 1), dtype=bool)] * B)
    tot = {"what": "sim2real_op code 0 (noise)", "n": 0, "excused": 0, "delta": delta, "cap": 4 * delta}
    for b in range(B):
        st = R.assert_equal_off_ties(out[b], refs[b][0], refs[b][1], delta, 4 * delta, "noise sample %d seed %#x" % (b, seeds[b]))
        tot["n"] += st["n"]; tot["excused"] += st["excused"]
        assert np.array_equal(out[b][..., 0], out[b][..., 1]) and np.array_equal(out[b][..., 0], out[b][..., 2])
    R.report(tot)
    flat = [out[b].astype(np.float64)[..., 0] - 128 for b in range(B - 1)]
    for n in flat:
        assert abs(n.mean()) < 0.15 and 2.2 < n.std() < 2.9
    for a in range(len(flat)):
        for b in range(a + 1, len(flat)):
            assert (flat[a] != flat[b]).mean() > 0.5, "seeds %#x and %#x give the same field" % (seeds[a], seeds[b])
    rows = flat[0]
    assert (rows[0] != rows[1]).mean() > 0.5 and (rows[:, 0] != rows[:, 1]).mean() > 0.5     # no row or column repeats


# ------------------------------------------------------------------------------------------------ the five-launch pipeline
def test_sim2real_batch_against_the_pipeline_reference():
    """augment.sim2real_batch on 8 frames of 512 x 640 with a hand-made draw: applied and skipped samples, five different stage orders (noise
    first, noise last), masks from 1 x 1 to 51 x 64.  Teacher-forced: after each of the five launches the DEVICE's batch is the input of the
    reference's next stage (a one-level difference at a tie in stage k is a legitimate input difference for stage k + 1), every stage judged
    off ties with its own delta.  Skipped samples equal the grey frame byte for byte after all five launches, and a sample in which no tie
    was excused equals the free-running reference pipeline byte for byte."""
    from ursonet_amd import augment as A
    B, H, W = 8, 512, 640
    frames = np.random.default_rng(21).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    draw = R.handmade_draw(B, H, W)
    applied = [tuple(o) for o, a in zip(draw["order"], draw["apply"]) if a]
    assert len(set(applied)) == 5 and any(o[0] == 0 for o in applied) and any(o[-1] == 0 for o in applied) and not draw["apply"].all()
    assert len({m.shape for m in draw["masks"]}) >= 5 and max(m.size for m in draw["masks"]) == int(0.1 * H) * int(0.1 * W)
    assert all(R.multiply_tie_free(p[3, 0]) for p, a in zip(draw["par"], draw["apply"]) if a)
    trace = []
    out = A.sim2real_batch(frames, draw=draw, trace=trace).cpu().numpy()
    assert len(trace) == 6
    grey, outs = trace[0].cpu().numpy(), [t.cpu().numpy() for t in trace[1:]]
    assert np.array_equal(out, outs[-1]) and np.array_equal(grey, R.grey3(frames))
    stats, excused = R.judge_pipeline_teacher_forced(grey, outs, draw, "sim2real_batch")
    for st in stats:
        R.report(st)
    skipped = ~draw["apply"]
    assert np.array_equal(out[skipped], grey[skipped])
    ref = R.sim2real_pipeline(frames, draw)
    clean = excused == 0
    assert np.array_equal(out[clean], ref[clean])
    d = np.abs(out.astype(int) - ref.astype(int))
    print("input-side sim2real_batch free-running: %d of %d samples without an excused tie; elsewhere %.3g of the elements differ, max %d levels"
          % (clean.sum(), B, (d[~clean] > 0).mean() if (~clean).any() else 0.0, d.max()))
    assert np.array_equal(A.sim2real_batch(frames, draw=draw).cpu().numpy(), out)          # the hook changes nothing


# ------------------------------------------------------------------------------------------------ mold
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B", [32, 64])
def test_mold_images_uint8_at_batch_size(B, dt):
    """urso_mold_images on B x 512 x 640 uint8 frames, with and without a mean, the 8-pixels-per-thread form and the scalar one (option
    mold_scalar), byte-exact on the stored 16-bit patterns against float32(pixel) - mean rounded once in NumPy.  The scalar form's stride loop
    runs ten times at B = 32 (the benchmark batch); the 8-pixel form handles 8 x 8192 x 256 pixels per iteration and needs B = 64 for a second."""
    hip = _hip()
    H, W = 512, 640
    npix = B * H * W
    # prep.hip, urso_mold_images: `int blocks = (int)((npix + 255) / 256); if (blocks > 4096) blocks = 4096;` (mold_kernel) and
    # `const size_t ng = npix / 8; int blocks = (int)((ng + 255) / 256); if (blocks > 8192) blocks = 8192;` (mold8_kernel)
    assert -(-npix // (min((npix + 255) // 256, 4096) * 256)) >= 2
    iters8 = -(-(npix // 8) // (min((npix // 8 + 255) // 256, 8192) * 256))
    assert iters8 == (2 if B == 64 else 1)
    img = np.random.default_rng(B + dt).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    src = _dev(img)
    mean = np.array([123.7, 116.8, 103.9], dtype=np.float32)
    for m in ((None, mean) if B == 32 else (mean,)):
        want = R.mold_bits(img, m, dt)
        for scalar in (0, 1):
            with hip.options(mold_scalar=scalar):
                out = torch.full((B, H, W, 4), 7.0, dtype=hip.TORCH_DT[dt], device="cuda")
                hip.mold_images(B, H, W, src, None if m is None else _dev(m), dt, out)
                torch.cuda.synchronize()
            got = out.view(torch.int16).cpu().numpy().view(np.uint16)
            del out
            assert np.array_equal(got, want), "mold dt %d mean %s scalar %d: %d values differ" % (dt, m is not None, scalar, (got != want).sum())
    print("input-side mold B %d dt %d: %d stored values compared bit for bit per form" % (B, dt, npix * 4))


# ------------------------------------------------------------------------------------------------ the max-pool's 32-bit guard
def test_maxpool_fwd_rejects_a_padded_count_past_32_bits():
    """B = 2^22, H = W = 2, C = 256 in bf16: B OH OW C/8 = 2^27 passes the old check, but the kernel iterates the count padded to 4 x 8
    output-pixel tiles, B TY TX 32 C/8 = 2^32, in a uint32_t: it used to wrap to 0, launch a loop of no iterations, write nothing and return
    URSO_OK.  Real, correctly sized tensors (8 GiB in, 2 GiB out; the arg-max buffer may be NULL), so that neither outcome can touch memory
    that is not there."""
    hip = _hip()
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("needs 12 GiB of free device memory, %.1f GiB reported" % (free / 2 ** 30))
    B, H, W, C = 1 << 22, 2, 2, 256
    assert B * (H // 2) * (W // 2) * (C // 8) == 1 << 27 and B * ((H // 2 + 3) >> 2) * ((W // 2 + 7) >> 3) * 32 * (C // 8) == 1 << 32
    x = torch.empty((B, H, W, C), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(hip.UrsoHipError, match="too large for 32-bit indexing"):
        hip.maxpool_fwd(B, H, W, C, 1, x, y, None)
    torch.cuda.synchronize()
    del x, y
    torch.cuda.empty_cache()
    # a small map just under the limit of neither count still runs
    xs = torch.zeros((4, 2, 2, 256), dtype=torch.bfloat16, device="cuda"); xs[:, 1, 1] = 3.0
    ys = torch.empty((4, 1, 1, 256), dtype=torch.bfloat16, device="cuda")
    hip.maxpool_fwd(4, 2, 2, 256, 1, xs, ys, None)
    torch.cuda.synchronize()
    assert bool((ys == 3.0).all())
