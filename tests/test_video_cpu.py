"""Host side of the video path (ursonet_amd/video.py) and the NumPy references the GPU tests lean on (tests/videoref.py): the literal
frame prep against an independently written loop, pose_unreal against the reference's own se3lib chain (tests/golden/video_pose.npz),
pose_axes_prims against hand-computed arrows and the reference's projection, and the rasteriser rule's own properties."""
import math
import os

import numpy as np
import pytest

import videoref as VR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "video_pose.npz")


# ------------------------------------------------------------------ VideoPrep
@pytest.mark.parametrize("crop,pad,grey", [((0, 0, 1, 3), 2, (0.21, 0.72, 0.07)), ((0, 0, 0, 0), 0, (0.21, 0.72, 0.07)),
                                           ((3, 2, 0, 0), 1, (0.3, 0.59, 0.11)), ((1, 1, 2, 2), 3, (1.0, 0.0, 0.0))])
def test_prep_host_against_a_pixel_loop(crop, pad, grey):
    from ursonet_amd.video import VideoPrep
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(7, 11, 3), dtype=np.uint8)
    frame[0, 1], frame[2, 4], frame[3, 3] = 255, 0, (255, 254, 255)
    prep = VideoPrep(crop=crop, pad=pad, grey=grey)
    keep = frame.copy()
    out = prep.host(frame)
    assert np.array_equal(frame, keep), "host() must not write into its input"
    assert out.dtype == np.uint8 and out.shape[:2] == prep.out_shape(7, 11)
    assert out.shape == (7 - crop[0] - crop[1] + 2 * pad, 11 - crop[2] - crop[3] + 2 * pad, 3)
    assert np.array_equal(out, VR.prep_loop(frame, crop, pad, grey))
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    if pad:
        assert not out[:pad].any() and not out[-pad:].any() and not out[:, :pad].any() and not out[:, -pad:].any()


def test_prep_defaults_and_white():
    """The reference's defaults; white maps to 254 (0.21 * 255 + 0.72 * 255 + 0.07 * 255 = 254.99999999999997 in float64, truncated)."""
    from ursonet_amd.video import VideoPrep
    prep = VideoPrep()
    assert prep.crop == (0, 0, 1, 150) and prep.pad == 400 and prep.grey == (0.21, 0.72, 0.07)
    assert prep.out_shape(960, 1280) == (1760, 1929)
    assert (0.21 * 255.0 + 0.72 * 255.0) + 0.07 * 255.0 == 254.99999999999997
    out = VideoPrep(pad=1).host(np.full((2, 152, 3), 255, dtype=np.uint8))
    assert out.shape == (4, 3, 3) and np.all(out[1:3, 1] == 254) and out.sum() == 254 * 6


def test_prep_bad_arguments_raise():
    from ursonet_amd.video import VideoPrep
    for crop in ((7, 0, 0, 0), (3, 4, 0, 0), (0, 0, 11, 0), (0, 0, 5, 6)):
        with pytest.raises(ValueError, match="leaves no pixel"):
            VideoPrep(crop=crop, pad=1).out_shape(7, 11)
        with pytest.raises(ValueError, match="leaves no pixel"):
            VideoPrep(crop=crop, pad=1).host(np.zeros((7, 11, 3), dtype=np.uint8))
    assert VideoPrep(crop=(3, 3, 5, 5), pad=0).out_shape(7, 11) == (1, 1)
    for kw in (dict(crop=(0, -1, 0, 0)), dict(pad=-1), dict(crop=(0, 0, 0)), dict(grey=(1.0, 0.0))):
        with pytest.raises(ValueError):
            VideoPrep(**kw)
    with pytest.raises(ValueError, match="uint8"):
        VideoPrep(pad=0, crop=(0, 0, 0, 0)).host(np.zeros((4, 4, 3), dtype=np.float32))


# ------------------------------------------------------------------ pose_unreal
def test_pose_unreal_against_the_reference_chain():
    """64 quaternions through se3lib as detect_video chains it, both gimbal-lock branches and the thresholds' neighbours at +-1e-4
    included: 1e-9 degrees."""
    from ursonet_amd.video import pose_unreal
    g = np.load(GOLD)
    assert g["q"].shape == (64, 4) and set(g["branch"].tolist()) == {-1, 0, 1}
    near = np.abs(np.abs(g["r20"]) - 0.998)
    assert (near < 2e-4).sum() == 12 and near.min() > 5e-5                   # +-0.9979 and +-0.9981, none on the boundary
    worst = 0.0
    for q, e, br in zip(g["q"], g["euler"], g["branch"]):
        row = pose_unreal([1.5, -2.5, 30.0], q)
        assert row.dtype == np.float64 and row.shape == (6,)
        assert np.array_equal(row[:3], [30.0, 1.5, -2.5])                    # [z, x, y]
        worst = max(worst, float(np.abs(row[3:] - e).max()))
        if br:                                                               # gimbal lock: "pitch" (SO32euler's yaw) = -+90, "yaw" (its roll) = 0
            assert row[3] == 90.0 * br and row[4] == 0.0
    print("pose_unreal max |diff| (degrees):", worst)
    assert worst <= 1e-9


# ------------------------------------------------------------------ pose_axes_prims
def test_axes_prims_hand_computed_arrows():
    """Identity rotation, loc (0, 0, 10), scale 5, K = [[200, 0, 100], [0, 200, 100]]: centre (100, 100); x tip (200, 100) -- an
    axis-aligned arrow of length 100, tip size 10, a = atan2(0, -100) = pi: strokes from (200 + 10 cos(pi +- pi/4), 100 + 10 sin(pi +- pi/4))
    = (192.93, 92.93) and (192.93, 107.07) -> (193, 93), (193, 107); y tip (100, 0) (the axes are diag(1, -1, 1)): a = atan2(100, 0) = pi/2,
    strokes from (100 + 10 cos(3 pi/4), 10 sin(3 pi/4)) = (92.93, 7.07) -> (93, 7) and (100 + 10 cos(pi/4), 7.07) -> (107, 7); z tip = the
    centre: a zero-length arrow whose strokes collapse onto it."""
    from ursonet_amd.video import pose_axes_prims
    K = np.array([[200.0, 0, 100], [0, 200.0, 100], [0, 0, 1]])
    rows = pose_axes_prims([0, 0, 0, 1.0], [0, 0, 10.0], K, scale=5.0)
    assert rows.dtype == np.int32 and rows.shape == (9, 9)
    assert np.all(rows[:, 0] == 0) and np.all(rows[:, 5] == 2)
    assert [tuple(r) for r in rows[:, 6:]] == [(0, 0, 255)] * 3 + [(0, 255, 0)] * 3 + [(255, 0, 0)] * 3
    assert [tuple(r) for r in rows[:, 1:5]] == [(100, 100, 200, 100), (193, 93, 200, 100), (193, 107, 200, 100),
                                                (100, 100, 100, 0), (93, 7, 100, 0), (107, 7, 100, 0),
                                                (100, 100, 100, 100), (100, 100, 100, 100), (100, 100, 100, 100)]


def test_axes_prims_45_degree_arrow():
    """A rotation by 45 degrees about z puts the x axis on the diagonal; fx, fy chosen so that the tip projects to (100.5, 100.5) -> (100, 100)
    with the centre at (0, 0): length 141.42, tip size 14.142, a = atan2(-100, -100) = -3 pi/4; a + pi/4 = -pi/2 -> (100, 100 - 14.142) ->
    (100, 86); a - pi/4 = -pi -> (100 - 14.142, 100) -> (86, 100)."""
    from ursonet_amd.video import pose_axes_prims
    h = math.pi / 8
    q = [0.0, 0.0, math.sin(h), math.cos(h)]                                 # quat2SO3: first column (cos 45, -sin 45, 0)
    Z, s = 10.0, 5.0
    K = np.array([[100.5 * Z / (s * math.cos(math.pi / 4)), 0, 0], [0, -100.5 * Z / (s * math.sin(math.pi / 4)), 0], [0, 0, 1]])
    rows = pose_axes_prims(q, [0, 0, Z], K, scale=s)
    assert [tuple(r) for r in rows[:3, 1:5]] == [(0, 0, 100, 100), (100, 86, 100, 100), (86, 100, 100, 100)]


def test_axes_prims_truncate_toward_zero_and_match_the_reference_projection():
    from ursonet_amd.video import camera_matrix, pose_axes_prims
    from ursonet_amd.dataset import Camera
    rows = pose_axes_prims([0, 0, 0, 1.0], [-3.7, -2.5, 1.0], np.eye(3), scale=5.0)
    # centre (-3.7, -2.5) -> (-3, -2), not (-4, -3); tips (1.3, -2.5), (-3.7, -7.5), (-3.7 / 6, -2.5 / 6)
    assert [tuple(r) for r in rows[::3, 1:5]] == [(-3, -2, 1, -2), (-3, -2, -3, -7), (-3, -2, 0, 0)]
    rng = np.random.default_rng(11)
    K = camera_matrix(Camera(), 640, 584)
    assert K[0, 0] > 0 and K[1, 1] < 0 and K[0, 2] == 320 and K[1, 2] == 292 and abs(K[0, 0] - 320.0) < 1e-9
    for _ in range(20):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        loc = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(8, 40)])
        rows = pose_axes_prims(q, loc, K)
        c, v = VR.project_axes(q, loc, K, 5.0)
        assert rows.shape == (9, 9)
        for i in range(3):
            assert tuple(rows[3 * i, 1:5]) == (c[0], c[1], v[0, i], v[1, i])
            assert np.array_equal(rows[3 * i + 1, 3:5], v[:, i]) and np.array_equal(rows[3 * i + 2, 3:5], v[:, i])


def test_axes_prims_drop_what_cannot_be_drawn():
    from ursonet_amd.video import pose_axes_prims
    K = np.array([[200.0, 0, 100], [0, 200.0, 100], [0, 0, 1]])
    ident = [0, 0, 0, 1.0]
    assert pose_axes_prims(ident, [0, 0, 0.0], K).shape == (0, 9)             # zero depth: the centre is not finite, nothing is drawn
    assert pose_axes_prims([np.nan, 0, 0, 1.0], [0, 0, 10.0], K).shape == (0, 9)      # every tip is NaN
    assert pose_axes_prims(ident, [np.inf, 0, 10.0], K).shape == (0, 9)
    # z tip at depth 0 (an object 5 behind the image plane, z axis of length 5 toward it): that arrow alone goes
    rows = pose_axes_prims(ident, [0, 0, -5.0], K)
    assert rows.shape == (6, 9) and [tuple(r) for r in rows[::3, 6:]] == [(0, 0, 255), (0, 255, 0)]
    # a huge focal length throws the x tip to 5e4: its three rows go, the others stay
    big = np.array([[1e5, 0, 100], [0, 10.0, 100], [0, 0, 1]])
    rows = pose_axes_prims(ident, [0, 0, 10.0], big)
    assert rows.shape == (6, 9) and [tuple(r) for r in rows[::3, 6:]] == [(0, 255, 0), (255, 0, 0)]
    assert np.all(np.abs(rows[:, 1:5]) <= 16384)
    # exactly at the cap stays, one beyond goes
    edge = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    rows = pose_axes_prims(ident, [16384.0 - 5, 0, 1.0], edge)               # x tip at 16384
    assert tuple(rows[0, 1:5]) == (16379, 0, 16384, 0)
    rows = pose_axes_prims(ident, [16385.0 - 5, 0, 1.0], edge)               # x tip at 16385
    assert [tuple(r) for r in rows[::3, 6:]] == [(0, 255, 0), (255, 0, 0)]


# ------------------------------------------------------------------ the rasteriser rule
def _painted(img):
    ys, xs = np.nonzero(img.any(axis=2))
    return set(zip(xs.tolist(), ys.tolist()))


def test_rule_horizontal_segment_by_hand():
    """(3, 5) - (8, 5), thickness 2: 4 d^2 <= 4 <=> d <= 1.  Between the ends that is rows 4 .. 6; beyond them d^2 = 1 + dy^2 <= 1 only
    on the segment's own row: the caps are the single pixels (2, 5) and (9, 5)."""
    out = VR.rasterise(np.zeros((12, 14, 3), np.uint8), [[0, 3, 5, 8, 5, 2, 9, 8, 7]])
    want = {(x, y) for x in range(3, 9) for y in (4, 5, 6)} | {(2, 5), (9, 5)}
    assert _painted(out) == want
    assert all(tuple(out[y, x]) == (9, 8, 7) for x, y in want)
    # thickness 1: 4 d^2 <= 1 <=> d = 0: the pixels of the segment alone; thickness 0 likewise
    for t in (0, 1):
        assert _painted(VR.rasterise(np.zeros((12, 14, 3), np.uint8), [[0, 3, 5, 8, 5, t, 1, 1, 1]])) == {(x, 5) for x in range(3, 9)}
    # the same segment given from the other end paints the same pixels
    assert _painted(VR.rasterise(np.zeros((12, 14, 3), np.uint8), [[0, 8, 5, 3, 5, 2, 9, 8, 7]])) == want


def test_rule_diagonal_segment_by_hand():
    """(2, 2) - (6, 6), thickness 2: off the diagonal by one pixel, (x, x + 1), the squared distance is 1/2 -> painted; by two, (x, x + 2),
    it is 2 -> not.  4 (|w|^2 |D|^2 - s^2) <= t^2 |D|^2 with |D|^2 = 32: cross^2 = 16 per unit offset, 4 * 16 <= 4 * 32."""
    out = VR.rasterise(np.zeros((10, 10, 3), np.uint8), [[0, 2, 2, 6, 6, 2, 5, 5, 5]])
    got = _painted(out)
    want = {(x, x) for x in range(2, 7)} | {(x, x + 1) for x in range(2, 6)} | {(x + 1, x) for x in range(2, 6)}
    want |= {(1, 2), (2, 1), (6, 7), (7, 6)}                                 # caps: distance 1 from an end point, s outside (0, |D|^2)
    assert got == want, got ^ want


def test_rule_zero_length_segment_is_a_disc():
    blank = np.zeros((20, 24, 3), np.uint8)
    for t in (0, 2, 6, 10):                                                  # diameter t <=> radius t / 2
        a = VR.rasterise(blank, [[0, 10, 7, 10, 7, t, 3, 2, 1]])
        b = VR.rasterise(blank, [[1, 10, 7, 0, 0, t // 2, 3, 2, 1]])
        assert np.array_equal(a, b) and a.any()
    a = VR.rasterise(blank, [[0, 10, 7, 10, 7, 5, 3, 2, 1]])                 # odd diameter: 4 |w|^2 <= 25 <=> |w|^2 <= 6
    assert _painted(a) == {(10 + dx, 7 + dy) for dx in range(-3, 4) for dy in range(-3, 4) if dx * dx + dy * dy <= 6}
    assert _painted(VR.rasterise(blank, [[1, 10, 7, 0, 0, 0, 1, 1, 1]])) == {(10, 7)}


def test_rule_draw_order_and_clipping():
    blank = np.full((16, 16, 3), 7, np.uint8)
    red, blue = [1, 6, 6, 0, 0, 3, 255, 0, 0], [1, 9, 6, 0, 0, 3, 0, 0, 255]
    ab, ba = VR.rasterise(blank, [red, blue]), VR.rasterise(blank, [blue, red])
    assert tuple(ab[6, 8]) == (0, 0, 255) and tuple(ba[6, 8]) == (255, 0, 0)   # (8, 6) lies in both discs: the later one wins
    assert tuple(ab[6, 4]) == (255, 0, 0) and tuple(ab[6, 11]) == (0, 0, 255) and tuple(ab[0, 0]) == (7, 7, 7)
    assert np.array_equal((ab != 7).any(axis=2), (ba != 7).any(axis=2))         # the same pixels either way, only the colours differ
    assert np.array_equal(VR.rasterise(blank, []), blank)
    # partly outside: only the part inside the frame; wholly outside: nothing; far endpoints do not overflow
    out = VR.rasterise(blank, [[0, -5, 3, 4, 3, 1, 1, 2, 3]])
    assert {(x, 3) for x in range(0, 5)} == {(x, y) for x in range(16) for y in range(16) if tuple(out[y, x]) == (1, 2, 3)}
    assert np.array_equal(VR.rasterise(blank, [[0, -9, -9, -2, -2, 2, 1, 2, 3], [1, 40, 40, 0, 0, 7, 1, 2, 3]]), blank)
    out = VR.rasterise(blank, [[0, -16384, -16384, 16384, 16384, 1, 1, 2, 3]])
    assert {(i, i) for i in range(16)} == {(x, y) for x in range(16) for y in range(16) if tuple(out[y, x]) == (1, 2, 3)}
