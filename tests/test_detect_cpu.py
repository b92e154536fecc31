"""detect_dataset without a GPU: the reference's own figures (tests/golden/detect_dataset.npz, recorded by make_detect_golden.py from
utils.visualize_weights / visualize_axes / polar_plot and a full pose_estimator.detect_dataset) against tests/detectref.py and the host
half of ursonet_amd/detect.py, and the sheet's near-tie rule on simulated kernels."""
import os
import random

import numpy as np
import pytest

import detectref as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detect_dataset.npz")
RUNS = ("quaternion", "euler", "angle_axis", "speed", "soft")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1.0)))


# ------------------------------------------------------------------ sheet
@pytest.mark.parametrize("n", [3, 4])
def test_reference_slices_are_the_sheets_cells(g, n):
    """What visualize_weights hands to imshow -- 2n slices [n,n] and vmax -- is what the sheet shows: slice z of row r, element [j, i], is
    the source value of the bin cell_map puts at cell row j, column i of slice z; the colour index of value / vmax is the sheet's.  The
    stored PMF's row is the GT rule; the estimate row of the reference is a softmax, which the GT rule normalises identically
    (exp(z - max) is softmax / max softmax), checked here on its logarithm as logits."""
    import ursonet_amd.detect  # noqa: F401  (the feature under test)
    gt, est = g["weights_n%d/gt" % n], g["weights_n%d/est" % n]
    slices, vmax = g["weights_n%d/slices" % n], g["weights_n%d/vmax" % n]
    assert slices.shape == (2 * n, n, n) and np.all(vmax[:n] == gt.max()) and np.all(vmax[n:] == est.max())
    cell, gap = 2, 1
    m = DR.cell_map(n, cell, gap, 2)
    for r, src in enumerate((gt, est)):
        for z in range(n):
            for j in range(n):
                for i in range(n):
                    y, x = gap + r * (n * cell + gap) + j * cell, gap + z * (n * cell + gap) + i * cell
                    k = m[y, x] - r * n ** 3
                    assert np.all(m[y:y + cell, x:x + cell] == m[y, x]) and slices[r * n + z, j, i] == src[k]
    assert (m < 0).sum() == m.size - 2 * n ** 3 * cell * cell
    lut = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) // 2], 1).astype(np.uint8)
    bg = (9, 8, 7)
    pic = DR.sheet(gt, est, n, cell, gap, lut, bg)                       # both rows by the GT rule: est is a PMF here
    want = np.minimum(255, np.floor(256.0 * (slices.astype(np.float64) / vmax[:, None, None]))).astype(int)
    for r in range(2):
        src_rule = DR.indices(DR.values((gt, est)[r], False))
        for z in range(n):
            for j in range(n):
                for i in range(n):
                    assert src_rule[i * n * n + j * n + z] == want[r * n + z, j, i]
    assert tuple(pic[0, 0]) == bg and pic.shape == DR.shape(n, cell, gap, 2) + (3,)
    gt_only = DR.sheet(gt, None, n, cell, gap, lut, bg)
    assert np.array_equal(gt_only[:gap + n * cell], pic[:gap + n * cell]) and gt_only.shape[0] == n * cell + 2 * gap
    # exp(z - max z) of the logits log(est) is est / max est up to the rounding of log and exp: the same indices except at near-ties
    v_log = DR.values(np.log(est.astype(np.float64)).astype(np.float32), True)
    v_pmf = DR.values(est, False)
    assert np.abs(v_log - v_pmf).max() < 1e-6


def test_sheet_value_rule_edge_cases():
    import ursonet_amd.detect  # noqa: F401
    assert np.array_equal(DR.values(np.zeros(8), False), np.zeros(8))
    v = DR.values(np.array([0.5, -1.0, np.nan, 0.25], dtype=np.float32), False)
    assert np.array_equal(v, [1.0, 0.0, 0.0, 0.5]) and list(DR.indices(v)) == [255, 0, 0, 128]
    v = DR.values(np.array([3.0, 3.0, -np.inf, np.nan], dtype=np.float32), True)
    assert np.array_equal(v, [1.0, 1.0, 0.0, 0.0])
    assert DR.shape(3, 1, 0, 1) == (3, 9) and DR.shape(8, 4, 2, 2) == (70, 274)


def _logits(seed, B, n, scale):
    return (np.random.default_rng(seed).normal(size=(B, n ** 3)) * scale).astype(np.float32)


@pytest.mark.parametrize("scale", [4.0, 1.5])
def test_near_tie_counts_of_the_gpu_cases(scale):
    """The inputs of tests/test_detect_gpu.py: logits N(0, 1) * scale rounded to fp32, default_rng seeds 0-3, B = 3, n in {3, 5, 8}.
    Scale 4: zero near-ties and 11-44 distinct indices per case (the issue's figures); scale 1.5: counted here -- also zero -- with a
    fuller index range."""
    import ursonet_amd.detect  # noqa: F401
    distinct, ties = [], 0
    for seed in range(4):
        for n in (3, 5, 8):
            z = _logits(seed, 3, n, scale)
            for b in range(3):
                v = DR.values(z[b], True)
                ties += int(DR.near_tie(v).sum())
            distinct.append(len(np.unique(DR.indices(np.concatenate([DR.values(z[b], True) for b in range(3)])))))
    print("scale %.1f: near-ties %d, distinct indices %d .. %d" % (scale, ties, min(distinct), max(distinct)))
    assert ties == 0
    if scale == 4.0:
        assert (min(distinct), max(distinct)) == (11, 44)
    else:
        assert min(distinct) > 11 and max(distinct) > 44


def test_near_tie_rule_on_simulated_kernels():
    """check_sheet accepts a kernel whose exp is one ulp off (a near-tie cell may take either neighbouring index) and refuses: a kernel
    that swaps i and j, one that divides by the softmax sum, one that shifts the sheet by a pixel, a wrong GT byte, an index off by one."""
    import ursonet_amd.detect  # noqa: F401
    n, cell, gap = 5, 3, 1
    lut = np.stack([np.arange(256), (np.arange(256) * 7) % 256, 255 - np.arange(256)], 1).astype(np.uint8)
    bg = (1, 2, 3)
    rng = np.random.default_rng(5)
    z = (rng.normal(size=n ** 3) * 1.5).astype(np.float32)
    gt = rng.random(n ** 3).astype(np.float32)
    m = DR.cell_map(n, cell, gap, 2)

    def render(idx_gt, idx_est):
        idx = np.concatenate([idx_gt, idx_est])
        out = np.empty(m.shape + (3,), dtype=np.uint8)
        out[:] = bg
        out[m >= 0] = lut[idx[m[m >= 0]]]
        return out

    i_gt, v = DR.indices(DR.values(gt, False)), DR.values(z, True)
    assert DR.check_sheet(render(i_gt, DR.indices(v)), gt, z, n, cell, gap, lut, bg) == (0, 0)
    for ulp_off in (np.nextafter(v, 2.0), np.nextafter(v, -1.0)):                    # a 1-ulp exp
        DR.check_sheet(render(i_gt, DR.indices(ulp_off)), gt, z, n, cell, gap, lut, bg)
    wrong = {
        "swapped i and j": render(i_gt, DR.indices(v).reshape(n, n, n).transpose(1, 0, 2).ravel()),
        "softmax with its sum": render(i_gt, DR.indices(v / v.sum())),
        "shifted": np.roll(render(i_gt, DR.indices(v)), 1, axis=1),
        "GT byte": render(np.where(np.arange(n ** 3) == 7, (i_gt + 1) % 256, i_gt), DR.indices(v)),
        "index off by one everywhere": render(i_gt, np.minimum(255, DR.indices(v) + 1)),
    }
    for what, pic in wrong.items():
        with pytest.raises(AssertionError):
            DR.check_sheet(pic, gt, z, n, cell, gap, lut, bg)
        print("refused:", what)
    # a planted near-tie: a logit whose exp(z - max) lies within 1e-12 of 128 / 256 -- found by walking fp32 logits around log 0.5 -- may
    # show index 127 or 128 and nothing else
    cand = np.float32(np.log(0.5)) + np.arange(-64, 65, dtype=np.float32) * np.float32(2.0 ** -24)
    vals = np.exp(cand.astype(np.float64))
    zt = z.copy()
    zt[0], zt[1] = 0.0, cand[np.argmin(np.abs(vals - 0.5))]
    zt = np.minimum(zt, 0.0).astype(np.float32)                           # 0 is the maximum: v = exp(z)
    vt = DR.values(zt, True)
    if DR.near_tie(vt)[1]:                                                  # no fp32 logit need land that close: then there is nothing to plant
        lo, hi = DR.indices(vt * (1 - DR.TIE_MARGIN))[1], DR.indices(vt * (1 + DR.TIE_MARGIN))[1]
        assert (lo, hi) == (127, 128)
        for k in (127, 128):
            idx = DR.indices(vt)
            idx[1] = k
            assert DR.check_sheet(render(i_gt, idx), gt, zt, n, cell, gap, lut, bg)[0] == 1
        idx[1] = 129
        with pytest.raises(AssertionError):
            DR.check_sheet(render(i_gt, idx), gt, zt, n, cell, gap, lut, bg)
    # the rule itself, on values: one ulp below 0.5 is a near-tie between 127 and 128, 0.5 + 1e-9 is not
    vt = np.array([np.nextafter(0.5, 0.0), 0.5 + 1e-9, 1.0, 0.0])
    assert list(DR.near_tie(vt)) == [True, False, False, False] and list(DR.indices(vt)) == [127, 128, 255, 0]
    # more near-ties than 0.1 % of the estimate bins are refused even where every pixel agrees
    z2 = np.array([0.0] + [-1.0] * 7, dtype=np.float32)
    v2 = DR.values(z2, True)
    real = DR.near_tie
    try:
        DR.near_tie = lambda v: np.arange(len(v)) == 1
        with pytest.raises(AssertionError, match="near-ties"):
            DR.check_sheet(DR.sheet(None, z2, 2, 1, 0, lut, bg), None, z2, 2, 1, 0, lut, bg)
    finally:
        DR.near_tie = real
    assert DR.check_sheet(DR.sheet(None, z2, 2, 1, 0, lut, bg), None, z2, 2, 1, 0, lut, bg) == (0, 0) and v2[0] == 1.0


# ------------------------------------------------------------------ arrows, centres, angles
def test_arrows_match_the_reference(g):
    """(c, v) of every ax.arrow call of utils.visualize_axes, poses through the Speed inversion among them: closed form in fp64, equal to
    1e-12 relative -- for tests/detectref.py and for ursonet_amd.detect.axes_arrows."""
    from ursonet_amd import detect
    q, loc, inv, K = g["axes/q"], g["axes/loc"], g["axes/inverted"], g["axes/K"]
    assert inv.any() and not inv.all()
    for i in range(len(q)):
        qi = detect.quat_inv(q[i]) if inv[i] else q[i]
        for c, v in (DR.arrows(qi, loc[i], K), detect.axes_arrows(qi, loc[i], K)):
            assert _close(c, g["axes/c"][i]) and _close(v, g["axes/v"][i]), i
        assert abs(np.linalg.norm(g["axes/v"][i]) - 100.0) < 1e-9        # the Frobenius norm of all three arrows together
        a = detect.detect_prims("axes", K, 1.0, q=q[i], loc=loc[i], speed=bool(inv[i]))
        b = DR.axes_prims(q[i], loc[i], K, 1.0, speed=bool(inv[i]))
        assert a.dtype == np.int32 and a.shape == (9, 9) and np.array_equal(a, b)
        assert [tuple(r[6:]) for r in a[::3]] == [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
        c, v = g["axes/c"][i], g["axes/v"][i]
        assert tuple(a[0, 1:5]) == tuple(int(np.rint(t)) for t in (c[0], c[1], c[0] + v[0, 0], c[1] + v[1, 0]))


def test_pyr_matches_the_reference(g):
    from ursonet_amd import detect
    q1, q2, angles = g["polar/q1"], g["polar/q2"], g["polar/angles"]
    for i in range(len(q1)):
        assert _close(detect.quat2euler(q1[i]) * np.pi / 180, angles[i, 0]) and _close(detect.quat2euler(q2[i]) * np.pi / 180, angles[i, 1])
    assert abs(angles[0, 0, 1]) == pytest.approx(np.pi / 2) and angles[0, 0, 1] == -angles[1, 0, 1]     # both pole branches are in the file


@pytest.mark.parametrize("run", RUNS)
def test_full_run_ids_centres_and_lines(g, run):
    """A full pose_estimator.detect_dataset: the ids random.choice draws under the stored seed; the circle centres, radii and colours
    against detect.project / detect_prims("overlap") on the printed locations; the seven labels; the printed errors against
    pose.pose_errors; the result's pyr through the Speed inversion."""
    from ursonet_amd import detect, pose
    c = "run_" + run
    H0, W0 = (int(v) for v in g["frame"])
    ids = g[c + "/ids"]
    random.seed(int(g[c + "/seed"]))
    pool = np.arange(int(g[c + "/n_dataset"]))
    assert [int(random.choice(pool)) for _ in range(len(ids))] == list(ids)
    assert tuple(g[c + "/labels"]) == detect.PRINT_LABELS

    class Cam(object):
        fx = W0 / (2 * np.tan(np.pi / 4))
        fy = -H0 / (2 * np.tan(73.7 * np.pi / 360))
    K = detect.frame_matrix(Cam, W0, H0)
    loc_gt, loc_est = g[c + "/print_loc_gt"], g[c + "/print_loc_est"]
    assert np.array_equal(loc_gt, g[c + "/loc_gt"][ids])
    xy, rad, col = g[c + "/circle_xy"], g[c + "/circle_r"], g[c + "/circle_colour"]
    assert xy.shape == (len(ids), 2, 2) and list(rad[0]) == [15, 10] and list(col[0]) == ["r", "g"]
    speed = str(g[c + "/dataset_name"]) == "Speed"
    assert speed == (run == "speed")
    for i in range(len(ids)):
        assert _close(detect.project(loc_gt[i], K), xy[i, 0]) and _close(detect.project(loc_est[i], K), xy[i, 1])
        assert _close(DR.centre(loc_gt[i], Cam.fx, Cam.fy, W0, H0), xy[i, 0])
        for scale in (1.0, 0.37):
            rows = detect.detect_prims("overlap", K, scale, loc=loc_est[i], loc_gt=loc_gt[i])
            assert np.array_equal(rows, DR.overlap_prims(loc_est[i], loc_gt[i], None, K, scale))
            assert [tuple(r[6:]) for r in rows] == [(255, 0, 0), (0, 255, 0)] and list(rows[:, 0]) == [1, 1]
            assert list(rows[:, 5]) == [max(1, int(np.rint(15 * scale))), max(1, int(np.rint(10 * scale)))]
            assert tuple(rows[0, 1:3]) == tuple(int(np.rint(v * scale)) for v in xy[i, 0])
        ori_err, loc_err = pose.pose_errors(loc_est[i], g[c + "/print_q_est"][i], loc_gt[i], g[c + "/print_q_gt"][i])[:2]
        assert abs(loc_err - g[c + "/print_loc_err"][i]) < 1e-9 and abs(ori_err - g[c + "/print_ori_err"][i]) < 1e-6
    table = np.full((len(ids), 16), np.nan)
    table[:, 0:3], table[:, 3:7] = loc_est, g[c + "/print_q_est"]
    table[:, 7], table[:, 8] = g[c + "/print_loc_err"], g[c + "/print_ori_err"]
    res = detect.DetectResult(ids, table, loc_gt, g[c + "/print_q_gt"], False, speed)
    flip = detect.quat_inv if speed else (lambda q: q)
    assert np.array_equal(res.pyr_gt[0], detect.quat2euler(flip(res.q_gt[0]))) and res.loc_encoded_err is None and res.pictures is None
    if speed:
        assert not np.array_equal(res.pyr_gt[0], detect.quat2euler(res.q_gt[0]))

    class Ds(object):
        image_info = [{"path": "golden://%d" % i} for i in pool]
    lines = detect.print_lines(res, Ds, 1)
    assert len(lines) == 7 and all(l.startswith(lab) for l, lab in zip(lines, detect.PRINT_LABELS))
    assert lines[2] == "Processed Image: golden://%d" % ids[1]


def test_overlap_with_an_encoded_target_and_dropped_rows():
    """Location classification: the blue disc of radius 7 comes first, at the first moment's projection (the reference cannot run this
    head to the end -- see make_detect_golden.py -- so the closed form is the reference).  A point at the image plane or far outside the
    +-16,384 box is dropped; radii and thickness never fall below 1."""
    from ursonet_amd import detect
    K = np.array([[64.0, 0, 64], [0, -64.0, 48], [0, 0, 1]])
    est, gt, enc = np.array([0.5, 0.25, 10.0]), np.array([-1.0, 0.5, 8.0]), np.array([-0.9, 0.45, 8.2])
    rows = detect.detect_prims("overlap", K, 0.5, loc=est, loc_gt=gt, loc_encoded=enc)
    assert np.array_equal(rows, DR.overlap_prims(est, gt, enc, K, 0.5)) and rows.shape == (3, 9)
    assert [tuple(r[6:]) for r in rows] == [(0, 0, 255), (255, 0, 0), (0, 255, 0)] and list(rows[:, 5]) == [4, 8, 5]
    assert tuple(rows[2, 1:3]) == (int(np.rint((0.05 * 64 + 64) * 0.5)), int(np.rint((48 - 0.025 * 64) * 0.5)))
    rows = detect.detect_prims("overlap", K, 0.01, loc=est, loc_gt=np.array([1.0, 1.0, 0.0]), loc_encoded=np.array([1e9, 0.0, 1.0]))
    assert rows.shape == (1, 9) and rows[0, 5] == 1 and tuple(rows[0, 6:]) == (0, 255, 0)
    q = np.array([0.0, 0.0, 0.0, 1.0])
    assert detect.detect_prims("axes", K, 0.01, q=q, loc=est)[0, 5] == 1
    assert detect.detect_prims("axes", K, 1.0, q=q, loc=np.array([0.0, 0.0, 0.0])).shape == (0, 9)
    with pytest.raises(ValueError):
        detect.detect_prims("dial", K, 1.0)


def test_binding_and_records():
    import ursonet_amd.hip as hip
    assert "urso_pmf_sheet_u8" in hip.EXPORTED_SYMBOLS and len(hip.EXPORTED_SYMBOLS) == 101
    assert hip.pmf_sheet_shape(8, 4, 2, 2) == DR.shape(8, 4, 2, 2) and hip.pmf_sheet_shape(3, 1, 0, 1) == (3, 9)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "(101 entry points)" in open(os.path.join(root, "README.md")).read()
