"""detect_dataset on the GPU: urso_pmf_sheet_u8 against the NumPy statement of its geometry and value rule (tests/detectref.py: the GT
row byte for byte, the estimate row byte for byte except at derived near-ties), and detect_dataset() end to end against evaluate()'s
table, the NumPy rasteriser on detect_prims' rows, and detectref's sheet."""
import random

import numpy as np
import pytest
import torch

import detectref as DR
import videoref as VR
from util import make_config

pytestmark = pytest.mark.gpu

GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
COLOUR = np.stack([np.arange(256), (np.arange(256) * 7 + 3) % 256, 255 - np.arange(256)], 1).astype(np.uint8)


def _gt(rng, B, n):
    p = rng.random((B, n ** 3)) ** 4
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def _logits(seed, B, n, scale):
    return (np.random.default_rng(seed).normal(size=(B, n ** 3)) * scale).astype(np.float32)


def _run(gt, logits, n, cell, gap, lut=GREY, bg=(255, 255, 255)):
    """-> (pictures [B,SH,SW,3], near-tie bins, differing pixels), every image checked under detectref's rule."""
    from ursonet_amd import augment
    out = augment.pmf_sheet(gt, logits, n, cell=cell, gap=gap, lut=lut, bg=bg)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    B = got.shape[0]
    ties = diff = 0
    for b in range(B):
        t, d = DR.check_sheet(got[b], None if gt is None else gt[b], None if logits is None else logits[b], n, cell, gap, lut, bg)
        ties, diff = ties + t, diff + d
    return got, ties, diff


# ------------------------------------------------------------------ urso_pmf_sheet_u8
@pytest.mark.parametrize("n,cell,gap,B", [(3, 1, 0, 2), (5, 3, 1, 2), (8, 4, 2, 3)])
def test_sheet_shapes(n, cell, gap, B):
    """n = 3, cell 1, gap 0: 27-byte rows, nothing aligned; n = 5, cell 3, gap 1; n = 8, cell 4, gap 2 with B = 3 (several blocks per
    image).  Both rows, GT only, logits only; the GT row and a GT-only sheet are equal byte for byte."""
    rng = np.random.default_rng(n)
    gt, z = _gt(rng, B, n), _logits(1, B, n, 4.0)
    got, ties, diff = _run(gt, z, n, cell, gap)
    print("n %d: near-ties %d, differing pixels %d" % (n, ties, diff))
    assert got.shape == (B,) + DR.shape(n, cell, gap, 2) + (3,) and ties == 0 and diff == 0
    only, _, d = _run(gt, None, n, cell, gap, lut=COLOUR, bg=(1, 2, 3))
    assert only.shape == (B,) + DR.shape(n, cell, gap, 1) + (3,) and d == 0
    for b in range(B):
        assert np.array_equal(only[b], DR.sheet(gt[b], None, n, cell, gap, COLOUR, (1, 2, 3)))
    est, t, d = _run(None, z, n, cell, gap, lut=COLOUR, bg=(0, 0, 0))
    assert est.shape == only.shape and t == 0 and d == 0


@pytest.mark.parametrize("scale", [4.0, 1.5])
def test_sheet_estimate_row_near_ties(scale):
    """Logits N(0, 1) * scale in fp32, default_rng seeds 0-3, B = 3, n in {3, 5, 8}: no near-tie among them (counted on the CPU in
    tests/test_detect_cpu.py; asserted here), so every byte is equal; scale 1.5 fills more of the index range."""
    ties = diff = 0
    for seed in range(4):
        for n in (3, 5, 8):
            _, t, d = _run(None, _logits(seed, 3, n, scale), n, 2, 1, lut=COLOUR)
            ties, diff = ties + t, diff + d
    print("scale %.1f: near-ties %d, differing pixels %d" % (scale, ties, diff))
    assert ties == 0 and diff == 0


def test_sheet_multi_pass_reduction_and_edge_values():
    """n = 32, cell 2, gap 1, B = 1: K = 32,768, 128 passes of the reduction's block, the maximum planted at the last bin.  An all-zero
    GT image shows index 0 everywhere; a NaN and a negative bin count as 0."""
    n = 32
    rng = np.random.default_rng(32)
    gt = _gt(rng, 1, n)
    gt[0, -1] = gt.max() * 3
    z = _logits(2, 1, n, 1.5)
    z[0, -1] = z.max() + 2
    got, ties, diff = _run(gt, z, n, 2, 1, lut=COLOUR)
    print("n 32: near-ties %d, differing pixels %d" % (ties, diff))
    assert got.shape == (1, 131, 2081, 3) and ties <= 0.001 * n ** 3
    n = 4
    gt = _gt(rng, 3, n)
    gt[0] = 0
    gt[1, 5], gt[1, 6] = np.nan, -1.0
    got, _, diff = _run(gt, _logits(3, 3, n, 4.0), n, 3, 2, lut=COLOUR, bg=(7, 7, 7))
    assert diff == 0
    m = DR.cell_map(n, 3, 2, 2)
    assert np.all(got[0][(m >= 0) & (m < n ** 3)] == COLOUR[0])
    assert np.all(got[1][(m == 5) | (m == 6)] == COLOUR[0]) and np.all(got[:, 0, 0] == 7)


def test_sheet_out_at_an_odd_address():
    """`out` starting 5 bytes into an allocation: the bytes around the batch stay as they were."""
    from ursonet_amd import augment
    n, cell, gap, B = 5, 3, 1, 2
    rng = np.random.default_rng(55)
    gt, z = _gt(rng, B, n), _logits(5, B, n, 4.0)
    sh, sw = DR.shape(n, cell, gap, 2)
    nb = B * sh * sw * 3
    assert (sh * sw * 3) % 16 != 0
    slab = torch.full((nb + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    out = slab[5:5 + nb].view(B, sh, sw, 3)
    assert augment.pmf_sheet(gt, z, n, cell=cell, gap=gap, lut=COLOUR, bg=(4, 5, 6), out=out).data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = slab.cpu().numpy()
    for b in range(B):
        DR.check_sheet(host[5:5 + nb].reshape(B, sh, sw, 3)[b], gt[b], z[b], n, cell, gap, COLOUR, (4, 5, 6))
    assert np.all(host[:5] == 0xAB) and np.all(host[5 + nb:] == 0xAB)


def test_sheet_bad_arguments_do_not_launch():
    from ursonet_amd import hip
    n = 3
    src = torch.zeros(1, n ** 3, dtype=torch.float32, device="cuda")
    lut = torch.as_tensor(GREY).cuda()
    out = torch.full((1 << 16,), 0xCD, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
    ok = dict(B=1, n=n, cell=2, gap=1, gt=src, logits=src, lut=lut, out=out)
    bad = [dict(lut=None), dict(out=None), dict(gt=None, logits=None), dict(B=0), dict(B=65536), dict(n=1), dict(n=65), dict(cell=0),
           dict(cell=65), dict(gap=-1), dict(gap=65)]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(hip.UrsoHipError):
            hip.pmf_sheet(a["B"], a["n"], a["cell"], a["gap"], a["gt"], a["logits"], a["lut"], (0, 0, 0), a["out"], scratch=scratch)
    big = torch.zeros(1, 64 ** 3, dtype=torch.float32, device="cuda")
    with pytest.raises(hip.UrsoHipError, match="2 GiB"):
        hip.pmf_sheet(1, 64, 64, 64, None, big, lut, (0, 0, 0), out)
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all())


# ------------------------------------------------------------------ detect_dataset()
FRAME_H, FRAME_W, N_IMAGES = 60, 90, 6
IDS = [3, 0, 5, 3, 1]                                                    # one repeat; five images at batch 2: the tail batch is padded
CASES = {"soft": dict(regress_ori=False, regress_loc=True), "quaternion": dict(regress_ori=True, regress_loc=True),
         "loc_class": dict(regress_ori=True, regress_loc=False)}


@pytest.fixture(scope="module")
def detected(tmp_path_factory):
    """ResNet-18 at 128 x 192, batch 2, fp32 (the configuration of tests/test_video_gpu.py), SyntheticPoses of 60 x 90 frames, ori_bins 8,
    loc_bins 4: per case the model, the dataset, evaluate()'s result over the whole dataset and detect_dataset's over IDS."""
    from ursonet_amd import detect, evaluate as ev, net
    from ursonet_amd.dataset import SyntheticPoses
    out = {}
    for name, heads in CASES.items():
        td = tmp_path_factory.mktemp("detect_" + name)
        cfg = make_config("resnet18", 128, 192, batch=2, ori_bins=8, loc_bins=4, dtype="float32", **heads)
        cfg.NAME = "syn"
        tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(td))
        path = str(td / "weights_0001.npz")
        tr.save_weights(path)
        del tr
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(td))
        model.load_weights(path, path, by_name=True)
        ds = SyntheticPoses(N_IMAGES, FRAME_H, FRAME_W, cfg, seed=31)
        ref = ev.evaluate(model, ds, out_dir=str(td), verbose=0)
        res = detect.detect_dataset(model, ds, len(IDS), image_ids=IDS, verbose=0)
        out[name] = (cfg, model, ds, ref, res)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_detect_table_is_evaluates(detected, case, capsys):
    from ursonet_amd import detect
    cfg, model, ds, ref, res = detected[case]
    assert list(res.image_ids) == IDS and res.loc_est.shape == (5, 3) and np.all(np.isfinite(res.q_est))
    for col in ("loc_est", "q_est", "loc_err", "ori_err"):
        assert np.array_equal(getattr(res, col), getattr(ref, col)[IDS]), col
    if case == "loc_class":
        assert np.array_equal(res.loc_encoded_err, ref.loc_encoded_err[IDS])
    else:
        assert res.loc_encoded_err is None
    assert np.array_equal(res.loc_gt, np.array([ds.load_location(i) for i in IDS], dtype=np.float64))
    assert np.array_equal(res.pyr_est, np.array([detect.quat2euler(q) for q in res.q_est])) and res.pyr_gt.shape == (5, 3)
    assert (res.ori_logits is not None) == (case == "soft")
    capsys.readouterr()
    plain = detect.detect_dataset(model, ds, 5, image_ids=IDS, render=False, verbose=1)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 7 * 5 and all(l.startswith(lab) for l, lab in zip(lines[7:14], detect.PRINT_LABELS))
    assert plain.pictures is None
    for col in ("loc_est", "q_est", "loc_err", "ori_err"):
        assert np.array_equal(getattr(plain, col), getattr(res, col)), col
    if case == "soft":
        assert np.array_equal(plain.ori_logits, res.ori_logits) and res.ori_logits.shape == (5, 512) and res.ori_logits.dtype == np.float32


@pytest.mark.parametrize("case", list(CASES))
def test_detect_pictures(detected, case):
    """Every axes_gt, axes_est and overlap picture is the NumPy rasteriser applied to the window of augment.resize_images with
    detect_prims' rows (which tests/test_detect_cpu.py ties to detectref and to the reference); every sheet is detectref's under the
    near-tie rule; a sink receives the arrays the result collects."""
    from ursonet_amd import augment, detect
    cfg, model, ds, ref, res = detected[case]
    names = ["axes_gt", "axes_est", "overlap"] + (["sheet"] if case == "soft" else [])
    assert len(res.pictures) == 5 and all(sorted(p) == sorted(names) for p in res.pictures)
    got = {}
    via_sink = detect.detect_dataset(model, ds, 5, image_ids=IDS, verbose=0, sink=lambda i, name, a: got.__setitem__((i, name), np.array(a)))
    assert via_sink.pictures is None and sorted(got) == sorted((i, nm) for i in range(5) for nm in names)
    K = detect.frame_matrix(ds.camera, FRAME_W, FRAME_H)
    painted = ties = 0
    for i, image_id in enumerate(IDS):
        out, window, scale, _pad = augment.resize_images(ds.load_image(image_id)[None], min_dim=cfg.IMAGE_MIN_DIM, max_dim=cfg.IMAGE_MAX_DIM,
                                                         min_scale=cfg.IMAGE_MIN_SCALE, mode=cfg.IMAGE_RESIZE_MODE)
        y0, x0, y1, x1 = window
        win = out[0, y0:y1, x0:x1].cpu().numpy()
        l_gt, q_gt = np.asarray(ds.load_location(image_id), dtype=np.float64), np.asarray(ds.load_quaternion(image_id), dtype=np.float64)
        l_enc = None
        if case == "loc_class":
            l_enc = np.asarray(ds.load_location_encoded(image_id), dtype=np.float32).astype(np.float64) @ np.asarray(ds.histogram_3D_map, dtype=np.float64)
        want = {"axes_gt": detect.detect_prims("axes", K, scale, q=q_gt, loc=l_gt),
                "axes_est": detect.detect_prims("axes", K, scale, q=res.q_est[i], loc=res.loc_est[i]),
                "overlap": detect.detect_prims("overlap", K, scale, loc=res.loc_est[i], loc_gt=l_gt, loc_encoded=l_enc)}
        assert np.array_equal(want["axes_gt"], DR.axes_prims(q_gt, l_gt, K, scale))
        assert np.array_equal(want["overlap"], DR.overlap_prims(res.loc_est[i], l_gt, l_enc, K, scale))
        assert len(want["overlap"]) == (3 if case == "loc_class" else 2)
        for name, prims in want.items():
            pic = res.pictures[i][name]
            ref_pic = VR.rasterise(win, prims)
            assert pic.shape == win.shape and pic.dtype == np.uint8 and np.array_equal(pic, ref_pic), (i, name)
            assert np.array_equal(got[(i, name)], pic)
            painted += int((ref_pic != win).any(axis=2).sum())
        if case == "soft":
            stored = np.asarray(ds.load_orientation_encoded(image_id), dtype=np.float32)
            t, _d = DR.check_sheet(res.pictures[i]["sheet"], stored, res.ori_logits[i], 8, 4, 2, GREY, detect.SHEET_BG)
            ties += t
            assert np.array_equal(got[(i, "sheet")], res.pictures[i]["sheet"])
    print("%s: pixels painted over the 15 pictures: %d; sheet near-ties: %d" % (case, painted, ties))
    assert painted > 0
    assert np.array_equal(res.pictures[0]["axes_gt"], res.pictures[3]["axes_gt"])         # the repeated id


def test_detect_draws_ids_like_the_reference_and_takes_a_lut(detected):
    from ursonet_amd import detect
    cfg, model, ds, ref, res = detected["soft"]
    random.seed(1234)
    want = [random.choice(ds.image_ids) for _ in range(3)]
    random.seed(1234)
    drawn = detect.detect_dataset(model, ds, 3, verbose=0, lut=COLOUR)
    assert list(drawn.image_ids) == list(want)
    assert np.array_equal(drawn.loc_est, ref.loc_est[want]) and np.array_equal(drawn.ori_err, ref.ori_err[want])
    for i, image_id in enumerate(want):
        stored = np.asarray(ds.load_orientation_encoded(image_id), dtype=np.float32)
        DR.check_sheet(drawn.pictures[i]["sheet"], stored, drawn.ori_logits[i], 8, 4, 2, COLOUR, detect.SHEET_BG)
    with pytest.raises(ValueError, match="lut"):
        detect.detect_dataset(model, ds, 1, image_ids=[0], verbose=0, lut=np.zeros((16, 3), dtype=np.uint8))


def test_detect_refuses_to_draw_on_molded_frames(detected):
    """Frames that are not uint8 RGB reach the engine molded to float: render=True raises, render=False runs."""
    from ursonet_amd import detect
    cfg, model, ds, ref, res = detected["quaternion"]

    class Float(object):
        def __init__(self, inner):
            self._ds = inner

        def load_image(self, i):
            return self._ds.load_image(i).astype(np.float32)

        def __getattr__(self, name):
            return getattr(self._ds, name)
    with pytest.raises(ValueError, match="uint8 RGB"):
        detect.detect_dataset(model, Float(ds), 2, image_ids=[0, 1], verbose=0)
    plain = detect.detect_dataset(model, Float(ds), 2, image_ids=[0, 1], render=False, verbose=0)
    assert plain.pictures is None and np.all(np.isfinite(plain.loc_err))
