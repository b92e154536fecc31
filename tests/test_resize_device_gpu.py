"""Config.DEVICE_RESIZE: utils.resize_image on the GPU (urso_resize_images_u8 / augment.resize_images) and the feeders, detect() and
evaluate() that use it.  The device result must have the BYTES of the host function -- the kernel performs the same float64 multiplies
and adds in the same order -- so every comparison here is torch.equal / array_equal, not a tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = ("0.18", "0.19")


def _host(frames, **kw):
    from ursonet_amd import utils
    res = [utils.resize_image(f, **kw) for f in frames]
    assert all(r[4] is None for r in res)
    return np.stack([r[0] for r in res]), res[0][1:4]


def _check_equal(frames, **kw):
    """augment.resize_images(frames) == utils.resize_image(frame) for every frame: zero differing bytes, equal window / scale / padding;
    the input is not modified and a second call gives the same bytes."""
    import torch
    from ursonet_amd import augment
    frames = np.ascontiguousarray(frames)
    want, (window, scale, padding) = _host(frames, **kw)
    dev_in = torch.as_tensor(frames).cuda()
    keep = dev_in.clone()
    got, w, s, p = augment.resize_images(dev_in, **kw)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert tuple(w) == tuple(window) and float(s) == float(scale) and [tuple(x) for x in p] == [tuple(x) for x in padding]
    nbad = int((got.cpu() != torch.as_tensor(want)).sum())
    print("resize %s %s -> %s: %d differing bytes of %d" % (kw, frames.shape, want.shape, nbad, want.size))
    assert torch.equal(got.cpu(), torch.as_tensor(want)), "%d differing bytes" % nbad
    assert torch.equal(dev_in, keep), "the input was modified"
    again = augment.resize_images(frames, **kw)[0]                          # from a host array this time
    assert torch.equal(again, got)
    return got.cpu().numpy()


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_skimage.npz"))
    for case in z["cases"]:
        name, mode = str(case).split()
        a = z[name + "/args"]
        yield name, z, dict(min_dim=int(a[0]), max_dim=int(a[1]) or None, min_scale=float(a[2]) or None, mode=mode)


@pytest.mark.parametrize("compat", COMPAT)
def test_golden_inputs_equal_the_host_bytes_and_stay_within_the_reference_bound(compat, monkeypatch):
    """The five inputs of tests/golden/resize_skimage.npz with their stored arguments: byte-equal to utils.resize_image in both compat
    modes; in the default mode (the one the file was recorded for: scikit-image 0.18.3) also within the bound the host test uses against
    the reference's recorded outputs -- <= 1 grey level on <= 2 % of the pixels, exact at scale 1."""
    monkeypatch.setenv("URSO_RESIZE_COMPAT", compat)
    for name, z, kw in _golden():
        got = _check_equal(z[name + "/in"][None], **kw)[0]
        if compat == "0.18":
            ref = z[name + "/out"]
            d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
            print("golden %s: max |d| %d on %.4f of the pixels" % (name, int(d.max()), float((d > 0).mean())))
            if float(z[name + "/scale"]) == 1.0:
                assert d.max() == 0, name
            else:
                assert d.max() <= 1 and (d > 0).mean() <= 0.02, (name, int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("compat", COMPAT)
@pytest.mark.parametrize("h,w,min_dim,max_dim", [(960, 1280, 512, 640), (1200, 1920, 640, 960)])
def test_noise_at_the_dataset_geometries(h, w, min_dim, max_dim, compat, monkeypatch):
    """uint8 noise (the worst case for truncation ties) at URSO 960 x 1280 -> 512 x 640 and SPEED 1200 x 1920 -> 640 x 960, pad64, B = 4."""
    monkeypatch.setenv("URSO_RESIZE_COMPAT", compat)
    frames = np.random.default_rng(h).integers(0, 256, size=(4, h, w, 3), dtype=np.uint8)
    out = _check_equal(frames, min_dim=min_dim, max_dim=max_dim, mode="pad64")
    assert out.shape == (4, min_dim, max_dim, 3)


CASES = {
    "odd 97 x 131, min_scale 0.4": ((2, 97, 131, 3), dict(min_dim=0, min_scale=0.4, mode="pad64")),          # the golden case's arguments: pad only
    "odd 97 x 131 shrunk to 0.4": ((2, 97, 131, 3), dict(min_dim=64, max_dim=52, mode="pad64")),
    "enlargement": ((2, 40, 56, 3), dict(min_dim=64, max_dim=96, mode="square")),
    "rows keep, columns shrink": ((2, 3, 100, 3), dict(min_dim=64, max_dim=99, mode="square")),
    "columns keep, rows shrink": ((2, 100, 3, 3), dict(min_dim=64, max_dim=99, mode="square")),
    "square with odd padding": ((2, 200, 121, 3), dict(max_dim=129, mode="square")),
    "strong shrink (radius 8)": ((1, 300, 420, 3), dict(min_dim=64, max_dim=84, mode="square")),
    "scale 1": ((3, 150, 240, 3), dict(min_dim=0, min_scale=0.5, mode="pad64")),
    "one channel": ((2, 120, 90, 1), dict(max_dim=64, mode="square")),
    "B = 1": ((1, 72, 96, 3), dict(min_dim=64, max_dim=64, mode="pad64")),
    "B = 32, every image different": ((32, 72, 96, 3), dict(min_dim=64, max_dim=64, mode="pad64")),
}


@pytest.mark.parametrize("compat", COMPAT)
@pytest.mark.parametrize("case", sorted(CASES))
def test_geometries(case, compat, monkeypatch):
    monkeypatch.setenv("URSO_RESIZE_COMPAT", compat)
    shape, kw = CASES[case]
    frames = np.random.default_rng(len(case)).integers(0, 256, size=shape, dtype=np.uint8)
    if shape[0] == 32:
        assert len({f.tobytes() for f in frames}) == 32
    from ursonet_amd import utils
    scale, (nh, nw), _, _ = utils.resize_geometry(shape[1], shape[2], kw.get("min_dim"), kw.get("max_dim"), kw.get("min_scale"), kw["mode"])
    if case == "scale 1":
        assert scale == 1
    if case == "enlargement":
        assert nh > shape[1] and nw > shape[2]
    if case.startswith("rows keep"):
        assert nh == shape[1] and nw < shape[2]
    if case.startswith("columns keep"):
        assert nw == shape[2] and nh < shape[1]
    if case.startswith("square with odd"):
        assert (129 - nw) % 2 == 1
    _check_equal(frames, **kw)


# ------------------------------------------------------------------ feeders, detect(), evaluate()
def _dataset(cfg, n, sizes, seed=11):
    """An in-memory dataset of native-size uint8 RGB frames (pre-generated: SyntheticPoses' poses and targets, its frames replaced)."""
    from ursonet_amd.dataset import SyntheticPoses

    class InMemory(SyntheticPoses):
        def load_image(self, image_id):
            return self.frames[int(image_id)]
    ds = InMemory(n, sizes[0][0], sizes[0][1], cfg, seed=seed)
    rng = np.random.default_rng(seed)
    ds.frames = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:h, 0:w]
        f = rng.integers(0, 40, size=(h, w, 3)) + (((yy - h * rng.uniform(0.3, 0.7)) ** 2 + (xx - w * rng.uniform(0.3, 0.7)) ** 2) < (0.2 * h) ** 2)[:, :, None] * rng.integers(60, 200, size=(1, 1, 3))
        ds.frames.append(f.astype(np.uint8))
    return ds


def _three_batches(eng, ds, cfg, device_resize, n=3):
    """DeviceFeeder from a fixed seed of every generator the input side draws from -> [(in_images_u8, gt_loc, gt_ori)] of n batches."""
    import random
    import torch
    from ursonet_amd import augment
    from ursonet_amd.feeder import DeviceFeeder
    cfg.DEVICE_RESIZE = device_resize
    np.random.seed(5); random.seed(5); augment._PIPELINE_RNG.seed(7)
    feed = DeviceFeeder(eng, ds, cfg, shuffle=True, workers=2)
    out = []
    try:
        for _ in range(n):
            feed.next_into()
            torch.cuda.synchronize()
            out.append((eng.in_images_u8.cpu().clone(), eng.gt_loc.cpu().clone(), eng.gt_ori.cpu().clone()))
        pinned = feed.pinned_bytes
    finally:
        feed.close()
        feed.thread.join(60)                                               # it draws from the global generators: it must be gone before the next seed
        assert not feed.thread.is_alive()
        cfg.DEVICE_RESIZE = False
    return out, pinned


def _same(a, b):
    import torch
    assert len(a) == len(b) == 3
    for k, (x, y) in enumerate(zip(a, b)):
        nbad = int((x[0] != y[0]).sum())
        print("batch %d: %d differing image bytes of %d" % (k, nbad, x[0].numel()))
        assert torch.equal(x[0], y[0]), "batch %d: %d differing image bytes" % (k, nbad)
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), "batch %d: targets differ" % k
    assert not torch.equal(a[0][0], a[1][0])                                # really three different batches


@pytest.mark.parametrize("aug", [False, True])
def test_device_feeder_hands_over_identical_batches(aug):
    """Same seed, in-memory native-size frames (130 x 200 -> 64 x 128, pad64), ResNet-18: DEVICE_RESIZE off and on give the engine identical
    in_images_u8 bytes and identical targets for three consecutive batches -- plain, and with ROT_AUG + SIM2REAL_AUG."""
    from util import make_config
    from ursonet_amd.engine import Engine
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=True, dtype="float32")
    cfg.ROT_AUG = cfg.SIM2REAL_AUG = aug
    ds = _dataset(cfg, 14, [(130, 200)])
    eng = Engine(cfg, "training", seed=1)
    off, pinned_off = _three_batches(eng, ds, cfg, False)
    on, pinned_on = _three_batches(eng, ds, cfg, True)
    _same(off, on)
    assert pinned_on - pinned_off == 4 * (130 * 200 - 64 * 128) * 3        # reported truthfully: the RAW frames are what is pinned now
    if aug:
        plain, _ = _three_batches(eng, ds, make_config("resnet18", 64, 128, batch=4, regress_ori=True, dtype="float32"), False)
        assert any(not np.array_equal(p[0].numpy(), o[0].numpy()) for p, o in zip(plain, off))       # the augmentation did something


def test_mixed_sizes_and_crop_fall_back_to_the_host_path():
    from util import make_config
    from ursonet_amd.engine import Engine
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=True, dtype="float32")
    ds = _dataset(cfg, 14, [(130, 200), (128, 256), (130, 200)])             # batches with both sizes
    eng = Engine(cfg, "training", seed=1)
    _same(_three_batches(eng, ds, cfg, False)[0], _three_batches(eng, ds, cfg, True)[0])
    crop = make_config("resnet18", 64, 64, batch=4, regress_ori=True, dtype="float32")
    crop.IMAGE_RESIZE_MODE = "crop"
    crop.update()
    ds = _dataset(crop, 14, [(130, 200)])
    eng = Engine(crop, "training", seed=1)
    _same(_three_batches(eng, ds, crop, False)[0], _three_batches(eng, ds, crop, True)[0])


def _inference_model(tmp_path, B):
    from util import make_config
    from ursonet_amd import net
    cfg = make_config("resnet18", 64, 128, batch=B, regress_ori=True, dtype="float32")
    cfg.NAME = "syn"
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    path = str(tmp_path / "weights_resize_0001.npz")
    tr.save_weights(path)
    del tr
    inf = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    inf.load_weights(path, path, by_name=True)
    return cfg, inf


def test_detect_and_evaluate_are_unchanged_by_the_switch(tmp_path, monkeypatch):
    """detect() on raw native-size frames: identical in_images_u8 and identical outputs with DEVICE_RESIZE off and on; evaluate(): an
    identical result table (10 images, batch 4: the padded tail batch included).  The 'on' legs really run the kernel (one launch for
    detect, one per batch for evaluate), the 'off' legs never do."""
    import torch
    from ursonet_amd import evaluate as ev, hip
    launches, real = [], hip.resize_images_u8

    def counted(*a, **kw):
        launches.append(a[0])
        return real(*a, **kw)
    monkeypatch.setattr(hip, "resize_images_u8", counted)
    seen = {}
    cfg, model = _inference_model(tmp_path, 4)
    ds = _dataset(cfg, 10, [(130, 200)])
    frames = [ds.load_image(i) for i in range(4)]
    keep = [f.copy() for f in frames]
    res = {}
    try:
        for on in (False, True):
            cfg.DEVICE_RESIZE = on
            out = model.detect(frames)
            torch.cuda.synchronize()
            n_detect = len(launches)
            res[on] = (model._engine.in_images_u8.cpu().clone(), out, ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0))
            seen[on] = (n_detect, len(launches) - n_detect)
            del launches[:]
    finally:
        cfg.DEVICE_RESIZE = False
    assert seen[False] == (0, 0) and seen[True] == (1, 3), seen             # 10 images at batch 4: three evaluation batches
    assert all(np.array_equal(f, k) for f, k in zip(frames, keep))
    assert torch.equal(res[False][0], res[True][0]) and int(res[True][0].max()) > 0
    for a, b in zip(res[False][1], res[True][1]):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    for k in ("loc_est", "q_est", "loc_err", "ori_err", "esa", "dist"):
        assert np.array_equal(getattr(res[False][2], k), getattr(res[True][2], k)), k
    assert list(res[True][2].image_ids) == list(ds.image_ids) and np.all(np.isfinite(res[True][2].esa))


def test_evaluate_on_frames_that_are_not_uint8_keeps_the_molded_host_path(tmp_path, monkeypatch):
    """A dataset of float32 frames (native size): evaluate() molds every batch on the host (UrsoNet.mold_inputs) with the switch off and
    on, never launches the resize kernel, and its estimates are those of detect() on the same batches, bit for bit.  A dataset that
    mixes uint8 and float32 frames inside its batches gives the same table off and on."""
    from ursonet_amd import evaluate as ev, hip
    from ursonet_amd.feeder import eval_batch_plan
    launches, real = [], hip.resize_images_u8

    def counted(*a, **kw):
        launches.append(a[0])
        return real(*a, **kw)
    monkeypatch.setattr(hip, "resize_images_u8", counted)
    cfg, model = _inference_model(tmp_path, 4)
    ds = _dataset(cfg, 10, [(130, 200)])
    mixed = _dataset(cfg, 10, [(130, 200)], seed=12)
    mixed.frames = [f.astype(np.float32) if i % 2 == 1 else f for i, f in enumerate(mixed.frames)]      # every batch of 4 holds both kinds
    ds.frames = [f.astype(np.float32) for f in ds.frames]
    res, res_mixed = {}, {}
    try:
        for on in (False, True):
            cfg.DEVICE_RESIZE = on
            res[on] = ev.evaluate(model, ds, out_dir=str(tmp_path), verbose=0)
            res_mixed[on] = ev.evaluate(model, mixed, out_dir=str(tmp_path), verbose=0)
    finally:
        cfg.DEVICE_RESIZE = False
    assert launches == []
    loc, ori = [], []
    for row0, n, slots in eval_batch_plan(ds.image_ids, 4):
        for r in model.detect([ds.load_image(i) for i in slots])[:n]:
            loc.append(np.asarray(r["loc"], np.float64)); ori.append(r["ori"].astype(np.float64))
    for on in (False, True):
        assert np.array_equal(res[on].loc_est, np.asarray(loc)) and np.array_equal(res[on].q_est, np.asarray(ori)), on
        assert np.all(np.isfinite(res[on].esa))
    for k in ("loc_est", "q_est", "loc_err", "ori_err", "esa", "dist"):
        assert np.array_equal(getattr(res_mixed[False], k), getattr(res_mixed[True], k)), k
    assert np.all(np.isfinite(res_mixed[True].esa))
