"""The video path on the GPU: urso_video_prep_u8 byte for byte against VideoPrep.host (all 2^24 RGB triples, odd geometry, the reference's
frame size), urso_draw_prims_u8 byte for byte against the NumPy statement of its integer rule (tests/videoref.py), and track() end to end
against predict() on host-prepared frames, with the rendered windows against the NumPy rasteriser."""
import itertools

import numpy as np
import pytest
import torch

import videoref as VR
from util import make_config

pytestmark = pytest.mark.gpu


def _prep_gpu(frames, prep):
    from ursonet_amd import augment
    out = augment.video_prep(frames, prep)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------ urso_video_prep_u8
def test_prep_all_rgb_triples():
    """Every (R, G, B) once, as 16 frames of 1024 x 1024, default weights, no crop, no pad: zero differing bytes.  27,801 triples change
    their byte when a multiply and an add of the mix are fused, so a contracted kernel fails here."""
    from ursonet_amd.video import VideoPrep
    idx = np.arange(1 << 24, dtype=np.uint32)
    frames = np.stack([(idx >> 16).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx & 255).astype(np.uint8)], axis=-1)
    frames = frames.reshape(16, 1024, 1024, 3)
    prep = VideoPrep(crop=(0, 0, 0, 0), pad=0)
    ref = np.stack([prep.host(f) for f in frames])
    got = _prep_gpu(frames, prep)
    diff = int((got != ref).sum())
    print("differing bytes over all 2^24 triples:", diff, " max byte:", int(got.max()))
    assert got.shape == ref.shape and diff == 0
    assert got.max() == 254 and tuple(got[15, 1023, 1023]) == (254, 254, 254)


def _one_by_one(h, w):
    return ((h - 1) // 2, h - 1 - (h - 1) // 2, (w - 1) // 2, w - 1 - (w - 1) // 2)


def test_prep_small_geometry():
    """Widths 1, 2, 5, 63, 64, 65, 129 (OW * 3 mod 4 takes all four values, rows shorter and longer than a 16-byte vector), heights 1 and
    17, B 1 and 3 (frames that start at any alignment), pads 0, 1, 7, four crops: every combination the crop leaves a pixel of, byte for
    byte; the others raise before anything is launched."""
    from ursonet_amd import augment
    from ursonet_amd.video import VideoPrep
    rng = np.random.default_rng(7)
    seen_mod, n_ok, n_bad = set(), 0, 0
    for w, h, B, pad in itertools.product((1, 2, 5, 63, 64, 65, 129), (1, 17), (1, 3), (0, 1, 7)):
        frames = rng.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
        frames[:, h // 2, w // 2] = 255
        for crop in ((0, 0, 0, 0), (0, 0, 1, 2), (3, 2, 0, 0), _one_by_one(h, w)):
            prep = VideoPrep(crop=crop, pad=pad)
            if h - crop[0] - crop[1] <= 0 or w - crop[2] - crop[3] <= 0:
                with pytest.raises(ValueError, match="leaves no pixel"):
                    augment.video_prep(frames, prep)
                n_bad += 1
                continue
            ref = np.stack([prep.host(f) for f in frames])
            got = _prep_gpu(frames, prep)
            assert got.shape == ref.shape and np.array_equal(got, ref), (w, h, B, pad, crop)
            seen_mod.add(ref.shape[2] * 3 % 4)
            n_ok += 1
    assert seen_mod == {0, 1, 2, 3} and n_ok > 200 and n_bad > 0
    assert VideoPrep(crop=_one_by_one(17, 129), pad=0).out_shape(17, 129) == (1, 1)


@pytest.mark.parametrize("grey", [(1.0, 0.0, 0.0), (0.3, 0.59, 0.11)])
def test_prep_other_weights(grey):
    from ursonet_amd.video import VideoPrep
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(3, 37, 131, 3), dtype=np.uint8)
    frames[0, :4] = 255
    frames[1, :4] = (255, 0, 255)
    for crop, pad in (((0, 0, 1, 2), 5), ((0, 0, 0, 0), 0)):
        prep = VideoPrep(crop=crop, pad=pad, grey=grey)
        ref = np.stack([prep.host(f) for f in frames])
        assert np.array_equal(_prep_gpu(frames, prep), ref)
    if grey == (1.0, 0.0, 0.0):
        assert np.array_equal(ref[..., 0], frames[..., 0])


def test_prep_reference_geometry():
    """2 x 960 x 1280 with the reference's crop, pad and weights -> 2 x 1760 x 1929 x 3: byte for byte, and no byte above 254."""
    from ursonet_amd.video import VideoPrep
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, size=(2, 960, 1280, 3), dtype=np.uint8)
    frames[0, 100:200, 300:500] = 255
    frames[1, :, :2] = 255
    frames[1, -1] = 255
    prep = VideoPrep()
    ref = np.stack([prep.host(f) for f in frames])
    got = _prep_gpu(frames, prep)
    assert got.shape == (2, 1760, 1929, 3) and np.array_equal(got, ref)
    assert got.max() == 254
    assert not got[:, :400].any() and not got[:, -400:].any() and not got[:, :, :400].any() and not got[:, :, -400:].any()


def test_prep_out_buffer_at_an_odd_address():
    """`out` given by the caller and starting 5 bytes into an allocation: the bytes around the frame stay as they were."""
    from ursonet_amd import augment
    from ursonet_amd.video import VideoPrep
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, size=(2, 9, 21, 3), dtype=np.uint8)
    prep = VideoPrep(crop=(0, 0, 1, 0), pad=2)
    oh, ow = prep.out_shape(9, 21)
    n = 2 * oh * ow * 3
    slab = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    out = slab[5:5 + n].view(2, oh, ow, 3)
    assert augment.video_prep(frames, prep, out=out).data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = slab.cpu().numpy()
    assert np.array_equal(host[5:5 + n].reshape(2, oh, ow, 3), np.stack([prep.host(f) for f in frames]))
    assert np.all(host[:5] == 0xAB) and np.all(host[5 + n:] == 0xAB)


def test_prep_bad_arguments_do_not_launch():
    from ursonet_amd import hip
    src = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), 0xCD, dtype=torch.uint8, device="cuda")
    grey = (0.21, 0.72, 0.07)
    for crop, pad, what in (((8, 0, 0, 0), 0, "leaves no pixel"), ((0, 0, 5, 3), 1, "leaves no pixel"), ((-1, 0, 0, 0), 0, "negative"),
                            ((0, 0, 0, -2), 0, "negative"), ((0, 0, 0, 0), -1, "negative"), ((0, 0, 0, 0), 15000, "2 GiB")):
        with pytest.raises(hip.UrsoHipError, match=what):
            hip.video_prep_u8(1, 8, 8, crop, pad, grey, src, dst)
    torch.cuda.synchronize()
    assert bool((dst == 0xCD).all())


# ------------------------------------------------------------------ urso_draw_prims_u8
SHAPES = ((48, 64), (33, 130))


def _draw_and_compare(h, w, per_frame, seed=0):
    """per_frame: a list of B primitive lists.  Device result == the NumPy rule applied to the same random background."""
    from ursonet_amd import augment
    rng = np.random.default_rng(seed)
    B = len(per_frame)
    bg = rng.integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    dev = torch.as_tensor(bg).cuda()
    assert augment.draw_prims(dev, [np.asarray(p, dtype=np.int32).reshape(-1, 9) for p in per_frame]) is dev
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    for b in range(B):
        ref = VR.rasterise(bg[b], per_frame[b])
        assert np.array_equal(got[b], ref), (h, w, b, per_frame[b], np.argwhere((got[b] != ref).any(axis=2))[:8])
    return bg, got


def _seg(x0, y0, x1, y1, t, c=(250, 120, 10)):
    return [0, x0, y0, x1, y1, t] + list(c)


def _disc(x, y, r, c=(10, 240, 130)):
    return [1, x, y, 0, 0, r] + list(c)


@pytest.mark.parametrize("h,w", SHAPES)
def test_draw_segments(h, w):
    lines = {"horizontal": (5, 11, w - 9, 11), "vertical": (w // 2, 2, w // 2, h - 3), "diagonal": (3, 4, 3 + h - 10, 4 + h - 10),
             "shallow": (2, h - 6, w - 4, h - 13), "steep-reversed": (w - 7, h - 2, w - 12, 1)}
    for name, (x0, y0, x1, y1) in lines.items():
        _draw_and_compare(h, w, [[_seg(x0, y0, x1, y1, t)] for t in (1, 2, 5)], seed=1)
    # zero-length segments of thickness 0, 1, 2, 5, 6, 11
    _draw_and_compare(h, w, [[_seg(20, 15, 20, 15, t)] for t in (0, 1, 2)], seed=2)
    _draw_and_compare(h, w, [[_seg(w - 3, h - 2, w - 3, h - 2, t)] for t in (5, 6, 11)], seed=3)


@pytest.mark.parametrize("h,w", SHAPES)
def test_draw_outside_and_far_endpoints(h, w):
    M = 16384
    bg, got = _draw_and_compare(h, w, [[_seg(-20, 10, 15, 25, 2)], [_seg(w - 10, h - 5, w + 30, h + 9, 5)], [_seg(-7, -3, w + 9, h + 2, 1)]], seed=4)
    assert all((got[b] != bg[b]).any() for b in range(3))                    # partly outside: something is drawn
    bg, got = _draw_and_compare(h, w, [[_seg(-30, -30, -3, -4, 5)], [_seg(w + 5, 0, w + 5, h, 2)], [_seg(0, h + 40, w, h + 3, 5), _disc(-9, -9, 7)]], seed=5)
    assert np.array_equal(got, bg)                                           # wholly outside: nothing is
    for t in (1, 2, 5):
        bg, got = _draw_and_compare(h, w, [[_seg(-M, -M, M, M, t)], [_seg(-M, 10, M, 30, t)], [_seg(M, -M, -M, M, t)]], seed=6)
        assert (got[0] != bg[0]).any() and (got[1] != bg[1]).any()
    _draw_and_compare(h, w, [[_seg(M, M, 5, 5, 5)], [_seg(-M, h // 2, M, h // 2, M)], [_seg(w // 2, -M, w // 2, M, 2), _disc(M, M, M)]], seed=7)


@pytest.mark.parametrize("h,w", SHAPES)
def test_draw_discs_order_and_counts(h, w):
    _draw_and_compare(h, w, [[_disc(10, 12, r)] for r in (0, 1, 7)], seed=8)
    _draw_and_compare(h, w, [[_disc(-3, 5, 7)], [_disc(w + 2, h + 1, 7)], [_disc(w - 1, h - 1, 1), _disc(0, 0, 0)]], seed=9)
    # 16 overlapping primitives per frame, in order, and the same 16 reversed: the later one wins
    rng = np.random.default_rng(10)
    full = []
    for _ in range(16):
        c = tuple(int(v) for v in rng.integers(0, 256, size=3))
        if rng.random() < 0.5:
            full.append(_seg(*(int(v) for v in rng.integers(-10, max(h, w) + 10, size=4)), int(rng.integers(0, 9)), c))
        else:
            full.append(_disc(int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 12)), c))
    _draw_and_compare(h, w, [full, full[::-1], full[:7]], seed=11)
    # per-frame counts that differ within one batch, a count of 0 among them
    bg, got = _draw_and_compare(h, w, [full[:1], [], full], seed=12)
    assert np.array_equal(got[1], bg[1])
    # all counts 0: the frames stay untouched
    bg, got = _draw_and_compare(h, w, [[], [], []], seed=13)
    assert np.array_equal(got, bg)


def test_draw_counts_array_form_and_bad_arguments():
    """prims [B, P, 9] + counts: rows behind a frame's count are ignored.  Unknown kinds, counts above 16 and coordinates beyond +-16,384
    raise and launch nothing."""
    from ursonet_amd import augment, hip
    h, w = 48, 64
    rng = np.random.default_rng(14)
    bg = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    prims = np.zeros((2, 3, 9), dtype=np.int32)
    prims[0] = [_seg(2, 2, 40, 30, 2), _disc(30, 20, 5), [7, 0, 0, 0, 0, 99999, 0, 0, 0]]      # the third row lies behind count 2: never looked at
    prims[1] = [_disc(5, 5, 3), _seg(0, 0, 63, 47, 5), _disc(9, 9, 9)]
    dev = torch.as_tensor(bg).cuda()
    augment.draw_prims(dev, prims, [2, 1])
    got = dev.cpu().numpy()
    assert np.array_equal(got[0], VR.rasterise(bg[0], prims[0, :2])) and np.array_equal(got[1], VR.rasterise(bg[1], prims[1, :1]))
    dev = torch.as_tensor(bg).cuda()
    bad = [[[2, 1, 1, 5, 5, 2, 1, 1, 1]], [[-1, 1, 1, 5, 5, 2, 1, 1, 1]], [_seg(16385, 0, 5, 5, 2)], [_seg(0, -16385, 5, 5, 2)], [_disc(0, 0, 16385)],
           [_seg(0, 0, 5, 5, -1)], [_disc(1, 1, 1)] * 17]
    for p in bad:
        with pytest.raises(hip.UrsoHipError):
            augment.draw_prims(dev, [[_disc(3, 3, 2)], p])
    host = np.zeros((2, 16, 9), dtype=np.int32)
    host[:, :, :] = _disc(3, 3, 2)
    pd, cd = torch.as_tensor(host).cuda(), torch.as_tensor(np.array([1, 17], dtype=np.int32)).cuda()
    with pytest.raises(hip.UrsoHipError, match="17 primitives"):
        hip.draw_prims_u8(2, h, w, host, np.array([1, 17], dtype=np.int32), pd, cd, dev)
    tall = torch.zeros(1, 16385, 1, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.UrsoHipError, match="H, W"):
        hip.draw_prims_u8(1, 16385, 1, host[:1], np.array([1], dtype=np.int32), pd[:1].contiguous(), cd[:1].contiguous(), tall)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), bg)


# ------------------------------------------------------------------ track()
FRAME_H, FRAME_W, N_FRAMES = 60, 90, 5


class _Prepared(object):
    """An unlabelled dataset whose images are the host-prepared video frames: what predict() must see to reproduce track()."""

    def __init__(self, ds, frames, prep):
        self._ds, self._frames, self._prep = ds, frames, prep
        self.image_info = [{"path": "video/frame%04d.jpg" % i} for i in range(len(frames))]
        self.camera = ds.camera

    @property
    def image_ids(self):
        return np.arange(len(self._frames))

    def load_image(self, image_id):
        return self._prep.host(self._frames[image_id])

    def __getattr__(self, name):
        if name in ("histogram_3D_map", "ori_histogram_map"):
            return getattr(self._ds, name)
        raise AttributeError(name)


@pytest.fixture(scope="module")
def tracked(tmp_path_factory):
    """ResNet-18 at 128 x 192 (the smallest configuration of tests/test_predict_gpu.py), engine batch 2, for the regression and the
    soft-classification orientation head; 5 frames of 60 x 90, so the tail batch is padded.  prep: pad 8, crop (0, 0, 1, 3) -> 76 x 102
    -> resized to 128 x 172 inside 128 x 192."""
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.video import VideoPrep
    prep = VideoPrep(pad=8, crop=(0, 0, 1, 3))
    out = {}
    for regress_ori in (True, False):
        td = tmp_path_factory.mktemp("video%d" % regress_ori)
        cfg = make_config("resnet18", 128, 192, batch=2, regress_ori=regress_ori, regress_loc=True, ori_bins=8, loc_bins=4, dtype="float32")
        cfg.NAME = "syn"
        tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(td))
        path = str(td / "weights_0001.npz")
        tr.save_weights(path)
        del tr
        model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(td))
        model.load_weights(path, path, by_name=True)
        ds = SyntheticPoses(N_FRAMES, FRAME_H, FRAME_W, cfg, seed=21)
        frames = [ds.load_image(i) for i in ds.image_ids]
        assert frames[0].shape == (FRAME_H, FRAME_W, 3) and frames[0].dtype == np.uint8
        out[regress_ori] = (cfg, model, _Prepared(ds, frames, prep), frames, prep)
    return out


@pytest.mark.parametrize("regress_ori", [True, False])
def test_track_equals_predict_on_host_prepared_frames(tracked, regress_ori):
    from ursonet_amd import predict as pr, video
    cfg, model, data, frames, prep = tracked[regress_ori]
    ref = pr.predict(model, data)
    res = video.track(model, iter(frames), data, prep=prep)                  # any iterable: a generator here
    assert res.loc_est.shape == (N_FRAMES, 3) and res.q_est.shape == (N_FRAMES, 4) and res.pose_unreal.shape == (N_FRAMES, 6)
    assert np.all(np.isfinite(res.loc_est)) and np.all(np.isfinite(res.q_est))
    assert np.array_equal(res.loc_est, ref.loc_est) and np.array_equal(res.q_est, ref.q_est)
    assert res.loc_peak is None and ref.loc_peak is None
    if regress_ori:
        assert res.ori_peak is None and res.ori_lambda is None
    else:
        assert np.array_equal(res.ori_peak, ref.ori_peak) and np.array_equal(res.ori_lambda, ref.ori_lambda)
    want = np.array([video.pose_unreal(l, q) for l, q in zip(ref.loc_est, ref.q_est)])
    assert np.array_equal(res.pose_unreal, want)
    assert res.frames is None
    # the same frames as a list, single-threaded pinned copy: the same bits
    again = video.track(model, frames, data, prep=prep, workers=1)
    assert np.array_equal(again.loc_est, res.loc_est) and np.array_equal(again.q_est, res.q_est)
    empty = video.track(model, [], data, prep=prep)
    assert empty.loc_est.shape == (0, 3) and empty.q_est.shape == (0, 4) and empty.pose_unreal.shape == (0, 6)
    with pytest.raises(ValueError, match="one size"):
        video.track(model, [frames[0], frames[1][:-1]], data, prep=prep)


def test_track_rendered_frames(tracked):
    """render=True: every returned frame is the NumPy rasteriser applied to the window of augment.resize_images(prep.host(frame)) with
    the primitives of that frame's own estimate; the sink receives the same arrays the result collects.  With a camera matrix that sends
    every point to (40, 30), all nine rows are zero-length segments of thickness 2 there: by the rule, (40, 30) and its four neighbours,
    in the last arrow's colour."""
    from ursonet_amd import augment, video
    cfg, model, data, frames, prep = tracked[True]
    plain = video.track(model, frames, data, prep=prep)
    res = video.track(model, frames, data, prep=prep, render=True)
    assert np.array_equal(res.loc_est, plain.loc_est) and np.array_equal(res.q_est, plain.q_est)
    assert len(res.frames) == N_FRAMES
    got = {}
    via_sink = video.track(model, frames, data, prep=prep, render=True, sink=lambda i, a: got.__setitem__(i, np.array(a)))
    assert via_sink.frames is None and sorted(got) == list(range(N_FRAMES))
    pin = np.array([[0.0, 0, 40], [0, 0.0, 30], [0, 0, 1]])
    pinned = video.track(model, frames, data, prep=prep, render=True, K=pin)
    painted = 0
    for i, f in enumerate(frames):
        out, window, _scale, _pad = augment.resize_images(prep.host(f)[None], min_dim=cfg.IMAGE_MIN_DIM, max_dim=cfg.IMAGE_MAX_DIM,
                                                          min_scale=cfg.IMAGE_MIN_SCALE, mode=cfg.IMAGE_RESIZE_MODE)
        y0, x0, y1, x1 = window
        assert (y1 - y0, x1 - x0) == (128, 172)
        win = out[0, y0:y1, x0:x1].cpu().numpy()
        K = video.camera_matrix(data.camera, x1 - x0, y1 - y0)
        prims = video.pose_axes_prims(res.q_est[i], res.loc_est[i], K)
        ref = VR.rasterise(win, prims)
        painted += int((ref != win).any(axis=2).sum())
        assert res.frames[i].shape == (128, 172, 3) and res.frames[i].dtype == np.uint8
        assert np.array_equal(res.frames[i], ref), i
        assert np.array_equal(got[i], res.frames[i]), i
        changed = {(int(x), int(y)) for y, x in np.argwhere((pinned.frames[i] != win).any(axis=2))}
        cross = {(40, 30), (39, 30), (41, 30), (40, 29), (40, 31)}
        assert changed <= cross and all(tuple(pinned.frames[i][y, x]) == (255, 0, 0) for x, y in cross), i
    print("pixels the default camera matrix painted over the 5 frames:", painted)
