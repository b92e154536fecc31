"""The host side of Config.DEVICE_RESIZE, checked without a GPU: utils.resize_tables is the one definition of the Gaussian taps, source
indices and fractions that utils._bilinear_resize and urso_resize_images_u8 share; the refactor changed no byte of utils.resize_image;
the new entry point is exported and validates its arguments; the switch is off by default."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("h,w,nh,nw", [(960, 1280, 512, 683), (1200, 1920, 600, 960), (97, 131, 39, 52), (40, 56, 64, 90),
                                       (3, 100, 3, 99), (100, 3, 99, 3), (300, 420, 60, 84), (64, 64, 64, 64)])
def test_resize_tables_restate_the_bilinear_resize_arithmetic(h, w, nh, nw):
    """Independent restatement: scipy.ndimage's truncate = 4 Gaussian of sigma = (in / out - 1) / 2 per shrinking axis, and the
    centre-aligned source coordinate (j + 0.5) in / out - 0.5 split into floor and fraction."""
    from ursonet_amd import utils
    t = utils.resize_tables(h, w, nh, nw)
    for axis, (n_in, n_out) in enumerate(((h, nh), (w, nw))):
        k = t["taps"][axis]
        if n_out >= n_in:
            assert k is None                                                # an axis that does not shrink is not smoothed
            continue
        sigma = (n_in / n_out - 1) / 2.0
        r = max(1, int(4.0 * sigma + 0.5))
        want = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
        want = want / want.sum()
        assert k.dtype == np.float64 and k.shape == (2 * r + 1,) and np.array_equal(k, want)
        assert np.array_equal(k, utils._gaussian_kernel1d(sigma))
    for idx, frac, n_in, n_out in ((t["y0"], t["fy"], h, nh), (t["x0"], t["fx"], w, nw)):
        s = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        assert idx.dtype == np.int32 and frac.dtype == np.float64 and idx.shape == frac.shape == (n_out,)
        assert np.array_equal(idx, np.floor(s).astype(int)) and np.array_equal(frac, s - np.floor(s).astype(int))
        assert idx.min() >= -1 and idx.max() <= n_in - 1 and frac.min() >= 0 and frac.max() < 1


def _old_bilinear_resize(image, out_h, out_w, trunc):
    """utils._bilinear_resize as it was before resize_tables existed (uint8 frames), restated."""
    from ursonet_amd import utils
    h, w = image.shape[:2]
    img = image.astype(np.float64)
    for axis, (n_in, n_out) in enumerate(((h, out_h), (w, out_w))):
        if n_out < n_in:
            img = utils._smooth_axis(img, (n_in / n_out - 1) / 2.0, axis)
            if trunc:
                img = np.trunc(img)
    ys = (np.arange(out_h) + 0.5) * h / out_h - 0.5
    xs = (np.arange(out_w) + 0.5) * w / out_w - 0.5
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    rows = lambda yy: img[np.clip(yy, 0, h - 1)] * ((yy >= 0) & (yy < h))[:, None, None]
    cols = lambda a, xx: a[:, np.clip(xx, 0, w - 1)] * ((xx >= 0) & (xx < w))[None, :, None]
    top, bot = rows(y0), rows(y0 + 1)
    return (cols(top, x0) * (1 - fx) + cols(top, x0 + 1) * fx) * (1 - fy) + (cols(bot, x0) * (1 - fx) + cols(bot, x0 + 1) * fx) * fy


@pytest.mark.parametrize("compat", ["0.18", "0.19"])
def test_the_refactor_changed_no_bit(compat, monkeypatch):
    from ursonet_amd import utils
    monkeypatch.setenv("URSO_RESIZE_COMPAT", compat)
    rng = np.random.default_rng(2)
    for (h, w), (nh, nw) in (((97, 131), (39, 52)), ((40, 56), (64, 90)), ((30, 100), (30, 61)), ((240, 320), (96, 128))):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        assert np.array_equal(utils._bilinear_resize(img, nh, nw), _old_bilinear_resize(img, nh, nw, compat == "0.18"))


def test_resize_image_still_returns_the_golden_bytes(monkeypatch):
    """tests/golden/resize_skimage.npz (the reference's utils.resize_image under scikit-image 0.18.3) under the existing bound: <= 1 grey
    level on <= 2 % of the pixels, exact at scale 1."""
    from ursonet_amd import utils
    monkeypatch.delenv("URSO_RESIZE_COMPAT", raising=False)
    z = np.load(os.path.join(ROOT, "tests", "golden", "resize_skimage.npz"))
    assert len(z["cases"]) == 5
    for case in z["cases"]:
        name, mode = str(case).split()
        a = z[name + "/args"]
        out, window, scale, padding, crop = utils.resize_image(z[name + "/in"], min_dim=int(a[0]), max_dim=int(a[1]) or None,
                                                               min_scale=float(a[2]) or None, mode=mode)
        ref = z[name + "/out"]
        assert out.shape == ref.shape and out.dtype == np.uint8 and crop is None
        assert tuple(window) == tuple(z[name + "/window"]) and float(scale) == float(z[name + "/scale"])
        d = np.abs(out.astype(np.int32) - ref.astype(np.int32))
        if float(scale) == 1.0:
            assert d.max() == 0, name
        else:
            assert d.max() <= 1 and (d > 0).mean() <= 0.02, (name, int(d.max()), float((d > 0).mean()))


def test_entry_point_is_exported_and_validates_its_arguments_without_a_gpu():
    import ursonet_amd.hip as hip
    assert "urso_resize_images_u8" in hip.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(lib, "urso_resize_images_u8")
    f = hip._lib.urso_resize_images_u8
    P = lambda n: ctypes.c_void_p(0x1000 * n)                               # never dereferenced: every call below is refused before a launch
    good = dict(B=2, H=100, W=120, C=3, NH=50, NW=60, OH=64, OW=64, top=7, left=2, ky=P(1), ry=2, kx=P(2), rx=2, y0=P(3), fy=P(4), x0=P(5),
                fx=P(6), trunc=1, src=P(7), dst=P(8), stream=None)

    def rc(**kw):
        a = dict(good, **kw)
        return f(*[a[k] for k in good])
    bad = [dict(src=None), dict(dst=None), dict(y0=None), dict(fy=None), dict(x0=None), dict(fx=None),
           dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(NH=0), dict(NW=0), dict(OH=0), dict(OW=-5),
           dict(top=-1), dict(left=-1), dict(top=15), dict(left=5), dict(OH=56), dict(OW=61),                 # window outside the output
           dict(ry=0), dict(rx=0), dict(rx=-3),                                                              # radius < 1 with a tap table
           dict(dst=good["src"]), dict(trunc=2)]
    for kw in bad:
        assert rc(**kw) == -1 and "urso_resize_images_u8" in hip.last_error(), kw
    assert rc(H=30000, W=30000, NH=8, NW=8, ry=7499, rx=7498) == -1                                           # the patch of ONE output pixel does not fit
    msg = hip.last_error()
    assert "30000 x 30000 -> 8 x 8 (radii 7499, 7498)" in msg and "more than 65536 bytes of LDS" in msg, msg


def test_switch_is_off_by_default_and_unsupported_input_is_refused_on_the_host():
    from ursonet_amd import augment
    from ursonet_amd.config import Config
    assert Config().DEVICE_RESIZE is False
    u8 = np.zeros((2, 40, 56, 3), dtype=np.uint8)
    for mode in ("crop", "none"):
        with pytest.raises(ValueError):
            augment.resize_images(u8, min_dim=64, max_dim=64, mode=mode)
    for imgs in (u8.astype(np.float32), u8.astype(np.float64), u8.astype(np.int16), u8[0]):
        with pytest.raises(ValueError):
            augment.resize_images(imgs, min_dim=64, max_dim=64, mode="square")
