"""Test-time view fusion without a GPU: the surface of the extension library liburso_ext.so (include/ursonet_ext.h), the argument checks
of urso_pose_fuse_views (they run before any launch), the de-rotation convention against the float64 oracle, the camera at model size
and the refusals of predict() / evaluate() / test_and_submit() with views."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from libsurface import header_symbols
from oracle import pose_math as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXT_HEADER = os.path.join(ROOT, "include", "ursonet_ext.h")


# ------------------------------------------------------------------ the extension's header (its surface: tests/test_side_libs_cpu.py)
def test_extension_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names = sorted(header_symbols(EXT_HEADER)[0])
    src = tmp_path / "ext_abi.c"
    src.write_text('#include "ursonet_ext.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\nfn table[] = {\n' +
                   "".join("    (fn)%s,\n" % n for n in names) + "};\nsize_t count(void) { return sizeof(table) / sizeof(table[0]); }\n"
                   "size_t args_size(void) { return sizeof(urso_pose_fuse_views_args); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-pedantic", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "ext_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_constants_are_mirrored():
    import ursonet_amd.hip as hip
    from ursonet_amd import views as vw
    hdr = open(EXT_HEADER).read()
    found = dict(re.findall(r"\bURSO_FUSE_(\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert set(found) == {"LOC_EST", "Q_EST", "LOC_ERR", "ORI_ERR", "ESA", "DIST", "LOC_SPREAD", "ORI_SPREAD", "VIEW_LAMBDA", "N_VIEWS",
                          "COLS", "MAX_VIEWS"}
    for name, value in found.items():
        assert getattr(hip, "FUSE_" + name) == int(value), name
    for name in ("LOC_EST", "Q_EST", "LOC_ERR", "ORI_ERR", "ESA", "DIST"):   # columns 0..10 sit at urso_pose_eval's positions
        assert getattr(hip, "FUSE_" + name) == getattr(hip, "EVAL_" + name), name
    assert hip.FUSE_Q_EST == hip.DEC_Q_EST and hip.FUSE_LOC_EST == hip.DEC_LOC_EST and vw.MAX_VIEWS == hip.FUSE_MAX_VIEWS
    # the ctypes struct has the C struct's size and layout (two int32, int64, two int32, int64, six pointers)
    assert ctypes.sizeof(hip.PoseFuseViewsArgs) == 80 and hip.PoseFuseViewsArgs.est.offset == 32 and hip.PoseFuseViewsArgs.table.offset == 72


# ------------------------------------------------------------------ argument validation
def _args(**kw):
    import ursonet_amd.hip as hip
    a = hip.PoseFuseViewsArgs()
    a.B, a.n, a.row0, a.V, a.est_ld, a.est_view_rows = 4, 4, 0, 3, 12, 4
    a.est = a.r = a.qr = a.table = 4096                                     # never dereferenced: every case fails validation
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_pose_fuse_views_argument_validation_without_gpu():
    import ursonet_amd.hip as hip
    lib = hip.side_lib("ext")
    cases = [
        (dict(est=None), "null"), (dict(r=None), "null"), (dict(qr=None), "null"), (dict(table=None), "null"),
        (dict(loc_gt=4096), "both or neither"), (dict(q_gt=4096), "both or neither"),
        (dict(B=0, n=0), "B > 0"), (dict(B=-1, n=0), "B > 0"), (dict(n=5), "n <= B"), (dict(n=-1), "n <= B"),
        (dict(row0=-1), "row0"),
        (dict(V=0), "V"), (dict(V=-3), "V"), (dict(V=65), "V"),
        (dict(est_ld=6), "est_ld"), (dict(est_ld=0), "est_ld"),
        (dict(est_view_rows=3), "est_view_rows"), (dict(est_view_rows=-1), "est_view_rows"),
    ]
    for kw, msg in cases:
        a = _args(**kw)
        assert lib.urso_pose_fuse_views(ctypes.byref(a), None) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_pose_fuse_views:") and msg in err, (kw, err)
    assert lib.urso_pose_fuse_views(None, None) == -1
    assert hip.last_error().startswith("urso_pose_fuse_views:") and "null" in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU), with and without a truth, at both ends of V
    for kw in (dict(n=0), dict(n=0, loc_gt=4096, q_gt=4096), dict(n=0, V=1), dict(n=0, V=64), dict(n=0, est_ld=7, est_view_rows=9)):
        assert lib.urso_pose_fuse_views(ctypes.byref(_args(**kw)), None) == 0, kw


# ------------------------------------------------------------------ conventions
def derotate(t, q, R, qR):
    """The de-rotation of include/ursonet_ext.h, written out: t R, and quat_mult(conj(qR), q) normalised."""
    t_hat = np.array([sum(t[i] * R[i][j] for i in range(3)) for j in range(3)])
    x, y, z, w = -qR[0], -qR[1], -qR[2], qR[3]
    m = np.array([w * q[0] + z * q[1] - y * q[2] + x * q[3],
                  -z * q[0] + w * q[1] + x * q[2] + y * q[3],
                  y * q[0] - x * q[1] + w * q[2] + z * q[3],
                  -x * q[0] - y * q[1] - z * q[2] + w * q[3]])
    return t_hat, m / np.sqrt(np.sum(m * m))


def test_derotation_inverts_the_augmentations_pose_update():
    """200 random poses under views drawn as the training augmentation draws them (ROT_AUG: pitch / yaw in +-10 degrees; ROT_IMAGE_AUG:
    roll in +-85): the pose rotated by augment.rotate_pose, whose algebra is pinned to the float64 oracle here, comes back."""
    from ursonet_amd import augment, views as vw
    rng = np.random.default_rng(0)
    worst_t = worst_q = 0.0
    for _ in range(200):
        t = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 40)])
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        pyr = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(-85, 85)])
        (R,), (qR,) = vw.view_rotations(pyr[None])
        assert np.allclose(R, P.euler2SO3_left(*pyr), rtol=0, atol=1e-15)
        assert 1 - abs(np.dot(qR, P.SO32quat(P.euler2SO3_left(*pyr)))) <= 1e-15
        t_rot, q_rot = augment.rotate_pose(t, q, R)
        q_ref = np.asarray(P.quat_mult(P.SO32quat(R), q), dtype=np.float64).ravel()
        assert np.allclose(t_rot, t @ R.T, rtol=0, atol=1e-13) and 1 - abs(np.dot(q_rot, q_ref / np.linalg.norm(q_ref))) <= 1e-15
        t_hat, q_hat = derotate(t_rot, q_rot, R, qR)
        worst_t, worst_q = max(worst_t, np.abs(t_hat - t).max()), max(worst_q, 1 - abs(np.dot(q_hat, q)))
    print("de-rotation: location %.2e  quaternion 1 - |dot| %.2e" % (worst_t, worst_q))
    assert worst_t <= 1e-12 and worst_q <= 1e-14


def test_view_rotations_and_roll_views():
    from ursonet_amd import views as vw
    R, qR = vw.view_rotations([[0, 0, 0], [0, 0, 40], [5, -5, -70]])
    assert R.shape == (3, 3, 3) and qR.shape == (3, 4) and R.dtype == np.float64
    assert np.array_equal(R[0], np.eye(3)) and np.array_equal(qR[0], [0, 0, 0, 1]) and vw.is_identity(R[0]) and not vw.is_identity(R[1])
    for r in R:
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(r) - 1) < 1e-15
    assert np.array_equal(vw.ROLL_VIEWS(1, 0), [[0, 0, 0]]) and np.array_equal(vw.ROLL_VIEWS(1, 45), [[0, 0, 0]])
    assert np.array_equal(vw.ROLL_VIEWS(3, 30), [[0, 0, -30], [0, 0, 0], [0, 0, 30]])
    assert np.allclose(vw.ROLL_VIEWS(4, 60)[:, 2], [-60, -20, 20, 60]) and np.array_equal(vw.ROLL_VIEWS(7, 60)[:, 2], [-60, -40, -20, 0, 20, 40, 60])
    for bad in ([0, 0, 0], [[0, 0]], [[[0, 0, 0]]], np.zeros((0, 3)), np.zeros((65, 3)), [[0, np.nan, 0]], [[np.inf, 0, 0]], "abc", None):
        with pytest.raises(ValueError, match="views"):
            vw.view_rotations(bad)
    with pytest.raises(ValueError):
        vw.ROLL_VIEWS(0, 10)


def test_views_module_imports_neither_torch_nor_the_library():
    import sys
    code = "import sys; import ursonet_amd.views; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ the camera at model size
class _Cfg(object):
    def __init__(self, **kw):
        self.REGRESS_LOC, self.REGRESS_ORI, self.REGRESS_KEYPOINTS = True, True, False
        self.ORIENTATION_PARAM, self.BETA, self.ORI_BINS_PER_DIM = "quaternion", 6.0, 8
        self.IMAGE_RESIZE_MODE, self.IMAGE_MIN_DIM, self.IMAGE_MAX_DIM, self.IMAGE_MIN_SCALE = "pad64", 128, 192, 0
        self.__dict__.update(kw)


class _Model(object):
    def __init__(self, mode="inference", **kw):
        self.mode, self.config = mode, _Cfg(**kw)


class _Data(object):
    image_ids = [0, 1]

    def __init__(self, width=192, height=128, camera=True):
        from ursonet_amd.dataset import Camera
        if camera:
            self.camera = Camera(width, height)


def test_model_camera():
    from ursonet_amd import utils, views as vw
    ds = _Data(192, 128)
    assert np.array_equal(vw.model_camera(ds, _Cfg()), ds.camera.K)          # frames at model size: K itself
    # 960 x 1280 frames at IMAGE_MIN_DIM 512 / IMAGE_MAX_DIM 640: scaled by 1/2 to 480 x 640, padded to 512 x 640 (16 rows above)
    big, cfg = _Data(1280, 960), _Cfg(IMAGE_MIN_DIM=512, IMAGE_MAX_DIM=640)
    scale, (nh, nw), pads, window = utils.resize_geometry(960, 1280, 512, 640, 0, "pad64")
    assert (scale, nh, nw, pads, window) == (0.5, 480, 640, ((16, 16), (0, 0)), (16, 0, 496, 640))
    K = big.camera.K
    want = np.array([[0.5 * K[0, 0], 0, 0.5 * K[0, 2] - 0.25], [0, 0.5 * K[1, 1], 0.5 * K[1, 2] + 16 - 0.25], [0, 0, 1]])
    got = vw.model_camera(big, cfg)
    assert np.allclose(got, want, rtol=0, atol=1e-12), got - want
    # the centre of raw pixel (u, v) lands on the centre-aligned position of the resize: ((u + 0.5) / 2 - 0.5, (v + 0.5) / 2 - 0.5 + 16)
    A = got @ np.linalg.inv(K)
    assert np.allclose(A @ [101.0, 57.0, 1.0], [(101 + 0.5) / 2 - 0.5, (57 + 0.5) / 2 - 0.5 + 16, 1.0], atol=1e-10)
    for mode in ("crop", "none"):
        with pytest.raises(ValueError, match="IMAGE_RESIZE_MODE"):
            vw.model_camera(big, _Cfg(IMAGE_RESIZE_MODE=mode))
    with pytest.raises(ValueError, match="dataset.camera"):
        vw.model_camera(_Data(camera=False), _Cfg())


def test_view_homographies_are_the_augmentations():
    from ursonet_amd import augment, views as vw
    K = _Data(192, 128).camera.K
    R, _ = vw.view_rotations([[0, 0, 0], [0, 0, 40], [5, -5, -70]])
    M = vw.view_homographies(K, R)
    assert M.shape == (3, 9) and M.dtype == np.float64 and np.allclose(M[0], np.eye(3).ravel(), atol=1e-12)
    for m, r in zip(M, R):
        fwd = K @ r @ np.linalg.inv(K)
        assert np.array_equal(m.reshape(3, 3), augment.invert_homography(augment.rotation_homography(K, r)))
        assert np.allclose(m.reshape(3, 3) @ fwd, np.eye(3), atol=1e-12)


# ------------------------------------------------------------------ refusals of the commands
def test_views_refusals_of_predict_and_evaluate(tmp_path):
    from ursonet_amd import evaluate as ev, predict as pr, submission as sub
    soft = dict(REGRESS_ORI=False)
    for call in (lambda **kw: pr.predict(_Model(**soft), _Data(), **kw), lambda **kw: ev.evaluate(_Model(**soft), _Data(), out_dir=str(tmp_path), **kw)):
        with pytest.raises(ValueError, match="multimodal"):
            call(views=[[0, 0, 0]], multimodal=True)
    calls = (lambda v: pr.predict(_Model(), _Data(), views=v), lambda v: ev.evaluate(_Model(), _Data(), out_dir=str(tmp_path), views=v),
             lambda v: sub.test_and_submit(_Model(), _Data(), _Data(), out_dir=str(tmp_path), views=v))
    for call in calls:
        for bad in ([0, 0, 0], [[0, 0]], np.zeros((2, 3, 3)), np.zeros((0, 3)), np.zeros((65, 3)), [[0, 0, np.nan]]):
            with pytest.raises(ValueError, match="views"):
                call(bad)
        with pytest.raises(ValueError, match="dataset.camera"):
            (pr.predict if call is calls[0] else ev.evaluate)(_Model(), _Data(camera=False), views=[[0, 0, 0]])
    with pytest.raises(ValueError, match="IMAGE_RESIZE_MODE"):
        pr.predict(_Model(IMAGE_RESIZE_MODE="crop"), _Data(), views=[[0, 0, 0]])
    assert not os.listdir(str(tmp_path))                                    # refused before anything was written
