"""Test-time view fusion, host side: which rotated views of a test image the network is shown and how they are rendered.

The network is trained under ROT_AUG / ROT_IMAGE_AUG (ursonet_amd/augment.py: the frame re-rendered through a rotated camera, the
label rotated with it).  predict(views=...) / evaluate(views=...) show it V such views of every test image with the same warp kernel,
rotate each view's estimate back and fuse the V estimates on the device (urso_pose_fuse_views, include/ursonet_ext.h; the pass is
ursonet_amd/infer.py's PosePass.fuse_batch).  Here is the 3x3 / quaternion algebra of the views, in float64 NumPy: the rotations, the
camera at model-input pixel coordinates and the homographies the warp kernel takes.  DESIGN.md section 15 has the geometry.
"""
import numpy as np

from . import augment, utils

MAX_VIEWS = 64                     # URSO_FUSE_MAX_VIEWS (include/ursonet_ext.h)


def ROLL_VIEWS(k, max_deg):
    """k views rolled about the optical axis by angles evenly spaced in [-max_deg, max_deg] (k odd: the unrotated view is one of
    them; k = 1: it alone) -> [k,3] (pitch, yaw, roll) in degrees."""
    k = int(k)
    if k < 1:
        raise ValueError("ROLL_VIEWS needs k >= 1 (got %d)" % k)
    rolls = np.zeros(1) if k == 1 else np.linspace(-float(max_deg), float(max_deg), k)
    if k % 2:
        rolls[k // 2] = 0.0
    return np.stack([np.zeros(k), np.zeros(k), rolls], axis=1)


def view_rotations(views):
    """views [V,3] (pitch, yaw, roll) in degrees -> (R [V,3,3], qR [V,4]): euler2SO3_left and its SO32quat, what rotate_cam applies
    to the camera and to the label.  ValueError: not [V,3], V outside 1..64, a non-finite angle."""
    try:
        v = np.asarray(views, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("views must be an array [V,3] of (pitch, yaw, roll) in degrees")
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("views must have shape [V,3] (pitch, yaw, roll), got %s" % (v.shape,))
    if not 1 <= v.shape[0] <= MAX_VIEWS:
        raise ValueError("views: 1 <= V <= %d views are supported (got %d)" % (MAX_VIEWS, v.shape[0]))
    if not np.all(np.isfinite(v)):
        raise ValueError("views: every angle must be finite")
    R = np.stack([augment.euler2SO3_left(*p) for p in v])
    return R, np.stack([augment.SO32quat(r) for r in R])


def model_camera(dataset, config):
    """The 3x3 camera matrix at model-input pixel coordinates: dataset.camera.K carried through the resize and padding every frame
    goes through (utils.resize_image; centre-aligned pixels, as the bilinear resize samples them).  dataset.camera describes every
    frame, as the reference's augmentation assumes.  ValueError: no dataset.camera, IMAGE_RESIZE_MODE 'crop' (a random window) or
    'none' (no common model size)."""
    cam = getattr(dataset, "camera", None)
    if cam is None:
        raise ValueError("views need dataset.camera (the intrinsics K, width and height of every frame)")
    mode = config.IMAGE_RESIZE_MODE
    if mode in ("crop", "none"):
        raise ValueError("views are not defined for IMAGE_RESIZE_MODE = %r" % (mode,))
    _scale, (nh, nw), _pads, window = utils.resize_geometry(cam.height, cam.width, config.IMAGE_MIN_DIM, config.IMAGE_MAX_DIM,
                                                            config.IMAGE_MIN_SCALE, mode)
    sx, sy = nw / cam.width, nh / cam.height
    A = np.array([[sx, 0.0, window[1] + (sx - 1) / 2], [0.0, sy, window[0] + (sy - 1) / 2], [0.0, 0.0, 1.0]])
    return A @ np.asarray(cam.K, dtype=np.float64)


def view_homographies(K_model, R):
    """[V,9] float64 destination -> source matrices for urso_warp_perspective: the forward homography K_model R_v K_model^-1 of
    rotate_cam (augment.rotation_homography), inverted as augment.warp_images inverts it."""
    return np.stack([augment.invert_homography(augment.rotation_homography(K_model, r)).reshape(9) for r in np.asarray(R, dtype=np.float64)])


def is_identity(r):
    """Whether a view rotation is exactly the identity: such a view is run without a warp and fused without arithmetic."""
    return bool(np.array_equal(np.asarray(r, dtype=np.float64).reshape(3, 3), np.eye(3)))


class ViewSet(object):
    """The host half of one call's views: views [V,3], R [V,3,3], qR [V,4], M [V,9] (None before a camera is known)."""

    def __init__(self, views, multimodal=False, who="predict"):
        if multimodal:
            raise ValueError("%s(views=...) fuses one estimate per view; it cannot be combined with multimodal=True" % who)
        self.R, self.qR = view_rotations(views)
        self.views, self.V, self.M = np.asarray(views, dtype=np.float64), len(self.R), None

    def with_camera(self, dataset, config):
        self.M = view_homographies(model_camera(dataset, config), self.R)
        return self
