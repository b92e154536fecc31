"""Batched video tracking on the GPU: the heavy half of the reference's `test` command (pose_estimator.detect_video,
pose_estimator.py:606-745).

Per frame the reference crops, zero-pads by 400 pixels (a 960 x 1280 frame becomes 1760 x 1929 x 3), mixes to grey in float64, resizes,
runs the network at batch 1, decodes, converts the pose to Unreal Euler angles and draws the object axes with OpenCV -- all on the host.
track() runs the same chain for whole engine batches on one stream: pinned upload of the RAW frames -> urso_video_prep_u8 (crop + pad +
grey, the bytes of VideoPrep.host) -> augment.resize_images (the bytes of utils.resize_image) -> the pass of ursonet_amd/infer.py as
predict() runs it (urso_pose_decode into a fp64 device table, read once at the end); with render=True the axes are drawn onto the resized frames where
they lie (urso_draw_prims_u8) and only the annotated windows come back.  The few hundred flops per frame of the Euler conversion and of
the axis projection stay on the host in float64.

Decoding a video container is the caller's job (OpenCV is no dependency): `frames` is any iterable of uint8 RGB arrays of one size.
"""
import math

import numpy as np

from .augment import quat2SO3
from .infer import PosePass, dec_columns, loader_workers

COORD_MAX = 16384                                                                 # URSO_DRAW_COORD_MAX
MAX_PRIMS, PRIM_INTS = 16, 9
R_CAM_UNREAL = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])     # pose_estimator.py:625
AXIS_COLOURS = ((0, 0, 255), (0, 255, 0), (255, 0, 0))                            # utils.py:215-217, in the frame's channel order


class VideoPrep(object):
    """pose_estimator.py:641-645: crop (top, bottom, left, right) pixels away, zero-pad by `pad` on all four sides, grey mix with the
    weights `grey` written to all three channels.  The defaults are the reference's: image[:, 1:-150, :], 400, (0.21, 0.72, 0.07)."""

    def __init__(self, crop=(0, 0, 1, 150), pad=400, grey=(0.21, 0.72, 0.07)):
        self.crop = tuple(int(v) for v in crop)
        self.pad = int(pad)
        self.grey = tuple(float(v) for v in grey)
        if len(self.crop) != 4 or min(self.crop) < 0 or self.pad < 0 or len(self.grey) != 3:
            raise ValueError("VideoPrep: crop is four non-negative ints (top, bottom, left, right), pad a non-negative int, grey three "
                             "weights; got %r, %r, %r" % (crop, pad, grey))

    def out_shape(self, h, w):
        """(height, width) of the prepared frame of an h x w input."""
        t, b, l, r = self.crop
        ch, cw = int(h) - t - b, int(w) - l - r
        if ch <= 0 or cw <= 0:
            raise ValueError("VideoPrep: crop %r leaves no pixel of a %d x %d frame" % (self.crop, h, w))
        return ch + 2 * self.pad, cw + 2 * self.pad

    def host(self, frame):
        """The reference's statements, literally, on one uint8 RGB frame [H,W,3] -> uint8 [OH,OW,3].  The float64 mix is ASSIGNED
        into the uint8 image (truncation; white -> 254 with the default weights).  This is the reference for urso_video_prep_u8."""
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("VideoPrep.host: a uint8 [H,W,3] frame expected, not %s %s" % (frame.dtype, frame.shape))
        h, w = frame.shape[:2]
        self.out_shape(h, w)
        t, b, l, r = self.crop
        p, (g0, g1, g2) = self.pad, self.grey
        image = frame[t:h - b, l:w - r, :]
        image = np.pad(image, [(p, p), (p, p), (0, 0)], mode="constant", constant_values=0)
        with np.errstate(invalid="ignore"):
            image[:, :, 0] = g0 * image[:, :, 0] + g1 * image[:, :, 1] + g2 * image[:, :, 2]
        image[:, :, 1] = image[:, :, 0]
        image[:, :, 2] = image[:, :, 0]
        return image


def euler2SO3_unreal(pitch, yaw, roll):
    """se3lib.py:8-21 (degrees, Unreal Engine order) -> 3x3 ndarray."""
    p, y, r = (float(a) * np.pi / 180 for a in (pitch, yaw, roll))
    cp, sp, cy, sy, cr, sr = np.cos(p), np.sin(p), np.cos(y), np.sin(y), np.cos(r), np.sin(r)
    R = np.array([[cp * cy, cp * sy, sp],
                  [sr * sp * cy - cr * sy, sr * sp * sy + cr * cy, -sr * cp],
                  [-(cr * sp * cy + sr * sy), cy * sr - cr * sp * sy, cr * cp]])
    return R.T


def SO32euler(R):
    """se3lib.py:117-133: (pitch, yaw, roll) in degrees, with both gimbal-lock branches at +-0.998."""
    if R[2, 0] > 0.998:
        yaw, roll, pitch = -np.pi / 2, 0.0, np.arctan2(R[0, 1], R[0, 2])
    elif R[2, 0] < -0.998:
        yaw, roll, pitch = np.pi / 2, 0.0, np.arctan2(R[0, 1], R[0, 2])
    else:
        yaw, pitch, roll = np.arcsin(-R[2, 0]), np.arctan2(R[2, 1], R[2, 2]), np.arctan2(R[1, 0], R[0, 0])
    return pitch * 180 / np.pi, yaw * 180 / np.pi, roll * 180 / np.pi


def pose_unreal(loc, q):
    """pose_estimator.py:669-678, float64 on the host: the row [z, x, y, -pitch, yaw, -roll] the reference stacks per frame, where
    `roll, pitch, yaw = se3lib.SO32euler(R_wo)` -- the reference unpacks SO32euler's (pitch, yaw, roll) under those names, and so does
    this function -- R_wo = euler2SO3_unreal(0, 0, 0) . (R_cam_unreal^T . quat2SO3(q))."""
    loc = np.asarray(loc, dtype=np.float64).ravel()
    R_co = quat2SO3(np.asarray(q, dtype=np.float64).ravel())
    R_co = R_CAM_UNREAL.T @ R_co
    R_wo = euler2SO3_unreal(0, 0, 0) @ R_co
    roll, pitch, yaw = SO32euler(R_wo)
    return np.array([loc[2], loc[0], loc[1], -pitch, yaw, -roll], dtype=np.float64)


def _int_point(x, y, rounded):
    """(x, y) as ints -- truncated toward zero as ndarray.astype(int) does, or rounded to nearest even as cvRound does -- or None when a
    coordinate is not finite or lies beyond +-COORD_MAX."""
    if not (math.isfinite(x) and math.isfinite(y)) or abs(x) > COORD_MAX + 1 or abs(y) > COORD_MAX + 1:
        return None
    xi, yi = (int(np.rint(x)), int(np.rint(y))) if rounded else (int(x), int(y))
    if abs(xi) > COORD_MAX or abs(yi) > COORD_MAX:
        return None
    return xi, yi


def arrow_prims(centre, tip, colour, thickness=2):
    """One arrow centre -> tip (integer pixel pairs) as segment rows of urso_draw_prims_u8: the shaft and two head strokes by
    cv2.arrowedLine's rule with tipLength 0.1: tip + 0.1 |tip - c| (cos(a +- pi/4), sin(a +- pi/4)), a = atan2(c.y - tip.y, c.x - tip.x),
    rounded to nearest, + before -.  A stroke whose end is not finite or lies beyond +-16,384 is dropped."""
    colour = tuple(int(v) for v in colour)
    rows = [(0, centre[0], centre[1], tip[0], tip[1], int(thickness)) + colour]
    size = math.hypot(centre[0] - tip[0], centre[1] - tip[1]) * 0.1
    angle = math.atan2(centre[1] - tip[1], centre[0] - tip[0])
    for sign in (1.0, -1.0):
        e = _int_point(tip[0] + size * math.cos(angle + sign * math.pi / 4), tip[1] + size * math.sin(angle + sign * math.pi / 4), True)
        if e is not None:
            rows.append((0, e[0], e[1], tip[0], tip[1], int(thickness)) + colour)
    return rows


def pose_axes_prims(q, loc, K, scale=5.0):
    """utils.plot_axes (utils.py:186-217) as primitives of urso_draw_prims_u8: int32 [n, 9] rows [kind 0, x0, y0, x1, y1, 2, cR, cG, cB].
    The axes diag(1, -1, 1) * scale are rotated by quat2SO3(q), translated by loc, divided by their depth and multiplied by K; centre and
    tips are truncated toward zero.  Three arrows centre -> tip in the colours (0, 0, 255), (0, 255, 0), (255, 0, 0), thickness 2, each a
    shaft and two head strokes (arrow_prims).  Nine rows; a primitive with a coordinate that is not finite or lies beyond +-16,384 (an
    object at or behind the image plane) is dropped."""
    loc = np.asarray(loc, dtype=np.float64).ravel()
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    rows = []
    with np.errstate(all="ignore"):
        P = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0]]) * scale
        P_t = quat2SO3(np.asarray(q, dtype=np.float64).ravel()) @ P + loc[:, None]
        p = K @ (P_t / P_t[-1, :])
        c = K @ (loc / loc[-1])
    centre = _int_point(c[0], c[1], False)
    for i in range(3):
        tip = _int_point(p[0, i], p[1, i], False)
        if centre is None or tip is None:
            continue
        rows += arrow_prims(centre, tip, AXIS_COLOURS[i])
    return np.asarray(rows, dtype=np.int32).reshape(-1, PRIM_INTS)


def camera_matrix(camera, width, height):
    """pose_estimator.py:618-623 with the annotated window's width and height in place of camera.width / 2 and camera.height / 2 (the
    reference's half-size output video); fy is negative, as there."""
    fx = width / (2 * np.tan(camera.fov_x / 2))
    fy = -height / (2 * np.tan(camera.fov_y / 2))
    return np.array([[fx, 0, width / 2], [0, fy, height / 2], [0, 0, 1]], dtype=np.float64)


class TrackResult(object):
    """Per-frame NumPy arrays in the order the frames came: loc_est [N,3], q_est [N,4] ([x, y, z, w]), pose_unreal [N,6] (rows
    [z, x, y, -pitch, yaw, -roll]) and predict()'s confidence columns loc_peak, ori_peak, ori_lambda (None where the head does not
    define them).  frames: the annotated windows (uint8 [h,w,3] each) of a render=True run without a sink, else None."""

    def __init__(self, table, loc_class, soft, frames=None):
        dec_columns(self, table, loc_class, soft)
        self.pose_unreal = np.array([pose_unreal(l, q) for l, q in zip(self.loc_est, self.q_est)], dtype=np.float64).reshape(-1, 6)
        self.frames = frames


def _batches(frames, B):
    """[(index of the first frame, n valid frames, list of B frames)]: the tail batch repeats its last frame (feeder.eval_batch_plan)."""
    chunk, i0, shape = [], 0, None
    for f in frames:
        f = np.asarray(f)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("track: uint8 RGB frames [H,W,3] expected, not %s %s" % (f.dtype, f.shape))
        if shape is None:
            shape = f.shape
        elif f.shape != shape:
            raise ValueError("track: frames of one size expected, got %s after %s" % (f.shape, shape))
        chunk.append(f)
        if len(chunk) == B:
            yield i0, B, chunk
            i0, chunk = i0 + B, []
    if chunk:
        yield i0, len(chunk), chunk + [chunk[-1]] * (B - len(chunk))


def track(model, frames, dataset, prep=None, render=False, K=None, sink=None, workers=None):
    """Pose of every frame of a video -> TrackResult.  frames: an iterable of uint8 RGB arrays of one size (decoding, and BGR -> RGB, are
    the caller's); dataset: the camera (render) and, for the classification heads, histogram_3D_map / ori_histogram_map; prep: a VideoPrep
    (default: the reference's crop, pad and weights).  The inference-mode model runs at its engine batch, the tail batch padded with its
    last frame; all five heads are handled as predict() handles them, with its bits.  The frames are resized on the device whatever
    Config.DEVICE_RESIZE says (modes square / pad64).
    render=True draws each frame's axes (pose_axes_prims with K; default: camera_matrix(dataset.camera, window width, window height))
    onto its resized frame on the device and hands the annotated window (utils.resize_geometry's window) to sink(index, uint8 array);
    without a sink the windows are collected in TrackResult.frames.  workers: threads that copy the raw frames into pinned memory."""
    ps = PosePass(model, dataset, scatter=True, who="track")
    import torch
    from . import augment, hip, utils
    cfg, eng, B, dev = ps.cfg, ps.eng, ps.B, ps.dev
    if cfg.IMAGE_RESIZE_MODE not in ("square", "pad64"):
        raise ValueError("track: IMAGE_RESIZE_MODE %r is not resized on the device (square / pad64 are)" % (cfg.IMAGE_RESIZE_MODE,))
    prep = prep if prep is not None else VideoPrep()
    workers = loader_workers(cfg, workers)
    pool = None
    if workers > 1 and B > 1:
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=min(int(workers), B))
    pinned, uploaded = [None, None], [None, None]              # two pinned batches, alternating: one is refilled while the other's batch computes
    prepared = resized = window = None
    tables, collected, N = [], ([] if render and sink is None else None), 0
    try:
        with torch.cuda.device(dev):
            for k, (i0, n, chunk) in enumerate(_batches(frames, B)):
                H, W = chunk[0].shape[:2]
                if k == 0:                                     # before anything is launched: the prepared, resized frame must be the engine's input
                    ph, pw = prep.out_shape(H, W)
                    _s, (nh, nw), pads, _w = utils.resize_geometry(ph, pw, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.IMAGE_MIN_SCALE, cfg.IMAGE_RESIZE_MODE)
                    got = (nh + sum(pads[0]), nw + sum(pads[1]))
                    if got != (eng.H, eng.W):
                        raise ValueError("track: %d x %d frames are prepared to %d x %d and resized (%s) to %d x %d, but the model takes %d x %d"
                                         % (H, W, ph, pw, cfg.IMAGE_RESIZE_MODE, got[0], got[1], eng.H, eng.W))
                slot = k & 1
                if pinned[slot] is None:
                    with hip.capture_lock:
                        pinned[slot] = torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory()
                elif uploaded[slot] is not None:
                    uploaded[slot].synchronize()               # the upload that last read this buffer has run
                host = pinned[slot].numpy()
                if pool is not None:
                    list(pool.map(lambda bf: np.copyto(host[bf[0]], bf[1]), enumerate(chunk)))
                else:
                    for b, f in enumerate(chunk):
                        host[b] = f
                raw = pinned[slot].to(dev, non_blocking=True)
                uploaded[slot] = torch.cuda.Event()
                uploaded[slot].record()
                prepared = augment.video_prep(raw, prep, out=prepared)
                resized, window, _scale, _padding = augment.resize_images(prepared, min_dim=cfg.IMAGE_MIN_DIM, max_dim=cfg.IMAGE_MAX_DIM,
                                                                          min_scale=cfg.IMAGE_MIN_SCALE, mode=cfg.IMAGE_RESIZE_MODE, out=resized)
                ps.run(resized)
                heads = ps.heads(n)
                table = ps.table(B, hip.DEC_COLS)              # a table per batch: the frame count is not known up front
                ps.decode_into(table, n, 0, heads)
                tables.append(table[:n])
                N += n
                if render:
                    y0, x0, y1, x1 = window
                    rows = table[:n].cpu().numpy()             # this batch's poses: the one read per batch
                    Kb = camera_matrix(dataset.camera, x1 - x0, y1 - y0) if K is None else K
                    prims = [pose_axes_prims(r[hip.DEC_Q_EST:hip.DEC_Q_EST + 4], r[hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3], Kb) for r in rows]
                    win = resized[:n, y0:y1, x0:x1].contiguous()                  # the annotated windows: drawn on and downloaded, the model's input stays as it is
                    augment.draw_prims(win, prims)
                    out = win.cpu().numpy()
                    for j in range(n):
                        if sink is not None:
                            sink(i0 + j, out[j])
                        else:
                            collected.append(out[j].copy())
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    host = torch.cat(tables).cpu().numpy() if tables else np.zeros((0, hip.DEC_COLS))      # the one read of the table
    return TrackResult(host[:N], ps.loc_class, ps.soft, collected)
