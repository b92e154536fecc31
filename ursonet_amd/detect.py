"""Batched inspection of sampled dataset images on the GPU: the dataset half of the reference's `test` command
(pose_estimator.detect_dataset, pose_estimator.py:462-604).

Per image the reference detects at batch 1, decodes in NumPy (40-318 ms for the soft-classification head), prints seven lines and opens
matplotlib windows: the ground-truth and the estimated object axes on the frame, the projected locations, and -- soft classification --
the predicted orientation PMF beside its encoded target, slice by slice.  detect_dataset() draws the image ids up front and runs them in
whole engine batches exactly as evaluate() does (EvalFeeder -> the pass of ursonet_amd/infer.py -> urso_pose_eval into one fp64 table, read
once at the end), so its table columns are evaluate()'s bits.  With render=True the pictures are made on the device and come
back per batch: `axes_gt`, `axes_est` and `overlap` are copies of the resized frame's window with segments / discs drawn by
urso_draw_prims_u8, `sheet` is urso_pmf_sheet_u8's picture of the stored orientation target above the head's logits.  The few hundred
flops per image of the projections stay on the host in float64.

Differences from matplotlib's figures, on purpose: no anti-aliasing (the rasteriser is exact and integer), arrow heads are two strokes
(cv2.arrowedLine's shape, as video.track draws them) instead of filled triangles, the frames are the network's window-sized resized frames
instead of the originals, the sheet has no axis labels, and the dashed polar dials of utils.polar_plot are returned as numbers (pyr_gt /
pyr_est) and not drawn.  matplotlib is not a dependency.
"""
import random

import numpy as np

from .augment import quat2SO3
from .infer import PosePass, eval_columns, loader_workers
from .video import PRIM_INTS, _int_point, arrow_prims

AXES_LENGTH = 100.0                                             # utils.visualize_axes' scale at its call sites (:572-573), original-frame pixels
AXES_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255))         # ax.arrow(color='r' / 'g' / 'b'), RGB
AXES_THICKNESS = 2.0                                            # original-frame pixels
# (colour, radius in original-frame pixels) in drawing order (:592-601): encoded, truth, estimate -- the last one wins
OVERLAP_DISCS = (((0, 0, 255), 7.0), ((255, 0, 0), 15.0), ((0, 255, 0), 10.0))
SHEET_BG = (255, 255, 255)                                      # between and around the slices: a matplotlib figure's white
PRINT_LABELS = ("GT location: ", "Est location: ", "Processed Image:", "Est orientation: ", "GT_orientation: ", "Location error: ",
                "Angular error: ")


def grey_lut():
    """The default colour table of the sheet: the grey ramp (i, i, i), uint8 [256,3]."""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def quat_inv(q):
    """se3lib.quat_inv: [-x, -y, -z, w]."""
    q = np.asarray(q, dtype=np.float64).ravel()
    return np.array([-q[0], -q[1], -q[2], q[3]])


def quat2euler(q):
    """se3lib.quat2euler (se3lib.py:185-211): (pitch, yaw, roll) in degrees of a left-handed quaternion [x, y, z, w], with the two pole
    branches at +-0.499 and the pitch folded back into [-180, 180] -- the angles utils.polar_plot draws."""
    x, y, z, w = (float(v) for v in np.asarray(q, dtype=np.float64).ravel())
    test = x * z + y * w
    if test > 0.499:
        pitch, yaw, roll = 2 * np.arctan2(x, w), -np.pi / 2, 0.0
    elif test < -0.499:
        pitch, yaw, roll = -2 * np.arctan2(x, w), np.pi / 2, 0.0
    else:
        pitch = np.arctan2(2 * (y * z - x * w), 1 - 2 * x * x - 2 * y * y)
        yaw = np.arcsin(-2 * (x * z + y * w))
        roll = np.arctan2(2 * (x * y - z * w), 1 - 2 * y * y - 2 * z * z)
    if pitch > np.pi:
        pitch = 2 * np.pi - pitch
    if pitch < -np.pi:
        pitch = 2 * np.pi + pitch
    return np.array([pitch * 180 / np.pi, yaw * 180 / np.pi, roll * 180 / np.pi])


def frame_matrix(camera, width, height):
    """pose_estimator.py:561-564: [[fx, 0, W0 / 2], [0, fy, H0 / 2], [0, 0, 1]] from dataset.camera and the ORIGINAL frame's size."""
    return np.array([[camera.fx, 0.0, width / 2], [0.0, camera.fy, height / 2], [0.0, 0.0, 1.0]], dtype=np.float64)


def axes_arrows(q, loc, K, length=AXES_LENGTH):
    """utils.visualize_axes (utils.py:154-184) in float64 -> (c [2], v [2,3]): the arrows ax.arrow draws go from c to c + v[:, i].
    The axes diag(1, -1, 1) are rotated by quat2SO3(q), translated by loc, divided by their depth and multiplied by K; v = length *
    (p - c) / ||p - c||_F, the Frobenius norm of the whole 3 x 3 difference, as the reference has it."""
    loc = np.asarray(loc, dtype=np.float64).ravel()
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        P_t = quat2SO3(np.asarray(q, dtype=np.float64).ravel()) @ np.diag([1.0, -1.0, 1.0]) + loc[:, None]
        p = K @ (P_t / P_t[-1, :])
        c = K @ (loc / loc[-1])
        v = p - c[:, None]
        v = length * v / np.linalg.norm(v)
    return c[:2].copy(), v[:2].copy()


def project(loc, K):
    """The circle centres of :582-601: (x / z * fx + W0 / 2, y / z * fy + H0 / 2)."""
    loc = np.asarray(loc, dtype=np.float64).ravel()
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        return np.array([loc[0] / loc[2] * K[0, 0] + K[0, 2], K[1, 2] + loc[1] / loc[2] * K[1, 1]])


def _length(v, scale):
    """A radius or thickness in window pixels: scaled, rounded to nearest even, at least 1."""
    return max(1, int(np.rint(float(v) * scale)))


def detect_prims(picture, K, scale, q=None, loc=None, loc_gt=None, loc_encoded=None, speed=False):
    """The pictures of detect_dataset as primitives of urso_draw_prims_u8: int32 [n, 9] rows [kind, x0, y0, x1, y1, r, cR, cG, cB].
    K: frame_matrix of the original frame; scale: the resize scale (utils.resize_geometry) that takes original-frame pixels to the
    window's.  Everything is computed in float64 in original-frame pixels, multiplied by `scale` and rounded to nearest even; radii and
    thickness are at least 1.
      picture "axes" (q, loc): utils.visualize_axes' three arrows (axes_arrows) from c to c + v_i, 100 original pixels long in all, in
        red, green, blue, thickness 2 original pixels; q is inverted first when speed is true (dataset.name == 'Speed', :568-570).  Each
        arrow is a shaft and two head strokes (video.arrow_prims): nine rows.
      picture "overlap" (loc = the estimate, loc_gt, loc_encoded or None): discs at project(.) -- blue, radius 7: the decoded encoded
        target (location classification only); red, radius 15: the truth; green, radius 10: the estimate; in that order, the last wins.
    A row with a coordinate that is not finite or lies beyond +-16,384 is dropped (an arrow whose centre or tip is: all three rows)."""
    rows = []
    if picture == "axes":
        c, v = axes_arrows(quat_inv(q) if speed else q, loc, K)
        centre = _int_point(c[0] * scale, c[1] * scale, True)
        for i in range(3):
            with np.errstate(all="ignore"):
                tip = _int_point((c[0] + v[0, i]) * scale, (c[1] + v[1, i]) * scale, True)
            if centre is not None and tip is not None:
                rows += arrow_prims(centre, tip, AXES_COLOURS[i], _length(AXES_THICKNESS, scale))
    elif picture == "overlap":
        for where, (colour, radius) in zip((loc_encoded, loc_gt, loc), OVERLAP_DISCS):
            if where is None:
                continue
            p = project(where, K)
            at = _int_point(p[0] * scale, p[1] * scale, True)
            if at is not None:
                rows.append((1, at[0], at[1], 0, 0, _length(radius, scale)) + colour)
    else:
        raise ValueError("detect_prims: picture %r (axes / overlap)" % (picture,))
    return np.asarray(rows, dtype=np.int32).reshape(-1, PRIM_INTS)


class DetectResult(object):
    """Per-image NumPy arrays in the order the images ran: image_ids, loc_gt [N,3], q_gt [N,4], loc_est [N,3], q_est [N,4] ([x, y, z, w]),
    loc_err, ori_err (degrees), loc_encoded_err (None when the location is regressed), pyr_gt / pyr_est [N,3] (se3lib.quat2euler degrees
    of the quaternions utils.polar_plot is handed: inverted for dataset.name == 'Speed'), ori_logits fp32 [N,K] (soft classification,
    else None).  pictures: with render=True and no sink, a list of N dicts name -> uint8 array [h,w,3] (axes_gt, axes_est, overlap and,
    soft classification, sheet); else None."""

    def __init__(self, image_ids, table, loc_gt, q_gt, loc_enc, speed, ori_logits=None, pictures=None):
        eval_columns(self, table, loc_enc)
        self.image_ids = np.asarray(image_ids)
        self.loc_gt, self.q_gt = loc_gt, q_gt
        flip = quat_inv if speed else (lambda q: q)
        self.pyr_gt = np.array([quat2euler(flip(q)) for q in self.q_gt], dtype=np.float64).reshape(-1, 3)
        self.pyr_est = np.array([quat2euler(flip(q)) for q in self.q_est], dtype=np.float64).reshape(-1, 3)
        self.ori_logits = ori_logits
        self.pictures = pictures


def print_lines(res, dataset, i):
    """The reference's seven per-image prints (:533-540) for image i of a DetectResult: the same labels in the same order."""
    info = dataset.image_info[res.image_ids[i]]
    values = (res.loc_gt[i], res.loc_est[i], info["path"], res.q_est[i], res.q_gt[i], res.loc_err[i], res.ori_err[i])
    return ["%s %s" % (label, v) for label, v in zip(PRINT_LABELS, values)]


class _Drawn(object):
    """The dataset as EvalFeeder sees it: image_ids is the drawn list (repeats included), everything else is the dataset's.  Remembers
    the size of every frame it loads: the pictures need the original frame's."""

    def __init__(self, dataset, ids):
        self._ds, self.image_ids, self.shapes = dataset, list(ids), {}

    def load_image(self, image_id):
        image = self._ds.load_image(image_id)
        self.shapes[image_id] = tuple(np.shape(image))
        return image

    def __getattr__(self, name):
        return getattr(self._ds, name)


def detect_dataset(model, dataset, nr_images, image_ids=None, render=True, cell=4, gap=2, lut=None, sink=None, verbose=1, workers=None):
    """pose_estimator.detect_dataset(model, dataset, nr_images) -> DetectResult.  With image_ids None the ids are drawn up front by
    nr_images calls of random.choice(dataset.image_ids) -- the reference's draws, repeats possible; else the given ids are used (and
    nr_images is ignored).  They run as engine batches in that order, the tail batch padded, through evaluate()'s pipeline: the table
    columns are the bits evaluate() gives for the same ids.  verbose: print the reference's seven lines per image (after the run).
    render=True makes three pictures per image on the device -- axes_gt, axes_est, overlap (detect_prims on copies of the resized frame's
    window) -- and, for the soft-classification head, sheet (urso_pmf_sheet_u8: the stored orientation target above the logits, `cell`
    pixels per bin edge, `gap` pixels between slices, colours from `lut`, a uint8 [256,3] table, default grey_lut(); the background is
    SHEET_BG).  A picture goes to sink(index, name, array) or, without a sink, into DetectResult.pictures.  The pictures are downloaded per
    batch.  render=False launches no picture kernel and returns the same table.  Frames that are not uint8 RGB raise ValueError when
    render is true (they reach the engine molded to float; there is nothing to draw on)."""
    ps = PosePass(model, dataset, who="detect_dataset")
    import torch
    from . import augment, hip, utils
    from .feeder import EvalFeeder
    cfg, B, dev, soft, loc_enc = ps.cfg, ps.B, ps.dev, ps.soft, ps.loc_class
    if image_ids is None:
        pool = dataset.image_ids
        ids = [random.choice(pool) for _ in range(int(nr_images))]
    else:
        ids = list(image_ids)
    N = len(ids)
    speed = getattr(dataset, "name", None) == "Speed"
    if render and cfg.IMAGE_RESIZE_MODE not in ("square", "pad64"):
        raise ValueError("detect_dataset(render=True): IMAGE_RESIZE_MODE %r has no window to draw on (square / pad64 have)" % (cfg.IMAGE_RESIZE_MODE,))
    table = ps.table(max(N, 1), hip.EVAL_COLS)
    loc_map_h = np.asarray(dataset.histogram_3D_map, dtype=np.float64) if loc_enc else None
    lut_d = scratch = sheets = None
    nbins = int(cfg.ORI_BINS_PER_DIM)
    if render and soft:
        lut_h = grey_lut() if lut is None else np.ascontiguousarray(lut)
        if lut_h.dtype != np.uint8 or lut_h.shape != (256, 3):
            raise ValueError("detect_dataset: lut is a uint8 [256,3] table, not %s %s" % (lut_h.dtype, lut_h.shape))
        lut_d = torch.as_tensor(lut_h).to(dev)
        sh, sw = hip.pmf_sheet_shape(nbins, cell, gap, 2)
        sheets = torch.empty((B, sh, sw, 3), dtype=torch.uint8, device=dev)
        scratch = torch.empty(B * 2 * nbins ** 3, dtype=torch.uint8, device=dev)        # the 8-bit indices between the two launches
    view = _Drawn(dataset, ids)
    logits, pictures = [], ([None] * N if render and sink is None else None)
    feed = EvalFeeder(model, view, cfg, enc_loc=loc_enc, enc_ori=soft, workers=loader_workers(cfg, workers))
    try:
        for bt in feed:
            if render and bt.images.dtype != torch.uint8:
                raise ValueError("detect_dataset(render=True) draws on uint8 RGB frames; this dataset's frames reach the engine as %s "
                                 "(molded on the host).  Call it with render=False." % (bt.images.dtype,))
            ps.run(bt.images)
            heads = ps.heads(bt.n)
            n, z = bt.n, heads[3]
            if soft:
                logits.append(z.clone())                       # z may be a view of the engine's output buffer
            ps.eval_into(table, bt, heads)
            if not render:
                continue
            rows = table[bt.row0:bt.row0 + n].cpu().numpy()    # this batch's poses: the one read per batch
            enc_h = bt.enc_loc[:n].cpu().numpy().astype(np.float64) if loc_enc else None
            out = {}
            if soft:
                augment.pmf_sheet(bt.enc_ori[:n], z, nbins, cell=cell, gap=gap, lut=lut_d, bg=SHEET_BG, out=sheets[:n], scratch=scratch)
                out["sheet"] = sheets[:n].cpu().numpy()
            groups = {}                                        # frames of one size share a window and go through one launch
            for j in range(n):
                groups.setdefault(view.shapes[ids[bt.row0 + j]], []).append(j)
            shots = {}
            for shape, members in groups.items():
                if len(shape) != 3 or shape[2] != 3:
                    raise ValueError("detect_dataset(render=True): a uint8 RGB frame [H,W,3] expected, not %s" % (shape,))
                H0, W0 = shape[:2]
                scale, _size, _pads, (y0, x0, y1, x1) = utils.resize_geometry(H0, W0, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.IMAGE_MIN_SCALE,
                                                                             cfg.IMAGE_RESIZE_MODE)
                K = frame_matrix(dataset.camera, W0, H0)
                win = bt.images[members, y0:y1, x0:x1]          # a copy: the model's input stays as it is
                win = win.unsqueeze(1).expand(-1, 3, -1, -1, -1).reshape(3 * len(members), y1 - y0, x1 - x0, 3).contiguous()
                prims = []
                for j in members:
                    i = bt.row0 + j
                    l_est, q_est = rows[j, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3], rows[j, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4]
                    l_gt, q_gt = np.asarray(dataset.load_location(ids[i]), dtype=np.float64), np.asarray(dataset.load_quaternion(ids[i]), dtype=np.float64)
                    l_enc = enc_h[j] @ loc_map_h if loc_enc else None               # the stored encoding's first moment (:496)
                    prims += [detect_prims("axes", K, scale, q=q_gt, loc=l_gt, speed=speed),
                              detect_prims("axes", K, scale, q=q_est, loc=l_est, speed=speed),
                              detect_prims("overlap", K, scale, loc=l_est, loc_gt=l_gt, loc_encoded=l_enc)]
                augment.draw_prims(win, prims)
                host = win.cpu().numpy()
                for m, j in enumerate(members):
                    shots[j] = {"axes_gt": host[3 * m], "axes_est": host[3 * m + 1], "overlap": host[3 * m + 2]}
            for j in range(n):
                if "sheet" in out:
                    shots[j]["sheet"] = out["sheet"][j]
                if sink is not None:
                    for name, a in shots[j].items():
                        sink(bt.row0 + j, name, a)
                else:
                    pictures[bt.row0 + j] = {name: a.copy() for name, a in shots[j].items()}
    finally:
        feed.close()
    host = table[:N].cpu().numpy()                              # the one read of the table
    loc_gt = np.array([np.asarray(dataset.load_location(i), dtype=np.float64) for i in ids], dtype=np.float64).reshape(-1, 3)
    q_gt = np.array([np.asarray(dataset.load_quaternion(i), dtype=np.float64) for i in ids], dtype=np.float64).reshape(-1, 4)
    ori_logits = None
    if soft:
        ori_logits = torch.cat(logits).cpu().numpy() if logits else np.zeros((0, nbins ** 3), dtype=np.float32)
    res = DetectResult(ids, host, loc_gt, q_gt, loc_enc, speed, ori_logits, pictures)
    if verbose:
        for i in range(N):
            for line in print_lines(res, dataset, i):
                print(line)
    return res
