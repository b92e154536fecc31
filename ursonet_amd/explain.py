"""Occlusion-sensitivity maps of the pose heads, batched on the GPU: what in the frame an estimate rests on.

The commands around predict() say how far to trust an estimate (members, calibrate, conformal, fit_domain, recalibrate_bn); none says
which pixels it was read from.  Occlusion sensitivity (Zeiler & Fergus, 2014) answers that without a backward pass and without a label,
for every head the project has: paint a patch of the frame with the value the network sees as nothing, run the network again, and record
how far the answer moved.  One frame becomes tens to hundreds of occluded copies, which go through the inference graph as whole engine
batches.

explain() takes each frame as a row of an EvalFeeder(labels=False) batch (only load_image is called) and, per chunk of B rows of
[the frame as it is] + [one row per patch], on the current stream: urso_occl_fill_u8 makes the chunk in a scratch batch on the device,
the pass of ursonet_amd/infer.py runs and decodes it into a DEC table (PosePass.run / heads / decode_into: a calibration applies there),
and urso_occl_score compares every row with the baseline -- row 0 of chunk 0 -- in fp64: the angle between the two decoded
orientations, the distance between the two decoded locations and, per classification head, the KL divergence, the total variation and the
drop of the baseline's peak bin between the two PMFs.  Behind the last chunk urso_occl_splat turns the per-patch scores into per-pixel
maps of the frame's resize window (a pixel's value is the mean score of the patches that cover it), and the score table and the maps
come back in one read per image.  With render, urso_heat_overlay_u8 blends one map through a colour table onto a copy of the window; its
range is the map's finite minimum and maximum, which the kernel takes by value, so the picture is a second, small read behind the maps'.

occlude_host, score64, splat64 and overlay_host are the same rules in NumPy and the written specification of the four kernels
(include/ursonet_explain.h): the fill, the splat and the overlay are equal byte for byte / bit for bit; the scores agree within the
operation-counted bounds of tests/occlref.py (exp and log are not correctly rounded on either side).

What the maps are, and are not.  The picture is patch-scale and first-order: one patch is removed at a time, so evidence that is present
twice (two solar panels, either of which fixes the roll) is under-reported -- the network still answers from the other -- and nothing
finer than the patch is resolved.  Painting with the neutral value is itself off-distribution: a grey square on a black sky is an
object the network never saw, and a large score can mean "this square disturbed the network" as well as "the evidence was here"; compare
patch sizes, and read the maps next to domain_score.  The maps say where the estimate is read from, not whether it is right.
"""

import numpy as np

from .infer import check_heads, loader_workers, refuse_launcher

# table columns of urso_occl_score (include/ursonet_explain.h, URSO_OCCL_*; hip.OCCL_* are the same numbers)
COLS, MAX_MAPS = 10, 8
D_ORI, D_LOC, ORI_KL, ORI_TV, ORI_DROP, ORI_ARGMAX, LOC_KL, LOC_TV, LOC_DROP, LOC_ARGMAX = range(10)
DEC_LOC_EST, DEC_Q_EST, DEC_COLS = 0, 3, 12                    # urso_pose_decode's (hip.DEC_*)
MAP_COLUMNS = (("d_ori", D_ORI), ("d_loc", D_LOC), ("ori_kl", ORI_KL), ("ori_tv", ORI_TV), ("ori_drop", ORI_DROP),
               ("loc_kl", LOC_KL), ("loc_tv", LOC_TV), ("loc_drop", LOC_DROP))
EMPTY_RECT = (0, 0, 0, 0)


def heat_lut():
    """The default colour table of the overlay: the ramp black - red - yellow - white, uint8 [256,3]."""
    i = 3 * np.arange(256, dtype=np.int64)
    return np.stack([np.clip(i, 0, 255), np.clip(i - 255, 0, 255), np.clip(i - 510, 0, 255)], axis=1).astype(np.uint8)


# ------------------------------------------------------------------ the patch grid
def _pair(v, name):
    try:
        p = (int(v), int(v)) if np.ndim(v) == 0 else tuple(int(x) for x in v)
        ok = len(p) == 2 and p[0] >= 1 and p[1] >= 1 and (np.ndim(v) != 0 or int(v) == v) and not isinstance(v, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("explain: %s is an int or a pair (h, w) of ints >= 1, in model-size pixels (got %r)" % (name, v))
    return p


def _positions(a, b, p, s):
    if p >= b - a:
        return [a]
    pos = list(range(a, b - p + 1, s))
    if pos[-1] != b - p:
        pos.append(b - p)
    return pos


def occlusion_rects(window, patch, stride=None):
    """The patch grid of a resize window (y0, x0, y1, x1) -> int32 [P, 4] rects (y0, x0, y1, x1), half open, row-major over (iy, ix).
    patch, stride: an int or (h, w), >= 1; stride None: half the patch (at least 1).  Along an axis [a, b) with patch p and stride s: one
    position a where p >= b - a (the rect is clipped to b), else a, a + s, ... while pos + p <= b, then b - p if that was not the last.
    Every window pixel is covered, no rect leaves the window."""
    y0, x0, y1, x1 = (int(v) for v in window)
    if y1 <= y0 or x1 <= x0:
        raise ValueError("explain: the window %r is empty" % (tuple(window),))
    ph, pw = _pair(patch, "patch")
    sh, sw = (max(1, ph // 2), max(1, pw // 2)) if stride is None else _pair(stride, "stride")
    return np.array([(y, x, min(y + ph, y1), min(x + pw, x1)) for y in _positions(y0, y1, ph, sh) for x in _positions(x0, x1, pw, sw)],
                    dtype=np.int32).reshape(-1, 4)


# ------------------------------------------------------------------ the kernels' statements
def occlude_host(frame, rects, fill):
    """urso_occl_fill_u8: uint8 [n, H, W, C], row j = frame with rect j (clamped to the frame; empty: a copy) painted with fill[:C]."""
    frame = np.asarray(frame)
    H, W, Cc = frame.shape
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    out = np.repeat(frame[None], len(rects), axis=0)
    colour = np.asarray(list(fill)[:Cc], dtype=np.uint8)
    for j, (y0, x0, y1, x1) in enumerate(rects):
        y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H), min(x1, W)
        if y1 > y0 and x1 > x0:
            out[j, y0:y1, x0:x1] = colour
    return out


def _pmf64(z):
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    d = z - z.max()
    Z = np.exp(d).sum()
    return np.exp(d) / Z, d - np.log(Z)


def head64(z0, z):
    """One classification head of urso_occl_score: (KL, TV, DROP, ARGMAX) of the row z [K] against the baseline z0 [K] (fp32 logits)."""
    z0, z = np.asarray(z0, dtype=np.float32), np.asarray(z, dtype=np.float32)
    if np.isnan(z0).any() or np.isnan(z).any():
        return np.full(4, np.nan)
    with np.errstate(all="ignore"):
        p0, lp0 = _pmf64(z0)
        p1, lp1 = _pmf64(z)
        t = np.where(p0 == 0, 0.0, np.where(p1 == 0, np.inf, p0 * (lp0 - lp1)))
        k0 = int(np.argmax(z0))
        out = np.array([t.sum(), 0.5 * np.abs(p0 - p1).sum(), p0[k0] - p1[k0], float(np.argmax(z))])
    if not (np.isfinite(z0.max()) and np.isfinite(z.max())):
        out[:] = np.nan
    return out


def pose64(dec0, dec):
    """The pose columns of urso_occl_score: (D_ORI degrees, D_LOC) of the DEC row `dec` against the baseline's `dec0`."""
    dec0, dec = np.asarray(dec0, dtype=np.float64), np.asarray(dec, dtype=np.float64)
    a, b = dec0[DEC_Q_EST:DEC_Q_EST + 4], dec[DEC_Q_EST:DEC_Q_EST + 4]
    with np.errstate(all="ignore"):
        d = abs(a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3])
        d = 1.0 if d > 1.0 else d
        ang = 2 * np.arccos(d)
        dl = dec[DEC_LOC_EST:DEC_LOC_EST + 3] - dec0[DEC_LOC_EST:DEC_LOC_EST + 3]
        return ang * 180 / np.pi, np.sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2])


def score64(dec0, dec, ori_z0=None, ori_z=None, loc_z0=None, loc_z=None):
    """urso_occl_score in NumPy float64: DEC rows dec [n, DEC_COLS] against the baseline's row dec0 and, per head given, logits z [n, K]
    against the baseline's z0 [K] -> [n, COLS]; the columns of an absent head are NaN."""
    dec = np.asarray(dec, dtype=np.float64).reshape(-1, DEC_COLS)
    out = np.full((len(dec), COLS), np.nan)
    for r in range(len(dec)):
        out[r, D_ORI], out[r, D_LOC] = pose64(dec0, dec[r])
        if ori_z0 is not None:
            out[r, ORI_KL:ORI_KL + 4] = head64(ori_z0, ori_z[r])
        if loc_z0 is not None:
            out[r, LOC_KL:LOC_KL + 4] = head64(loc_z0, loc_z[r])
    return out


def splat64(scores, cols, rects, window):
    """urso_occl_splat: fp64 [M, h, w]; a window pixel's value in map m is the sum, from +0.0 in ascending patch order, of
    scores[p, cols[m]] over the patches p whose rect covers it, divided once by their count; NaN where no patch covers it."""
    scores = np.asarray(scores, dtype=np.float64)
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    wy0, wx0, wy1, wx1 = (int(v) for v in window)
    h, w = wy1 - wy0, wx1 - wx0
    s, cnt = np.zeros((len(cols), h, w)), np.zeros((h, w))
    with np.errstate(all="ignore"):
        for p, (y0, x0, y1, x1) in enumerate(rects):
            a, b, c, d = max(y0 - wy0, 0), min(y1 - wy0, h), max(x0 - wx0, 0), min(x1 - wx0, w)
            if b <= a or d <= c:
                continue
            cnt[a:b, c:d] += 1
            for m, col in enumerate(cols):
                s[m, a:b, c:d] = s[m, a:b, c:d] + scores[p, col]
        return np.where(cnt > 0, s / np.where(cnt > 0, cnt, 1.0), np.nan)


def overlay_host(img, heat, lo, scale, lut, alpha):
    """urso_heat_overlay_u8: a copy of img (uint8 [h, w, 3]) with, wherever t = (heat - lo) * scale is not NaN, lut[min(255, max(0,
    rint(t)))] blended in: px = (alpha * colour + (256 - alpha) * px + 128) >> 8."""
    out = np.array(img, dtype=np.uint8, copy=True)
    lut = np.asarray(lut, dtype=np.uint8)
    with np.errstate(all="ignore"):
        t = (np.asarray(heat, dtype=np.float64) - np.float64(lo)) * np.float64(scale)
    ok = ~np.isnan(t)
    idx = np.clip(np.rint(t[ok]), 0, 255).astype(np.int64)
    alpha = int(alpha)
    out[ok] = ((alpha * lut[idx].astype(np.int64) + (256 - alpha) * out[ok].astype(np.int64) + 128) >> 8).astype(np.uint8)
    return out


def heat_range(heat):
    """(lo, scale) of a map for the overlay: its finite minimum and 255 / (max - min); None where no value is finite or all are equal."""
    fin = np.asarray(heat, dtype=np.float64)
    fin = fin[np.isfinite(fin)]
    if fin.size == 0 or fin.max() == fin.min() or not np.isfinite(255.0 / (fin.max() - fin.min())):
        return None
    return float(fin.min()), float(255.0 / (fin.max() - fin.min()))


# ------------------------------------------------------------------ the result
class ExplainResult(object):
    """Per-image lists / arrays in the order the images ran: image_ids; loc_est [N,3], q_est [N,4] (the baseline's DEC columns: the
    unoccluded frame's estimate at the batch composition of explain()'s first chunk); window [N,4] (the frame's resize window);
    rects (int32 [P,4] per image); scores (fp64 [P, COLS] per image, one row per patch; COLS columns D_ORI, D_LOC and per classification
    head KL, TV, DROP, ARGMAX -- NaN for a regression head); baseline_scores [N, COLS] (the unoccluded row against itself); maps (per image
    a dict name -> fp64 [h, w] over the window: d_ori, d_loc and, per classification head, ori_kl / ori_tv / ori_drop, loc_kl / loc_tv /
    loc_drop); the host summaries in float64 peak_xy [N,2] (the window pixel (x, y) of the largest d_ori, the first in row-major order on
    ties), centroid_xy [N,2] (the d_ori-weighted mean pixel; NaN where the map sums to 0), centroid_offset [N] (its distance in window pixels
    to the baseline's projected location, detect.project(loc_est, K) * scale; NaN without a dataset.camera), patches and passes [N];
    pictures: with render and no sink a list of uint8 [h, w, 3], else None."""

    def __init__(self, image_ids):
        self.image_ids = np.asarray(image_ids)
        self.loc_est, self.q_est, self.window, self.rects, self.scores, self.baseline_scores, self.maps = [], [], [], [], [], [], []
        self.peak_xy, self.centroid_xy, self.centroid_offset, self.patches, self.passes = [], [], [], [], []
        self.pictures = None

    def _close(self):
        for k, shape in (("loc_est", (-1, 3)), ("q_est", (-1, 4)), ("window", (-1, 4)), ("baseline_scores", (-1, COLS)), ("peak_xy", (-1, 2)),
                         ("centroid_xy", (-1, 2)), ("centroid_offset", (-1,))):
            setattr(self, k, np.asarray(getattr(self, k), dtype=np.int64 if k == "window" else np.float64).reshape(shape))
        self.patches, self.passes = np.asarray(self.patches, dtype=np.int64), np.asarray(self.passes, dtype=np.int64)
        return self


def summaries(heat, target_xy=None):
    """(peak_xy, centroid_xy, centroid_offset) of a d_ori map in float64, in window pixels (x, y)."""
    heat = np.asarray(heat, dtype=np.float64)
    h, w = heat.shape
    k = int(np.argmax(np.where(np.isnan(heat), -np.inf, heat)))
    peak = np.array([k % w, k // w], dtype=np.float64)
    with np.errstate(all="ignore"):
        tot = heat.sum()
        centroid = np.array([(heat.sum(axis=0) * np.arange(w)).sum() / tot, (heat.sum(axis=1) * np.arange(h)).sum() / tot]) if tot != 0 \
            else np.full(2, np.nan)
        off = np.nan if target_xy is None else float(np.sqrt(((centroid - np.asarray(target_xy, dtype=np.float64)) ** 2).sum()))
    return peak, centroid, off


# ------------------------------------------------------------------ the command
def _fill_bytes(fill, cfg):
    if isinstance(fill, str):
        if fill != "mean":
            raise ValueError("explain: fill is \"mean\" or three ints in 0 .. 255 (got %r)" % (fill,))
        return tuple(int(v) for v in np.rint(np.asarray(cfg.MEAN_PIXEL, dtype=np.float64)).astype(np.uint8)[:3])
    try:
        vals = [v for v in fill]
        ok = len(vals) == 3 and all(not isinstance(v, bool) and int(v) == v and 0 <= int(v) <= 255 for v in vals)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("explain: fill is \"mean\" or three ints in 0 .. 255 (got %r)" % (fill,))
    return tuple(int(v) for v in vals)


def _u8_rgb(image):
    return getattr(image, "dtype", None) == np.uint8 and np.ndim(image) == 3 and np.shape(image)[-1] == 3


def _float_frames(dtype):
    return ValueError("explain occludes uint8 RGB frames; this dataset's frames reach the engine as %s (molded on the host)." % (dtype,))


def explain(model, dataset, image_ids=None, nr_images=None, patch=32, stride=None, fill="mean", calibration=None, render=False, lut=None,
            alpha=128, sink=None, workers=None):
    """Occlusion-sensitivity maps of the pose heads -> ExplainResult.  model: an inference model; dataset: images (only load_image is
    called; uint8 RGB frames, IMAGE_RESIZE_MODE square / pad64) and, for the classification heads, the bin maps.  image_ids: the images,
    in that order; None: the first nr_images of dataset.image_ids (None: all).  patch, stride: an int or (h, w) in model-size pixels,
    >= 1; stride None: half the patch.  The patches tile the frame's resize window (occlusion_rects): padding is never occluded.
    fill: what a patch is painted with: "mean" (np.rint(Config.MEAN_PIXEL): the value that molds to about 0, which is what the zero
    padding is to the network) or three ints 0 .. 255.  calibration: a calibrate.Calibration, applied to the logits the PMF columns are
    computed from (and to the decoded poses of the classification heads).  render: True or a map's name ("d_ori" for True): that map is
    blended onto a copy of the frame's window through lut (uint8 [256,3], default heat_lut()) at weight alpha / 256 (0 .. 256) between
    the map's finite minimum and maximum (a constant map draws nothing); the picture goes to sink(index, "heat", array) or, without a
    sink, into ExplainResult.pictures.  Per image P + 1 rows run in ceil((P + 1) / B) passes; the model's weights, statistics and input
    are not changed.  ValueError, before any GPU work: a training-mode model, what check_heads refuses, a data-parallel launcher, frames
    that are not uint8 RGB, a bad patch / stride / fill / lut / alpha / render, a resize mode without a window."""
    refuse_launcher(model, "explain", "walk the whole dataset")
    if getattr(model, "mode", None) != "inference":
        raise ValueError("explain needs a model created in inference mode (got mode %r): the maps explain what predict() computes" % (getattr(model, "mode", None),))
    cfg = model.config
    check_heads(model, dataset, False, who="explain")
    if calibration is not None:
        from .calibrate import check_calibration
        check_calibration(calibration, None, "explain")
    ph, pw = _pair(patch, "patch")
    sh, sw = (max(1, ph // 2), max(1, pw // 2)) if stride is None else _pair(stride, "stride")
    colour = _fill_bytes(fill, cfg)
    if cfg.IMAGE_RESIZE_MODE not in ("square", "pad64"):
        raise ValueError("explain: IMAGE_RESIZE_MODE %r has no window to occlude (square / pad64 have)" % (cfg.IMAGE_RESIZE_MODE,))
    names = [nm for nm, col in MAP_COLUMNS if col < ORI_KL or (col < LOC_KL and not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS)) or
             (col >= LOC_KL and not cfg.REGRESS_LOC)]
    shown = None
    if render:
        shown = "d_ori" if render is True else render
        if shown not in names:
            raise ValueError("explain: render is True or one of the maps %s of this model (got %r)" % (", ".join(names), render))
        if isinstance(alpha, bool) or int(alpha) != alpha or not 0 <= int(alpha) <= 256:
            raise ValueError("explain: alpha is an int in 0 .. 256 (got %r)" % (alpha,))
        lut_h = heat_lut() if lut is None else np.ascontiguousarray(lut)
        if lut_h.dtype != np.uint8 or lut_h.shape != (256, 3):
            raise ValueError("explain: lut is a uint8 [256,3] table, not %s %s" % (lut_h.dtype, lut_h.shape))
    ids = list(dataset.image_ids if image_ids is None else image_ids)
    if image_ids is None and nr_images is not None:
        if int(nr_images) < 0:
            raise ValueError("explain: nr_images must be >= 0 or None (got %r)" % (nr_images,))
        ids = ids[:int(nr_images)]
    if ids:
        first = dataset.load_image(ids[0])                     # the one refusal that needs a frame: looked at before any GPU work
        if not _u8_rgb(first):
            raise _float_frames(getattr(first, "dtype", type(first).__name__))
        del first
    res = ExplainResult(ids)
    if render and sink is None:
        res.pictures = [None] * len(ids)
    if not ids:
        return res._close()

    from .detect import _Drawn, frame_matrix, project
    from .infer import PosePass
    ps = PosePass(model, dataset, scatter=True, who="explain", calibration=calibration)
    import torch
    from . import hip, utils
    from .feeder import EvalFeeder
    B, dev = ps.B, ps.dev
    cols = [col for nm, col in MAP_COLUMNS if nm in names]
    M = len(cols)
    fill_d = list(colour) + [0]
    lut_d = torch.as_tensor(lut_h).to(dev) if render else None
    view = _Drawn(dataset, ids)
    scratch = None                                             # the occluded batch, uint8 [B,H,W,3]
    plans = {}                                                 # per frame size: window, rects and the device buffers of one image
    camera = getattr(dataset, "camera", None)
    feed = EvalFeeder(model, view, cfg, workers=loader_workers(cfg, workers), labels=False)
    try:
        for bt in feed:
            if bt.images.dtype != torch.uint8:
                raise _float_frames(bt.images.dtype)
            if scratch is None or scratch.shape != bt.images.shape:
                scratch = torch.zeros_like(bt.images)           # rows a tail chunk leaves out keep the chunk before's (zeros in a first chunk)
            for j in range(bt.n):
                i = bt.row0 + j
                shape = view.shapes[ids[i]]
                if len(shape) != 3 or shape[2] != 3:
                    raise ValueError("explain: a uint8 RGB frame [H,W,3] expected, not %s" % (shape,))
                if shape not in plans:
                    H0, W0 = shape[:2]
                    scale, _size, _pads, window = utils.resize_geometry(H0, W0, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.IMAGE_MIN_SCALE,
                                                                        cfg.IMAGE_RESIZE_MODE)
                    rects = occlusion_rects(window, (ph, pw), (sh, sw))
                    P, h, w = len(rects), window[2] - window[0], window[3] - window[1]
                    # one buffer per frame size for what is read back: the score table [P + 1, COLS], the maps [M, h, w], the baseline's DEC row
                    a, b = (P + 1) * COLS, (P + 1) * COLS + M * h * w
                    back = torch.full((b + hip.DEC_COLS,), float("nan"), dtype=torch.float64, device=dev)
                    plans[shape] = dict(scale=scale, window=window, rects=rects, P=P, h=h, w=w, back=back, table=back[:a].view(P + 1, COLS),
                                        maps=back[a:b].view(M, h, w), base=back[b:], dec=ps.table(P + 1, hip.DEC_COLS),
                                        rects_all=torch.as_tensor(np.concatenate([np.array([EMPTY_RECT], dtype=np.int32), rects])).to(dev))
                pl = plans[shape]
                P, window = pl["P"], pl["window"]
                frame = bt.images[j]
                z0 = l0 = None
                passes = 0
                for r0 in range(0, P + 1, B):
                    n = min(B, P + 1 - r0)
                    hip.occl_fill_u8(frame, pl["rects_all"][r0:r0 + n], fill_d, scratch, n)
                    ps.run(scratch)
                    heads = ps.heads(n)
                    ps.decode_into(pl["dec"], n, r0, heads)
                    loc, _ori, _ori2, z = heads
                    if r0 == 0:                                # the baseline's logits: the next pass overwrites the engine's output buffer
                        z0 = z[0].clone() if ps.soft else None
                        l0 = loc[0].clone() if ps.loc_class else None
                    hip.occl_score(B, n, r0, pl["dec"][0], pl["dec"], pl["table"], ori_z0=z0, ori_z=z if ps.soft else None,
                                   loc_z0=l0, loc_z=loc if ps.loc_class else None)
                    passes += 1
                hip.occl_splat(pl["table"][1:], cols, pl["rects_all"][1:], window, pl["maps"])
                pl["base"].copy_(pl["dec"][0])
                host = pl["back"].cpu().numpy()                # the one read of the image: the score table, the maps, the baseline's pose
                a, b = (P + 1) * COLS, (P + 1) * COLS + M * pl["h"] * pl["w"]
                table, maps, row = host[:a].reshape(P + 1, COLS), host[a:b].reshape(M, pl["h"], pl["w"]), host[b:]
                res.loc_est.append(row[hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3].copy())
                res.q_est.append(row[hip.DEC_Q_EST:hip.DEC_Q_EST + 4].copy())
                res.maps.append({nm: maps[m].copy() for m, nm in enumerate(names)})
                res.scores.append(table[1:].copy())
                res.baseline_scores.append(table[0].copy())
                res.rects.append(pl["rects"].copy())
                res.window.append(window)
                res.patches.append(P)
                res.passes.append(passes)
                target = None
                if camera is not None:
                    target = project(res.loc_est[-1], frame_matrix(camera, shape[1], shape[0])) * pl["scale"]
                peak, centroid, off = summaries(res.maps[-1]["d_ori"], target)
                res.peak_xy.append(peak)
                res.centroid_xy.append(centroid)
                res.centroid_offset.append(off)
                if render:
                    rng = heat_range(res.maps[-1][shown])
                    win = frame[window[0]:window[2], window[1]:window[3]].clone(memory_format=torch.contiguous_format)   # the feeder's batch stays as it is
                    if rng is not None:
                        hip.heat_overlay_u8(pl["maps"][names.index(shown)], rng[0], rng[1], lut_d, int(alpha), win)
                    pic = win.cpu().numpy()
                    if sink is not None:
                        sink(i, "heat", pic)
                    else:
                        res.pictures[i] = pic
    finally:
        feed.close()
    return res._close()
