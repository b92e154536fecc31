"""Rotation augmentation with the image work on the GPU ("next" scope row f-1).

Mirrors utils.rotate_cam / utils.rotate_image (utils.py:30-86) as load_image_gt calls them
(net.py:415-438): a random camera rotation R_change is applied to the image as the homography
M = K R_change K^-1 and to the pose (t' = t R^T, q' = q_change (x) q); the soft-classification
target is then re-encoded (utils.encode_ori_fast).  The reference's
`cv2.warpPerspective(image, M, (w, h), cv2.WARP_INVERSE_MAP)` passes the constant in the binding's
`dst` slot, so the call runs with default flags: forward map, INTER_LINEAR, zero border -- the only
reading under which image and pose stay consistent; that is what is implemented.  The warp and the
re-encode run as HIP kernels (urso_warp_perspective, urso_encode_ori) on whole batches that stay
in HBM; the 3x3 / quaternion algebra per sample stays on the host in float64.
"""
import math
import threading

import numpy as np


def euler2SO3_left(pitch, yaw, roll):
    """se3lib.py:38-51 (degrees) -> 3x3 ndarray."""
    p, y, r = (float(a) * np.pi / 180 for a in (pitch, yaw, roll))
    cp, sp, cy, sy, cr, sr = np.cos(p), np.sin(p), np.cos(y), np.sin(y), np.cos(r), np.sin(r)
    return np.array([[cy * cr, sp * sy * cr - cp * sr, cp * sy * cr + sp * sr],
                     [cy * sr, sp * sy * sr + cp * cr, cp * sy * sr - sp * cr],
                     [-sy, sp * cy, cp * cy]])


def SO32quat(R):
    """se3lib.py:77-113: rotation matrix -> [x, y, z, w] (largest-diagonal branch selection)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    d = [R[0, 0], R[1, 1], R[2, 2]]
    if tr > 0:
        Z = math.sqrt(tr + 1) * 2
        return np.array([(R[1, 2] - R[2, 1]) / Z, (R[2, 0] - R[0, 2]) / Z, (R[0, 1] - R[1, 0]) / Z, 0.25 * Z])
    if d[0] > d[1] and d[0] > d[2]:
        i, j, k = 0, 1, 2
    elif d[1] > d[2]:
        i, j, k = 1, 2, 0
    else:
        i, j, k = 2, 0, 1
    Z = math.sqrt(1.0 + 2 * d[i] - tr) * 2
    q = np.zeros(4)
    q[i] = 0.25 * Z
    q[j] = (R[i, j] + R[j, i]) / Z
    q[k] = (R[i, k] + R[k, i]) / Z
    q[3] = (R[j, k] - R[k, j]) / Z
    return q


def quat_mult(a, b):
    """se3lib.py:164-179 for a 1-D b; result normalised."""
    x, y, z, w = (float(v) for v in a)
    b = np.asarray(b, dtype=np.float64).ravel()
    res = np.array([w * b[0] + z * b[1] - y * b[2] + x * b[3],
                    -z * b[0] + w * b[1] + x * b[2] + y * b[3],
                    y * b[0] - x * b[1] + w * b[2] + z * b[3],
                    -x * b[0] - y * b[1] - z * b[2] + w * b[3]])
    return res / np.linalg.norm(res)


def quat2SO3(q):
    """se3lib.py:134-144: [x, y, z, w] -> rotation matrix."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * (x * y + z * w), 2 * (x * z - y * w)],
                     [2 * (x * y - z * w), 1 - 2 * x * x - 2 * z * z, 2 * (y * z + x * w)],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * x * x - 2 * y * y]])


def encode_as_keypoints(oris, centroids, scale=1.0):
    """utils.py:220-244: a pose as two virtual 3-D keypoints on the body z and y axes.  One pose -> two 3x1 columns (the caller
    transposes them, net.py:456); a batch [N,4], [N,3] -> two float32 [N,3] arrays."""
    if np.ndim(oris) == 1:
        R = quat2SO3(oris)
        c = np.asarray(centroids, dtype=np.float64).reshape(3, 1)
        return R @ (scale * np.array([[0.0], [0.0], [1.0]])) + c, R @ (scale * np.array([[0.0], [1.0], [0.0]])) + c
    oris, centroids = np.asarray(oris), np.asarray(centroids)
    K1 = np.zeros((len(oris), 3), dtype=np.float32); K2 = np.zeros((len(oris), 3), dtype=np.float32)
    for i in range(len(oris)):
        k1, k2 = encode_as_keypoints(oris[i], centroids[i], scale)
        K1[i], K2[i] = k1[:, 0], k2[:, 0]
    return K1, K2


def rotation_homography(K, R_change):
    K = np.asarray(K, dtype=np.float64)
    return K @ np.asarray(R_change, dtype=np.float64) @ np.linalg.inv(K)


def rotate_pose(t, q, R_change):
    """Pose update of utils.py:53-56."""
    R_change = np.asarray(R_change, dtype=np.float64)
    return np.asarray(t, dtype=np.float64) @ R_change.T, quat_mult(SO32quat(R_change), q)


def invert_homography(M):
    """3x3 inverse in closed form (adjugate / determinant), as cv::invert does for 3x3."""
    m = np.asarray(M, dtype=np.float64).reshape(3, 3)
    c = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                  [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                  [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    det = m[0, 0] * c[0, 0] - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    return c * (1.0 / det)


def warp_images(images, M, inverse_map=False, interp="linear"):
    """cv2.warpPerspective on a batch: images uint8 [B,H,W,C] (device tensor or array), M [B,3,3] forward
    homographies (source -> destination; destination -> source with inverse_map=True).
    Returns a uint8 CUDA tensor [B,H,W,C] (urso_warp_perspective)."""
    import torch
    from . import hip
    x = torch.as_tensor(images)
    assert x.dtype == torch.uint8 and x.dim() == 4, "uint8 [B,H,W,C] images expected"
    x = x.cuda().contiguous()
    B, H, W, C = x.shape
    M = np.asarray(M, dtype=np.float64).reshape(B, 3, 3)
    if not inverse_map:
        M = np.stack([invert_homography(m) for m in M])
    m = torch.as_tensor(np.ascontiguousarray(M.reshape(B, 9))).cuda()
    out = torch.empty_like(x)
    hip.warp_perspective(B, H, W, C, {"nearest": 0, "linear": 1}[interp], x, m, out)
    return out


def encode_orientations(q, H_quat, redundant, beta):
    """Batched utils.encode_ori_fast on the GPU: q [B,4] -> float32 CUDA tensor [B, n^3] of PMFs."""
    import torch
    from . import hip
    K = len(H_quat)
    n = round(K ** (1. / 3))
    var = (float(beta) / n) ** 2 / 12
    qd = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(np.asarray(q, dtype=np.float64)))).cuda()
    hq = torch.as_tensor(np.ascontiguousarray(H_quat, dtype=np.float32)).cuda()
    rd = torch.as_tensor(np.ascontiguousarray(np.asarray(redundant, dtype=bool).astype(np.uint8))).cuda()
    out = torch.empty(qd.shape[0], K, dtype=torch.float32, device="cuda")
    hip.encode_ori(qd.shape[0], K, qd, hq, rd, var, out)
    return out


def rotate_cam_batch(images, t, q, K, pyr_change):
    """Batched rotate_cam for GIVEN per-sample Euler perturbations pyr_change [B,3] (degrees):
    returns (warped uint8 CUDA tensor, t_new [B,3], q_new [B,4])."""
    t, q, pyr = np.atleast_2d(t), np.atleast_2d(q), np.atleast_2d(pyr_change)
    Rs = [euler2SO3_left(*p) for p in pyr]
    Ms = np.stack([rotation_homography(K, R) for R in Rs])
    poses = [rotate_pose(t[i], q[i], Rs[i]) for i in range(len(Rs))]
    return warp_images(images, Ms), np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])


def rotate_cam(image, t, q, K, magnitude):
    """Drop-in for utils.rotate_cam (same NumPy global-RNG draw): one image [H,W,C] uint8 -> (image_warped ndarray, t_new, q_new)."""
    pyr_change = (np.random.rand(3) - 0.5) * magnitude
    w, tn, qn = rotate_cam_batch(np.asarray(image)[None], t, q, K, pyr_change[None])
    return w[0].cpu().numpy(), tn[0], qn[0]


def rotate_image(image, t, q, K):
    """Drop-in for utils.rotate_image: random in-plane rotation of up to +-85 degrees."""
    change = (np.random.rand(1) - 0.5) * 170
    w, tn, qn = rotate_cam_batch(np.asarray(image)[None], t, q, K, np.array([[0.0, 0.0, change[0]]]))
    return w[0].cpu().numpy(), tn[0], qn[0]


# --------------------------------------------------------------------------- sim2real (net.py:390-406)
SIM2REAL_OPS = ("noise", "blur", "add", "multiply", "dropout")


_PIPELINE_RNG = np.random.RandomState()      # stands for imgaug's own generator: the stage parameters never consume NumPy's global stream


def sim2real_draw(n, height, width, rng=np.random, prng=None):
    """The random decisions of the reference's sim2real branch for `n` samples, sample by sample: whether the pipeline runs (p = 0.5)
    from `rng` (NumPy's global generator by default: net.py:395 `np.random.rand(1) > 0.5`), and -- only for the samples it runs on, as
    imgaug draws when `to_deterministic()` is called (net.py:405) -- the random order of its five stages and each stage's parameter
    from `prng` (imgaug's own generator in the reference, not NumPy's global stream; default: the same generator as `rng`, which the
    distribution tests seed): AdditiveGaussianNoise(scale=0.01*255), GaussianBlur(sigma=(0, 1.5)), Add((-20, 20)), Multiply((0.5, 2.0)),
    CoarseDropout([0.0, 0.03], size_percent=(0.02, 0.1)).  Returns a dict of arrays."""
    prng = rng if prng is None else prng
    apply = np.zeros(n, dtype=bool)
    order = np.tile(np.arange(5), (n, 1))
    par = np.zeros((n, 5, 4), dtype=np.float32)
    seeds = np.zeros(n, dtype=np.uint32)
    masks = []
    for i in range(n):
        apply[i] = rng.rand(1)[0] > 0.5
        par[i, 0, 0] = 0.01 * 255
        par[i, 4, 0], par[i, 4, 1] = 1, 1
        if not apply[i]:
            masks.append(np.zeros((1, 1), dtype=bool))
            continue
        order[i] = prng.permutation(5)
        par[i, 1, 0] = prng.uniform(0.0, 1.5)
        par[i, 2, 0] = float(prng.randint(-20, 21))
        par[i, 3, 0] = prng.uniform(0.5, 2.0)
        p = (0.0, 0.03)[prng.randint(0, 2)]                  # a LIST of two values is a choice in imgaug, not a range
        sp = prng.uniform(0.02, 0.1)
        dh, dw = max(int(height * sp), 1), max(int(width * sp), 1)
        par[i, 4, 0], par[i, 4, 1] = dh, dw
        masks.append(prng.rand(dh, dw) < p)
        seeds[i] = prng.randint(0, 2 ** 31 - 1)
    return {"apply": apply, "order": order, "par": par, "seeds": seeds, "masks": masks}


def sim2real_batch(images, draw=None, rng=np.random, trace=None):
    """net.py:390-406 for a uint8 batch [B,H,W,3] (array or device tensor): grey conversion, then for the samples whose dice say
    so the five imgaug stages in their drawn order -- five passes of urso_sim2real_op over the batch, ping-ponging two HBM
    buffers.  Returns a uint8 CUDA tensor.  trace (tests only): a list that receives a copy of the grey batch and of the batch after each
    of the five launches."""
    import torch
    from . import hip
    x = torch.as_tensor(images)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3
    x = x.cuda().contiguous()
    B, H, W, _ = x.shape
    d = draw if draw is not None else sim2real_draw(B, H, W, rng)
    a, b = torch.empty_like(x), torch.empty_like(x)
    hip.rgb_to_grey3(B, H, W, x, a)
    if trace is not None:
        trace.append(a.clone())
    if not d["apply"].any():
        return a
    stride = max(m.size for m in d["masks"])
    drop = np.zeros((B, stride), dtype=np.uint8)
    for i, m in enumerate(d["masks"]):
        drop[i, :m.size] = m.reshape(-1)
    drop_d = torch.as_tensor(drop).cuda()
    seed_d = torch.as_tensor(d["seeds"].view(np.int32).copy()).cuda()
    for slot in range(5):
        ops = np.where(d["apply"], d["order"][:, slot], -1).astype(np.int32)
        par = np.stack([d["par"][i, d["order"][i, slot]] for i in range(B)]).astype(np.float32)
        hip.sim2real_op(B, H, W, a, b, torch.as_tensor(ops).cuda(), torch.as_tensor(par).cuda(), seed_d, drop_d, stride)
        a, b = b, a
        if trace is not None:
            trace.append(a.clone())
    return a


# --------------------------------------------------------------------------- resize / pad (utils.py:398-511)
_RESIZE_TABLES = {}                          # (h, w, nh, nw, device) -> device tables of utils.resize_tables: a feeder asks for the same geometry every batch
_RESIZE_TABLES_LOCK = threading.Lock()       # feeder producer threads and the main thread (detect) share the cache
_RESIZE_TABLES_MAX = 64


def _resize_device_tables(h, w, nh, nw, device):
    import torch
    from . import utils
    key = (h, w, nh, nw, str(device))
    with _RESIZE_TABLES_LOCK:
        if key in _RESIZE_TABLES:
            _RESIZE_TABLES[key] = _RESIZE_TABLES.pop(key)      # most recently used last
            return _RESIZE_TABLES[key]
        t = utils.resize_tables(h, w, nh, nw)
        up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device)
        if len(_RESIZE_TABLES) >= _RESIZE_TABLES_MAX:
            # the least recently used entry goes; a kernel launched on some thread's stream may still read its tables, so they are freed
            # only after the device has drained (rare: one or two geometries per run is the normal case)
            torch.cuda.synchronize(device)
            _RESIZE_TABLES.pop(next(iter(_RESIZE_TABLES)))
        _RESIZE_TABLES[key] = {"ky": up(t["taps"][0]), "kx": up(t["taps"][1]), "ry": 0 if t["taps"][0] is None else len(t["taps"][0]) // 2,
                               "rx": 0 if t["taps"][1] is None else len(t["taps"][1]) // 2,
                               "y0": up(t["y0"]), "fy": up(t["fy"]), "x0": up(t["x0"]), "fx": up(t["fx"])}
        return _RESIZE_TABLES[key]


def resize_images(images, min_dim=None, max_dim=None, min_scale=None, mode="square", out=None):
    """utils.resize_image for a uint8 batch [B,H,W,C] of one frame size (array or device tensor), on the GPU and with the host function's
    BYTES (urso_resize_images_u8; scale 1: urso_pad_images_u8): -> (uint8 CUDA tensor [B,OH,OW,C], window, scale, padding), the last three
    as utils.resize_image returns them for one frame.  Modes 'square' and 'pad64'; 'none', 'crop' (which draws from `random`) and
    non-uint8 input raise ValueError -- callers keep the host path for those.  `out`: a uint8 CUDA tensor of the result's shape to write into."""
    from . import utils
    if mode not in ("square", "pad64"):
        raise ValueError("resize_images: mode %r stays on the host (utils.resize_image)" % (mode,))
    dtype, shape = getattr(images, "dtype", None), tuple(getattr(images, "shape", ()))
    if str(dtype).replace("torch.", "") != "uint8" or len(shape) != 4:
        raise ValueError("resize_images: uint8 [B,H,W,C] frames expected, not %s %s" % (dtype, shape))
    import torch
    from . import hip
    B, H, W, C = shape
    scale, (nh, nw), pads, window = utils.resize_geometry(H, W, min_dim, max_dim, min_scale, mode)
    padding = [pads[0], pads[1], (0, 0)]
    OH, OW = nh + sum(pads[0]), nw + sum(pads[1])
    x = torch.as_tensor(images).cuda().contiguous()
    if out is None:
        out = torch.empty((B, OH, OW, C), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (B, OH, OW, C) and out.is_contiguous()
    if scale == 1:
        hip.pad_images_u8(B, H, W, C, OH, OW, window[0], window[1], x, out)
    else:
        t = _resize_device_tables(H, W, nh, nw, x.device)
        hip.resize_images_u8(B, H, W, C, nh, nw, OH, OW, window[0], window[1], t["ky"], t["ry"], t["kx"], t["rx"], t["y0"], t["fy"], t["x0"],
                             t["fx"], 1 if utils._resize_compat() == "0.18" else 0, x, out)
    return out, window, scale, padding


# --------------------------------------------------------------------------- video path (pose_estimator.py:606-745; ursonet_amd/video.py)
def video_prep(frames, prep, out=None):
    """video.VideoPrep.host for a uint8 batch [B,H,W,3] of one frame size (array or device tensor), on the GPU and with the host function's
    BYTES (urso_video_prep_u8: crop + zero pad + grey mix in one pass) -> uint8 CUDA tensor [B,OH,OW,3], (OH, OW) = prep.out_shape(H, W).
    `out`: a uint8 CUDA tensor of the result's shape to write into."""
    dtype, shape = getattr(frames, "dtype", None), tuple(getattr(frames, "shape", ()))
    if str(dtype).replace("torch.", "") != "uint8" or len(shape) != 4 or shape[-1] != 3:
        raise ValueError("video_prep: uint8 [B,H,W,3] frames expected, not %s %s" % (dtype, shape))
    import torch
    from . import hip
    B, H, W, _ = shape
    OH, OW = prep.out_shape(H, W)
    x = torch.as_tensor(frames).cuda().contiguous()
    if out is None or tuple(out.shape) != (B, OH, OW, 3):
        out = torch.empty((B, OH, OW, 3), dtype=torch.uint8, device=x.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    hip.video_prep_u8(B, H, W, prep.crop, prep.pad, prep.grey, x, out)
    return out


def draw_prims(frames, prims, counts=None):
    """Draws primitives onto a contiguous uint8 CUDA batch [B,H,W,3] IN PLACE (urso_draw_prims_u8: exact integer segments and discs; rows
    [kind, x0, y0, x1, y1, r, cR, cG, cB], later rows on top).  prims: an int array [B, P <= 16, 9] with counts [B] (rows at and behind a
    frame's count are ignored), or, with counts None, a list of B arrays [n_b <= 16, 9].  Unknown kinds, more than 16 primitives and
    coordinates beyond +-16,384 raise hip.UrsoHipError: drop such primitives first (video.pose_axes_prims does).  Returns `frames`."""
    import torch
    from . import hip
    assert torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and \
        frames.is_contiguous(), "draw_prims draws in place: a contiguous uint8 CUDA tensor [B,H,W,3] expected"
    B, H, W, _ = frames.shape
    host = np.zeros((B, hip.DRAW_MAX_PRIMS, hip.DRAW_PRIM_INTS), dtype=np.int32)
    if counts is None:
        if len(prims) != B:
            raise ValueError("draw_prims: %d primitive lists for %d frames" % (len(prims), B))
        rows = [np.asarray(p, dtype=np.int64).reshape(-1, hip.DRAW_PRIM_INTS) for p in prims]
        cnt = np.array([len(r) for r in rows], dtype=np.int64)
    else:
        arr = np.asarray(prims, dtype=np.int64)
        if arr.ndim != 3 or arr.shape[0] != B or arr.shape[2] != hip.DRAW_PRIM_INTS:
            raise ValueError("draw_prims: prims [B, P, 9] expected, not %s" % (arr.shape,))
        cnt = np.asarray(counts, dtype=np.int64).reshape(-1)
        if cnt.shape != (B,):
            raise ValueError("draw_prims: counts [B] expected")
        rows = [arr[b, :max(0, min(int(cnt[b]), arr.shape[1]))] for b in range(B)]
        if np.any(cnt > arr.shape[1]):
            raise ValueError("draw_prims: a count exceeds the %d rows given" % arr.shape[1])
    if np.any(cnt > hip.DRAW_MAX_PRIMS) or np.any(cnt < 0):
        raise hip.UrsoHipError("urso_draw_prims_u8: a frame has %d primitives (0 .. %d)" % (int(cnt.max() if cnt.max() > hip.DRAW_MAX_PRIMS else cnt.min()),
                                                                                          hip.DRAW_MAX_PRIMS))
    for b, r in enumerate(rows):
        if np.any(np.abs(r) > 2 ** 31 - 1):
            raise hip.UrsoHipError("urso_draw_prims_u8: frame %d: a value outside int32" % b)
        host[b, :len(r)] = r
    cnt32 = np.ascontiguousarray(cnt, dtype=np.int32)
    hip.draw_prims_u8(B, H, W, host, cnt32, torch.as_tensor(host).to(frames.device), torch.as_tensor(cnt32).to(frames.device), frames)
    return frames


def pmf_sheet(gt, logits, n, cell=4, gap=2, lut=None, bg=(255, 255, 255), out=None, scratch=None):
    """utils.visualize_weights (utils.py:117-151) as a picture, on the GPU (urso_pmf_sheet_u8): the slice sheet of B orientation PMFs over
    n^3 bins -> uint8 CUDA tensor [B,SH,SW,3], SW = n n cell + (n + 1) gap, SH = rows n cell + (rows + 1) gap.  gt: stored PMFs, logits:
    the head's raw output, each fp32 [B, n^3] (array or device tensor) or None; rows = how many of the two are given, gt first.  Slice z
    sits at x = gap + z (n cell + gap) and shows bin i n^2 + j n + z at cell row j, column i; a GT bin's value is p / max p, an
    estimate's exp(z - max z); colour = lut[min(255, floor(256 v))] (lut: uint8 [256,3], default the grey ramp), every other pixel is bg.
    `out`: a dense uint8 CUDA tensor of the result's shape, at any address; `scratch`: uint8 CUDA, >= B rows n^3 bytes."""
    import torch
    from . import hip
    up = lambda a: None if a is None else torch.as_tensor(a).cuda().contiguous()
    gt, logits = up(gt), up(logits)
    first = gt if gt is not None else logits
    if first is None:
        raise ValueError("pmf_sheet: neither a stored PMF nor logits given")
    for t in (gt, logits):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != tuple(first.shape)):
            raise ValueError("pmf_sheet: fp32 [B, n^3] sources of one shape expected, not %s %s" % (t.dtype, tuple(t.shape)))
    B, K = first.shape
    if K != int(n) ** 3:
        raise ValueError("pmf_sheet: %d bins are not n^3 for n = %d" % (K, n))
    if lut is None:
        lut = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    lut = torch.as_tensor(lut).to(first.device).contiguous()
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError("pmf_sheet: lut is a uint8 [256,3] table, not %s %s" % (lut.dtype, tuple(lut.shape)))
    rows = (gt is not None) + (logits is not None)
    SH, SW = hip.pmf_sheet_shape(int(n), int(cell), int(gap), rows)
    if out is None:
        if not (1 <= cell <= 64 and 0 <= gap <= 64 and 2 <= n <= 64) or SH * SW * 3 >= 2 ** 31:
            raise hip.UrsoHipError("urso_pmf_sheet_u8: n %d, cell %d, gap %d: outside 2 .. 64, 1 .. 64, 0 .. 64, or an image of 2 GiB or more" % (n, cell, gap))
        out = torch.empty((B, SH, SW, 3), dtype=torch.uint8, device=first.device)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (B, SH, SW, 3) and out.is_contiguous()
    hip.pmf_sheet(B, int(n), int(cell), int(gap), gt, logits, lut, bg, out, scratch=scratch)
    return out
