"""NumPy references of the video path, written independently of ursonet_amd/video.py and of the kernels: the frame prep of
pose_estimator.py:641-645 pixel by pixel, the integer rasteriser rule of urso_draw_prims_u8 (include/ursonet_hip.h) over whole pixel
grids in int64, and the projection of utils.plot_axes (utils.py:186-217) with np.matrix as the reference writes it."""
import numpy as np


def prep_loop(frame, crop, pad, grey):
    """Crop + zero pad + grey mix, one output pixel at a time: Python floats are IEEE float64, each * and + rounds on its own, int()
    truncates."""
    t, b, l, r = crop
    h, w = frame.shape[:2]
    ch, cw = h - t - b, w - l - r
    out = np.zeros((ch + 2 * pad, cw + 2 * pad, 3), dtype=np.uint8)
    for y in range(ch):
        for x in range(cw):
            R, G, B = (float(v) for v in frame[y + t, x + l])
            v = (grey[0] * R + grey[1] * G) + grey[2] * B
            out[y + pad, x + pad, :] = int(v)
    return out


def _covered(kind, x0, y0, x1, y1, r, H, W):
    """Boolean [H,W]: the pixels the rule paints, all in int64."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    x0, y0, x1, y1, r = (np.int64(v) for v in (x0, y0, x1, y1, r))
    if kind == 1:
        return (xx - x0) ** 2 + (yy - y0) ** 2 <= r * r
    assert kind == 0
    Dx, Dy = x1 - x0, y1 - y0
    wx, wy = xx - x0, yy - y0
    s = wx * Dx + wy * Dy
    DD = Dx * Dx + Dy * Dy
    ww = wx * wx + wy * wy
    ux, uy = xx - x1, yy - y1
    tt = r * r
    before = 4 * ww <= tt
    after = 4 * (ux * ux + uy * uy) <= tt
    # the middle test needs 4 (|w|^2 |D|^2 - s^2) < 2^63: true for the frame sizes of the tests (|w|^2 < 2^30, |D|^2 <= 2^31, and the
    # difference is the squared cross product, far smaller); asserted so that a wrap can never pass silently
    inner = (s > 0) & (s < DD)
    assert float(ww.max()) * float(DD) * 4 < 2.0 ** 63
    middle = 4 * (ww * DD - s * s) <= tt * DD
    return np.where(s <= 0, before, np.where(s >= DD, after, middle & inner))


def rasterise(img, prims):
    """prims: rows [kind, x0, y0, x1, y1, r, cR, cG, cB] in drawing order -> a painted COPY of the uint8 image [H,W,3]."""
    out = np.array(img, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    for p in np.asarray(prims, dtype=np.int64).reshape(-1, 9):
        out[_covered(int(p[0]), p[1], p[2], p[3], p[4], p[5], H, W)] = p[6:9].astype(np.uint8)
    return out


def quat2SO3_matrix(q):
    return np.matrix([[1 - 2 * q[1] ** 2 - 2 * q[2] ** 2, 2 * (q[0] * q[1] + q[2] * q[3]), 2 * (q[0] * q[2] - q[1] * q[3])],
                      [2 * (q[0] * q[1] - q[2] * q[3]), 1 - 2 * q[0] ** 2 - 2 * q[2] ** 2, 2 * (q[1] * q[2] + q[0] * q[3])],
                      [2 * (q[0] * q[2] + q[1] * q[3]), 2 * (q[1] * q[2] - q[0] * q[3]), 1 - 2 * q[0] ** 2 - 2 * q[1] ** 2]])


def project_axes(q, C, K, scale):
    """The projection half of utils.plot_axes as the reference states it -> (c [2] ints, v [2,3] ints: one column per axis tip)."""
    C = np.asarray(C, dtype=np.float64)
    P = np.matrix([[1, 0, 0], [0, -1, 0], [0, 0, 1]]) * scale
    P_r = quat2SO3_matrix(q) * P
    P_t = np.asarray(P_r) + np.transpose([C])
    p = P_t / P_t[-1, :]
    c = C / C[-1]
    p = np.matrix(K) * p
    c = np.matrix(K) * np.matrix(c).transpose()
    c = c.astype(int)
    v = p.astype(int)
    return np.array([c[0, 0], c[1, 0]]), np.asarray(v[:2, :])
