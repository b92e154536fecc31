"""Plain float64 / integer references of the input-side kernels (urso_rgb_to_grey3, urso_sim2real_op, urso_warp_perspective,
urso_mold_images) and the judge that compares a uint8 result with them.  CPU only: NumPy, nothing from the library.  Every
reference is written from the arithmetic the kernel's header comment documents (ursonet_amd/csrc/augment.hip), not from its loops.

Judging.  A stage that rounds a float32 value to a grey level can legitimately differ from the float64 reference where the
float64 value lies next to a .5 boundary.  assert_equal_off_ties() therefore demands equality everywhere, excuses a difference of
exactly one level only where the float64 value is within `delta` of a tie, and lets at most a share `cap` of the elements be excused.
Both are conditions derived below from the number formats, never from what a device returned:

  u = 2^-24 (half a float32 ulp, relative), K_ULP = 2: the bound taken for the device's expf / logf / sqrtf / cosf (ROCm's HIP math
  table lists 1 to 2 ulp for them; no fast-math in the build: -ffp-contract=off, no -ffast-math), one ulp = 2 u relative.

  noise  v = float32(p + n), n = sigma * sqrtf(-2 logf(u1)) * cosf(a) with u1, u2 and the angle a = 6.283185307f * u2 being the same
         float32 numbers in the reference.  Relative error of n: logf K_ULP ulp, halved by the square root, + sqrtf K_ULP ulp + cosf
         K_ULP ulp + the two float32 products: (2.5 K_ULP * 2 + 2) u.  |n| <= sigma * sqrt(2 ln 2^24) = 5.768 sigma.  The final float32
         addition rounds a value below 256 + |n|: half an ulp of it.
  blur   acc_c / wsum over N = (2r+1)^2 taps, w = expf(ay) * expf(ax), a = -0.5 d^2 / (sigma sigma) <= a_max = 0.5 (r / sigma)^2.
         Relative error of a weight: eps_w = 2 (2 a_max u + 2 K_ULP u) + u (argument: sigma*sigma and the division, one rounding each;
         expf; the product).  Each of the two sums: N float32 additions and one product per term, (N + 1) u relative to the sum of
         magnitudes; the quotient one more rounding.  Result <= 255:  delta = 255 (2 (N + 1) u + 2 eps_w + u).
  add    float32(p) + integer: exact.  delta = 0.
  multiply  float32(p) * f rounded once: half a float32 ulp of 255 f.  Exact (delta = 0) when f is a power of two: the .5 products are
         decided by round-half-to-even, which the reference reproduces.
  dropout, copy  bytes moved.  delta = 0.
  cap = 4 delta: a uniformly distributed fractional part lies within delta of a tie with probability 2 delta."""
import math

import numpy as np

U = 2.0 ** -24
K_ULP = 2


def _ulp32(x):
    """float32 ulp of |x| (float64 arithmetic)."""
    return float(np.spacing(np.float32(abs(x))))


def delta_noise(sigma):
    nmax = 5.768 * float(sigma)
    return nmax * (2.5 * K_ULP * 2 + 2) * U + 0.5 * _ulp32(255.0 + nmax)


def blur_radius(sigma):
    return int(np.ceil(np.float32(3.0) * np.float32(sigma)))


def delta_blur(sigma):
    if float(sigma) < 1e-3:
        return 0.0
    r = blur_radius(sigma)
    n = (2 * r + 1) ** 2
    a_max = 0.5 * (r / float(sigma)) ** 2
    eps_w = 2 * (2 * a_max * U + 2 * K_ULP * U) + U
    return 255.0 * (2 * (n + 1) * U + 2 * eps_w + U)


def delta_multiply(f):
    f = float(np.float32(f))
    m, _ = math.frexp(f)
    return 0.0 if m == 0.5 else 0.5 * _ulp32(255.0 * f)


def multiply_tie_free(f):
    """True if no grey level times the float32 factor comes within delta_multiply of a tie.  The 256 products are discrete, not uniformly
    distributed (1.7 puts every multiple of 5 next to a tie, 3 % of a random frame), so the cap's premise has to be checked for a factor."""
    d = delta_multiply(f)
    return d == 0.0 or not near_tie(np.arange(256, dtype=np.float64) * float(np.float32(f)), d).any()


def stage_delta(code, par):
    """delta of one urso_sim2real_op stage (module docstring)."""
    code = int(code)
    if code == 0:
        return delta_noise(par[0])
    if code == 1:
        return delta_blur(par[0])
    if code == 3:
        return delta_multiply(par[0])
    return 0.0


# ------------------------------------------------------------------------------------------------ the judge
def near_tie(unrounded, delta):
    """True where the float64 value lies within delta of a .5 boundary between two grey levels."""
    u = np.asarray(unrounded, dtype=np.float64)
    return np.abs((u - np.floor(u)) - 0.5) <= delta


def assert_equal_off_ties(got, ref_rounded, unrounded, delta, cap, what=""):
    """Every element of `got` equals `ref_rounded`, except that an element may be the OTHER neighbour of a tie (one level away) where the
    float64 value is within `delta` of a .5 boundary; at most a share `cap` of all elements may be excused so.  Returns the figures."""
    got, ref = np.asarray(got), np.asarray(ref_rounded)
    assert got.shape == ref.shape and got.dtype == np.uint8 and ref.dtype == np.uint8, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    u = np.broadcast_to(np.asarray(unrounded, dtype=np.float64), got.shape)
    diff = got != ref
    nd = int(diff.sum())
    stats = {"what": what, "n": int(got.size), "excused": nd, "delta": float(delta), "cap": float(cap)}
    if nd:
        g, r, uu = got[diff].astype(np.int64), ref[diff].astype(np.int64), u[diff]
        lo = np.floor(uu)
        ok = (np.abs(g - r) == 1) & near_tie(uu, delta) & ((g == np.clip(lo, 0, 255)) | (g == np.clip(lo + 1, 0, 255)))
        if not ok.all():
            k = int(np.flatnonzero(~ok)[0])
            raise AssertionError("%s: %d of %d elements differ, %d of them not at a tie (first: got %d, reference %d from %.9f; delta %.3g)"
                                 % (what, nd, got.size, int((~ok).sum()), g[k], r[k], uu[k], delta))
        assert nd <= cap * got.size, "%s: %d of %d elements differ at ties, more than the cap %.3g allows" % (what, nd, got.size, cap)
    return stats


def tie_share(unrounded, delta):
    """Share of elements within delta of a tie (asserted to stay under the cap before a device result is looked at)."""
    return float(near_tie(unrounded, delta).mean())


def report(stats):
    print("input-side %-28s compared %9d  excused as ties %6d  delta %.3g  cap %.3g" %
          (stats["what"], stats["n"], stats["excused"], stats["delta"], stats["cap"]))
    return stats


def sat_u8(v):
    """np.clip(np.round(.), 0, 255): round half to even, saturate."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ grey
def grey3(rgb):
    """net.py:391-394: 0.2126 R + 0.7152 G + 0.0722 B in float64, truncated by the uint8 assignment, written to the three channels."""
    rgb = np.asarray(rgb)
    g = (0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]).astype(np.uint8)
    return np.repeat(g[..., None], 3, -1)


# ------------------------------------------------------------------------------------------------ noise
def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def noise_uniforms(seed, npix):
    """(u1, u2, angle) of every pixel index as the float32 numbers the generator is defined on: h1 = lowbias32(seed ^ (2 i + 1)),
    h2 = lowbias32(h1 ^ 0x9e3779b9 ^ i), u1 = ((h1 >> 8) + 1) * (1.0f / 16777217.0f) in (0, 1], u2 = (h2 >> 8) * (1.0f / 16777216.0f) in [0, 1),
    angle = 6.283185307f * u2."""
    i = np.arange(npix, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h1 = lowbias32(np.uint32(int(seed) & 0xFFFFFFFF) ^ (i * np.uint32(2) + np.uint32(1)))
        h2 = lowbias32(h1 ^ np.uint32(0x9e3779b9) ^ i)
    c1 = np.float32(1.0) / np.float32(16777217.0)             # the float32 literal 16777217.0f is 2^24: c1 = 2^-24
    c2 = np.float32(1.0) / np.float32(16777216.0)
    u1 = ((h1 >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * c1
    u2 = (h2 >> np.uint32(8)).astype(np.float32) * c2
    ang = np.float32(6.283185307) * u2
    assert u1.dtype == np.float32 and ang.dtype == np.float32
    return u1, u2, ang


def noise_field(seed, npix, sigma, dtype=np.float64):
    """n_i = sigma sqrt(-2 ln u1_i) cos(angle_i) (Box-Muller) for pixel indices 0 .. npix - 1: float64 by default; dtype float32 evaluates the
    same restatement in float32 throughout (the simulated kernel of the CPU tests)."""
    u1, _, ang = noise_uniforms(seed, npix)
    s = np.float32(sigma)
    if dtype == np.float32:
        return s * np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(ang)
    return float(s) * np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(ang.astype(np.float64))


# ------------------------------------------------------------------------------------------------ sim2real stages
def blur_taps(sigma):
    """Normalised taps exp(-d^2 / 2 sigma^2), d = -r .. r, r = ceil(3 sigma) (sigma the float32 parameter)."""
    s = float(np.float32(sigma))
    r = blur_radius(sigma)
    d = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-0.5 * d * d / (s * s))
    return k / k.sum()


def _blur_axis(f, k, axis):
    r = len(k) // 2
    pad = [(0, 0)] * f.ndim
    pad[axis] = (r, r)
    p = np.pad(f, pad, mode="reflect")                        # reflect-101: the edge sample is not repeated
    n = f.shape[axis]
    out = np.zeros_like(f)
    for j in range(2 * r + 1):
        sl = [slice(None)] * f.ndim
        sl[axis] = slice(j, j + n)
        out += k[j] * p[tuple(sl)]
    return out


def blur_reference(img, sigma):
    """Separable reflect-101 Gaussian of a uint8 frame [H, W, C] in float64, unrounded."""
    f = np.asarray(img).astype(np.float64)
    k = blur_taps(sigma)
    return _blur_axis(_blur_axis(f, k, 0), k, 1)


def dropout_index(n, dn):
    """Nearest-neighbour upsampling of a dn-cell mask axis to n pixels: cell = min(i * dn // n, dn - 1)."""
    return np.minimum(np.arange(n, dtype=np.int64) * int(dn) // int(n), int(dn) - 1)


def sim2real_stage(img, code, par, seed=0, mask=None):
    """One urso_sim2real_op stage on one uint8 frame [H, W, 3]: (rounded uint8, unrounded float64).  code -1 copy, 0 noise (par[0] = sigma,
    one sample per pixel for the three channels), 1 blur (par[0] = sigma; below 1e-3: copy), 2 add (par[0] integer), 3 multiply (par[0]),
    4 coarse dropout (par[0], par[1] = mask height, width; mask the first dh * dw flags of the sample's row)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    code = int(code)
    f = img.astype(np.float64)
    if code == 0:
        un = f + noise_field(seed, H * W, par[0]).reshape(H, W, 1)
    elif code == 1 and float(np.float32(par[0])) >= 1e-3:
        un = blur_reference(img, par[0])
    elif code == 2:
        un = f + float(np.float32(par[0]))
    elif code == 3:
        un = f * float(np.float32(par[0]))
    elif code == 4:
        dh, dw = int(par[0]), int(par[1])
        m = np.asarray(mask).reshape(-1)[:dh * dw].reshape(dh, dw).astype(bool)
        un = np.where(m[dropout_index(H, dh)][:, dropout_index(W, dw)][:, :, None], 0.0, f)
    else:
        un = f
    return sat_u8(un), un


def sim2real_pipeline(frames, draw, trace=None):
    """net.py:390-406 on a uint8 RGB batch [B, H, W, 3] with the decisions of `draw` (augment.sim2real_draw's dict): grey, then -- for the
    samples with apply -- the five stages in the sample's drawn order, every stage reading the previous stage's uint8 output.  Returns the
    uint8 batch; `trace` (a list) receives per slot a list of (code, par, rounded, unrounded) per sample."""
    frames = np.asarray(frames)
    out = grey3(frames)
    B = frames.shape[0]
    for slot in range(5):
        row = []
        for b in range(B):
            code = int(draw["order"][b, slot]) if draw["apply"][b] else -1
            par = draw["par"][b, draw["order"][b, slot]]
            r, un = sim2real_stage(out[b], code, par, int(draw["seeds"][b]), draw["masks"][b])
            row.append((code, par, r, un))
        for b in range(B):
            out[b] = row[b][2]
        if trace is not None:
            trace.append(row)
    return out


# ------------------------------------------------------------------------------------------------ warp
def warp_int_reference(img, Minv, interp="linear"):
    """Integer statement of cv2.warpPerspective for uint8 [H, W, C] with the destination -> source map Minv (WARP_INVERSE_MAP), border 0;
    int64 throughout after the coordinates.  [X, Y, W] = Minv [x, y, 1]; W == 0 -> (0, 0); coordinates clamped to [-2^31, 2^31 - 1] and
    rounded half to even (cvRound).  nearest: src(cvRound(X/W), cvRound(Y/W)).  linear: q = cvRound(32 X/W), pixel q >> 5, fraction q & 31 in
    1/32, the four taps weighted by the 15-bit products (32 - ax)(32 - ay) 32, ax (32 - ay) 32, (32 - ax) ay 32, ax ay 32 (sum 2^15), result
    (sum + 2^14) >> 15; taps outside the image read 0."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, C = img.shape
    M = np.asarray(Minv, dtype=np.float64).reshape(3, 3)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    X = M[0, 0] * x + M[0, 1] * y + M[0, 2]
    Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]
    Wd = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    scale = 32.0 if interp == "linear" else 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = np.where(Wd != 0.0, scale / np.where(Wd != 0.0, Wd, 1.0), 0.0)
        fx, fy = X * iw, Y * iw
    assert not (np.isnan(fx).any() or np.isnan(fy).any()), "NaN coordinates: the clamp is undefined there"
    qx = np.rint(np.clip(fx, -2147483648.0, 2147483647.0)).astype(np.int64)
    qy = np.rint(np.clip(fy, -2147483648.0, 2147483647.0)).astype(np.int64)
    src = img.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.where(inside, yy, 0), np.where(inside, xx, 0)]
        return np.where(inside[..., None], v, 0)

    if interp != "linear":
        return tap(qy, qx).astype(np.uint8)
    sx, sy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    w00, w01, w10, w11 = (32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32
    acc = w00[..., None] * tap(sy, sx) + w01[..., None] * tap(sy, sx + 1) + w10[..., None] * tap(sy + 1, sx) + w11[..., None] * tap(sy + 1, sx + 1)
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def warp_reference(img, Minv, interp="linear", rows=None):
    """Both statements of the warp for one frame: (oracle.pose_math.warp_perspective -- the primary, a per-pixel Python loop, evaluated on
    the destination rows `rows` only when given -- , warp_int_reference on every pixel)."""
    from oracle import pose_math as P
    return P.warp_perspective(img, Minv, inverse_map=True, interp=interp, rows=rows), warp_int_reference(img, Minv, interp)


# ------------------------------------------------------------------------------------------------ mold
def bf16_bits(f32):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even (finite inputs)."""
    b = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def mold_bits(img_u8, mean, dt):
    """urso_mold_images on uint8 frames: float32(pixel) - float32(mean) in float32, rounded once to the 16-bit type (dt 1 bf16, 2 fp16), a zero
    fourth channel; the stored 16-bit patterns [..., 4] as uint16."""
    f = np.asarray(img_u8).astype(np.float32)
    if mean is not None:
        f = f - np.asarray(mean, dtype=np.float32)
    bits = bf16_bits(f) if dt == 1 else f.astype(np.float16).view(np.uint16)
    out = np.zeros(f.shape[:-1] + (4,), dtype=np.uint16)
    out[..., :3] = bits
    return out


# ------------------------------------------------------------------------------------------------ pipeline, teacher-forced
def handmade_draw(B, H, W, seed=0):
    """A hand-made draw: applied and skipped samples, five different stage orders (noise first, noise last), masks of different sizes."""
    rng = np.random.RandomState(seed)
    orders = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 4, 0, 2, 3], [2, 0, 3, 4, 1], [3, 1, 4, 0, 2]]
    sizes = [(1, 1), (int(0.1 * H), int(0.1 * W)), (3, 5), (2, 7), (5, 2)]
    apply = np.array([(i % 3) != 2 for i in range(B)])
    order = np.tile(np.arange(5), (B, 1))
    par = np.zeros((B, 5, 4), dtype=np.float32)
    seeds = np.zeros(B, dtype=np.uint32)
    masks = []
    k = 0
    for i in range(B):
        par[i, 0, 0] = 0.01 * 255
        par[i, 4, 0], par[i, 4, 1] = 1, 1
        if not apply[i]:
            masks.append(np.zeros((1, 1), dtype=bool))
            continue
        order[i] = orders[k % 5]
        par[i, 1, 0] = (0.34, 1.0, 1.5, 0.0005, 0.8)[k % 5]
        par[i, 2, 0] = (-20, 20, 7, -3, 13)[k % 5]
        par[i, 3, 0] = (0.5, 2.0, 1.7183, 0.8317, 1.2113)[k % 5]
        dh, dw = sizes[k % 5]
        par[i, 4, 0], par[i, 4, 1] = dh, dw
        m = rng.rand(dh, dw) < 0.3
        m.reshape(-1)[0] = (k % 2 == 0)
        masks.append(m)
        seeds[i] = (0x80000000 | rng.randint(0, 2 ** 31 - 1)) if k % 2 else rng.randint(0, 2 ** 31 - 1)
        k += 1
    return {"apply": apply, "order": order, "par": par, "seeds": seeds, "masks": masks}


def judge_pipeline_teacher_forced(grey, outs, draw, what="pipeline", check_share=True):
    """The five launches of augment.sim2real_batch judged one at a time: the reference stage of every sample is fed the batch the DEVICE (or a
    simulation) produced in the previous launch -- a one-level difference at a tie in stage k is a legitimate input of stage k + 1 -- and
    its output compared off ties with the stage's own delta.  grey: the batch after urso_rgb_to_grey3; outs: the batch after each launch.
    Returns (the figures per op code, the number of excused elements per sample)."""
    assert len(outs) == 5
    per_code = {}
    excused = np.zeros(len(grey), dtype=np.int64)
    for slot in range(5):
        prev = grey if slot == 0 else outs[slot - 1]
        for b in range(len(grey)):
            op = int(draw["order"][b, slot])
            code = op if draw["apply"][b] else -1
            par = draw["par"][b, op]
            ref, un = sim2real_stage(prev[b], code, par, int(draw["seeds"][b]), draw["masks"][b])
            delta = stage_delta(code, par)
            if delta > 0 and check_share:                     # (a frame of a few thousand pixels is too small for the share to be a stable figure)
                assert tie_share(un, delta) <= 4 * delta, (what, slot, b, code, tie_share(un, delta), delta)
            st = assert_equal_off_ties(outs[slot][b], ref, un, delta, 4 * delta, "%s slot %d sample %d code %d" % (what, slot, b, code))
            agg = per_code.setdefault(code, {"what": "%s code %d" % (what, code), "n": 0, "excused": 0, "delta": 0.0, "cap": 0.0})
            agg["n"] += st["n"]; agg["excused"] += st["excused"]; excused[b] += st["excused"]
            agg["delta"] = max(agg["delta"], st["delta"]); agg["cap"] = max(agg["cap"], st["cap"])
    return [per_code[c] for c in sorted(per_code)], excused


# ------------------------------------------------------------------------------------------------ warp edge maps
def _shift_check(tx, ty):
    """Expected result of the pure translation dst(x, y) = src(x + tx, y + ty), tx / ty integers or integers + 0.5: shifted integer averages
    with the .5 of the fixed-point sum rounded up ((a + b + 1) >> 1, (a + b + c + d + 2) >> 2), zero taps outside.  Linear only when fractional."""
    ix, iy = int(np.floor(tx)), int(np.floor(ty))
    hx, hy = tx != ix, ty != iy

    def check(img, out, interp):
        if (hx or hy) and interp != "linear":
            return
        H, W, C = img.shape
        big = np.zeros((H + 2, W + 2, C), dtype=np.int64)

        def shifted(dy, dx):                                   # src(x + ix + dx, y + iy + dy) on the destination grid, 0 outside
            o = np.zeros((H, W, C), dtype=np.int64)
            ys, xs = np.arange(H) + iy + dy, np.arange(W) + ix + dx
            vy, vx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            if vy.any() and vx.any():
                o[np.ix_(vy, vx)] = img[np.ix_(ys[vy], xs[vx])]
            return o
        del big
        a = shifted(0, 0)
        if hx and hy:
            exp = (a + shifted(0, 1) + shifted(1, 0) + shifted(1, 1) + 2) >> 2
        elif hx:
            exp = (a + shifted(0, 1) + 1) >> 1
        elif hy:
            exp = (a + shifted(1, 0) + 1) >> 1
        else:
            exp = a
        assert np.array_equal(out, exp.astype(np.uint8)), "translation (%g, %g)" % (tx, ty)
    return check


def warp_edge_maps(H, W):
    """Hand-built destination -> source maps for the edges of the warp: name -> (3x3 map, check(img, out, interp) or None)."""
    x0 = 8
    maps = {}

    def w_zero(img, out, interp):                              # W == 0 -> coordinates (0, 0): the column reads src(0, 0) exactly
        assert np.array_equal(out[:, x0], np.broadcast_to(img[0, 0], out[:, x0].shape))
    maps["w_zero_on_a_column"] = (np.array([[1.0, 0, 0], [0, 1.0, 0], [0.125, 0, -0.125 * x0]]), w_zero)
    c = W / 2 - 0.5                                            # W = (x - c) / 4: negative on the left half, never zero; X / W = 10 + 1 / W
    maps["w_negative_on_half"] = (np.array([[2.5, 0, -2.5 * c + 1.0], [0, 0.25, 0], [0.25, 0, -0.25 * c]]), None)

    def overflow(img, out, interp):                            # everything clamps to +-2^31 and reads 0, except the pixel mapped to (0, 0)
        exp = np.zeros_like(out); exp[3, 5] = img[0, 0]
        assert np.array_equal(out, exp)
    maps["past_2_31"] = (np.array([[1e10, 0, -5e10], [0, -1e10, 3e10], [0, 0, 1.0]]), overflow)
    for name, tx, ty in (("tap_at_minus_1", -1.0, 0.0), ("tap_at_minus_1_half", -1.5, 0.0), ("tap_at_w_minus_1", W - 1.0, 0.0),
                         ("tap_at_w_minus_1_half", W - 1.5, 0.0), ("tap_at_32767", 32767.0, 0.0), ("tap_at_32768_half", 32767.5, 0.0),
                         ("tap_at_32768", 32768.0, 0.0), ("half_x", 0.5, 0.0), ("half_y", 0.0, 0.5), ("half_xy", 0.5, 0.5),
                         ("half_xy_shifted", 2.5, -3.5)):
        maps[name] = (np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]]), _shift_check(tx, ty))
    return maps
