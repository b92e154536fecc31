// The video path of the reference's `test` command (pose_estimator.detect_video, pose_estimator.py:606-745) around the network:
//   urso_video_prep_u8   crop + zero pad + grey mix of a uint8 batch in one pass (pose_estimator.py:641-645), BYTE-EXACT to
//                        ursonet_amd/video.py::VideoPrep.host.  The mix is (w0 R + w1 G) + w2 B in IEEE float64, two roundings per
//                        multiply-add as NumPy performs them, truncated to uint8.  27,801 of the 2^24 RGB triples change their byte when
//                        a multiply and an add are fused, so contraction is off for this file (the pragma below; the library's build
//                        flags say -ffp-contract=off as well) -- do not remove either.
//   urso_draw_prims_u8   an exact integer rasteriser (segments with thickness, filled discs) that draws the pose axes onto frames that
//                        exist only on the device (utils.plot_axes, utils.py:186-217, without OpenCV).
// Plain C++ with vector stores only.
#pragma clang fp contract(off)
#include "common.h"

// ---------------------------------------------------------------- prep
// The padded border is most of the output (a 960 x 1129 crop inside 1760 x 1929), so the kernel is organised around its STORES: one
// thread owns 16 consecutive output bytes of a frame and issues one aligned 16-byte store; a wave writes 1 KiB contiguously.  OW * 3 is
// in general no multiple of 4 and a frame's first byte sits wherever B frames of OH * OW * 3 bytes put it, so rows and frames do not
// start aligned: per frame, the bytes before the first 16-byte boundary (head) and behind the last whole vector (tail) are stored one by
// one by block 0, as frame_cache.hip does.  A thread finds the pixel of its first byte with two 32-bit divisions and then walks; vectors
// that lie in the border altogether skip the walk.  Every source index is checked against the frame, every output offset is below the
// frame's size by construction (vector v covers [head + 16 v, head + 16 v + 16) with v < (n - head) / 16).
struct VprepArgs {
    int H, W, OH, OW, top, left, ch, cw, pad;      // ch x cw: the cropped frame
    double w0, w1, w2;
    const uint8_t* src;
    uint8_t* dst;
};

#define VPREP_THREADS 256

// grey byte of output pixel (oy, ox); 0 in the border
__device__ __forceinline__ uint32_t vprep_pixel(const VprepArgs& a, const uint8_t* img, int oy, int ox) {
    const int y = oy - a.pad, x = ox - a.pad;
    if ((unsigned)y >= (unsigned)a.ch || (unsigned)x >= (unsigned)a.cw) return 0u;
    const int sy = y + a.top, sx = x + a.left;
    if ((unsigned)sy >= (unsigned)a.H || (unsigned)sx >= (unsigned)a.W) return 0u;
    const uint8_t* s = img + ((size_t)sy * a.W + sx) * 3;
    const double v = (a.w0 * (double)s[0] + a.w1 * (double)s[1]) + a.w2 * (double)s[2];
    return (uint32_t)(uint8_t)v;                                         // float64 -> uint8 assignment: truncation
}

__global__ __launch_bounds__(VPREP_THREADS) void video_prep_kernel(VprepArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint32_t row3 = (uint32_t)a.OW * 3u, n = (uint32_t)a.OH * row3;        // n < 2^31 (host check)
    const uint8_t* img = a.src + (size_t)b * a.H * a.W * 3;
    uint8_t* out = a.dst + (size_t)b * n;
    const uint32_t head = min(n, (16u - ((uint32_t)(uintptr_t)out & 15u)) & 15u);
    const uint32_t nv = (n - head) >> 4;
    if (blockIdx.x == 0) {                                               // head and tail bytes, one per thread
        const uint32_t tail0 = head + (nv << 4);
        uint32_t r = n;
        if ((uint32_t)tid < head) r = tid;
        else if (tid >= 64 && tail0 + (uint32_t)(tid - 64) < n) r = tail0 + (uint32_t)(tid - 64);
        if (r < n) {
            const uint32_t oy = r / row3, q = r - oy * row3;
            out[r] = (uint8_t)vprep_pixel(a, img, (int)oy, (int)(q / 3u));
        }
    }
    const uint32_t v = blockIdx.x * VPREP_THREADS + tid;
    if (v >= nv) return;
    const uint32_t r = head + (v << 4);                                  // r + 15 < n
    uint32_t oy = r / row3;
    const uint32_t q = r - oy * row3;
    uint32_t ox = q / 3u, c = q - ox * 3u;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    // the rows and byte columns the 16 bytes can touch: [oy, oy_last], and within ONE row [q, q + 15]
    const uint32_t oy_last = (r + 15u) / row3;
    const uint32_t lo = (uint32_t)a.pad, hi_y = (uint32_t)a.pad + (uint32_t)a.ch, hi_q = ((uint32_t)a.pad + (uint32_t)a.cw) * 3u;
    const bool border = oy_last < lo || oy >= hi_y || (oy == oy_last && (q + 15u < lo * 3u || q >= hi_q));
    if (!border) {
        uint32_t val = vprep_pixel(a, img, (int)oy, (int)ox);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            w[k >> 2] |= val << (8 * (k & 3));
            if (++c == 3u) {
                c = 0u;
                if (++ox == (uint32_t)a.OW) { ox = 0u; ++oy; }
                if (k < 15) val = vprep_pixel(a, img, (int)oy, (int)ox);         // oy <= oy_last < OH while bytes remain
            }
        }
    }
    *(uint4*)(out + r) = make_uint4(w[0], w[1], w[2], w[3]);             // out + r is 16-byte aligned: r = head mod 16
}

extern "C" int urso_video_prep_u8(int B, int H, int W, int top, int bottom, int left, int right, int pad, double w0, double w1, double w2,
                                  const uint8_t* src_d, uint8_t* dst_d, void* stream) {
    if (!src_d || !dst_d) { urso_set_error("urso_video_prep_u8: null pointer"); return URSO_EINVAL; }
    if (src_d == dst_d) { urso_set_error("urso_video_prep_u8: src and dst must differ"); return URSO_EINVAL; }
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0) { urso_set_error("urso_video_prep_u8: sizes must be positive (B <= 65535)"); return URSO_EINVAL; }
    if (top < 0 || bottom < 0 || left < 0 || right < 0 || pad < 0) {
        urso_set_error("urso_video_prep_u8: negative crop (%d, %d, %d, %d) or pad %d", top, bottom, left, right, pad); return URSO_EINVAL;
    }
    const long long ch = (long long)H - top - bottom, cw = (long long)W - left - right;
    if (ch <= 0 || cw <= 0) {
        urso_set_error("urso_video_prep_u8: crop (%d, %d, %d, %d) leaves no pixel of a %d x %d frame", top, bottom, left, right, H, W); return URSO_EINVAL;
    }
    const long long OH = ch + 2LL * pad, OW = cw + 2LL * pad;
    if (OH >= (1LL << 31) || OW >= (1LL << 31) || (double)OH * (double)OW * 3.0 >= 2147483648.0 || (long long)H * W * 3 >= (1LL << 31)) {
        urso_set_error("urso_video_prep_u8: a frame of 2 GiB or more (%lld x %lld x 3 out, %d x %d x 3 in)", OH, OW, H, W); return URSO_EINVAL;
    }
    VprepArgs a;
    a.H = H; a.W = W; a.OH = (int)OH; a.OW = (int)OW; a.top = top; a.left = left; a.ch = (int)ch; a.cw = (int)cw; a.pad = pad;
    a.w0 = w0; a.w1 = w1; a.w2 = w2; a.src = src_d; a.dst = dst_d;
    const long long n = OH * OW * 3;
    const unsigned chunks = (unsigned)((n >> 4) / VPREP_THREADS + 1);   // a frame has at most n / 16 whole vectors
    hipStream_t st = (hipStream_t)stream;
    // profiled under URSO_K_MOLD like the other input-side kernels (resize.hip); bytes: the cropped source once + the whole output
    ProfScope ps(st, URSO_K_MOLD, 5.0 * B * (double)ch * cw, (double)B * (3.0 * ch * cw + (double)n));
    URSO_KLAUNCH(video_prep_kernel, dim3(chunks, (unsigned)B), dim3(VPREP_THREADS), 0, st, a);
    return urso_check_launch("urso_video_prep_u8");
}

// ---------------------------------------------------------------- rasteriser
// One thread per pixel of an 8-row x 32-column tile; the frame's primitives sit in LDS.  A primitive whose bounding box (grown by its
// radius / thickness) misses the pixel is skipped before any 64-bit arithmetic -- a necessary condition of both rules, so the painted set
// is exactly the rules'.  The LAST primitive of the list that covers a pixel gives its colour; pixels no primitive covers are not
// written.  With |coordinate| <= 16,384 and a pixel inside a frame of H, W <= 16,384 (both checked by the host entry): every component
// of w = p - a is below 2^15 in magnitude and every component of D = b - a at most 2^15, so |w|^2 < 2^31, |D|^2 <= 2^31, and
// |w|^2 |D|^2, s^2 and their difference stay below 2^62 (see seg_covers for the factor 4).
#define DRAW_TW 32
#define DRAW_TH 8

__device__ __forceinline__ bool seg_covers(long long px, long long py, const int32_t* p) {
    const long long ax = p[1], ay = p[2], bx = p[3], by = p[4], t = p[5];
    const long long Dx = bx - ax, Dy = by - ay, wx = px - ax, wy = py - ay;
    const long long s = wx * Dx + wy * Dy, DD = Dx * Dx + Dy * Dy, tt = t * t;
    if (s <= 0) return 4 * (wx * wx + wy * wy) <= tt;
    if (s >= DD) { const long long ux = px - bx, uy = py - by; return 4 * (ux * ux + uy * uy) <= tt; }
    // 4 (|w|^2 |D|^2 - s^2) <= t^2 |D|^2.  The left side is 4 x an integer A >= 0; A <= floor(T / 4) is the same statement without the
    // factor that could leave int64 (T = t^2 |D|^2 <= 2^28 2^31).
    const long long A = (wx * wx + wy * wy) * DD - s * s;
    return A <= ((tt * DD) >> 2);
}

__global__ __launch_bounds__(DRAW_TW * DRAW_TH) void draw_prims_kernel(int H, int W, const int32_t* prims, const int32_t* counts, uint8_t* img) {
    __shared__ int32_t sp[URSO_DRAW_MAX_PRIMS * URSO_DRAW_PRIM_INTS];
    const int b = blockIdx.z, tid = threadIdx.y * DRAW_TW + threadIdx.x;
    const int n = min(max(counts[b], 0), URSO_DRAW_MAX_PRIMS);
    for (int e = tid; e < n * URSO_DRAW_PRIM_INTS; e += DRAW_TW * DRAW_TH) sp[e] = prims[(size_t)b * URSO_DRAW_MAX_PRIMS * URSO_DRAW_PRIM_INTS + e];
    __syncthreads();
    const int x = blockIdx.x * DRAW_TW + threadIdx.x, y = blockIdx.y * DRAW_TH + threadIdx.y;
    if (x >= W || y >= H) return;
    int hit = -1;
    for (int i = 0; i < n; ++i) {
        const int32_t* p = sp + i * URSO_DRAW_PRIM_INTS;
        const int r = p[5];
        bool in = false;
        if (p[0] == URSO_DRAW_SEGMENT) {
            if (r >= 0 && x >= min(p[1], p[3]) - r && x <= max(p[1], p[3]) + r && y >= min(p[2], p[4]) - r && y <= max(p[2], p[4]) + r)
                in = seg_covers(x, y, p);
        } else if (p[0] == URSO_DRAW_DISC) {
            if (r >= 0 && x >= p[1] - r && x <= p[1] + r && y >= p[2] - r && y <= p[2] + r) {
                const long long dx = x - p[1], dy = y - p[2];
                in = dx * dx + dy * dy <= (long long)r * r;
            }
        }
        if (in) hit = i;
    }
    if (hit < 0) return;
    const int32_t* p = sp + hit * URSO_DRAW_PRIM_INTS;
    uint8_t* o = img + (((size_t)b * H + y) * W + x) * 3;               // x < W, y < H, b < B
    o[0] = (uint8_t)p[6]; o[1] = (uint8_t)p[7]; o[2] = (uint8_t)p[8];
}

extern "C" int urso_draw_prims_u8(int B, int H, int W, const int32_t* prims_host, const int32_t* counts_host, const int32_t* prims_d,
                                  const int32_t* counts_d, uint8_t* img_d, void* stream) {
    if (!prims_host || !counts_host || !prims_d || !counts_d || !img_d) { urso_set_error("urso_draw_prims_u8: null pointer"); return URSO_EINVAL; }
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > URSO_DRAW_COORD_MAX || W > URSO_DRAW_COORD_MAX) {
        urso_set_error("urso_draw_prims_u8: 1 <= B <= 65535 and 1 <= H, W <= %d (B %d, H %d, W %d)", URSO_DRAW_COORD_MAX, B, H, W); return URSO_EINVAL;
    }
    bool any = false;
    for (int b = 0; b < B; ++b) {
        const int n = counts_host[b];
        if (n < 0 || n > URSO_DRAW_MAX_PRIMS) { urso_set_error("urso_draw_prims_u8: frame %d has %d primitives (0 .. %d)", b, n, URSO_DRAW_MAX_PRIMS); return URSO_EINVAL; }
        any = any || n > 0;
        for (int i = 0; i < n; ++i) {
            const int32_t* p = prims_host + ((size_t)b * URSO_DRAW_MAX_PRIMS + i) * URSO_DRAW_PRIM_INTS;
            if (p[0] != URSO_DRAW_SEGMENT && p[0] != URSO_DRAW_DISC) { urso_set_error("urso_draw_prims_u8: frame %d primitive %d: unknown kind %d", b, i, p[0]); return URSO_EINVAL; }
            for (int k = 1; k <= 5; ++k)
                if (p[k] > URSO_DRAW_COORD_MAX || p[k] < -URSO_DRAW_COORD_MAX || (k == 5 && p[k] < 0)) {
                    urso_set_error("urso_draw_prims_u8: frame %d primitive %d: coordinate %d outside +-%d (or a negative radius)", b, i, p[k], URSO_DRAW_COORD_MAX);
                    return URSO_EINVAL;
                }
            for (int k = 6; k <= 8; ++k)
                if (p[k] < 0 || p[k] > 255) { urso_set_error("urso_draw_prims_u8: frame %d primitive %d: colour %d outside 0 .. 255", b, i, p[k]); return URSO_EINVAL; }
        }
    }
    if (!any) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * H * W * 3);            // upper bound: every pixel painted
    URSO_KLAUNCH(draw_prims_kernel, dim3((W + DRAW_TW - 1) / DRAW_TW, (H + DRAW_TH - 1) / DRAW_TH, B), dim3(DRAW_TW, DRAW_TH), 0, st, H, W,
                 prims_d, counts_d, img_d);
    return urso_check_launch("urso_draw_prims_u8");
}
