// utils.resize_image (utils.py:398-511: skimage.transform.resize(order=1, mode='constant', preserve_range=True) + zero padding) for a whole
// uint8 batch on the device, BYTE-EXACT to ursonet_amd/utils.py::_bilinear_resize.  That host function is a fixed sequence of IEEE float64
// multiplies and adds per pixel; the kernel performs the same operations in the same order, so it gets the same bits.  Everything
// transcendental or geometric (Gaussian taps, source index and fraction per output row / column) is computed by the host with the very
// expressions _bilinear_resize uses (utils.resize_tables) and arrives as small fp64 / int32 tables: no exp, no division here.
//
// The one thing that silently breaks the equality is fused multiply-add: hipcc contracts a*b+c into v_fma_f64 by default, which rounds
// once where NumPy rounds twice.  Contraction is therefore switched off for this file (the pragma below; the library's build flags say
// -ffp-contract=off as well) -- do not remove either.
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>
#include <type_traits>

// One workgroup (256 threads) per TH x TW tile of the OUTPUT frame.
//   phase 1  the row-smoothed source patch the tile's bilinear taps can touch -- rows ya .. ya+nr-1, columns xa .. xa+nc-1 (the column
//            pass' halo of rx included) -- goes into LDS: S1[y][x] = sum_i ky[i] * src[y - ry + i][x] in tap order, zero outside the frame
//            (bytes when the passes truncate, "0.18"; fp64 otherwise, "0.19").  The source bytes are read straight from global memory:
//            a byte is needed by 2 ry + 1 rows of the same patch, so all but the first read hit L1 / L2, and the patch needs no LDS copy.
//   phase 2  every output byte of the tile: the column pass at its 2 x 2 neighbours from S1 (at scale <= 1/2 no smoothed value is
//            shared between two outputs, so it is not stored), then ((v00 (1-fx) + v01 fx)(1-fy) + (v10 (1-fx) + v11 fx) fy), truncated.
// Every LDS index is checked against the patch, every global index against the frame: tables that do not describe a resize give wrong
// pixels, never an access out of bounds.
struct RszArgs {
    int H, W, C, NH, NW, OH, OW, top, left, ry, rx, TH, TW, capR, capC;
    const double *ky, *kx, *fy, *fx;
    const int32_t *y0, *x0;
    const uint8_t* src;
    uint8_t* dst;
};

template <bool TRUNC>
__global__ __launch_bounds__(256) void resize_kernel(RszArgs a) {
    typedef typename std::conditional<TRUNC, uint8_t, double>::type S1T;
    extern __shared__ double rsz_lds[];
    S1T* s1 = (S1T*)rsz_lds;
    const int H = a.H, W = a.W, C = a.C, rx = a.kx ? a.rx : 0, ry = a.ky ? a.ry : 0;
    const int OY = blockIdx.y * a.TH, OX = blockIdx.x * a.TW;
    const uint8_t* img = a.src + (size_t)blockIdx.z * H * W * C;
    uint8_t* out = a.dst + (size_t)blockIdx.z * a.OH * a.OW * C;
    // rows / columns of the rescaled window [0,NH) x [0,NW) this tile covers
    const int j0 = max(OY - a.top, 0), j1 = min(OY + a.TH - a.top, a.NH), i0 = max(OX - a.left, 0), i1 = min(OX + a.TW - a.left, a.NW);
    int ya = 0, xa = 0, nr = 0, nc = 0;
    if (j0 < j1 && i0 < i1) {
        ya = a.y0[j0]; nr = min(a.capR, max(a.y0[j1 - 1] + 2 - ya, 0));
        xa = a.x0[i0] - rx; nc = min(a.capC, max(a.x0[i1 - 1] + 2 + rx - xa, 0));
    }
    const int stride = nc * C;
    for (int e = threadIdx.x; e < nr * stride; e += 256) {
        const int r = e / stride, q = e - r * stride, cx = q / C, c = q - cx * C;
        const int y = ya + r, x = xa + cx;
        double acc = 0.0;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            if (a.ky) {
                for (int i = 0; i <= 2 * ry; ++i) {
                    const int yy = y - ry + i;
                    if ((unsigned)yy < (unsigned)H) acc = acc + a.ky[i] * (double)img[((size_t)yy * W + x) * C + c];
                }
                if (TRUNC) acc = trunc(acc);
            } else acc = (double)img[((size_t)y * W + x) * C + c];
        }
        s1[e] = (S1T)acc;
    }
    __syncthreads();
    const int tw = a.TW * C;
    for (int e = threadIdx.x; e < a.TH * tw; e += 256) {
        const int ty = e / tw, q = e - ty * tw, tx = q / C, c = q - tx * C;
        const int oy = OY + ty, ox = OX + tx;
        if (oy >= a.OH || ox >= a.OW) continue;
        const int j = oy - a.top, i = ox - a.left;
        uint8_t res = 0;
        if ((unsigned)j < (unsigned)a.NH && (unsigned)i < (unsigned)a.NW) {
            const int yy0 = a.y0[j], xx0 = a.x0[i];
            const double fy = a.fy[j], fx = a.fx[i];
            double v[2][2];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int yy = yy0 + dy, xx = xx0 + dx, r = yy - ya;
                    double acc = 0.0;
                    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W && (unsigned)r < (unsigned)nr) {
                        const S1T* row = s1 + r * stride + c;
                        if (a.kx) {
                            for (int t = 0; t <= 2 * rx; ++t) {
                                const int xs = xx - rx + t, cx = xs - xa;
                                if ((unsigned)xs < (unsigned)W && (unsigned)cx < (unsigned)nc) acc = acc + a.kx[t] * (double)row[cx * C];
                            }
                            if (TRUNC) acc = trunc(acc);
                        } else {
                            const int cx = xx - xa;
                            if ((unsigned)cx < (unsigned)nc) acc = (double)row[cx * C];
                        }
                    }
                    v[dy][dx] = acc;
                }
            const double val = (v[0][0] * (1 - fx) + v[0][1] * fx) * (1 - fy) + (v[1][0] * (1 - fx) + v[1][1] * fx) * fy;
            res = (uint8_t)val;                                              // float64 -> uint8 assignment: truncation
        }
        out[((size_t)oy * a.OW + ox) * C + c] = res;
    }
}

#define RSZ_LDS_MAX 65536

extern "C" int urso_resize_images_u8(int B, int H, int W, int C, int NH, int NW, int OH, int OW, int top, int left,
                                     const double* ky_d, int ry, const double* kx_d, int rx, const int32_t* y0_d, const double* fy_d,
                                     const int32_t* x0_d, const double* fx_d, int trunc_passes, const uint8_t* src_d, uint8_t* dst_d, void* stream) {
    if (!src_d || !dst_d || !y0_d || !fy_d || !x0_d || !fx_d) { urso_set_error("urso_resize_images_u8: null pointer"); return URSO_EINVAL; }
    if (src_d == dst_d) { urso_set_error("urso_resize_images_u8: src and dst must differ"); return URSO_EINVAL; }
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0 || NH <= 0 || NW <= 0 || OH <= 0 || OW <= 0) {
        urso_set_error("urso_resize_images_u8: sizes must be positive (B <= 65535)"); return URSO_EINVAL;
    }
    if (top < 0 || left < 0 || (long long)top + NH > OH || (long long)left + NW > OW) {
        urso_set_error("urso_resize_images_u8: window (%d, %d) + %d x %d outside the %d x %d output", top, left, NH, NW, OH, OW); return URSO_EINVAL;
    }
    if ((ky_d && ry < 1) || (kx_d && rx < 1) || (trunc_passes != 0 && trunc_passes != 1)) {
        urso_set_error("urso_resize_images_u8: a tap table needs a radius >= 1; trunc_passes is 0 or 1"); return URSO_EINVAL;
    }
    RszArgs a;
    a.H = H; a.W = W; a.C = C; a.NH = NH; a.NW = NW; a.OH = OH; a.OW = OW; a.top = top; a.left = left;
    a.ry = ky_d ? ry : 0; a.rx = kx_d ? rx : 0;
    a.ky = ky_d; a.kx = kx_d; a.fy = fy_d; a.fx = fx_d; a.y0 = y0_d; a.x0 = x0_d; a.src = src_d; a.dst = dst_d;
    // Tile: the largest of the list whose S1 patch fits.  T consecutive outputs span at most ceil((T-1) n_in / n_out) + 2 source rows
    // (floor(b) - floor(a) <= ceil(b - a), plus the +1 neighbour); one more for the rounding of the table's own arithmetic.
    static const int tiles[][2] = {{16, 32}, {8, 32}, {8, 16}, {4, 16}, {4, 8}, {2, 4}, {1, 2}, {1, 1}};
    size_t lds = 0;
    bool found = false;
    for (size_t t = 0; t < sizeof(tiles) / sizeof(tiles[0]) && !found; ++t) {
        a.TH = tiles[t][0]; a.TW = tiles[t][1];
        const long long capR = ((long long)(a.TH - 1) * H + NH - 1) / NH + 3, capC = ((long long)(a.TW - 1) * W + NW - 1) / NW + 3 + 2LL * a.rx;
        const long long need = capR * capC * C * (trunc_passes ? 1 : 8);
        if (need <= RSZ_LDS_MAX) { a.capR = (int)capR; a.capC = (int)capC; lds = (size_t)((need + 7) & ~7LL); found = true; }
    }
    if (!found) { urso_set_error("urso_resize_images_u8: %d x %d -> %d x %d (radii %d, %d): one output pixel needs more than %d bytes of LDS", H, W, NH, NW, a.ry, a.rx, RSZ_LDS_MAX); return URSO_EINVAL; }
    const long long gx = (OW + a.TW - 1) / a.TW, gy = (OH + a.TH - 1) / a.TH;
    if (gy > 65535 || gx > 2147483647LL) { urso_set_error("urso_resize_images_u8: output too large for the tile grid"); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    // profiled under URSO_K_MOLD like urso_pad_images_u8 (the opt-in profiler has no id of its own for the input side); the byte figure
    // is the algorithmic one: the source counted once, although phase 1 reads each byte 2 ry + 1 times (all but the first from cache)
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * C * ((double)H * W + (double)OH * OW));
    if (trunc_passes) URSO_KLAUNCH(resize_kernel<true>, dim3((unsigned)gx, (unsigned)gy, B), dim3(256), lds, st, a);
    else URSO_KLAUNCH(resize_kernel<false>, dim3((unsigned)gx, (unsigned)gy, B), dim3(256), lds, st, a);
    return urso_check_launch("urso_resize_images_u8");
}
