// The PMF picture of the reference's `test` command on a dataset (utils.visualize_weights, utils.py:117-151; ursonet_amd/detect.py):
//   urso_pmf_sheet_u8   the two-row "slice sheet" of a batch of n^3-bin orientation PMFs as uint8 RGB, on the device.
// Two launches.  pmf_index_kernel: one block per (image, source row) takes the maximum over the K = n^3 bins and writes every bin's 8-bit
// colour index (fp64 value rule, include/ursonet_hip.h) into the caller's scratch.  pmf_sheet_kernel: the expansion of those K bytes to
// 3 cell^2 K and more output bytes, organised around its stores as video_prep_kernel is.
// Plain C++ with vector stores only.
#include "common.h"

#define PMF_THREADS 256

struct PmfArgs {
    int n, n2, K, cell, gap, rows, SW, SH;
    int band, span;                                // n * cell + gap: distance between two slices / two source rows; n * cell: pixels of one
    const float* src[2];                           // source of row 0 / row 1; est[r] != 0: logits
    int est[2];
    uint32_t bg;                                   // R | G << 8 | B << 16
    const uint8_t* lut;
    uint8_t* idx;                                  // [B][rows][K]
    uint8_t* out;
};

// ---------------------------------------------------------------- indices
// GT row: v = p / max p (p < 0 or NaN counts as 0; max 0: every v is 0).  Estimate row: v = exp(z - max z), the softmax divided by its own
// maximum -- the sum cancels.  index = min(255, floor(256 v)), all in fp64: the division is IEEE, 256 v is exact.
__global__ __launch_bounds__(PMF_THREADS) void pmf_index_kernel(PmfArgs a) {
    __shared__ float red[PMF_THREADS / 64];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const bool est = a.est[r] != 0;
    const float* s = a.src[r] + (size_t)b * a.K;
    float m = est ? -INFINITY : 0.0f;
    for (int k = tid; k < a.K; k += PMF_THREADS) {                     // K = 32,768 at n = 32: 128 passes of the block
        const float x = s[k];
        if (x > m) m = x;                                                // a NaN never compares greater; GT: nothing below 0 counts
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < PMF_THREADS / 64; ++w) m = fmaxf(m, red[w]);
    const double md = (double)m;
    uint8_t* o = a.idx + ((size_t)b * a.rows + r) * a.K;                // k < K below
    for (int k = tid; k < a.K; k += PMF_THREADS) {
        const float x = s[k];
        double v;
        if (est) v = exp((double)x - md);
        else v = (x > 0.0f && m > 0.0f) ? (double)x / md : 0.0;
        if (!(v >= 0.0)) v = 0.0;                                        // NaN logit, or a row of -inf
        const double t = 256.0 * v;
        o[k] = (uint8_t)(t >= 255.0 ? 255 : (int)t);                     // t >= 0: the conversion is floor
    }
}

// ---------------------------------------------------------------- expansion
// One thread owns 16 consecutive output bytes of an image and issues one aligned 16-byte store; SW * 3 is in general no multiple of 16 and
// `out` may sit at any address, so per image the bytes before the first 16-byte boundary (head) and behind the last whole vector (tail)
// are stored one by one by block 0 (video_prep_kernel's scheme).  The 256 LUT entries and the background are packed colours in LDS.
// Every index read is idx[(b * rows + r) * K + i n^2 + j n + z] with r < rows and i, j, z < n; every output offset is below the image's
// size by construction (vector v covers [head + 16 v, head + 16 v + 16) with v < (bytes - head) / 16).
struct PmfRow { int r, j; };                       // source row and bin row of a pixel row; r < 0: background

__device__ __forceinline__ PmfRow pmf_row(const PmfArgs& a, int y) {
    const int ry = y - a.gap;
    if (ry < 0) return { -1, 0 };
    const int r = ry / a.band, jy = ry - r * a.band;
    if (r >= a.rows || jy >= a.span) return { -1, 0 };
    return { r, jy / a.cell };
}

__device__ __forceinline__ uint32_t pmf_pixel(const PmfArgs& a, const uint32_t* lut, const uint8_t* idx, PmfRow row, int x) {
    const int rx = x - a.gap;
    if (row.r < 0 || rx < 0) return a.bg;
    const int z = rx / a.band, ix = rx - z * a.band;
    if (z >= a.n || ix >= a.span) return a.bg;
    const int i = ix / a.cell;
    return lut[idx[(size_t)row.r * a.K + i * a.n2 + row.j * a.n + z]];
}

__global__ __launch_bounds__(PMF_THREADS) void pmf_sheet_kernel(PmfArgs a) {
    __shared__ uint32_t lut[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    lut[tid] = (uint32_t)a.lut[tid * 3] | ((uint32_t)a.lut[tid * 3 + 1] << 8) | ((uint32_t)a.lut[tid * 3 + 2] << 16);   // PMF_THREADS == 256
    __syncthreads();
    const uint32_t row3 = (uint32_t)a.SW * 3u, nb = (uint32_t)a.SH * row3;       // nb < 2^31 (host check)
    const uint8_t* idx = a.idx + (size_t)b * a.rows * a.K;
    uint8_t* out = a.out + (size_t)b * nb;
    const uint32_t head = min(nb, (16u - ((uint32_t)(uintptr_t)out & 15u)) & 15u);
    const uint32_t nv = (nb - head) >> 4;
    if (blockIdx.x == 0) {                                               // head and tail bytes, one per thread
        const uint32_t tail0 = head + (nv << 4);
        uint32_t p = nb;
        if ((uint32_t)tid < head) p = tid;
        else if (tid >= 64 && tail0 + (uint32_t)(tid - 64) < nb) p = tail0 + (uint32_t)(tid - 64);
        if (p < nb) {
            const uint32_t y = p / row3, q = p - y * row3, x = q / 3u;
            out[p] = (uint8_t)(pmf_pixel(a, lut, idx, pmf_row(a, (int)y), (int)x) >> (8u * (q - x * 3u)));
        }
    }
    const uint32_t v = blockIdx.x * PMF_THREADS + tid;
    if (v >= nv) return;
    const uint32_t p = head + (v << 4);                                  // p + 15 < nb
    uint32_t y = p / row3;
    const uint32_t q = p - y * row3;
    uint32_t x = q / 3u, c = q - x * 3u;
    PmfRow row = pmf_row(a, (int)y);
    uint32_t val = pmf_pixel(a, lut, idx, row, (int)x);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        w[k >> 2] |= ((val >> (8u * c)) & 255u) << (8 * (k & 3));
        if (++c == 3u) {
            c = 0u;
            if (++x == (uint32_t)a.SW) { x = 0u; ++y; row = pmf_row(a, (int)y); }
            if (k < 15) val = pmf_pixel(a, lut, idx, row, (int)x);      // y < SH while bytes remain
        }
    }
    *(uint4*)(out + p) = make_uint4(w[0], w[1], w[2], w[3]);             // out + p is 16-byte aligned: p = head mod 16
}

extern "C" int urso_pmf_sheet_u8(int B, int n, int cell, int gap, const float* gt_d, const float* logits_d, const uint8_t* lut_d,
                                 const uint8_t* bg, uint8_t* idx_d, uint8_t* out_d, void* stream) {
    if (!lut_d || !out_d || !idx_d || !bg) { urso_set_error("urso_pmf_sheet_u8: null pointer (lut, bg, scratch or out)"); return URSO_EINVAL; }
    if (!gt_d && !logits_d) { urso_set_error("urso_pmf_sheet_u8: neither a stored PMF nor logits given"); return URSO_EINVAL; }
    if (B < 1 || B > 65535) { urso_set_error("urso_pmf_sheet_u8: 1 <= B <= 65535 (B %d)", B); return URSO_EINVAL; }
    if (n < 2 || n > 64 || cell < 1 || cell > 64 || gap < 0 || gap > 64) {
        urso_set_error("urso_pmf_sheet_u8: 2 <= n <= 64, 1 <= cell <= 64, 0 <= gap <= 64 (n %d, cell %d, gap %d)", n, cell, gap); return URSO_EINVAL;
    }
    const int rows = (gt_d ? 1 : 0) + (logits_d ? 1 : 0);
    const long long SW = (long long)n * n * cell + (long long)(n + 1) * gap, SH = (long long)rows * n * cell + (long long)(rows + 1) * gap;
    const long long bytes = SW * SH * 3;
    if (bytes >= (1LL << 31)) { urso_set_error("urso_pmf_sheet_u8: an image of 2 GiB or more (%lld x %lld x 3)", SH, SW); return URSO_EINVAL; }
    PmfArgs a;
    a.n = n; a.n2 = n * n; a.K = n * n * n; a.cell = cell; a.gap = gap; a.rows = rows; a.SW = (int)SW; a.SH = (int)SH;
    a.span = n * cell; a.band = a.span + gap;
    a.src[0] = gt_d ? gt_d : logits_d; a.est[0] = gt_d ? 0 : 1;
    a.src[1] = logits_d; a.est[1] = 1;                                   // read only when rows == 2
    a.bg = (uint32_t)bg[0] | ((uint32_t)bg[1] << 8) | ((uint32_t)bg[2] << 16);
    a.lut = lut_d; a.idx = idx_d; a.out = out_d;
    const unsigned chunks = (unsigned)((bytes >> 4) / PMF_THREADS + 1);  // an image has at most bytes / 16 whole vectors
    hipStream_t st = (hipStream_t)stream;
    // profiled under URSO_K_MOLD like the other picture kernels; bytes: the sources once, the indices written and read, the whole output
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * (rows * a.K * 6.0 + (double)bytes));
    URSO_KLAUNCH(pmf_index_kernel, dim3((unsigned)rows, (unsigned)B), dim3(PMF_THREADS), 0, st, a);
    URSO_KLAUNCH(pmf_sheet_kernel, dim3(chunks, (unsigned)B), dim3(PMF_THREADS), 0, st, a);
    return urso_check_launch("urso_pmf_sheet_u8");
}
