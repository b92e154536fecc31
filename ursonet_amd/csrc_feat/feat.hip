// Feature-space statistics of the bottleneck features (liburso_feat.so; fit_domain(), predict / evaluate with domain=..., DESIGN.md
// section 27).  urso_feat_pool turns the bottleneck_layer output into one fp64 feature row per image (cell means), urso_feat_gram_add adds a
// batch's centred rows and their outer products into the running sums s and G (the upper triangle), urso_feat_maha scores a batch's rows
// against a fitted mean and whitening matrix.  The rule, the operation order and the argument rules: include/ursonet_feat.h;
// ursonet_amd/domain.py (pool64 / gram_add64 / maha64) is the same in NumPy.  Everything is fp64 with one stated order per sum, the library
// is built with -ffp-contract=off, and the products below are named temporaries: a product is rounded before it is added.
#include "../csrc/common.h"
#include <math.h>
#include "../../include/ursonet_feat.h"

static constexpr int FT = 256;                                             // threads per workgroup (4 waves), all three kernels
static constexpr int GT = 32;                                              // gram: edge of a tile of G
static constexpr int GR = 32;                                              // gram: batch rows staged in LDS at a time
static constexpr int MR = URSO_FEAT_MAHA_ROWS;                             // maha: batch rows per workgroup
static constexpr int MJ = 64;                                              // maha: j per LDS stage
static constexpr int MU = 16;                                              // maha: W elements a thread loads ahead of their terms
static_assert(MJ % MU == 0, "a stage is whole groups of loads");
static_assert(GT * GT == 4 * FT, "a thread keeps a 2 x 2 register tile");
static_assert(MR * MJ == 2 * FT, "a thread stages two d values");
static_assert(MR <= 64 && FT >= 64 + MR, "the reductions take a thread per row in the first wave and one in the second");

// ------------------------------------------------------------------------------------------------ pool
template <typename T>
__global__ void __launch_bounds__(FT) feat_pool_kernel(urso_feat_pool_args a) {
    const int C = a.C, D = a.gh * a.gw * C;
    const long long idx = (long long)blockIdx.x * FT + threadIdx.x;
    if (idx >= (long long)a.n * D) return;
    const int b = (int)(idx / D), f = (int)(idx % D);
    const int cell = f / C, c = f % C, gy = cell / a.gw, gx = cell % a.gw;
    const int ch = a.h / a.gh, cw = a.w / a.gw;
    const T* __restrict__ p = (const T*)a.act + (((size_t)b * a.h + (size_t)gy * ch) * a.w + (size_t)gx * cw) * C + c;
    double s = 0.0;
    for (int y = 0; y < ch; ++y)
        for (int x = 0; x < cw; ++x) {
            const double v = (double)Elem<T>::to_f(p[((size_t)y * a.w + x) * C]);
            s = s + v;
        }
    a.out[((size_t)a.row0 + b) * (size_t)a.ld + f] = s / (double)(ch * cw);
}

// ------------------------------------------------------------------------------------------------ gram
// Workgroup k takes the tile (ti, tj), tj >= ti, of the upper triangle, the tiles counted row by row.  Thread (ty, tx) = (t / 16, t % 16)
// keeps G at rows ti * 32 + ty + {0, 16} and columns tj * 32 + tx + {0, 16}: a wave touches 16 consecutive doubles of four rows.
__global__ void __launch_bounds__(FT) feat_gram_kernel(urso_feat_gram_args a, int T) {
    __shared__ double di[GR][GT], dj[GR][GT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, D = a.D;
    int k = blockIdx.x, ti = 0;
    while (k >= T - ti) { k -= T - ti; ++ti; }
    const int tj = ti + k;
    const bool diag = ti == tj;
    const int i[2] = {ti * GT + ty, ti * GT + ty + 16}, j[2] = {tj * GT + tx, tj * GT + tx + 16};
    bool m[2][2];
    double g[2][2];
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q) {
            m[p][q] = i[p] < D && j[q] < D && j[q] >= i[p];
            g[p][q] = m[p][q] ? a.g[(size_t)i[p] * (size_t)a.ld_g + j[q]] : 0.0;
        }
    const int si = ti * GT + t;
    const bool ms = diag && t < GT && si < D;
    double sv = ms ? a.s[si] : 0.0;
    for (int r0 = 0; r0 < a.n; r0 += GR) {
        const int rows = min(GR, a.n - r0);
        __syncthreads();                                                   // the stage before has been consumed
        for (int e = t; e < rows * GT; e += FT) {
            const int rr = e / GT, cc = e % GT;
            const double* __restrict__ xr = a.x + ((size_t)a.row0 + r0 + rr) * (size_t)a.ld_x;
            const int ci = ti * GT + cc, cj = tj * GT + cc;
            di[rr][cc] = ci < D ? xr[ci] - a.centre[ci] : 0.0;
            dj[rr][cc] = cj < D ? xr[cj] - a.centre[cj] : 0.0;
        }
        __syncthreads();
        for (int rr = 0; rr < rows; ++rr) {
            const double a0 = di[rr][ty], a1 = di[rr][ty + 16], b0 = dj[rr][tx], b1 = dj[rr][tx + 16];
            const double p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
            g[0][0] = g[0][0] + p00; g[0][1] = g[0][1] + p01; g[1][0] = g[1][0] + p10; g[1][1] = g[1][1] + p11;
            if (ms) sv = sv + di[rr][t];
        }
    }
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q)
            if (m[p][q]) a.g[(size_t)i[p] * (size_t)a.ld_g + j[q]] = g[p][q];
    if (ms) a.s[si] = sv;
}

// ------------------------------------------------------------------------------------------------ maha
// One workgroup per MR batch rows.  i runs in tiles of FT (thread t has i = it + t and MR accumulators); j runs in stages of MJ whose d of the
// MR rows sit in LDS (dj[j][row]: a wave reads one address per row, a broadcast), so a W element is loaded once for MR rows.  Behind an i
// tile, thread r < rows adds y_i^2 (and keeps the maximum) and thread 64 + r adds d_i^2, from LDS, i ascending.
__global__ void __launch_bounds__(FT) feat_maha_kernel(urso_feat_maha_args a) {
    __shared__ double dj[MJ][MR];
    __shared__ double yt[MR][FT], dt[MR][FT];
    __shared__ int bad[MR];
    const int t = threadIdx.x, D = a.D, b0 = blockIdx.x * MR, rows = min(MR, a.n - b0);
    const double* __restrict__ x0 = a.x + (size_t)b0 * (size_t)a.ld_x;
    if (t < MR) bad[t] = 0;
    double score = 0.0, dist2 = 0.0, zmax = -1.0;
    int zarg = 0;
    for (int it = 0; it < D; it += FT) {
        const int i = it + t, jend = min(D, it + FT);
        double acc[MR];
#pragma unroll
        for (int r = 0; r < MR; ++r) acc[r] = 0.0;
        for (int jt = 0; jt < jend; jt += MJ) {
            __syncthreads();                                               // the stage before has been consumed (and bad[] is zeroed)
            for (int e = t; e < MR * MJ; e += FT) {
                const int rr = e / MJ, jj = e % MJ, jx = jt + jj;
                double d = 0.0;
                if (rr < rows && jx < D) {
                    const double xv = x0[(size_t)rr * (size_t)a.ld_x + jx];
                    if (!__builtin_isfinite(xv)) bad[rr] = 1;
                    d = xv - a.mean[jx];
                }
                dj[jj][rr] = d;
            }
            __syncthreads();
            if (i < D) {
                const int jmax = min(MJ, i - jt + 1);                      // j <= i: nothing above the diagonal is read
                // The loads of W run a group of MU ahead of their terms: a thread's chain is bound by their latency, not by the arithmetic.
                const double* __restrict__ wcol = a.wt + (size_t)jt * (size_t)a.ld_w + i;
                double wn[MU];
#pragma unroll
                for (int u = 0; u < MU; ++u) wn[u] = u < jmax ? wcol[(size_t)u * (size_t)a.ld_w] : 0.0;
                for (int jj = 0; jj < jmax; jj += MU) {                    // j ascending
                    double wv[MU];
#pragma unroll
                    for (int u = 0; u < MU; ++u) wv[u] = wn[u];
#pragma unroll
                    for (int u = 0; u < MU; ++u) wn[u] = jj + MU + u < jmax ? wcol[(size_t)(jj + MU + u) * (size_t)a.ld_w] : 0.0;
#pragma unroll
                    for (int u = 0; u < MU; ++u) {
                        if (jj + u < jmax) {
#pragma unroll
                            for (int r = 0; r < MR; ++r) {
                                const double p = wv[u] * dj[jj + u][r];
                                acc[r] = acc[r] + p;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            yt[r][t] = acc[r];
            dt[r][t] = (r < rows && i < D) ? x0[(size_t)r * (size_t)a.ld_x + i] - a.mean[i] : 0.0;
        }
        __syncthreads();
        // i ascending, eight LDS reads ahead of their terms.  The entries behind D are +0.0 (y and d alike): adding their squares changes no
        // bit of a sum that is >= +0.0 or NaN, and |y| = 0 is no new maximum behind the first entry.
        const int cnt = min(FT, (D - it + 7) & ~7);
        if (t < rows) {
            for (int k = 0; k < cnt; k += 8) {
                double y[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) y[u] = yt[t][k + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double yy = y[u] * y[u], ay = fabs(y[u]);
                    score = score + yy;
                    if (ay > zmax || (ay != ay && zmax == zmax)) { zmax = ay; zarg = it + k + u; }
                }
            }
        } else if (t >= 64 && t < 64 + rows) {
            for (int k = 0; k < cnt; k += 8) {
                double d[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) d[u] = dt[t - 64][k + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double dd = d[u] * d[u];
                    dist2 = dist2 + dd;
                }
            }
        }
        // the next tile's stages begin with a barrier: yt / dt are rewritten only behind it
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    if (t < rows) {
        double* out = a.out + ((size_t)a.row0 + b0 + t) * URSO_FEAT_COLS;
        const bool nf = bad[t] != 0;
        out[URSO_FEAT_SCORE] = nf ? nan : score;
        out[URSO_FEAT_ZMAX] = nf ? nan : zmax;
        out[URSO_FEAT_ZARG] = nf ? nan : (double)zarg;
    } else if (t >= 64 && t < 64 + rows) {
        double* out = a.out + ((size_t)a.row0 + b0 + (t - 64)) * URSO_FEAT_COLS;
        out[URSO_FEAT_DIST2] = bad[t - 64] != 0 ? nan : dist2;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static bool ft_bad_rows(const char* fn, int B, int n, long long row0) {
    if (n < 0 || n > B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, B, n); return true; }
    if (row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, row0); return true; }
    return false;
}

static bool ft_bad_d(const char* fn, long long D) {
    if (D < 1 || D > URSO_FEAT_MAX_D) { urso_set_error("%s: need 1 <= D <= %d (got %lld)", fn, URSO_FEAT_MAX_D, D); return true; }
    return false;
}

extern "C" int urso_feat_pool(const urso_feat_pool_args* a, void* stream) {
    const char* fn = "urso_feat_pool";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->act || !a->out) { urso_set_error("%s: null pointer (act, out)", fn); return URSO_EINVAL; }
    if (ft_bad_rows(fn, a->B, a->n, (long long)a->row0)) return URSO_EINVAL;
    if (a->h < 1 || a->w < 1 || a->C < 1) { urso_set_error("%s: need h, w, C >= 1 (got %d, %d, %d)", fn, a->h, a->w, a->C); return URSO_EINVAL; }
    if (a->gh < 1 || a->gw < 1 || a->h % a->gh || a->w % a->gw) {
        urso_set_error("%s: the grid (%d, %d) does not divide the feature map (%d, %d)", fn, a->gh, a->gw, a->h, a->w);
        return URSO_EINVAL;
    }
    const long long D = (long long)a->gh * a->gw * a->C;
    if (ft_bad_d(fn, D)) return URSO_EINVAL;
    if (a->dtype != URSO_F32 && a->dtype != URSO_BF16 && a->dtype != URSO_F16) { urso_set_error("%s: unknown dtype %d", fn, a->dtype); return URSO_EINVAL; }
    if (a->ld < D) { urso_set_error("%s: ld %lld < D %lld", fn, (long long)a->ld, D); return URSO_EINVAL; }
    if ((uintptr_t)a->act & (dt_size(a->dtype) - 1)) { urso_set_error("%s: act must be %d-byte aligned", fn, (int)dt_size(a->dtype)); return URSO_EINVAL; }
    if ((uintptr_t)a->out & 7) { urso_set_error("%s: out must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const double pix = (double)a->n * a->h * a->w * a->C;
    ProfScope ps(st, URSO_K_DECODE, 0, pix * (double)dt_size(a->dtype) + 8.0 * (double)a->n * (double)D);
    const dim3 grid((unsigned)(((long long)a->n * D + FT - 1) / FT));
    if (a->dtype == URSO_F32) URSO_KLAUNCH(feat_pool_kernel<float>, grid, dim3(FT), 0, st, *a);
    else if (a->dtype == URSO_BF16) URSO_KLAUNCH(feat_pool_kernel<__bf16>, grid, dim3(FT), 0, st, *a);
    else URSO_KLAUNCH(feat_pool_kernel<_Float16>, grid, dim3(FT), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_feat_gram_add(const urso_feat_gram_args* a, void* stream) {
    const char* fn = "urso_feat_gram_add";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->x || !a->centre || !a->s || !a->g) { urso_set_error("%s: null pointer (x, centre, s, g)", fn); return URSO_EINVAL; }
    if (ft_bad_rows(fn, a->B, a->n, (long long)a->row0)) return URSO_EINVAL;
    if (ft_bad_d(fn, a->D)) return URSO_EINVAL;
    if (a->ld_x < a->D) { urso_set_error("%s: ld_x %lld < D %d", fn, (long long)a->ld_x, a->D); return URSO_EINVAL; }
    if (a->ld_g < a->D) { urso_set_error("%s: ld_g %lld < D %d", fn, (long long)a->ld_g, a->D); return URSO_EINVAL; }
    if (((uintptr_t)a->x | (uintptr_t)a->centre | (uintptr_t)a->s | (uintptr_t)a->g) & 7) {
        urso_set_error("%s: x, centre, s and g must be 8-byte aligned", fn);
        return URSO_EINVAL;
    }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const int T = (a->D + GT - 1) / GT;
    ProfScope ps(st, URSO_K_DECODE, (double)a->n * a->D * (a->D + 1.0), 8.0 * a->D * (a->D + 1.0) + 8.0 * (double)a->n * a->D);
    URSO_KLAUNCH(feat_gram_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(FT), 0, st, *a, T);
    return urso_check_launch(fn);
}

extern "C" int urso_feat_maha(const urso_feat_maha_args* a, void* stream) {
    const char* fn = "urso_feat_maha";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->x || !a->mean || !a->wt || !a->out) { urso_set_error("%s: null pointer (x, mean, wt, out)", fn); return URSO_EINVAL; }
    if (ft_bad_rows(fn, a->B, a->n, (long long)a->row0)) return URSO_EINVAL;
    if (ft_bad_d(fn, a->D)) return URSO_EINVAL;
    if (a->ld_x < a->D) { urso_set_error("%s: ld_x %lld < D %d", fn, (long long)a->ld_x, a->D); return URSO_EINVAL; }
    if (a->ld_w < a->D) { urso_set_error("%s: ld_w %lld < D %d", fn, (long long)a->ld_w, a->D); return URSO_EINVAL; }
    if (((uintptr_t)a->x | (uintptr_t)a->mean | (uintptr_t)a->wt | (uintptr_t)a->out) & 7) {
        urso_set_error("%s: x, mean, wt and out must be 8-byte aligned", fn);
        return URSO_EINVAL;
    }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const int groups = (a->n + MR - 1) / MR;
    ProfScope ps(st, URSO_K_DECODE, (double)a->n * a->D * (a->D + 1.0), 4.0 * a->D * (a->D + 1.0) * groups + 8.0 * (double)a->n * a->D);
    URSO_KLAUNCH(feat_maha_kernel, dim3((unsigned)groups), dim3(FT), 0, st, *a);
    return urso_check_launch(fn);
}
