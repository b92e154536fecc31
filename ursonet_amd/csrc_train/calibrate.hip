// Temperature scaling of the classification heads (liburso_train.so; calibrate(), predict / evaluate / test_and_submit with
// calibration=...).  urso_temp_stats turns a batch of logit rows and their encoded targets into the fp64 statistics
// of the cross-entropy at up to eight inverse temperatures at once, urso_temp_reduce adds a table of such rows into the loss, its slope
// and its curvature, and urso_temp_scale multiplies logits by the fitted beta in front of the decode kernels.  Rules, reduction order,
// table layout and argument rules: include/ursonet_train.h; ursonet_amd/calibrate.py (stats64 / reduce64 / scale32) is the same in NumPy.
//
// The stats launch has urso_ens_add's shape: one workgroup of TT = 1024 threads per valid row, columns dealt to threads by their index
// alone, one 16-byte load per group of four where the row is aligned and four 4-byte loads where it is not.  A row is read twice (max and
// the target's sums, then the exponential sums; the second time out of L2) whatever J is: the J sets {Z, A, Q} are 3 J doubles of
// registers, and one exp per column and temperature is the work.  The row is not parked in LDS: at 32^3 bins it would take 128 KiB and
// one workgroup per CU either way, and the second read comes out of L2.
#include "../csrc/common.h"
#include <float.h>
#include <math.h>
#include "../../include/ursonet_train.h"

static constexpr int TT = 1024;                                            // threads per workgroup (16 waves)
static constexpr int TW = TT / 64;
static constexpr int TJ = URSO_TEMP_MAX_J;

// ------------------------------------------------------------------------------------------------ reductions
// The header's order: the xor shuffle 32 .. 1 across a wave; the wave sums are parked in LDS and added in wave order by one thread.
__device__ __forceinline__ double tmp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double tmp_waves(const double* sh) {
    double r = 0.0;
    for (int w = 0; w < TW; ++w) r += sh[w];
    return r;
}

// the larger of two, a NaN winning over everything (fmax would drop it)
__device__ __forceinline__ float tmp_max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ float tmp_block_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = tmp_max_nan(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < TW; ++w) r = tmp_max_nan(r, sh[w]);
    return r;
}

// ------------------------------------------------------------------------------------------------ column walk
// Calls f(first column, count) for the calling thread's groups in index order: count = 4 for a group of four columns, the ragged end
// (count = K % 4) once, by the thread whose turn it is.
template <class F>
__device__ __forceinline__ void tmp_walk(int K, F f) {
    const int ng = K >> 2;
    for (int g = threadIdx.x; g < ng; g += TT) f(4 * g, 4);
    const int tail = K & 3;
    if (tail && (ng % TT) == (int)threadIdx.x) f(4 * ng, tail);
}

// columns [c, c + cnt) of a row: one 16-byte load for a whole group of an aligned row
__device__ __forceinline__ void tmp_load(const float* __restrict__ row, bool aligned, int c, int cnt, float (&z)[4]) {
    if (aligned && cnt == 4) {
        const f32x4_t v = *(const f32x4_t*)(row + c);
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        for (int j = 0; j < cnt; ++j) z[j] = row[c + j];
    }
}

// ------------------------------------------------------------------------------------------------ stats
template <int J>
__global__ void __launch_bounds__(TT) temp_stats_kernel(urso_temp_stats_args a) {
    __shared__ double shd[2 + 3 * TJ][TW];
    __shared__ float shf[TW];
    const int b = blockIdx.x, K = a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ zrow = a.logits + (size_t)b * (size_t)a.ld_z;
    const float* __restrict__ yrow = a.target + (size_t)b * (size_t)a.ld_y;
    const bool zal = ((uintptr_t)zrow & 15) == 0, yal = ((uintptr_t)yrow & 15) == 0;

    // sweep 1: the row's maximum (exact whatever the order) and the target's two sums, per thread in column order
    float mt = -INFINITY;
    double syt = 0.0, yzt = 0.0;
    tmp_walk(K, [&](int c, int cnt) {
        float z[4], y[4];
        tmp_load(zrow, zal, c, cnt, z);
        tmp_load(yrow, yal, c, cnt, y);
        for (int i = 0; i < cnt; ++i) {
            mt = tmp_max_nan(mt, z[i]);
            const double yd = (double)y[i];
            const double t = y[i] == 0.0f ? 0.0 : yd * (double)z[i];
            syt = syt + yd;
            yzt = yzt + t;
        }
    });
    const float mf = tmp_block_max(mt, shf);
    const double m = (double)mf;
    syt = tmp_wave_sum(syt);
    yzt = tmp_wave_sum(yzt);
    if (lane == 0) { shd[0][wave] = syt; shd[1][wave] = yzt; }

    // sweep 2: Z, A, Q of every temperature from one read of the row
    double beta[J], Zt[J], At[J], Qt[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { beta[j] = a.beta[j]; Zt[j] = 0.0; At[j] = 0.0; Qt[j] = 0.0; }
    tmp_walk(K, [&](int c, int cnt) {
        float z[4];
        tmp_load(zrow, zal, c, cnt, z);
        for (int i = 0; i < cnt; ++i) {
            const double d = (double)z[i] - m;
            const double dd = d * d;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double x = beta[j] * d;
                const double e = exp(x);
                const double ta = e == 0.0 ? 0.0 : e * d;
                const double tq = e == 0.0 ? 0.0 : e * dd;
                Zt[j] = Zt[j] + e;
                At[j] = At[j] + ta;
                Qt[j] = Qt[j] + tq;
            }
        }
    });
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double zs = tmp_wave_sum(Zt[j]), as = tmp_wave_sum(At[j]), qs = tmp_wave_sum(Qt[j]);
        if (lane == 0) { shd[2 + 3 * j][wave] = zs; shd[3 + 3 * j][wave] = as; shd[4 + 3 * j][wave] = qs; }
    }
    __syncthreads();

    // close: thread j has temperature j, thread 0 the target's sums as well
    const int t = threadIdx.x;
    if (t >= J) return;
    double* out = a.out + ((size_t)a.row0 + (size_t)b) * URSO_TEMP_COLS;
    double bj = beta[0];
#pragma unroll
    for (int j = 1; j < J; ++j) bj = t == j ? beta[j] : bj;
    const double Z = tmp_waves(shd[2 + 3 * t]), A = tmp_waves(shd[3 + 3 * t]), Q = tmp_waves(shd[4 + 3 * t]);
    const double r = A / Z;
    const double lz = log(Z);
    const double bm = bj * m;
    const double qz = Q / Z;
    const double rr = r * r;
    out[URSO_TEMP_LSE + 3 * t] = lz + bm;
    out[URSO_TEMP_M1 + 3 * t] = m + r;
    out[URSO_TEMP_VAR + 3 * t] = qz - rr;
    if (t == 0) {
        const double poison = 0.0 * m;                                     // NaN unless m is finite
        out[URSO_TEMP_SY] = tmp_waves(shd[0]) + poison;
        out[URSO_TEMP_YZ] = tmp_waves(shd[1]) + poison;
    }
}

// ------------------------------------------------------------------------------------------------ reduce
__global__ void __launch_bounds__(TT) temp_reduce_kernel(urso_temp_reduce_args a) {
    __shared__ double shd[TJ * URSO_TEMP_TOTALS][TW];
    const int J = a.J, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[TJ][URSO_TEMP_TOTALS];
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int k = 0; k < URSO_TEMP_TOTALS; ++k) acc[j][k] = 0.0;
    for (int64_t r = threadIdx.x; r < a.N; r += TT) {
        const double* __restrict__ row = a.rows + (size_t)r * URSO_TEMP_COLS;
        const double sy = row[URSO_TEMP_SY], yz = row[URSO_TEMP_YZ];
        const bool fin = __builtin_isfinite(sy) && __builtin_isfinite(yz);
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            if (j < J) {
                const double lse = row[URSO_TEMP_LSE + 3 * j], m1 = row[URSO_TEMP_M1 + 3 * j], var = row[URSO_TEMP_VAR + 3 * j];
                const double p0 = sy * lse, p1 = a.beta[j] * yz, p2 = sy * m1, p3 = sy * var;
                const double ce = p0 - p1;
                const double g = p2 - yz;
                const bool ok = fin && __builtin_isfinite(lse) && __builtin_isfinite(m1) && __builtin_isfinite(var);
                acc[j][0] = acc[j][0] + ce;
                acc[j][1] = acc[j][1] + g;
                acc[j][2] = acc[j][2] + p3;
                acc[j][3] = acc[j][3] + (ok ? 0.0 : 1.0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int k = 0; k < URSO_TEMP_TOTALS; ++k) {
            const double s = tmp_wave_sum(acc[j][k]);
            if (lane == 0) shd[j * URSO_TEMP_TOTALS + k][wave] = s;
        }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < J * URSO_TEMP_TOTALS) a.totals[t] = tmp_waves(shd[t]);
}

// ------------------------------------------------------------------------------------------------ scale
__global__ void __launch_bounds__(TT) temp_scale_kernel(urso_temp_scale_args a) {
    const int b = blockIdx.x, K = a.K, ng = K >> 2, tail = K & 3;
    const int g = (int)blockIdx.y * TT + (int)threadIdx.x;
    const int cnt = g < ng ? 4 : (g == ng ? tail : 0);
    if (cnt == 0) return;
    const float* __restrict__ src = a.in + (size_t)b * (size_t)a.ld_in;
    float* dst = a.out + (size_t)b * (size_t)a.ld_out;
    const bool sal = ((uintptr_t)src & 15) == 0, dal = ((uintptr_t)dst & 15) == 0;
    const int c = 4 * g;
    float z[4], s[4];
    tmp_load(src, sal, c, cnt, z);
    for (int i = 0; i < cnt; ++i) {
        const double p = (double)z[i] * a.beta;
        s[i] = (float)p;
    }
    if (dal && cnt == 4) {
        f32x4_t v;
        v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
        *(f32x4_t*)(dst + c) = v;
    } else {
        for (int i = 0; i < cnt; ++i) dst[c + i] = s[i];
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static bool tmp_bad_betas(const char* fn, int J, const double* beta) {
    if (J < 1 || J > TJ) { urso_set_error("%s: need 1 <= J <= %d (got %d)", fn, TJ, J); return true; }
    for (int j = 0; j < J; ++j)
        if (!(beta[j] > 0.0) || !(beta[j] <= DBL_MAX)) { urso_set_error("%s: beta[%d] must be finite and > 0 (got %g)", fn, j, beta[j]); return true; }
    return false;
}

template <int J>
static void tmp_launch_stats(const urso_temp_stats_args& a, hipStream_t st) {
    URSO_KLAUNCH(temp_stats_kernel<J>, dim3(a.n), dim3(TT), 0, st, a);
}

extern "C" int urso_temp_stats(const urso_temp_stats_args* a, void* stream) {
    const char* fn = "urso_temp_stats";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->logits || !a->target || !a->out) { urso_set_error("%s: null pointer (logits, target, out)", fn); return URSO_EINVAL; }
    if (tmp_bad_betas(fn, a->J, a->beta)) return URSO_EINVAL;
    if (a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->K < 1) { urso_set_error("%s: K must be >= 1 (got %d)", fn, a->K); return URSO_EINVAL; }
    if (a->ld_z < a->K) { urso_set_error("%s: ld_z %d < K %d", fn, a->ld_z, a->K); return URSO_EINVAL; }
    if (a->ld_y < a->K) { urso_set_error("%s: ld_y %d < K %d", fn, a->ld_y, a->K); return URSO_EINVAL; }
    if (((uintptr_t)a->logits | (uintptr_t)a->target) & 3) { urso_set_error("%s: logits and target must be 4-byte aligned", fn); return URSO_EINVAL; }
    if ((uintptr_t)a->out & 7) { urso_set_error("%s: out must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * ((double)a->K * 8 + (2 + 3 * a->J) * 8));
    switch (a->J) {
        case 1: tmp_launch_stats<1>(*a, st); break;
        case 2: tmp_launch_stats<2>(*a, st); break;
        case 3: tmp_launch_stats<3>(*a, st); break;
        case 4: tmp_launch_stats<4>(*a, st); break;
        case 5: tmp_launch_stats<5>(*a, st); break;
        case 6: tmp_launch_stats<6>(*a, st); break;
        case 7: tmp_launch_stats<7>(*a, st); break;
        default: tmp_launch_stats<8>(*a, st); break;
    }
    return urso_check_launch(fn);
}

extern "C" int urso_temp_reduce(const urso_temp_reduce_args* a, void* stream) {
    const char* fn = "urso_temp_reduce";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->rows || !a->totals) { urso_set_error("%s: null pointer (rows, totals)", fn); return URSO_EINVAL; }
    if (tmp_bad_betas(fn, a->J, a->beta)) return URSO_EINVAL;
    if (a->N < 1) { urso_set_error("%s: N must be >= 1 (got %lld)", fn, (long long)a->N); return URSO_EINVAL; }
    if (((uintptr_t)a->rows | (uintptr_t)a->totals) & 7) { urso_set_error("%s: rows and totals must be 8-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->N * (2 + 3 * a->J) * 8);
    URSO_KLAUNCH(temp_reduce_kernel, dim3(1), dim3(TT), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_temp_scale(const urso_temp_scale_args* a, void* stream) {
    const char* fn = "urso_temp_scale";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->in || !a->out) { urso_set_error("%s: null pointer (in, out)", fn); return URSO_EINVAL; }
    if (!(a->beta > 0.0) || !(a->beta <= DBL_MAX)) { urso_set_error("%s: beta must be finite and > 0 (got %g)", fn, a->beta); return URSO_EINVAL; }
    if (a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->K < 1) { urso_set_error("%s: K must be >= 1 (got %d)", fn, a->K); return URSO_EINVAL; }
    if (a->ld_in < a->K) { urso_set_error("%s: ld_in %d < K %d", fn, a->ld_in, a->K); return URSO_EINVAL; }
    if (a->ld_out < a->K) { urso_set_error("%s: ld_out %d < K %d", fn, a->ld_out, a->K); return URSO_EINVAL; }
    if (((uintptr_t)a->in | (uintptr_t)a->out) & 3) { urso_set_error("%s: in and out must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (double)a->K * 8);
    const int groups = (a->K >> 2) + 1;
    URSO_KLAUNCH(temp_scale_kernel, dim3(a->n, (groups + TT - 1) / TT), dim3(TT), 0, st, *a);
    return urso_check_launch(fn);
}
