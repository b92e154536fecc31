// Ensemble inference (liburso_train.so; predict / evaluate / test_and_submit with members=...): the Bayesian model
// average of a classification head.  urso_ens_add folds one member's softmax over a batch of logit rows into fp64 accumulators (the sum of
// the members' PMFs and of their entropies); urso_ens_settle turns accumulated rows into log-probabilities the decode kernels take in the
// place of logits, and the uncertainty columns.  Rules, reduction order, table layout and argument rules: include/ursonet_train.h;
// ursonet_amd/ensemble.py (add64 / settle64) is the same in NumPy float64.
//
// One workgroup of ET = 1024 threads per valid row.  A row of K = 32^3 .. 64^3 logits is 128 KiB .. 1 MiB: it does not fit in registers or
// LDS, so the add reads it three times (max, sums, write) -- the second and third time out of L2 -- and computes exp twice rather than
// park K doubles anywhere.  Columns are dealt to threads by their index alone: thread t owns the groups of four columns t, ET + t,
// 2 ET + t, ... and the ragged end K % 4 belongs to the group behind the last whole one.  Where the row's first logit sits on a 16-byte
// boundary a group is one 16-byte load, elsewhere the same four columns are four 4-byte loads -- so the sums do not depend on where the
// row lies.  The accumulator rows take 16-byte stores under the same rule.
#include "../csrc/common.h"
#include <float.h>
#include <math.h>
#include "../../include/ursonet_train.h"

static constexpr int ET = 1024;                                            // threads per workgroup (16 waves)
static constexpr int EW = ET / 64;

typedef __attribute__((ext_vector_type(2))) double f64x2_t;

// ------------------------------------------------------------------------------------------------ reductions
// The header's order: the xor shuffle 32 .. 1 across a wave, then the wave sums in wave order -- by every thread alike, so that all of
// them hold the block's sum.  sh: EW doubles of the caller's, free to be reused behind the call.
__device__ __forceinline__ double ens_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double ens_block_sum(double v, double* sh) {
    v = ens_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < EW; ++w) r += sh[w];
    __syncthreads();
    return r;
}

// the larger of two, a NaN winning over everything (fmax would drop it)
__device__ __forceinline__ float ens_max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ float ens_block_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = ens_max_nan(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < EW; ++w) r = ens_max_nan(r, sh[w]);
    __syncthreads();
    return r;
}

// (value, index): the larger value, a NaN winning over everything, the lower index among equals (and among NaNs)
struct EnsPeak { double v; int i; };
__device__ __forceinline__ EnsPeak ens_peak_of(const EnsPeak& a, const EnsPeak& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    bool take_b;
    if (an || bn) take_b = bn && (!an || b.i < a.i);
    else take_b = b.v > a.v || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}

// ------------------------------------------------------------------------------------------------ column walk
// Calls f(first column, count) for the calling thread's groups in index order: count = 4 for a group of four columns, the ragged end
// (count = K % 4) once, by the thread whose turn it is.
template <class F>
__device__ __forceinline__ void ens_walk(int K, F f) {
    const int ng = K >> 2;
    for (int g = threadIdx.x; g < ng; g += ET) f(4 * g, 4);
    const int tail = K & 3;
    if (tail && (ng % ET) == (int)threadIdx.x) f(4 * ng, tail);
}

// the logits of columns [c, c + cnt) of a row: one 16-byte load for a whole group of an aligned row
__device__ __forceinline__ void ens_load(const float* __restrict__ row, bool aligned, int c, int cnt, float (&z)[4]) {
    if (aligned && cnt == 4) {
        const f32x4_t v = *(const f32x4_t*)(row + c);
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        for (int j = 0; j < cnt; ++j) z[j] = row[c + j];
    }
}

// ------------------------------------------------------------------------------------------------ add
__global__ void __launch_bounds__(ET) ens_add_kernel(urso_ens_add_args a) {
    __shared__ double shd[EW];
    __shared__ float shf[EW];
    const int b = blockIdx.x, K = a.K;
    const size_t r = (size_t)a.row0 + (size_t)b;
    const float* __restrict__ row = a.logits + (size_t)b * (size_t)a.ld;
    double* __restrict__ acc = a.acc + r * (size_t)K;
    const bool zal = ((uintptr_t)row & 15) == 0, aal = ((uintptr_t)acc & 15) == 0;

    // the row's maximum (exact whatever the order)
    float mt = -INFINITY;
    ens_walk(K, [&](int c, int cnt) {
        float z[4];
        ens_load(row, zal, c, cnt, z);
        for (int j = 0; j < cnt; ++j) mt = ens_max_nan(mt, z[j]);
    });
    const double m = (double)ens_block_max(mt, shf);

    // Z = sum e, S = sum e * (-d): per thread in read order
    double zt = 0.0, st = 0.0;
    ens_walk(K, [&](int c, int cnt) {
        float z[4];
        ens_load(row, zal, c, cnt, z);
        for (int j = 0; j < cnt; ++j) {
            const double d = (double)z[j] - m;
            const double e = exp(d);
            const double nd = -d;
            const double t = e == 0.0 ? 0.0 : e * nd;
            zt = zt + e;
            st = st + t;
        }
    });
    const double Z = ens_block_sum(zt, shd);
    const double S = ens_block_sum(st, shd);

    // p = e / Z into the accumulator
    const bool first = a.first != 0;
    ens_walk(K, [&](int c, int cnt) {
        float z[4];
        double p[4];
        ens_load(row, zal, c, cnt, z);
        for (int j = 0; j < cnt; ++j) {
            const double d = (double)z[j] - m;
            const double e = exp(d);
            p[j] = e / Z;
        }
        if (aal && cnt == 4) {
            f64x2_t* dst = (f64x2_t*)(acc + c);
            f64x2_t lo, hi;
            if (first) { lo.x = p[0]; lo.y = p[1]; hi.x = p[2]; hi.y = p[3]; }
            else {
                lo = dst[0]; hi = dst[1];
                lo.x = lo.x + p[0]; lo.y = lo.y + p[1]; hi.x = hi.x + p[2]; hi.y = hi.y + p[3];
            }
            dst[0] = lo; dst[1] = hi;
        } else {
            for (int j = 0; j < cnt; ++j) acc[c + j] = first ? p[j] : acc[c + j] + p[j];
        }
    });

    if (threadIdx.x != 0) return;
    const double lz = log(Z);
    const double q = S / Z;
    const double H = lz + q;
    double* st4 = a.stat + r * URSO_ENS_STAT;
    if (first) { st4[0] = H; st4[1] = 1.0; st4[2] = 0.0; st4[3] = 0.0; }
    else { st4[0] = st4[0] + H; st4[1] = st4[1] + 1.0; }
}

// ------------------------------------------------------------------------------------------------ settle
__global__ void __launch_bounds__(ET) ens_settle_kernel(urso_ens_settle_args a) {
    __shared__ double shd[EW];
    __shared__ EnsPeak shp[EW];
    const int b = blockIdx.x, K = a.K;
    const size_t r = (size_t)a.row0 + (size_t)b;
    const double* __restrict__ acc = a.acc + r * (size_t)K;
    float* __restrict__ logp = a.logp + (size_t)b * (size_t)K;
    const bool aal = ((uintptr_t)acc & 15) == 0, lal = ((uintptr_t)logp & 15) == 0;
    const double M = (double)a.M;

    double ht = 0.0;
    EnsPeak pk = {-INFINITY, 0x7fffffff};
    ens_walk(K, [&](int c, int cnt) {
        double s[4];
        float l[4];
        if (aal && cnt == 4) {
            const f64x2_t lo = ((const f64x2_t*)(acc + c))[0], hi = ((const f64x2_t*)(acc + c))[1];
            s[0] = lo.x; s[1] = lo.y; s[2] = hi.x; s[3] = hi.y;
        } else {
            for (int j = 0; j < cnt; ++j) s[j] = acc[c + j];
        }
        for (int j = 0; j < cnt; ++j) {
            const double p = s[j] / M;
            const double lg = log(p);
            const double t = p == 0.0 ? 0.0 : p * lg;
            ht = ht + t;
            l[j] = p == 0.0 ? -FLT_MAX : (float)lg;
            const EnsPeak here = {p, c + j};
            pk = ens_peak_of(pk, here);
        }
        if (lal && cnt == 4) {
            f32x4_t v;
            v.x = l[0]; v.y = l[1]; v.z = l[2]; v.w = l[3];
            *(f32x4_t*)(logp + c) = v;
        } else {
            for (int j = 0; j < cnt; ++j) logp[c + j] = l[j];
        }
    });
    const double hs = ens_block_sum(ht, shd);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        EnsPeak other;
        other.v = __shfl_xor(pk.v, o, 64);
        other.i = __shfl_xor(pk.i, o, 64);
        pk = ens_peak_of(pk, other);
    }
    if ((threadIdx.x & 63) == 0) shp[threadIdx.x >> 6] = pk;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < EW; ++w) pk = ens_peak_of(pk, shp[w]);

    const double* st4 = a.stat + r * URSO_ENS_STAT;
    const double hbar = -hs;
    const double hmem = st4[0] / M;
    const double diff = hbar - hmem;
    double* row = a.table + r * URSO_ENS_COLS;
    row[URSO_ENS_H_MEAN] = hbar;
    row[URSO_ENS_H_MEMBERS] = hmem;
    row[URSO_ENS_MI] = diff < 0.0 ? 0.0 : diff;                            // (a NaN stays)
    row[URSO_ENS_PEAK] = pk.v;
    row[URSO_ENS_ARGMAX] = (double)pk.i;
    row[URSO_ENS_N_MEMBERS] = st4[1];
    row[6] = 0.0;
    row[7] = 0.0;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int urso_ens_add(const urso_ens_add_args* a, void* stream) {
    const char* fn = "urso_ens_add";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->logits || !a->acc || !a->stat) { urso_set_error("%s: null pointer (logits, acc, stat)", fn); return URSO_EINVAL; }
    if (a->B <= 0 || a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B and B > 0 (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->K < 1) { urso_set_error("%s: K must be >= 1 (got %d)", fn, a->K); return URSO_EINVAL; }
    if (a->ld < a->K) { urso_set_error("%s: ld %d < K %d", fn, a->ld, a->K); return URSO_EINVAL; }
    if ((uintptr_t)a->logits & 3) { urso_set_error("%s: logits must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)a->acc | (uintptr_t)a->stat) & 7) { urso_set_error("%s: acc and stat must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * ((double)a->K * (4 + (a->first ? 8 : 16)) + URSO_ENS_STAT * 8));
    URSO_KLAUNCH(ens_add_kernel, dim3(a->n), dim3(ET), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_ens_settle(const urso_ens_settle_args* a, void* stream) {
    const char* fn = "urso_ens_settle";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->acc || !a->stat || !a->logp || !a->table) { urso_set_error("%s: null pointer (acc, stat, logp, table)", fn); return URSO_EINVAL; }
    if (a->n < 0) { urso_set_error("%s: n must be >= 0 (got %d)", fn, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->K < 1) { urso_set_error("%s: K must be >= 1 (got %d)", fn, a->K); return URSO_EINVAL; }
    if (a->M < 1 || a->M > URSO_ENS_MAX_MEMBERS) { urso_set_error("%s: need 1 <= M <= %d (got %d)", fn, URSO_ENS_MAX_MEMBERS, a->M); return URSO_EINVAL; }
    if ((uintptr_t)a->logp & 3) { urso_set_error("%s: logp must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)a->acc | (uintptr_t)a->stat | (uintptr_t)a->table) & 7) {
        urso_set_error("%s: acc, stat and table must be 8-byte aligned", fn);
        return URSO_EINVAL;
    }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * ((double)a->K * (8 + 4) + (URSO_ENS_STAT + URSO_ENS_COLS) * 8));
    URSO_KLAUNCH(ens_settle_kernel, dim3(a->n), dim3(ET), 0, st, *a);
    return urso_check_launch(fn);
}
