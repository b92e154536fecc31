// Split conformal prediction on a classification head's PMF (liburso_infer.so; conformal(), predict / evaluate / test_and_submit with
// conformal=...).  urso_conf_score gives, per labelled row, the PMF mass of the bins strictly closer to the estimate
// than the truth is; urso_conf_bound gives, per row, the smallest ball around the estimate that holds more than a level q of the PMF mass:
// a weighted selection over the bins.  The rule, the table layout and the argument rules: include/ursonet_infer.h;
// ursonet_amd/conformal.py (weights64 / score64 / bound64) is the same in NumPy.
//
// Both launches have urso_ens_add's shape: one workgroup of TT = 1024 threads per valid row, columns dealt to threads by their index alone,
// one 16-byte load per group of four where the row is aligned and four 4-byte loads where it is not.  The weights are integers
// (rint(exp(z - m) 2^34) as uint64), so every sum below is exact in any order and LDS atomics may add them.  The selection is a radix
// select over the bit pattern of the keys: after the sweep for the maximum, CP = 6 sweeps of CD = 11 bits from the top; each adds the
// weights and counts of the bins under the prefix chosen so far into 2048-entry histograms in LDS, and a block scan over the histogram
// finds the first digit whose prefix sum passes q.  The first of them sees every bin, so its total is W.  Nothing of size K is kept: the
// row and the map are read again on every sweep, out of L2, and exp is taken again (the work of the kernel: 7 sweeps, 6 exp per bin).
#include "../csrc/common.h"
#include <float.h>
#include <math.h>
#include "../../include/ursonet_infer.h"

typedef unsigned long long u64;
typedef unsigned int u32;

static constexpr int TT = 1024;                                            // threads per workgroup (16 waves)
static constexpr int TW = TT / 64;
static constexpr int CD = URSO_CONF_DIGIT, CP = URSO_CONF_PASSES;
static constexpr int HB = 1 << CD;                                         // histogram entries: two per thread
static_assert(HB == 2 * TT, "the scan takes two histogram entries per thread");
static_assert(CD * CP >= 64 && CD * (CP - 1) < 64, "the digits cover the 64 bits of a key");

// ------------------------------------------------------------------------------------------------ the row
// the larger of two, a NaN winning over everything (fmax would drop it)
__device__ __forceinline__ float cf_max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ float cf_block_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = cf_max_nan(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
    for (int w = 1; w < TW; ++w) r = cf_max_nan(r, sh[w]);
    return r;
}

// Calls f(first column, count) for the calling thread's groups in index order: count = 4 for a group of four columns, the ragged end
// (count = K % 4) once, by the thread whose turn it is.
template <class F>
__device__ __forceinline__ void cf_walk(int K, F f) {
    const int ng = K >> 2;
    for (int g = threadIdx.x; g < ng; g += TT) f(4 * g, 4);
    const int tail = K & 3;
    if (tail && (ng % TT) == (int)threadIdx.x) f(4 * ng, tail);
}

// columns [c, c + cnt) of a row: one 16-byte load for a whole group of an aligned row
__device__ __forceinline__ void cf_load(const float* __restrict__ row, bool aligned, int c, int cnt, float (&z)[4]) {
    if (aligned && cnt == 4) {
        const f32x4_t v = *(const f32x4_t*)(row + c);
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        for (int j = 0; j < cnt; ++j) z[j] = row[c + j];
    }
}

__device__ __forceinline__ float cf_row_max(const float* __restrict__ zrow, bool zal, int K, float* sh) {
    float mt = -INFINITY;
    cf_walk(K, [&](int c, int cnt) {
        float z[4];
        cf_load(zrow, zal, c, cnt, z);
        for (int i = 0; i < cnt; ++i) mt = cf_max_nan(mt, z[i]);
    });
    return cf_block_max(mt, sh);
}

__device__ __forceinline__ u64 cf_weight(float z, double m) {
    const double d = (double)z - m;
    const double e = exp(d);
    const double s = e * 17179869184.0;                                    // 2^URSO_CONF_SHIFT: exact
    return (u64)rint(s);
}
static_assert(URSO_CONF_SHIFT == 34, "cf_weight's constant is 2^34");

// ------------------------------------------------------------------------------------------------ keys
// The rank of a key: its bit pattern, complemented for the angle metric, so that a smaller rank is closer under either metric.
template <int METRIC>
struct CfKey {
    double e[4];
    __device__ __forceinline__ bool load(const double* __restrict__ est) {
        bool fin = true;
        for (int j = 0; j < (METRIC == URSO_CONF_ANGLE ? 4 : 3); ++j) { e[j] = est[j]; fin = fin && __builtin_isfinite(e[j]); }
        return fin;
    }
    __device__ __forceinline__ double key(double h0, double h1, double h2, double h3) const {
        if (METRIC == URSO_CONF_ANGLE) {
            const double p0 = e[0] * h0, p1 = e[1] * h1, p2 = e[2] * h2, p3 = e[3] * h3;
            const double s = ((p0 + p1) + p2) + p3;
            const double a = fabs(s);
            return a > 1.0 ? 1.0 : a;
        }
        const double dx = h0 - e[0], dy = h1 - e[1], dz = h2 - e[2];
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        return (xx + yy) + zz;
    }
    __device__ __forceinline__ double bin(const void* __restrict__ map, int i) const {
        if (METRIC == URSO_CONF_ANGLE) {
            const f32x4_t h = ((const f32x4_t*)map)[i];
            return key((double)h.x, (double)h.y, (double)h.z, (double)h.w);
        }
        const double* __restrict__ p = (const double*)map + 3 * (size_t)i;
        return key(p[0], p[1], p[2], 0.0);
    }
    static __device__ __forceinline__ u64 rank(double key) {
        const u64 b = (u64)__double_as_longlong(key);
        return METRIC == URSO_CONF_ANGLE ? ~b : b;
    }
    static __device__ __forceinline__ double unrank(u64 r) { return __longlong_as_double((long long)(METRIC == URSO_CONF_ANGLE ? ~r : r)); }
    static __device__ __forceinline__ double value(double key) {
        if (METRIC == URSO_CONF_ANGLE) {
            const double a = acos(key);
            return ((2.0 * a) * 180.0) / 3.141592653589793;
        }
        return sqrt(key);
    }
};

__device__ __forceinline__ void cf_nan_row(double* out) {
    if (threadIdx.x < URSO_CONF_COLS) out[threadIdx.x] = __builtin_nan("");
}

__device__ __forceinline__ u64 cf_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ score
template <int METRIC>
__global__ void __launch_bounds__(TT) conf_score_kernel(urso_conf_score_args a) {
    __shared__ u64 shs[3][TW];
    __shared__ float shf[TW];
    const int b = blockIdx.x, K = a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ zrow = a.logits + (size_t)b * (size_t)a.ld_z;
    const bool zal = ((uintptr_t)zrow & 15) == 0;
    double* out = a.out + ((size_t)a.row0 + (size_t)b) * URSO_CONF_COLS;
    const double* __restrict__ ref = a.ref + (size_t)b * (size_t)a.ld_ref;

    const float mf = cf_row_max(zrow, zal, K, shf);
    CfKey<METRIC> ck;
    bool fin = ck.load(a.est + ((size_t)a.row0 + (size_t)b) * (size_t)a.ld_est);
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < (METRIC == URSO_CONF_ANGLE ? 4 : 3); ++j) { r[j] = ref[j]; fin = fin && __builtin_isfinite(r[j]); }
    if (!fin || !__builtin_isfinite(mf)) { cf_nan_row(out); return; }      // the same for every thread of the row
    const double m = (double)mf;
    const double key_ref = ck.key(r[0], r[1], r[2], r[3]);
    const u64 rank_ref = CfKey<METRIC>::rank(key_ref);

    u64 Wt = 0, Ct = 0, Nt = 0;
    cf_walk(K, [&](int c, int cnt) {
        float z[4];
        cf_load(zrow, zal, c, cnt, z);
        for (int i = 0; i < cnt; ++i) {
            const u64 w = cf_weight(z[i], m);
            const bool near = CfKey<METRIC>::rank(ck.bin(a.map, c + i)) < rank_ref;
            Wt += w;
            Ct += near ? w : 0;
            Nt += near ? 1 : 0;
        }
    });
    Wt = cf_wave_sum(Wt); Ct = cf_wave_sum(Ct); Nt = cf_wave_sum(Nt);
    if (lane == 0) { shs[0][wave] = Wt; shs[1][wave] = Ct; shs[2][wave] = Nt; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 W = 0, Cs = 0, N = 0;
    for (int w = 0; w < TW; ++w) { W += shs[0][w]; Cs += shs[1][w]; N += shs[2][w]; }
    out[URSO_CONF_SCORE] = (double)Cs / (double)W;
    out[URSO_CONF_C] = (double)Cs;
    out[URSO_CONF_W] = (double)W;
    out[URSO_CONF_KEY_REF] = key_ref;
    out[URSO_CONF_ERR] = CfKey<METRIC>::value(key_ref);
    out[URSO_CONF_NEAR] = (double)N;
    out[6] = 0.0;
    out[7] = 0.0;
}

// ------------------------------------------------------------------------------------------------ bound
template <int METRIC>
__global__ void __launch_bounds__(TT) conf_bound_kernel(urso_conf_bound_args a) {
    __shared__ u64 hm[HB];                                                 // mass per digit
    __shared__ u32 hc[HB];                                                 // bins per digit
    __shared__ u64 wm[TW];
    __shared__ u32 wc[TW];
    __shared__ float shf[TW];
    __shared__ u64 sel_base, sel_g;
    __shared__ u32 sel_cbase, sel_cnt;
    __shared__ int sel_digit;
    const int b = blockIdx.x, K = a.K, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* __restrict__ zrow = a.logits + (size_t)b * (size_t)a.ld_z;
    const bool zal = ((uintptr_t)zrow & 15) == 0;
    double* out = a.out + ((size_t)a.row0 + (size_t)b) * URSO_CONF_COLS;
    const double q = a.q;

    const float mf = cf_row_max(zrow, zal, K, shf);
    CfKey<METRIC> ck;
    const bool fin = ck.load(a.est + ((size_t)a.row0 + (size_t)b) * (size_t)a.ld_est);
    if (!fin || !__builtin_isfinite(mf)) { cf_nan_row(out); return; }      // the same for every thread of the row
    const double m = (double)mf;

    u64 prefix = 0, base = 0, G = 0, W = 0;                                // base: the mass of the bins whose rank lies below the prefix
    u32 cbase = 0, cnt = 0;
    for (int L = 0; L < CP; ++L) {
        const int top = 64 - CD * L;                                       // the bits [top, 64) are the prefix
        const int shift = top > CD ? top - CD : 0, width = top - shift;
        hm[2 * t] = 0; hm[2 * t + 1] = 0; hc[2 * t] = 0; hc[2 * t + 1] = 0;
        __syncthreads();
        if (t == 0) sel_digit = -1;                                        // behind the barrier: every thread has read the last sweep's choice
        // A thread adds up its bins for as long as they fall under one digit and hands the run to LDS when the digit changes: in the top
        // sweeps nearly all bins share a digit, and one atomic per bin on one address would serialise the workgroup.
        int run_d = -1;
        u64 run_w = 0;
        u32 run_c = 0;
        auto flush = [&]() {
            if (run_d < 0) return;
            if (run_w) atomicAdd(&hm[run_d], run_w);
            atomicAdd(&hc[run_d], run_c);
        };
        cf_walk(K, [&](int c, int cnt4) {
            float z[4];
            cf_load(zrow, zal, c, cnt4, z);
            for (int i = 0; i < cnt4; ++i) {
                const u64 r = CfKey<METRIC>::rank(ck.bin(a.map, c + i));
                if (L == 0 || (r >> top) == prefix) {
                    const int d = (int)((r >> shift) & (u64)((1 << width) - 1));
                    if (d != run_d) { flush(); run_d = d; run_w = 0; run_c = 0; }
                    run_w += cf_weight(z[i], m);
                    run_c += 1;
                }
            }
        });
        flush();
        __syncthreads();
        // the scan: thread t has the digits 2 t and 2 t + 1
        const u64 a0 = hm[2 * t], a1 = hm[2 * t + 1];
        const u32 c0 = hc[2 * t], c1 = hc[2 * t + 1];
        u64 s = a0 + a1;
        u32 sc = c0 + c1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 v = __shfl_up(s, o, 64);
            const u32 vc = __shfl_up(sc, o, 64);
            if (lane >= o) { s += v; sc += vc; }
        }
        if (lane == 63) { wm[wave] = s; wc[wave] = sc; }
        __syncthreads();
        u64 off = 0, total = 0;
        u32 coff = 0;
        for (int w = 0; w < TW; ++w) {
            const u64 x = wm[w];
            const u32 xc = wc[w];
            if (w < wave) { off += x; coff += xc; }
            total += x;
        }
        if (L == 0) W = total;                                             // the first sweep sees every bin
        const double Wd = (double)W;
        const u64 g0 = base + off + (s - (a0 + a1)), g1 = g0 + a0, g2 = g1 + a1;          // the mass below digit 2 t, up to it, up to 2 t + 1
        const u32 n0 = cbase + coff + (sc - (c0 + c1)), n1 = n0 + c0, n2 = n1 + c1;
        const bool p0 = (double)g0 / Wd > q, p1 = (double)g1 / Wd > q, p2 = (double)g2 / Wd > q;
        if (!p0 && p1) { sel_digit = 2 * t; sel_base = g0; sel_g = g1; sel_cbase = n0; sel_cnt = n1; }
        else if (!p1 && p2) { sel_digit = 2 * t + 1; sel_base = g1; sel_g = g2; sel_cbase = n1; sel_cnt = n2; }
        __syncthreads();
        const int digit = sel_digit;
        if (digit < 0) {                                                   // no key qualifies (q >= 1); only the first sweep can end so
            if (t == 0) {
                out[URSO_CONF_BOUND] = METRIC == URSO_CONF_ANGLE ? 180.0 : (double)INFINITY;
                out[URSO_CONF_KEY] = __builtin_nan("");
                out[URSO_CONF_MASS] = 1.0;
                out[URSO_CONF_COUNT] = (double)K;
                out[URSO_CONF_BW] = Wd;
                out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
            }
            return;
        }
        base = sel_base; G = sel_g; cbase = sel_cbase; cnt = sel_cnt;
        prefix = (L == 0 ? 0 : prefix << width) | (u64)digit;
    }
    if (t != 0) return;
    const double key = CfKey<METRIC>::unrank(prefix);
    out[URSO_CONF_BOUND] = CfKey<METRIC>::value(key);
    out[URSO_CONF_KEY] = key;
    out[URSO_CONF_MASS] = (double)G / (double)W;
    out[URSO_CONF_COUNT] = (double)cnt;
    out[URSO_CONF_BW] = (double)W;
    out[5] = 0.0; out[6] = 0.0; out[7] = 0.0;
}

// ------------------------------------------------------------------------------------------------ entry points
static bool cf_bad_common(const char* fn, int B, int n, long long row0, int K, int ld_z, int metric, int ld_est, const void* logits,
                          const void* map, const void* est, const void* out) {
    if (!logits || !map || !est || !out) { urso_set_error("%s: null pointer (logits, map, est, out)", fn); return true; }
    if (n < 0 || n > B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, B, n); return true; }
    if (row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, row0); return true; }
    if (K < 1 || K > URSO_CONF_MAX_K) { urso_set_error("%s: need 1 <= K <= %d (got %d)", fn, URSO_CONF_MAX_K, K); return true; }
    if (ld_z < K) { urso_set_error("%s: ld_z %d < K %d", fn, ld_z, K); return true; }
    if (metric != URSO_CONF_ANGLE && metric != URSO_CONF_EUCLID) { urso_set_error("%s: unknown metric %d", fn, metric); return true; }
    const int D = metric == URSO_CONF_ANGLE ? 4 : 3;
    if (ld_est < D) { urso_set_error("%s: ld_est %d < %d", fn, ld_est, D); return true; }
    if ((uintptr_t)logits & 3) { urso_set_error("%s: logits must be 4-byte aligned", fn); return true; }
    if (((uintptr_t)est | (uintptr_t)out) & 7) { urso_set_error("%s: est and out must be 8-byte aligned", fn); return true; }
    if ((uintptr_t)map & (metric == URSO_CONF_ANGLE ? 15 : 7)) {
        urso_set_error("%s: the map must be %d-byte aligned", fn, metric == URSO_CONF_ANGLE ? 16 : 8);
        return true;
    }
    return false;
}

extern "C" int urso_conf_score(const urso_conf_score_args* a, void* stream) {
    const char* fn = "urso_conf_score";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->ref) { urso_set_error("%s: null pointer (ref)", fn); return URSO_EINVAL; }
    if (cf_bad_common(fn, a->B, a->n, (long long)a->row0, a->K, a->ld_z, a->metric, a->ld_est, a->logits, a->map, a->est, a->out)) return URSO_EINVAL;
    const int D = a->metric == URSO_CONF_ANGLE ? 4 : 3;
    if (a->ld_ref < D) { urso_set_error("%s: ld_ref %d < %d", fn, a->ld_ref, D); return URSO_EINVAL; }
    if ((uintptr_t)a->ref & 7) { urso_set_error("%s: ref must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (double)a->K * (8 + (a->metric == URSO_CONF_ANGLE ? 16 : 24)));
    if (a->metric == URSO_CONF_ANGLE) URSO_KLAUNCH(conf_score_kernel<URSO_CONF_ANGLE>, dim3(a->n), dim3(TT), 0, st, *a);
    else URSO_KLAUNCH(conf_score_kernel<URSO_CONF_EUCLID>, dim3(a->n), dim3(TT), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_conf_bound(const urso_conf_bound_args* a, void* stream) {
    const char* fn = "urso_conf_bound";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (cf_bad_common(fn, a->B, a->n, (long long)a->row0, a->K, a->ld_z, a->metric, a->ld_est, a->logits, a->map, a->est, a->out)) return URSO_EINVAL;
    if (!(a->q > 0.0)) { urso_set_error("%s: q must be > 0 and not NaN (got %g)", fn, a->q); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (double)a->K * (4 + CP * (4 + (a->metric == URSO_CONF_ANGLE ? 16 : 24))));
    if (a->metric == URSO_CONF_ANGLE) URSO_KLAUNCH(conf_bound_kernel<URSO_CONF_ANGLE>, dim3(a->n), dim3(TT), 0, st, *a);
    else URSO_KLAUNCH(conf_bound_kernel<URSO_CONF_EUCLID>, dim3(a->n), dim3(TT), 0, st, *a);
    return urso_check_launch(fn);
}
