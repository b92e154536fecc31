// Stochastic weight averaging and SWAG-diagonal (liburso_train.so; Config.SWA): one streaming pass behind the optimizer
// that folds the weights into a running mean (and a running mean of squares) on the steps the device-side state collects, a one-thread
// kernel that advances that state, and the pass that draws one weight set from the diagonal Gaussian.  Rules, state layout and argument
// rules: include/ursonet_train.h; ursonet_amd/swa.py is the same in NumPy.
//
// Walk: csrc/flat_stream.h.  The grid covers the vectors, or the scalars where the buffers share none.  The exchange of the average with
// the weights is urso_ema_swap's (liburso_ext.so).
#include "../csrc/flat_stream.h"
#include "../../include/ursonet_train.h"
#include "../../include/ursonet_loss_scale.h"

static int swa_blocks(size_t n, const FlatSplit& s) { return flat_blocks(s.nvec > 0 ? s.nvec : n); }

// ------------------------------------------------------------------------------------------------ collection
// The step the state stands in front of: its tick and whether it collects.  The same statements in every thread and in the advance.
__device__ __forceinline__ bool swa_gate(const int32_t* __restrict__ state, int32_t& ticks) {
    const int32_t period = state[URSO_SWA_PERIOD], start = state[URSO_SWA_START], t = state[URSO_SWA_TICKS];
    ticks = t < INT32_MAX ? t + 1 : INT32_MAX;
    if (period <= 0 || ticks <= start) return false;
    return (ticks - start) % period == 0 && state[URSO_SWA_MODELS] < URSO_SWA_MAX_MODELS;
}

template <class T>                                                          // float or f32x4_t: three fp32 operations, each rounded once
__device__ __forceinline__ T swa_one(const T& avg, const T& x, float r) {
    const T diff = x - avg;
    const T prod = diff * r;
    return avg + prod;
}

template <bool SQ>
__global__ void __launch_bounds__(FLAT_T) swa_update_kernel(size_t n, size_t head, size_t nvec, const float* __restrict__ w, float* __restrict__ mean,
                                                            float* __restrict__ sq, const int32_t* __restrict__ state, const float* __restrict__ ls) {
    if (ls && ls[URSO_LS_LAST_SKIPPED] != 0.f) return;                      // the optimizer skipped this step
    if ((state[URSO_SWA_VARIANCE] != 0) != SQ) return;                      // a sq buffer the state does not ask for, or none where it does
    int32_t ticks;
    if (!swa_gate(state, ticks)) return;                                    // the gate is shut: no block touches memory
    const int32_t m = state[URSO_SWA_MODELS] + 1;                           // this model's number
    const f32x4_t* wv = (const f32x4_t*)(w + head);
    f32x4_t* mv = (f32x4_t*)(mean + head);
    f32x4_t* qv = (f32x4_t*)(sq + head);                                    // (never dereferenced without SQ)
    if (m == 1) {                                                           // the first model is copied: mean + (w - mean) would round
        flat_walk(n, head, nvec,
                  [&](size_t i) { const f32x4_t a = wv[i]; mv[i] = a; if (SQ) qv[i] = a * a; },
                  [&](size_t i) { const float a = w[i]; mean[i] = a; if (SQ) sq[i] = a * a; });
        return;
    }
    // fl32(1 / m): the fp64 quotient of two fp32-exact values rounds to fp32 as the exact quotient does (53 >= 2 * 24 + 2 bits)
    const float r = (float)(1.0 / (double)m);
    flat_walk(n, head, nvec,
              [&](size_t i) {
                  const f32x4_t a = wv[i];
                  mv[i] = swa_one(mv[i], a, r);
                  if (SQ) { const f32x4_t aa = a * a; qv[i] = swa_one(qv[i], aa, r); }
              },
              [&](size_t i) {
                  const float a = w[i];
                  mean[i] = swa_one(mean[i], a, r);
                  if (SQ) { const float aa = a * a; sq[i] = swa_one(sq[i], aa, r); }
              });
}

// One thread, behind the update on the same stream: every block of the update has read the state by then.
__global__ void swa_advance_kernel(int32_t* __restrict__ state, const float* __restrict__ ls, int has_sq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ls && ls[URSO_LS_LAST_SKIPPED] != 0.f) return;
    if ((state[URSO_SWA_VARIANCE] != 0) != (has_sq != 0)) { state[URSO_SWA_COLLECTED] = URSO_SWA_REFUSED; return; }
    int32_t ticks;
    const bool collect = swa_gate(state, ticks);
    state[URSO_SWA_TICKS] = ticks;
    if (collect) state[URSO_SWA_MODELS] = state[URSO_SWA_MODELS] + 1;
    state[URSO_SWA_COLLECTED] = collect ? 1 : 0;
}

// [a, a + n) and [b, b + n) of 4-byte elements share a byte
static inline bool swa_overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * 4;
    return x < y + len && y < x + len;
}

extern "C" int urso_swa_update(int64_t n, const float* w_d, float* mean_d, float* sq_d, int32_t* state_d, const float* ls_state_d, void* stream) {
    const char* fn = "urso_swa_update";
    if (flat_refuse(fn, n, "w, mean, state", nullptr, {w_d, mean_d, state_d}, ls_state_d) != URSO_OK) return URSO_EINVAL;
    if ((uintptr_t)sq_d & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (w_d == mean_d || (sq_d && (sq_d == w_d || sq_d == mean_d)) || (n > 0 && (swa_overlap(w_d, mean_d, n) ||
        (sq_d && (swa_overlap(sq_d, w_d, n) || swa_overlap(sq_d, mean_d, n)))))) {
        urso_set_error("%s: w, mean and sq must be distinct buffers that do not overlap", fn);
        return URSO_EINVAL;
    }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, w_d, mean_d, sq_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * (sq_d ? 20 : 12));
    if (sq_d)
        URSO_KLAUNCH(swa_update_kernel<true>, dim3(swa_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, w_d, mean_d, sq_d,
                     (const int32_t*)state_d, ls_state_d);
    else
        URSO_KLAUNCH(swa_update_kernel<false>, dim3(swa_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, w_d, mean_d, sq_d,
                     (const int32_t*)state_d, ls_state_d);
    URSO_KLAUNCH(swa_advance_kernel, dim3(1), dim3(64), 0, st, state_d, ls_state_d, sq_d ? 1 : 0);
    return urso_check_launch(fn);
}

// ------------------------------------------------------------------------------------------------ sampling
// Philox-4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t x[4]) {
#pragma unroll
    for (int rnd = 0; rnd < 10; ++rnd) {
        if (rnd) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// The four normals of elements 4 b .. 4 b + 3 of the flat buffer, in float64 (each operation rounded once) and rounded to float32 at the end
__device__ __forceinline__ f32x4_t swag_normals(uint64_t b, uint64_t seed, uint32_t sample) {
    uint32_t x[4];
    philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), sample, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    const double u0 = ((double)x[0] + 0.5) * 0x1p-32, u1 = ((double)x[1] + 0.5) * 0x1p-32;      // exact: 33 bits
    const double u2 = ((double)x[2] + 0.5) * 0x1p-32, u3 = ((double)x[3] + 0.5) * 0x1p-32;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    const double t0 = 6.283185307179586 * u1, t1 = 6.283185307179586 * u3;
    double s0, c0, s1, c1;
    sincos(t0, &s0, &c0);
    sincos(t1, &s1, &c1);
    f32x4_t z;
    z.x = (float)(r0 * c0); z.y = (float)(r0 * s0); z.z = (float)(r1 * c1); z.w = (float)(r1 * s1);
    return z;
}

template <class T>                                                          // float or f32x4_t: five fp32 operations and sqrtf, each rounded once
__device__ __forceinline__ T swag_one(const T& mean, const T& sq, const T& z, float s);
template <>
__device__ __forceinline__ float swag_one<float>(const float& mean, const float& sq, const float& z, float s) {
    const float mm = mean * mean;
    const float d = sq - mm;
    const float sd = sqrtf(d > 0.f ? d : 0.f);                              // (a NaN difference counts as 0)
    const float t = s * sd;
    const float p = t * z;
    return mean + p;
}
template <>
__device__ __forceinline__ f32x4_t swag_one<f32x4_t>(const f32x4_t& mean, const f32x4_t& sq, const f32x4_t& z, float s) {
    f32x4_t o;
    o.x = swag_one(mean.x, sq.x, z.x, s); o.y = swag_one(mean.y, sq.y, z.y, s);
    o.z = swag_one(mean.z, sq.z, z.z, s); o.w = swag_one(mean.w, sq.w, z.w, s);
    return o;
}

__device__ __forceinline__ float lane_of(const f32x4_t& v, unsigned k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// first: the flat-buffer index of element 0 (a multiple of 4).  A 16-byte vector of the walk begins at element head + 4 i, so with
// head == 0 it is one Philox block; otherwise it takes the end of one block and the beginning of the next.
__global__ void __launch_bounds__(FLAT_T) swag_sample_kernel(size_t n, size_t head, size_t nvec, uint64_t first, const float* __restrict__ mean,
                                                             const float* __restrict__ sq, float* __restrict__ out, float* __restrict__ zout,
                                                             float s, uint64_t seed, uint32_t sample) {
    const f32x4_t* mv = (const f32x4_t*)(mean + head);
    const f32x4_t* qv = (const f32x4_t*)(sq + head);
    f32x4_t* ov = (f32x4_t*)(out + head);
    f32x4_t* zv = (f32x4_t*)(zout + head);                                  // (never dereferenced where zout is null)
    const uint64_t b0 = first >> 2;
    const unsigned k = (unsigned)head;                                      // 0 .. 3
    flat_walk(n, head, nvec,
              [&](size_t i) {
                  f32x4_t z = swag_normals(b0 + i, seed, sample);
                  if (k) {
                      const f32x4_t y = swag_normals(b0 + i + 1, seed, sample);
                      f32x4_t t;
                      t.x = lane_of(z, k);
                      t.y = k + 1 < 4 ? lane_of(z, k + 1) : lane_of(y, k + 1 - 4);
                      t.z = k + 2 < 4 ? lane_of(z, k + 2) : lane_of(y, k + 2 - 4);
                      t.w = lane_of(y, k + 3 - 4);
                      z = t;
                  }
                  if (zout) zv[i] = z;
                  ov[i] = swag_one(mv[i], qv[i], z, s);
              },
              [&](size_t i) {
                  const float z = lane_of(swag_normals(b0 + (i >> 2), seed, sample), (unsigned)(i & 3));
                  if (zout) zout[i] = z;
                  out[i] = swag_one(mean[i], sq[i], z, s);
              });
}

extern "C" int urso_swag_sample(int64_t n, int64_t first, const float* mean_d, const float* sq_d, float* out_d, float* z_out_d, float s,
                                uint64_t seed, int sample, void* stream) {
    const char* fn = "urso_swag_sample";
    if (flat_refuse(fn, n, "mean, sq, out", nullptr, {mean_d, sq_d, out_d}, z_out_d) != URSO_OK) return URSO_EINVAL;
    if (first < 0 || (first & 3)) { urso_set_error("%s: first must be a multiple of 4 and >= 0 (got %lld)", fn, (long long)first); return URSO_EINVAL; }
    if (!(s >= 0.f) || !(s <= 3.402823466e38f)) { urso_set_error("%s: s must be finite and >= 0 (got %g)", fn, (double)s); return URSO_EINVAL; }
    if (sample < 0) { urso_set_error("%s: sample must be >= 0 (got %d)", fn, sample); return URSO_EINVAL; }
    const bool alias = out_d == mean_d || out_d == sq_d || (z_out_d && (z_out_d == mean_d || z_out_d == sq_d || z_out_d == out_d)) ||
                       (n > 0 && (swa_overlap(out_d, mean_d, n) || swa_overlap(out_d, sq_d, n) ||
                                  (z_out_d && (swa_overlap(z_out_d, mean_d, n) || swa_overlap(z_out_d, sq_d, n) || swa_overlap(z_out_d, out_d, n)))));
    if (alias) { urso_set_error("%s: out and z_out must be buffers of their own that overlap nothing", fn); return URSO_EINVAL; }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    FlatSplit sp = flat_split((size_t)n, mean_d, sq_d, out_d);
    if (z_out_d && (((uintptr_t)z_out_d ^ (uintptr_t)out_d) & 15)) sp = FlatSplit{(size_t)n, 0};       // z_out sits differently: scalars alone
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * (z_out_d ? 16 : 12));
    URSO_KLAUNCH(swag_sample_kernel, dim3(swa_blocks(n, sp)), dim3(FLAT_T), 0, st, (size_t)n, sp.head, sp.nvec, (uint64_t)first, mean_d, sq_d, out_d,
                 z_out_d, s, seed, (uint32_t)sample);
    return urso_check_launch(fn);
}
