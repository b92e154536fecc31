// Exponential moving average of the weights (liburso_ext.so; Config.WEIGHT_EMA): one streaming pass over a second flat
// fp32 buffer behind the optimizer, a one-thread kernel that advances the schedule, and the in-place exchange of two flat buffers that
// evaluates or saves the average.  Formula, state layout and argument rules: include/ursonet_ext.h; ursonet_amd/weight_ema.py is the same
// rule in NumPy float32.
//
// Walk: csrc/flat_stream.h.  The grid covers the vectors, or the scalars where the two buffers share none: flat_blocks(nvec > 0 ? nvec : n).
#include "../csrc/flat_stream.h"
#include "../../include/ursonet_ext.h"

static int ema_blocks(size_t n, const FlatSplit& s) { return flat_blocks(s.nvec > 0 ? s.nvec : n); }

template <class T>                                                          // float or f32x4_t
__device__ __forceinline__ T ema_one(const T& e, const T& w, float c) {
    const T diff = w - e;                                                   // per element three fp32 operations, each rounded once
    const T prod = c * diff;                                                // (-ffp-contract=off)
    return e + prod;
}

__global__ void __launch_bounds__(FLAT_T) ema_update_kernel(size_t n, size_t head, size_t nvec, const float* __restrict__ w, float* __restrict__ ema,
                                                            const float* __restrict__ state, const float* __restrict__ ls) {
    if (ls && ls[URSO_LS_LAST_SKIPPED] != 0.f) return;                      // the optimizer skipped this step: the average keeps its bits
    const float c = 1.0f - state[URSO_EMA_NEXT_DECAY];
    const f32x4_t* wv = (const f32x4_t*)(w + head);
    f32x4_t* ev = (f32x4_t*)(ema + head);
    flat_walk(n, head, nvec, [&](size_t i) { const f32x4_t a = wv[i]; ev[i] = ema_one(ev[i], a, c); }, [&](size_t i) { ema[i] = ema_one(ema[i], w[i], c); });
}

// One thread, behind the update on the same stream: every block of the update has read NEXT_DECAY by then.
__global__ void ema_advance_kernel(float* __restrict__ state, const float* __restrict__ ls) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ls && ls[URSO_LS_LAST_SKIPPED] != 0.f) return;
    const float decay = state[URSO_EMA_DECAY];
    const float t = fminf(state[URSO_EMA_UPDATES] + 1.0f, 16777216.0f);
    float next = decay;
    if (state[URSO_EMA_WARMUP] != 0.f) {
        // fl32((1 + t) / (10 + t)): the two sums are fp32 (exact below 2^24), and the fp64 quotient of two fp32 values rounds to fp32 as
        // the exact quotient does (53 >= 2 * 24 + 2 bits).  Written this way the value does not depend on the fp32 division mode the
        // library is compiled under (the compiler may narrow it to its correctly rounded fp32 division: the same value by that argument)
        const float num = 1.0f + t, den = 10.0f + t;
        next = fminf(decay, (float)((double)num / (double)den));
    }
    state[URSO_EMA_UPDATES] = t;
    state[URSO_EMA_NEXT_DECAY] = next;
}

extern "C" int urso_ema_update(int64_t n, const float* w_d, float* ema_d, float* state_d, const float* ls_state_d, void* stream) {
    const char* fn = "urso_ema_update";
    if (flat_refuse(fn, n, "w, ema, state", nullptr, {w_d, ema_d, state_d}, ls_state_d) != URSO_OK) return URSO_EINVAL;
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, w_d, ema_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 12);
    URSO_KLAUNCH(ema_update_kernel, dim3(ema_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, w_d, ema_d, (const float*)state_d, ls_state_d);
    URSO_KLAUNCH(ema_advance_kernel, dim3(1), dim3(64), 0, st, state_d, ls_state_d);
    return urso_check_launch(fn);
}

__global__ void __launch_bounds__(FLAT_T) ema_swap_kernel(size_t n, size_t head, size_t nvec, int32_t* a, int32_t* b) {
    i32x4_t* av = (i32x4_t*)(a + head);
    i32x4_t* bv = (i32x4_t*)(b + head);
    flat_walk(n, head, nvec,
              [&](size_t i) { const i32x4_t x = av[i], y = bv[i]; av[i] = y; bv[i] = x; },
              [&](size_t i) { const int32_t x = a[i], y = b[i]; a[i] = y; b[i] = x; });
}

extern "C" int urso_ema_swap(int64_t n, float* a_d, float* b_d, void* stream) {
    const char* fn = "urso_ema_swap";
    // (this entry point refuses one buffer given twice ahead of n < 0)
    if (a_d && a_d == b_d) { urso_set_error("%s: a and b are the same buffer", fn); return URSO_EINVAL; }
    if (flat_refuse(fn, n, "a, b", nullptr, {a_d, b_d}) != URSO_OK) return URSO_EINVAL;
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, a_d, b_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 16);
    URSO_KLAUNCH(ema_swap_kernel, dim3(ema_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, (int32_t*)a_d, (int32_t*)b_d);
    return urso_check_launch(fn);
}

