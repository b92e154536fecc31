// Sharpness-aware minimization (liburso_train.so; Config.SAM): the ascent to w + rho g / |g| in front of the step's
// second forward / backward pass, the way back behind it, and the one-thread settlement of the ascent count of a loss-scaled step.
// Rule, state layout and argument rules: include/ursonet_train.h; ursonet_amd/sam.py is the same rule in NumPy float32.
//
// Walk: csrc/flat_stream.h.  Both passes are HBM-bound streams (16 and 8 bytes per parameter): the grid covers the vectors, or the
// scalars where the buffers share none.  The ascent walks three buffers: vectors only where all three sit alike against the 16-byte boundary.
#include "../csrc/flat_stream.h"
#include "../../include/ursonet_train.h"

static int sam_blocks(size_t n, const FlatSplit& s) { return flat_blocks(s.nvec > 0 ? s.nvec : n); }

// s = rho / (sqrtf(N) + eps): three fp32 operations, each rounded once (-ffp-contract=off), by the same statements in every thread.
// False where nothing moves: a NaN, infinite or zero norm.
__device__ __forceinline__ bool sam_scale(const float* __restrict__ state, float& s) {
    const float nsq = state[URSO_SAM_NORMSQ];
    s = 0.f;
    if (!(isfinite(nsq) && nsq > 0.f)) return false;
    const float root = sqrtf(nsq);
    const float den = root + state[URSO_SAM_EPS];
    s = state[URSO_SAM_RHO] / den;
    return true;
}

template <class T>                                                          // float or f32x4_t: the product rounded, then the sum
__device__ __forceinline__ T sam_one(const T& w, const T& g, float s) {
    const T e = g * s;
    return w + e;
}

// w0 = w (the bits, whatever they are); w = w + s g where the ascent applies.  Thread 0 of block 0 writes the fields nobody reads here.
__global__ void __launch_bounds__(FLAT_T) sam_ascend_kernel(size_t n, size_t head, size_t nvec, float* __restrict__ w, const float* __restrict__ g,
                                                            float* __restrict__ w0, float* __restrict__ state) {
    float s;
    const bool applied = sam_scale(state, s);
    f32x4_t* wv = (f32x4_t*)(w + head);
    const f32x4_t* gv = (const f32x4_t*)(g + head);
    f32x4_t* w0v = (f32x4_t*)(w0 + head);
    if (applied)
        flat_walk(n, head, nvec, [&](size_t i) { const f32x4_t a = wv[i], b = gv[i]; w0v[i] = a; wv[i] = sam_one(a, b, s); },
                  [&](size_t i) { const float a = w[i], b = g[i]; w0[i] = a; w[i] = sam_one(a, b, s); });
    else
        flat_walk(n, head, nvec, [&](size_t i) { w0v[i] = wv[i]; }, [&](size_t i) { w0[i] = w[i]; });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float a = applied ? 1.f : 0.f;
        state[URSO_SAM_SCALE] = s;
        state[URSO_SAM_APPLIED] = a;
        state[URSO_SAM_APPLIED_TOTAL] = state[URSO_SAM_APPLIED_TOTAL] + a;
        state[URSO_SAM_PENDING] = state[URSO_SAM_PENDING] + a;
    }
}

// w = w0, as integers: no float operation ever sees the bits
__global__ void __launch_bounds__(FLAT_T) sam_descend_kernel(size_t n, size_t head, size_t nvec, int32_t* __restrict__ w, const int32_t* __restrict__ w0) {
    i32x4_t* wv = (i32x4_t*)(w + head);
    const i32x4_t* w0v = (const i32x4_t*)(w0 + head);
    flat_walk(n, head, nvec, [&](size_t i) { wv[i] = w0v[i]; }, [&](size_t i) { w[i] = w0[i]; });
}

// One thread, behind the optimizer's norm: a skipped step takes its ascents out of the count.
__global__ void sam_settle_kernel(float* __restrict__ state, const float* __restrict__ normsq, int guard) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (step_skipped(guard, normsq)) state[URSO_SAM_APPLIED_TOTAL] = state[URSO_SAM_APPLIED_TOTAL] - state[URSO_SAM_PENDING];
    state[URSO_SAM_PENDING] = 0.f;
}

// ------------------------------------------------------------------------------------------------ host
extern "C" int urso_sam_ascend(int64_t n, float* w_d, const float* g_d, float* w0_d, float* state_d, void* stream) {
    const char* fn = "urso_sam_ascend";
    if (flat_refuse(fn, n, "w, g, w0, state", nullptr, {w_d, g_d, w0_d, state_d}) != URSO_OK) return URSO_EINVAL;
    if (w_d == g_d || w_d == w0_d || g_d == w0_d) { urso_set_error("%s: w, g and w0 must be three buffers", fn); return URSO_EINVAL; }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, w_d, g_d, w0_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 16);
    URSO_KLAUNCH(sam_ascend_kernel, dim3(sam_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, w_d, g_d, w0_d, state_d);
    return urso_check_launch(fn);
}

extern "C" int urso_sam_descend(int64_t n, float* w_d, const float* w0_d, void* stream) {
    const char* fn = "urso_sam_descend";
    if (flat_refuse(fn, n, "w, w0", "w and w0", {w_d, w0_d}) != URSO_OK) return URSO_EINVAL;
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, w_d, w0_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 8);
    URSO_KLAUNCH(sam_descend_kernel, dim3(sam_blocks(n, s)), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, (int32_t*)w_d, (const int32_t*)w0_d);
    return urso_check_launch(fn);
}

extern "C" int urso_sam_settle(float* state_d, const float* normsq_d, int guard, void* stream) {
    const char* fn = "urso_sam_settle";
    if (flat_refuse(fn, 0, "state, normsq", nullptr, {state_d, normsq_d}) != URSO_OK) return URSO_EINVAL;
    if (guard != 0 && guard != 1) { urso_set_error("%s: guard must be 0 or 1 (got %d)", fn, guard); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, 8.0 * 4);
    URSO_KLAUNCH(sam_settle_kernel, dim3(1), dim3(64), 0, st, state_d, normsq_d, guard);
    return urso_check_launch(fn);
}
