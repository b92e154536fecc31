// Exponential moving average of the weights (liburso_ext.so; Config.WEIGHT_EMA): one streaming pass over a second flat
// fp32 buffer behind the optimizer, a one-thread kernel that advances the schedule, and the in-place exchange of two flat buffers that
// evaluates or saves the average.  Formula, state layout and argument rules: include/ursonet_ext.h; ursonet_amd/weight_ema.py is the same
// rule in NumPy float32.
//
// Both passes are HBM-bound streams (update: two 4-byte reads and one 4-byte write per parameter; swap: two and two), so they move 16 bytes
// per lane and access, 256 threads per block and at most 4096 blocks walking the vectors with a grid stride: the shape and the grid of
// sgd_kernel (csrc/pool_loss_optim.hip).  The entry points ask only for 4-byte alignment, so the host splits [0, n) into a scalar head up
// to the first 16-byte boundary, the vectors and a scalar tail; two buffers that sit differently against that boundary are walked by
// scalars alone.  Every element is read and written by exactly one thread, once.
#include "../csrc/common.h"
#include "../../include/ursonet_ext.h"

static constexpr int ET = 256;                                             // threads per block
static constexpr size_t EMA_MAX_BLOCKS = 4096;

// [0, head) scalar, [head, head + 4 nvec) as 16-byte vectors, [head + 4 nvec, n) scalar
struct EmaSplit { size_t head, nvec; int blocks; };
static EmaSplit ema_split(size_t n, const void* a, const void* b) {
    EmaSplit s{n, 0, 1};
    const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15;
    if (ma == mb) {
        s.head = ((16 - ma) & 15) / 4;
        if (s.head > n) s.head = n;
        s.nvec = (n - s.head) / 4;
    }
    size_t work = s.nvec > 0 ? s.nvec : n;                                 // (no vectors: the scalars are dealt to the whole grid)
    size_t blocks = (work + ET - 1) / ET;
    if (blocks > EMA_MAX_BLOCKS) blocks = EMA_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    s.blocks = (int)blocks;
    return s;
}

__device__ __forceinline__ float ema_one(float e, float w, float c) {
    const float diff = w - e;                                               // three fp32 operations, each rounded once (-ffp-contract=off)
    const float prod = c * diff;
    return e + prod;
}

__global__ void __launch_bounds__(ET) ema_update_kernel(size_t n, size_t head, size_t nvec, const float* __restrict__ w, float* __restrict__ ema,
                                                        const float* __restrict__ state, const float* __restrict__ ls) {
    if (ls && ls[URSO_LS_LAST_SKIPPED] != 0.f) return;                      // the optimizer skipped this step: the average keeps its bits
    const float c = 1.0f - state[URSO_EMA_NEXT_DECAY];
    const size_t tid = (size_t)blockIdx.x * ET + threadIdx.x, stride = (size_t)gridDim.x * ET;
    const f32x4_t* wv = (const f32x4_t*)(w + head);
    f32x4_t* ev = (f32x4_t*)(ema + head);
    for (size_t i = tid; i < nvec; i += stride) {
        const f32x4_t a = wv[i];
        f32x4_t e = ev[i];
        e.x = ema_one(e.x, a.x, c); e.y = ema_one(e.y, a.y, c); e.z = ema_one(e.z, a.z, c); e.w = ema_one(e.w, a.w, c);
        ev[i] = e;
    }
    const size_t tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
    for (size_t j = tid; j < nscalar; j += stride) {
        const size_t i = j < head ? j : tail0 + (j - head);
        ema[i] = ema_one(ema[i], w[i], c);
    }
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
    if (!w_d || !ema_d || !state_d) { urso_set_error("%s: null pointer (w, ema, state)", fn); return URSO_EINVAL; }
    if (n < 0) { urso_set_error("%s: n must be >= 0 (got %lld)", fn, (long long)n); return URSO_EINVAL; }
    if ((((uintptr_t)w_d) | ((uintptr_t)ema_d) | ((uintptr_t)state_d) | ((uintptr_t)ls_state_d)) & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const EmaSplit s = ema_split((size_t)n, w_d, ema_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 12);
    URSO_KLAUNCH(ema_update_kernel, dim3(s.blocks), dim3(ET), 0, st, (size_t)n, s.head, s.nvec, w_d, ema_d, (const float*)state_d, ls_state_d);
    URSO_KLAUNCH(ema_advance_kernel, dim3(1), dim3(64), 0, st, state_d, ls_state_d);
    return urso_check_launch(fn);
}

__global__ void __launch_bounds__(ET) ema_swap_kernel(size_t n, size_t head, size_t nvec, int32_t* a, int32_t* b) {
    const size_t tid = (size_t)blockIdx.x * ET + threadIdx.x, stride = (size_t)gridDim.x * ET;
    i32x4_t* av = (i32x4_t*)(a + head);
    i32x4_t* bv = (i32x4_t*)(b + head);
    for (size_t i = tid; i < nvec; i += stride) {
        const i32x4_t x = av[i], y = bv[i];
        av[i] = y; bv[i] = x;
    }
    const size_t tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
    for (size_t j = tid; j < nscalar; j += stride) {
        const size_t i = j < head ? j : tail0 + (j - head);
        const int32_t x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

extern "C" int urso_ema_swap(int64_t n, float* a_d, float* b_d, void* stream) {
    const char* fn = "urso_ema_swap";
    if (!a_d || !b_d) { urso_set_error("%s: null pointer (a, b)", fn); return URSO_EINVAL; }
    if (a_d == b_d) { urso_set_error("%s: a and b are the same buffer", fn); return URSO_EINVAL; }
    if (n < 0) { urso_set_error("%s: n must be >= 0 (got %lld)", fn, (long long)n); return URSO_EINVAL; }
    if ((((uintptr_t)a_d) | ((uintptr_t)b_d)) & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const EmaSplit s = ema_split((size_t)n, a_d, b_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 16);
    URSO_KLAUNCH(ema_swap_kernel, dim3(s.blocks), dim3(ET), 0, st, (size_t)n, s.head, s.nvec, (int32_t*)a_d, (int32_t*)b_d);
    return urso_check_launch(fn);
}
