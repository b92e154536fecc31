// Gradient accumulation over micro-batches (liburso_ext.so; Config.GRAD_ACCUM_STEPS): the streaming launch behind the
// backward pass of a micro-step that does not close (acc = g, bit copy | acc += g) and the launch in front of the optimizer of the one that
// does (g = (acc + g) * c, and the sum of squares of what each block stored).  Formula, grid shape and argument rules: include/ursonet_ext.h;
// ursonet_amd/grad_accum.py is the same rule in NumPy float32.  Walk and slot order: csrc/flat_stream.h.  The block count is a function of
// n alone (urso_grad_accum_parts), whatever the alignment: the close launch writes one slot per block.
#include "../csrc/flat_stream.h"
#include "../../include/ursonet_ext.h"

extern "C" int urso_grad_accum_parts(int64_t n) { return n <= 0 ? 0 : flat_blocks(((size_t)n + 3) / 4); }

// first: the bits of g, NaN payloads included (they move as 32-bit integers); else one fp32 add, rounded once
template <bool FIRST>
__global__ void __launch_bounds__(FLAT_T) grad_accum_kernel(size_t n, size_t head, size_t nvec, const float* __restrict__ g, float* __restrict__ acc) {
    if (FIRST) {
        const i32x4_t* gv = (const i32x4_t*)(g + head);
        i32x4_t* av = (i32x4_t*)(acc + head);
        const int32_t* gi = (const int32_t*)g;
        int32_t* ai = (int32_t*)acc;
        flat_walk(n, head, nvec, [&](size_t i) { av[i] = gv[i]; }, [&](size_t i) { ai[i] = gi[i]; });
    } else {
        const f32x4_t* gv = (const f32x4_t*)(g + head);
        f32x4_t* av = (f32x4_t*)(acc + head);
        flat_walk(n, head, nvec, [&](size_t i) { const f32x4_t x = gv[i]; av[i] = av[i] + x; }, [&](size_t i) { acc[i] = acc[i] + g[i]; });
    }
}

__device__ __forceinline__ float close_one(float a, float x, float c, float& sq) {
    const float sum = a + x;                                                // two fp32 operations on the value, each rounded once
    const float v = sum * c;                                                // (-ffp-contract=off), and the slot's step
    sumsq(sq, v);
    return v;
}

// g = (acc + g) * c; sqpart[block] = the sum of squares of what the block stored, per thread in the order it stores
__global__ void __launch_bounds__(FLAT_T) grad_close_kernel(size_t n, size_t head, size_t nvec, float* __restrict__ g, const float* __restrict__ acc,
                                                            float c, float* __restrict__ sqpart) {
    const f32x4_t* av = (const f32x4_t*)(acc + head);
    f32x4_t* gv = (f32x4_t*)(g + head);
    float sq = 0.f;
    flat_walk(n, head, nvec,
              [&](size_t i) {
                  const f32x4_t a = av[i];
                  f32x4_t x = gv[i];
                  x.x = close_one(a.x, x.x, c, sq); x.y = close_one(a.y, x.y, c, sq); x.z = close_one(a.z, x.z, c, sq); x.w = close_one(a.w, x.w, c, sq);
                  gv[i] = x;
              },
              [&](size_t i) { g[i] = close_one(acc[i], g[i], c, sq); });
    if (flat_block_sums(sq)) sqpart[blockIdx.x] = sq;
}

extern "C" int urso_grad_accum(int64_t n, const float* g_d, float* acc_d, int first, void* stream) {
    const char* fn = "urso_grad_accum";
    if (flat_refuse(fn, n, "g, acc", "g and acc", {g_d, acc_d}) != URSO_OK) return URSO_EINVAL;
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, g_d, acc_d);
    const int blocks = urso_grad_accum_parts(n);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * (first ? 8 : 12));
    if (first) URSO_KLAUNCH(grad_accum_kernel<true>, dim3(blocks), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d);
    else       URSO_KLAUNCH(grad_accum_kernel<false>, dim3(blocks), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d);
    return urso_check_launch(fn);
}

extern "C" int urso_grad_accum_close(int64_t n, float* g_d, const float* acc_d, float c, float* sqpart_d, int nparts, void* stream) {
    const char* fn = "urso_grad_accum_close";
    if (flat_refuse(fn, n, "g, acc, sqpart", "g and acc", {g_d, acc_d, sqpart_d}) != URSO_OK) return URSO_EINVAL;
    if (nparts != urso_grad_accum_parts(n)) {
        urso_set_error("%s: nparts must be urso_grad_accum_parts(n) = %d (got %d)", fn, urso_grad_accum_parts(n), nparts); return URSO_EINVAL;
    }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatSplit s = flat_split((size_t)n, g_d, acc_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 12);
    URSO_KLAUNCH(grad_close_kernel, dim3(nparts), dim3(FLAT_T), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d, c, sqpart_d);
    return urso_check_launch(fn);
}
