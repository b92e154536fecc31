// Gradient accumulation over micro-batches (liburso_ext.so; Config.GRAD_ACCUM_STEPS): the streaming launch behind the
// backward pass of a micro-step that does not close (acc = g, bit copy | acc += g) and the launch in front of the optimizer of the one that
// does (g = (acc + g) * c, and the sum of squares of what each block stored).  Formula, grid shape and argument rules: include/ursonet_ext.h;
// ursonet_amd/grad_accum.py is the same rule in NumPy float32.
//
// All three are HBM-bound streams (copy: one 4-byte read and one write per parameter; add and close: two and one), so they move 16 bytes per
// lane and access, 256 threads per block and at most 4096 blocks walking the vectors with a grid stride: the shape of ema_update_kernel
// (weight_ema.hip) and sgd_kernel (csrc/pool_loss_optim.hip).  The entry points ask only for 4-byte alignment, so the host splits [0, n)
// into a scalar head up to the first 16-byte boundary, the vectors and a scalar tail; two buffers that sit differently against that
// boundary are walked by scalars alone.  Every element is read and written by exactly one thread, once.  The block count is a function of n
// alone (urso_grad_accum_parts), whatever the alignment: the close launch writes one slot per block.
#include "../csrc/common.h"
#include "../../include/ursonet_ext.h"

static constexpr int GT = 256;                                             // threads per block
static constexpr int64_t GA_MAX_BLOCKS = 4096;

// [0, head) scalar, [head, head + 4 nvec) as 16-byte vectors, [head + 4 nvec, n) scalar
struct GaSplit { size_t head, nvec; };
static GaSplit ga_split(size_t n, const void* a, const void* b) {
    GaSplit s{n, 0};
    const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15;
    if (ma == mb) {
        s.head = ((16 - ma) & 15) / 4;
        if (s.head > n) s.head = n;
        s.nvec = (n - s.head) / 4;
    }
    return s;
}

extern "C" int urso_grad_accum_parts(int64_t n) {
    if (n <= 0) return 0;
    const int64_t blocks = ((n + 3) / 4 + GT - 1) / GT;                     // one thread per 16 bytes, until the grid stride takes over
    return (int)(blocks > GA_MAX_BLOCKS ? GA_MAX_BLOCKS : blocks);
}

// first: the bits of g, NaN payloads included (they move as 32-bit integers); else one fp32 add, rounded once
template <bool FIRST>
__global__ void __launch_bounds__(GT) grad_accum_kernel(size_t n, size_t head, size_t nvec, const float* __restrict__ g, float* __restrict__ acc) {
    const size_t tid = (size_t)blockIdx.x * GT + threadIdx.x, stride = (size_t)gridDim.x * GT;
    const size_t tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
    if (FIRST) {
        const i32x4_t* gv = (const i32x4_t*)(g + head);
        i32x4_t* av = (i32x4_t*)(acc + head);
        for (size_t i = tid; i < nvec; i += stride) av[i] = gv[i];
        const int32_t* gi = (const int32_t*)g;
        int32_t* ai = (int32_t*)acc;
        for (size_t j = tid; j < nscalar; j += stride) {
            const size_t i = j < head ? j : tail0 + (j - head);
            ai[i] = gi[i];
        }
    } else {
        const f32x4_t* gv = (const f32x4_t*)(g + head);
        f32x4_t* av = (f32x4_t*)(acc + head);
        for (size_t i = tid; i < nvec; i += stride) {
            const f32x4_t x = gv[i];
            f32x4_t a = av[i];
            a.x = a.x + x.x; a.y = a.y + x.y; a.z = a.z + x.z; a.w = a.w + x.w;
            av[i] = a;
        }
        for (size_t j = tid; j < nscalar; j += stride) {
            const size_t i = j < head ? j : tail0 + (j - head);
            acc[i] = acc[i] + g[i];
        }
    }
}

__device__ __forceinline__ float close_one(float a, float x, float c, float& sq) {
    const float sum = a + x;                                                // three fp32 operations on the value and two on the running
    const float v = sum * c;                                                // sum of squares, each rounded once (-ffp-contract=off)
    const float vv = v * v;
    sq = sq + vv;
    return v;
}

// g = (acc + g) * c; sqpart[block] = the sum of squares of what the block stored: per thread in the order it stores (its vectors, x y z w
// each, then its scalars), then the wave's xor shuffle (32, 16, ... 1), then the four wave partials in wave order -- the order of the
// finalisation launches' slots (block_sum, csrc/loss_dev.h)
__global__ void __launch_bounds__(GT) grad_close_kernel(size_t n, size_t head, size_t nvec, float* __restrict__ g, const float* __restrict__ acc,
                                                        float c, float* __restrict__ sqpart) {
    __shared__ float sh[GT / 64];
    const size_t tid = (size_t)blockIdx.x * GT + threadIdx.x, stride = (size_t)gridDim.x * GT;
    const f32x4_t* av = (const f32x4_t*)(acc + head);
    f32x4_t* gv = (f32x4_t*)(g + head);
    float sq = 0.f;
    for (size_t i = tid; i < nvec; i += stride) {
        const f32x4_t a = av[i];
        f32x4_t x = gv[i];
        x.x = close_one(a.x, x.x, c, sq); x.y = close_one(a.y, x.y, c, sq); x.z = close_one(a.z, x.z, c, sq); x.w = close_one(a.w, x.w, c, sq);
        gv[i] = x;
    }
    const size_t tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
    for (size_t j = tid; j < nscalar; j += stride) {
        const size_t i = j < head ? j : tail0 + (j - head);
        g[i] = close_one(acc[i], g[i], c, sq);
    }
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int i = 0; i < GT / 64; ++i) r += sh[i];
        sqpart[blockIdx.x] = r;
    }
}

extern "C" int urso_grad_accum(int64_t n, const float* g_d, float* acc_d, int first, void* stream) {
    const char* fn = "urso_grad_accum";
    if (!g_d || !acc_d) { urso_set_error("%s: null pointer (g, acc)", fn); return URSO_EINVAL; }
    if (n < 0) { urso_set_error("%s: n must be >= 0 (got %lld)", fn, (long long)n); return URSO_EINVAL; }
    if ((((uintptr_t)g_d) | ((uintptr_t)acc_d)) & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (g_d == acc_d) { urso_set_error("%s: g and acc are the same buffer", fn); return URSO_EINVAL; }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const GaSplit s = ga_split((size_t)n, g_d, acc_d);
    const int blocks = urso_grad_accum_parts(n);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * (first ? 8 : 12));
    if (first) URSO_KLAUNCH(grad_accum_kernel<true>, dim3(blocks), dim3(GT), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d);
    else       URSO_KLAUNCH(grad_accum_kernel<false>, dim3(blocks), dim3(GT), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d);
    return urso_check_launch(fn);
}

extern "C" int urso_grad_accum_close(int64_t n, float* g_d, const float* acc_d, float c, float* sqpart_d, int nparts, void* stream) {
    const char* fn = "urso_grad_accum_close";
    if (!g_d || !acc_d || !sqpart_d) { urso_set_error("%s: null pointer (g, acc, sqpart)", fn); return URSO_EINVAL; }
    if (n < 0) { urso_set_error("%s: n must be >= 0 (got %lld)", fn, (long long)n); return URSO_EINVAL; }
    if ((((uintptr_t)g_d) | ((uintptr_t)acc_d) | ((uintptr_t)sqpart_d)) & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (g_d == acc_d) { urso_set_error("%s: g and acc are the same buffer", fn); return URSO_EINVAL; }
    if (nparts != urso_grad_accum_parts(n)) {
        urso_set_error("%s: nparts must be urso_grad_accum_parts(n) = %d (got %d)", fn, urso_grad_accum_parts(n), nparts); return URSO_EINVAL;
    }
    if (n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const GaSplit s = ga_split((size_t)n, g_d, acc_d);
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)n * 12);
    URSO_KLAUNCH(grad_close_kernel, dim3(nparts), dim3(GT), 0, st, (size_t)n, s.head, s.nvec, g_d, acc_d, c, sqpart_d);
    return urso_check_launch(fn);
}
