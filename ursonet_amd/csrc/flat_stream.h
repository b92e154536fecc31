// What the streaming kernels over the flat fp32 parameter buffers share (both libraries; internal, nothing exported): the element walk, the
// order of a block's sum-of-squares slot, the SGD rule and the refusals of the entry points.  Each exists once, here.
//
// The walk.  The passes are HBM-bound streams, so they move 16 bytes per lane and access: 256 threads per block, at most 4096 blocks
// walking the vectors with a grid stride.  The entry points ask only for 4-byte alignment, so the host splits [0, n) into a scalar head up
// to the first 16-byte boundary, the vectors and a scalar tail; buffers (two, or three) that sit differently against that boundary are
// walked by scalars alone.  Thread t of the grid handles the vectors t, t + 256 B, ... and then the scalars t, t + 256 B, ... of head and tail
// counted through.  Every element is read and written by exactly one thread, once.
//
// The slot.  A thread's running sum from 0.0f, squares rounded once, in the order it visits (x y z w of a vector); then the wave's xor
// shuffle (32, 16, ... 1); then the wave partials in wave order from 0.0f: the order of block_sum (loss_dev.h) and so of the finalisation
// launches' slots, which urso_sqnorm_final adds alike (include/ursonet_ext.h).
#ifndef URSO_FLAT_STREAM_H
#define URSO_FLAT_STREAM_H

#include "common.h"
#include <initializer_list>

static constexpr int FLAT_T = 256;                                         // threads per block

// ---------------------------------------------------------------- host: split, grid, refusals
// [0, head) scalar, [head, head + 4 nvec) as 16-byte vectors, [head + 4 nvec, n) scalar
struct FlatSplit { size_t head, nvec; };
// (c: a third buffer walked with the two, or null: vectors only where all of them sit alike)
static inline FlatSplit flat_split(size_t n, const void* a, const void* b, const void* c = nullptr) {
    FlatSplit s{n, 0};
    const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15, mc = c ? (uintptr_t)c & 15 : ma;
    if (ma == mb && ma == mc) {
        s.head = ((16 - ma) & 15) / 4;
        if (s.head > n) s.head = n;
        s.nvec = (n - s.head) / 4;
    }
    return s;
}

// one thread per unit of work, until the grid stride takes over
static inline int flat_blocks(size_t work) {
    const size_t blocks = (work + FLAT_T - 1) / FLAT_T;
    return (int)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}

// The refusals every streaming entry point begins with, in this order: a null pointer among `need` (listed as `names`), n < 0, a pointer
// of `need` or `opt` (which may be null) off the 4-byte boundary, and -- where `same` names them -- the first two of `need` being one buffer.
static inline int flat_refuse(const char* fn, int64_t n, const char* names, const char* same, std::initializer_list<const void*> need,
                              const void* opt = nullptr) {
    uintptr_t bits = (uintptr_t)opt;
    for (const void* p : need) {
        if (!p) { urso_set_error("%s: null pointer (%s)", fn, names); return URSO_EINVAL; }
        bits |= (uintptr_t)p;
    }
    if (n < 0) { urso_set_error("%s: n must be >= 0 (got %lld)", fn, (long long)n); return URSO_EINVAL; }
    if (bits & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (same && need.begin()[0] == need.begin()[1]) { urso_set_error("%s: %s are the same buffer", fn, same); return URSO_EINVAL; }
    return URSO_OK;
}

// ---------------------------------------------------------------- device: walk and slot
// vec(i) for the calling thread's vectors (i counts 16-byte vectors from element `head`), then one(i) for its scalar elements
template <class Vec, class One>
__device__ __forceinline__ void flat_walk(size_t n, size_t head, size_t nvec, Vec vec, One one) {
    const size_t tid = (size_t)blockIdx.x * FLAT_T + threadIdx.x, stride = (size_t)gridDim.x * FLAT_T;
    for (size_t i = tid; i < nvec; i += stride) vec(i);
    const size_t tail0 = head + 4 * nvec, nscalar = head + (n - tail0);
    for (size_t j = tid; j < nscalar; j += stride) one(j < head ? j : tail0 + (j - head));
}

__device__ __forceinline__ void sumsq(float& s, float x) {
    const float xx = x * x;                                                 // the square rounded once (-ffp-contract=off)
    s = s + xx;
}
__device__ __forceinline__ void sumsq4(float& s, const f32x4_t& x) {
    const float a = x.x * x.x, b = x.y * x.y, c = x.z * x.z, d = x.w * x.w;
    s = s + a; s = s + b; s = s + c; s = s + d;
}

// The threads' running sums become the block's, all of them behind one barrier.  True on thread 0 alone, which then holds the sums.
template <class... F>
__device__ __forceinline__ bool flat_block_sums(F&... s) {
    constexpr int N = sizeof...(F);
    __shared__ float sh[N][FLAT_T / 64];
    int k = 0;                                                              // the row of sh of the sum at hand
    ((s = wave_sum(s)), ...);
    if ((threadIdx.x & 63) == 0) ((sh[k++][threadIdx.x >> 6] = s), ...);
    __syncthreads();
    if (threadIdx.x != 0) return false;
    auto waves = [](const float* part) { float r = 0.f; for (int i = 0; i < FLAT_T / 64; ++i) r += part[i]; return r; };
    k = 0;
    ((s = waves(sh[k++])), ...);
    return true;
}

// ---------------------------------------------------------------- device: the SGD rule
// guard (the loss-scaled forms): a step whose squared gradient norm is not finite -- an overflow of the scaled backward pass -- changes nothing
__device__ __forceinline__ bool step_skipped(int guard, const float* __restrict__ normsq) {
    if (guard && !isfinite(normsq[0])) return true;                         // (a branch, not a returned &&: the form under which every
    return false;                                                           // caller compiles to what it compiled to with the test inline)
}

// c, the global-norm clip factor
__device__ __forceinline__ float clip_factor(float clip, const float* __restrict__ normsq) {
    const float norm = sqrtf(normsq[0]);
    return (clip > 0.f && norm >= clip) ? clip / norm : 1.f;
}

// v = mom * v - step * g; w = w + v (T: float or f32x4_t): per element two products, one subtraction, one addition, each rounded once
template <class T>
__device__ __forceinline__ void sgd_one(T& w, const T& g, T& v, float mom, float step) {
    const T a = v * mom;
    const T b = g * step;
    v = a - b;
    w = w + v;
}

#endif
