// What the layer-wise optimizer kernels share (liburso_ext.so: LARS, csrc_ext/lars.hip; liburso_opt.so: LAMB, csrc_opt/lamb.hip; internal,
// nothing exported): the host's check of the tensor table, the block's chunk, the group load and store with a tensor's ragged end by
// scalars, and the float64 sum of a tensor's slots in index order.  Each exists once, here.
//
// The block map (urso_lars_blocks / urso_lars_plan, include/ursonet_ext.h): one block of 256 threads per chunk of URSO_LARS_CHUNK = 4096
// elements of ONE tensor, so that a block's slots belong to one tensor and the result does not depend on how the tensors sit in the flat
// buffer.  Thread t of a block owns the 16-byte groups t, 256 + t, 512 + t, 768 + t of its chunk: four independent accesses per operand in
// flight, consecutive lanes on consecutive addresses.  Nothing outside [offset, offset + numel) is read or written.
#ifndef URSO_LARS_CHUNK_H
#define URSO_LARS_CHUNK_H

#include "flat_stream.h"
#include "../../include/ursonet_ext.h"

#include <algorithm>
#include <vector>

static constexpr int LT = FLAT_T;                                          // threads per block (the slot sum's)
static constexpr int LG = URSO_LARS_CHUNK / (4 * LT);                      // 16-byte groups per thread
static_assert(LG * 4 * LT == URSO_LARS_CHUNK, "a chunk is a whole number of groups per thread");

// ------------------------------------------------------------------------------------------------ host
static inline int lars_count(const char* fn, int T, const int64_t* n_h, int64_t* out) {
    if (T < 0) { urso_set_error("%s: T must be >= 0 (got %d)", fn, T); return URSO_EINVAL; }
    if (T > 0 && !n_h) { urso_set_error("%s: null pointer (n)", fn); return URSO_EINVAL; }
    int64_t nb = 0;
    for (int t = 0; t < T; ++t) {
        if (n_h[t] < 0) { urso_set_error("%s: tensor %d has a negative size (%lld)", fn, t, (long long)n_h[t]); return URSO_EINVAL; }
        nb += (n_h[t] + URSO_LARS_CHUNK - 1) / URSO_LARS_CHUNK;
        if (nb > 0x7fffffff) { urso_set_error("%s: more than 2^31 - 1 blocks", fn); return URSO_EINVAL; }
    }
    *out = nb;
    return URSO_OK;
}

// What the launches over the block map share: the tensor table as the host sees it, checked before any launch.
static inline int lars_check_tensors(const char* fn, int T, const int64_t* off_h, const int64_t* n_h, int nblocks) {
    int64_t nb = 0;
    const int rc = lars_count(fn, T, n_h, &nb);
    if (rc != URSO_OK) return rc;
    if (T > 0 && !off_h) { urso_set_error("%s: null pointer (offsets)", fn); return URSO_EINVAL; }
    if (nblocks != (int)nb) { urso_set_error("%s: nblocks must be urso_lars_blocks(T, n) = %d (got %d)", fn, (int)nb, nblocks); return URSO_EINVAL; }
    bool sorted = true;
    for (int t = 0; t < T; ++t) {
        if (off_h[t] < 0 || (off_h[t] & 3)) {
            urso_set_error("%s: tensor %d: offset %lld is not a non-negative multiple of 4 floats", fn, t, (long long)off_h[t]); return URSO_EINVAL;
        }
        if (off_h[t] > INT64_MAX - n_h[t]) { urso_set_error("%s: tensor %d: offset + size overflows", fn, t); return URSO_EINVAL; }
        if (t > 0 && off_h[t] < off_h[t - 1]) sorted = false;
    }
    std::vector<int> order;
    if (!sorted) {                                                         // (the engine's slices ascend: no allocation on its path)
        order.resize(T);
        for (int t = 0; t < T; ++t) order[t] = t;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return off_h[a] != off_h[b] ? off_h[a] < off_h[b] : a < b; });
    }
    int prev = -1;                                                         // the last non-empty tensor in offset order
    for (int k = 0; k < T; ++k) {
        const int t = sorted ? k : order[k];
        if (n_h[t] == 0) continue;
        if (prev >= 0 && off_h[prev] + n_h[prev] > off_h[t]) {
            urso_set_error("%s: tensors %d and %d overlap ([%lld, +%lld) and [%lld, +%lld))", fn, prev, t, (long long)off_h[prev],
                           (long long)n_h[prev], (long long)off_h[t], (long long)n_h[t]);
            return URSO_EINVAL;
        }
        prev = t;
    }
    return URSO_OK;
}

static inline bool lars_misaligned16(const void* p) { return (((uintptr_t)p) & 15) != 0; }

// ------------------------------------------------------------------------------------------------ device
// The block's chunk: element range [lo, lo + cnt) of the flat buffers, and its tensor.
struct LarsChunk { size_t lo; int cnt; int tensor; };
__device__ __forceinline__ LarsChunk lars_chunk(const int64_t* __restrict__ tab, const int32_t* __restrict__ blockmap) {
    const int t = blockmap[2 * blockIdx.x], c = blockmap[2 * blockIdx.x + 1];
    const int64_t off = tab[2 * t], n = tab[2 * t + 1];
    const int64_t done = (int64_t)c * URSO_LARS_CHUNK, left = n - done;
    return LarsChunk{(size_t)(off + done), (int)(left < URSO_LARS_CHUNK ? left : URSO_LARS_CHUNK), t};
}

// the group's four floats; elements past the chunk's end read as +0 (their squares change no bit of a sum that began at +0) and a
// ragged group is read by scalars: no address outside the tensor is formed
__device__ __forceinline__ f32x4_t lars_load(const float* __restrict__ p, int e, int cnt) {
    f32x4_t x = {0.f, 0.f, 0.f, 0.f};
    if (e + 4 <= cnt) return *(const f32x4_t*)(p + e);
    if (e < cnt) x.x = p[e];
    if (e + 1 < cnt) x.y = p[e + 1];
    if (e + 2 < cnt) x.z = p[e + 2];
    return x;
}

// its counterpart: a whole group in one access, the tensor's ragged end by scalars, so that the padding keeps its bits
__device__ __forceinline__ void lars_store(float* __restrict__ p, int e, int cnt, const f32x4_t& x) {
    if (e + 4 <= cnt) { *(f32x4_t*)(p + e) = x; return; }
    if (e < cnt) p[e] = x.x;
    if (e + 1 < cnt) p[e + 1] = x.y;
    if (e + 2 < cnt) p[e + 2] = x.z;
}

// The float64 sum of a tensor's slots in index order, by one wave.  One lane alone would do that at one dependent load per slot; here the
// 64 lanes of a wave fetch 64 slots at once (the next batch in flight behind the current one), widen them, and every lane adds them in
// index order out of the lanes' registers (two constant-lane reads per slot): the order of a single thread, the loads of a wave.  All
// lanes of the wave return the same sum.  pp: the tensor's first slot of the kind at hand, in a table of slot pairs (stride 2).
__device__ __forceinline__ double lars_readlane(double x, int k) {
    const long long b = __builtin_bit_cast(long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), k);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)lo);
}

__device__ __forceinline__ double lars_slot_sum(const float* __restrict__ pp, int ns, int lane) {
    double s = 0.0;
    double cur = 0.0;
    if (lane < ns) cur = (double)pp[2 * lane];
    for (int base = 0; base < ns; base += 64) {
        double nxt = 0.0;
        if (base + 64 + lane < ns) nxt = (double)pp[2 * (base + 64 + lane)];
        const int m = ns - base;                                            // slots of this batch: min(m, 64), uniform over the wave
        if (m >= 64) {                                                      // a whole batch: straight-line code
#pragma unroll
            for (int k = 0; k < 64; ++k) s = s + lars_readlane(cur, k);
        } else {                                                            // the tensor's last batch (k is uniform over the wave)
            for (int k = 0; k < m; ++k) s = s + lars_readlane(cur, k);
        }
        cur = nxt;
    }
    return s;
}

#endif
