// Device-resident cache of RAW frames (ursonet_amd/frame_cache.py, Config.DEVICE_CACHE_GB): three kernels of pure byte movement.
//   urso_frames_grey_flags_u8   which frames of an uploaded RGB batch are grey (R == G == B everywhere): those are stored as ONE plane
//   urso_frames_put_u8          uploaded frame b -> its cache slot (kind 0: channel 0 only, kind 1: all 3 HW bytes, kind 2: nothing)
//   urso_frames_gather_u8       batch slot b <- a cache slot or an uploaded frame (kind 0: grey plane expanded to RGB, 1: copy, 2: nothing)
// A frame is a flat array of HW pixels.  All three are HBM-bound, so the whole design is "16 bytes per lane per access, enough of
// them in flight": one grid over (chunk, batch slot), 256 threads, a chunk = FC_UNITS units of 16 pixels (16 grey bytes <-> 48 RGB bytes)
// = 48 KiB of RGB, which gives 2,400 blocks for 32 URSO frames and keeps 12 independent 16-byte loads in flight per thread before the
// first store (the source and destination come from address tables, so the compiler may not move a load across a store itself).
//
// Alignment.  The 16-byte STORES are always aligned: a slot starts with a bytewise head up to the first 16-byte boundary of its
// destination (for the RGB side of an expansion: the first PIXEL whose first byte lies on one, 3 p = -dst mod 16 <=> p = 11 (-dst) mod 16,
// 11 being the inverse of 3), then the vector body, then a bytewise tail.  The LOADS are aligned whenever source and destination agree
// mod 16 -- always for real frames (HW a multiple of 16, slot strides multiples of 16) -- and are left to the compiler as alignment-1
// accesses otherwise (odd test shapes).  The flags kernel only reads and aligns its source the same way.
//
// Every offset is derived from HW and the slot's address and stays inside [0, HW) resp. [0, 3 HW) of that slot; chunks past a slot's
// body return.  Slots of kind 2 (and null addresses) touch no memory.  Plain C++ with vector stores only.
#include "common.h"
#include <string.h>

#define FC_THREADS 256
#define FC_UPT 4                               // units of 16 pixels per thread and chunk
#define FC_UNITS (FC_THREADS * FC_UPT)         // units per chunk: 16,384 pixels
#define FC_VPT (3 * FC_UPT)                    // 16-byte vectors per thread and chunk on the RGB side

template <bool ALIGNED>
__device__ __forceinline__ uint4 fc_load16(const uint8_t* p) {
    uint4 v;
    if (ALIGNED) v = *(const uint4*)p;
    else __builtin_memcpy(&v, p, 16);          // alignment 1: the compiler picks the widest access the target allows
    return v;
}
__device__ __forceinline__ void fc_store16(uint8_t* p, uint4 v) { *(uint4*)p = v; }     // p is 16-byte aligned by construction

// byte i (compile-time after unrolling) of a little-endian dword array
__device__ __forceinline__ uint32_t fc_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

__device__ __forceinline__ int fc_head_bytes(const void* p) { return (int)((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u); }
// pixels before the first pixel whose RGB triple starts on a 16-byte boundary
__device__ __forceinline__ int fc_head_pixels_rgb(const void* p) { return (int)((fc_head_bytes(p) * 11u) & 15u); }

// 48 RGB bytes (12 dwords): nonzero iff some pixel has R != G or G != B.  x[i] = byte i ^ byte i+1 must vanish unless i = 2 mod 3.
__device__ __forceinline__ uint32_t fc_unit_not_grey(const uint32_t* w) {
    uint32_t bad = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const uint32_t next = k < 11 ? w[k + 1] : 0u;
        const uint32_t x = w[k] ^ ((w[k] >> 8) | (next << 24));
        const uint32_t mask = (k % 3 == 0) ? 0xFF00FFFFu : ((k % 3 == 1) ? 0xFFFF00FFu : 0x00FFFF00u);
        bad |= x & mask;
    }
    return bad;
}

__global__ void frames_flags_init_kernel(int B, uint8_t* flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) flags[b] = 1;
}

template <bool ALIGNED>
__device__ __forceinline__ uint32_t fc_flags_body(const uint8_t* body, long long nu, long long u0) {
    uint32_t bad = 0;
    uint32_t w[FC_UPT][12];
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) {
        const long long u = u0 + (long long)k * FC_THREADS;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (u < nu) v = fc_load16<ALIGNED>(body + u * 48 + j * 16);
            w[k][4 * j] = v.x; w[k][4 * j + 1] = v.y; w[k][4 * j + 2] = v.z; w[k][4 * j + 3] = v.w;
        }
    }
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) bad |= fc_unit_not_grey(w[k]);      // a unit past the end is all zeros: grey
    return bad;
}

// flags[b] &= "chunk blockIdx.x of frame b is grey".  One __syncthreads_or per block, then at most one BYTE store of the constant 0
// per block.  frames_flags_init_kernel has set the flag to 1 earlier on the stream and every writer here stores the same value into a
// single byte, so the combination is an integer AND that is idempotent and independent of the order in which the blocks run -- and,
// unlike a 32-bit atomic on the word around the byte, it touches nothing outside [flags, flags + B), wherever flags sits.
__global__ __launch_bounds__(FC_THREADS) void frames_grey_flags_kernel(int HW, const uint8_t* src, uint8_t* flags) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint8_t* f = src + (size_t)b * 3 * (size_t)HW;
    const int hp = min(HW, fc_head_pixels_rgb(f));
    const long long nu = (HW - hp) >> 4;
    const long long c0 = (long long)blockIdx.x * FC_UNITS;
    if (blockIdx.x > 0 && c0 >= nu) return;
    const uint8_t* body = f + 3 * (size_t)hp;
    const bool aligned = (((uintptr_t)body) & 15) == 0;                  // false only when HW < the head (no body at all)
    uint32_t bad = 0;
    if (c0 < nu) bad = aligned ? fc_flags_body<true>(body, nu, c0 + tid) : fc_flags_body<false>(body, nu, c0 + tid);
    if (blockIdx.x == 0) {                                              // head and tail pixels, one per thread
        const int tail0 = hp + (int)(nu << 4);
        int p = -1;
        if (tid < hp) p = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < HW) p = tail0 + (tid - 64);
        if (p >= 0) {
            const uint8_t r = f[3 * (size_t)p], g = f[3 * (size_t)p + 1], bl = f[3 * (size_t)p + 2];
            bad |= (uint32_t)((r ^ g) | (g ^ bl));
        }
    }
    if (__syncthreads_or(bad != 0) && tid == 0) *(volatile uint8_t*)(flags + b) = 0;
}

// n bytes s -> d (any alignment of either), chunk `chunk` of FC_UNITS * 3 vectors.
__device__ __forceinline__ void fc_copy_chunk(const uint8_t* s, uint8_t* d, long long n, int chunk, int tid) {
    const int head = (int)min((long long)fc_head_bytes(d), n);
    const long long nv = (n - head) >> 4;
    const long long v0 = (long long)chunk * (FC_UNITS * 3) + tid;
    if (chunk == 0) {
        const long long tail0 = head + (nv << 4);
        if (tid < head) d[tid] = s[tid];
        else if (tid >= 64 && tail0 + (tid - 64) < n) d[tail0 + (tid - 64)] = s[tail0 + (tid - 64)];
    }
    if (v0 >= nv) return;
    const uint8_t* sb = s + head;
    uint8_t* db = d + head;
    uint4 v[FC_VPT];
    if ((((uintptr_t)sb) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < FC_VPT; ++k) { const long long i = v0 + (long long)k * FC_THREADS; if (i < nv) v[k] = fc_load16<true>(sb + i * 16); }
    } else {
#pragma unroll
        for (int k = 0; k < FC_VPT; ++k) { const long long i = v0 + (long long)k * FC_THREADS; if (i < nv) v[k] = fc_load16<false>(sb + i * 16); }
    }
#pragma unroll
    for (int k = 0; k < FC_VPT; ++k) { const long long i = v0 + (long long)k * FC_THREADS; if (i < nv) fc_store16(db + i * 16, v[k]); }
}

// grey plane d[p] = RGB s[3 p] for HW pixels
template <bool ALIGNED>
__device__ __forceinline__ void fc_extract_body(const uint8_t* sb, uint8_t* db, long long nu, long long u0) {
    uint32_t w[FC_UPT][12];
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) {
        const long long u = u0 + (long long)k * FC_THREADS;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (u < nu) v = fc_load16<ALIGNED>(sb + u * 48 + j * 16);
            w[k][4 * j] = v.x; w[k][4 * j + 1] = v.y; w[k][4 * j + 2] = v.z; w[k][4 * j + 3] = v.w;
        }
    }
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) {
        const long long u = u0 + (long long)k * FC_THREADS;
        if (u >= nu) continue;
        uint32_t o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            o[q] = fc_byte(w[k], 12 * q) | (fc_byte(w[k], 12 * q + 3) << 8) | (fc_byte(w[k], 12 * q + 6) << 16) | (fc_byte(w[k], 12 * q + 9) << 24);
        fc_store16(db + u * 16, make_uint4(o[0], o[1], o[2], o[3]));
    }
}

__device__ __forceinline__ void fc_extract_chunk(const uint8_t* s, uint8_t* d, int HW, int chunk, int tid) {
    const int hp = min(HW, fc_head_bytes(d));
    const long long nu = (HW - hp) >> 4;
    const long long c0 = (long long)chunk * FC_UNITS;
    if (chunk == 0) {
        const int tail0 = hp + (int)(nu << 4);
        if (tid < hp) d[tid] = s[3 * (size_t)tid];
        else if (tid >= 64 && tail0 + (tid - 64) < HW) d[tail0 + (tid - 64)] = s[3 * (size_t)(tail0 + (tid - 64))];
    }
    if (c0 >= nu) return;
    const uint8_t* sb = s + 3 * (size_t)hp;
    uint8_t* db = d + hp;
    if ((((uintptr_t)sb) & 15) == 0) fc_extract_body<true>(sb, db, nu, c0 + tid);
    else fc_extract_body<false>(sb, db, nu, c0 + tid);
}

// RGB d[3 p + c] = grey s[p] for HW pixels: 16 grey bytes in, 48 out
template <bool ALIGNED>
__device__ __forceinline__ void fc_expand_body(const uint8_t* sb, uint8_t* db, long long nu, long long u0) {
    uint4 g[FC_UPT];
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) {
        const long long u = u0 + (long long)k * FC_THREADS;
        g[k] = make_uint4(0, 0, 0, 0);
        if (u < nu) g[k] = fc_load16<ALIGNED>(sb + u * 16);
    }
#pragma unroll
    for (int k = 0; k < FC_UPT; ++k) {
        const long long u = u0 + (long long)k * FC_THREADS;
        if (u >= nu) continue;
        const uint32_t w[4] = {g[k].x, g[k].y, g[k].z, g[k].w};
        uint32_t o[12];
#pragma unroll
        for (int q = 0; q < 12; ++q)
            o[q] = fc_byte(w, (4 * q) / 3) | (fc_byte(w, (4 * q + 1) / 3) << 8) | (fc_byte(w, (4 * q + 2) / 3) << 16) | (fc_byte(w, (4 * q + 3) / 3) << 24);
#pragma unroll
        for (int q = 0; q < 12; ++q) asm volatile("" : "+v"(o[q]));       // opaque: keeps three 16-byte stores (the period-3 dword pattern otherwise becomes four 12-byte ones)
#pragma unroll
        for (int j = 0; j < 3; ++j) fc_store16(db + u * 48 + j * 16, make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]));
    }
}

__device__ __forceinline__ void fc_expand_chunk(const uint8_t* s, uint8_t* d, int HW, int chunk, int tid) {
    const int hp = min(HW, fc_head_pixels_rgb(d));
    const long long nu = (HW - hp) >> 4;
    const long long c0 = (long long)chunk * FC_UNITS;
    if (chunk == 0) {
        const int tail0 = hp + (int)(nu << 4);
        int p = -1;
        if (tid < hp) p = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < HW) p = tail0 + (tid - 64);
        if (p >= 0) { const uint8_t v = s[p]; d[3 * (size_t)p] = v; d[3 * (size_t)p + 1] = v; d[3 * (size_t)p + 2] = v; }
    }
    if (c0 >= nu) return;
    const uint8_t* sb = s + hp;
    uint8_t* db = d + 3 * (size_t)hp;
    if ((((uintptr_t)sb) & 15) == 0) fc_expand_body<true>(sb, db, nu, c0 + tid);
    else fc_expand_body<false>(sb, db, nu, c0 + tid);
}

__global__ __launch_bounds__(FC_THREADS) void frames_put_kernel(int HW, const uint8_t* src, const uint64_t* dst_addr, const uint8_t* kind) {
    const int b = blockIdx.y;
    const uint8_t k = kind[b];
    uint8_t* d = (uint8_t*)(uintptr_t)dst_addr[b];
    if (k > 1 || d == nullptr) return;
    const uint8_t* s = src + (size_t)b * 3 * (size_t)HW;
    if (k == 0) fc_extract_chunk(s, d, HW, blockIdx.x, threadIdx.x);
    else fc_copy_chunk(s, d, 3LL * HW, blockIdx.x, threadIdx.x);
}

__global__ __launch_bounds__(FC_THREADS) void frames_gather_kernel(int HW, const uint64_t* src_addr, const uint8_t* kind, uint8_t* dst) {
    const int b = blockIdx.y;
    const uint8_t k = kind[b];
    const uint8_t* s = (const uint8_t*)(uintptr_t)src_addr[b];
    if (k > 1 || s == nullptr) return;
    uint8_t* d = dst + (size_t)b * 3 * (size_t)HW;
    if (k == 0) fc_expand_chunk(s, d, HW, blockIdx.x, threadIdx.x);
    else fc_copy_chunk(s, d, 3LL * HW, blockIdx.x, threadIdx.x);
}

// B > 0, HW > 0 and a grid that fits; 1 = launch, 0 = nothing to do, < 0 = error
static int fc_check(const char* what, int B, int HW, unsigned* chunks) {
    if (B < 0 || HW < 0) { urso_set_error("%s: negative size (B %d, HW %d)", what, B, HW); return URSO_EINVAL; }
    if (B > 65535 || HW > 2147483647 / 3) { urso_set_error("%s: B <= 65535 and 3 HW < 2^31 (B %d, HW %d)", what, B, HW); return URSO_EINVAL; }
    if (B == 0 || HW == 0) return 0;
    *chunks = (unsigned)((HW >> 4) / FC_UNITS + 1);     // a slot's body has at most HW / 16 units
    return 1;
}

extern "C" int urso_frames_grey_flags_u8(int B, int HW, const uint8_t* src_d, uint8_t* flags_d, void* stream) {
    unsigned chunks = 0;
    const int go = fc_check("urso_frames_grey_flags_u8", B, HW, &chunks);
    if (go < 0) return go;
    if (!src_d || !flags_d) { urso_set_error("urso_frames_grey_flags_u8: null pointer"); return URSO_EINVAL; }
    if (B == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * (3.0 * HW + 1));
    URSO_KLAUNCH(frames_flags_init_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, flags_d);
    if (go) URSO_KLAUNCH(frames_grey_flags_kernel, dim3(chunks, B), dim3(FC_THREADS), 0, st, HW, src_d, flags_d);     // HW == 0: vacuously grey
    return urso_check_launch("urso_frames_grey_flags_u8");
}

extern "C" int urso_frames_put_u8(int B, int HW, const uint8_t* src_d, const uint64_t* dst_addr_d, const uint8_t* kind_d, void* stream) {
    unsigned chunks = 0;
    const int go = fc_check("urso_frames_put_u8", B, HW, &chunks);
    if (go < 0) return go;
    if (!src_d || !dst_addr_d || !kind_d) { urso_set_error("urso_frames_put_u8: null pointer or table"); return URSO_EINVAL; }
    if (!go) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    // Profiled under URSO_K_MOLD like the other input-side kernels (resize.hip); the launch profiler names the kernel by its symbol.  The
    // kinds live on the device, so the byte figure is the UPPER bound of an all-RGB batch (read 3 HW + write 3 HW per slot): a grey
    // slot moves 4 HW, a skipped one nothing.
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * 6.0 * HW);
    URSO_KLAUNCH(frames_put_kernel, dim3(chunks, B), dim3(FC_THREADS), 0, st, HW, src_d, dst_addr_d, kind_d);
    return urso_check_launch("urso_frames_put_u8");
}

extern "C" int urso_frames_gather_u8(int B, int HW, const uint64_t* src_addr_d, const uint8_t* kind_d, uint8_t* dst_d, void* stream) {
    unsigned chunks = 0;
    const int go = fc_check("urso_frames_gather_u8", B, HW, &chunks);
    if (go < 0) return go;
    if (!src_addr_d || !kind_d || !dst_d) { urso_set_error("urso_frames_gather_u8: null pointer or table"); return URSO_EINVAL; }
    if (!go) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_MOLD, 0, (double)B * 6.0 * HW);      // upper bound, as in urso_frames_put_u8
    URSO_KLAUNCH(frames_gather_kernel, dim3(chunks, B), dim3(FC_THREADS), 0, st, HW, src_addr_d, kind_d, dst_d);
    return urso_check_launch("urso_frames_gather_u8");
}
