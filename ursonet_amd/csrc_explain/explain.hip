// Occlusion-sensitivity maps of the pose heads (liburso_explain.so; explain()).  urso_occl_fill_u8 makes a batch of
// copies of one frame with one rect each painted over, urso_occl_score compares every occluded row's decoded pose and logits with the
// baseline's, urso_occl_splat turns per-patch scores into per-pixel maps, urso_heat_overlay_u8 blends a map through a colour table onto
// the frame's window.  The rules, the order of the sums and the argument rules: include/ursonet_explain.h; ursonet_amd/explain.py
// (occlude_host / score64 / splat64 / overlay_host) is the same in NumPy.  The library is built with -ffp-contract=off and the products
// below are named temporaries: a product is rounded before it is added.  Plain C++ with vector stores only.
#include "../csrc/common.h"
#include <math.h>
#include "../csrc/pose_dev.h"
#include "../../include/ursonet_explain.h"

// ------------------------------------------------------------------------------------------------ fill
// A row of out is a flat array of N = H W C bytes, copied as frame_cache.hip copies a frame: chunk = OF_THREADS * OF_VPT vectors of 16
// bytes (48 KiB), all of a thread's loads in flight before its first store.  The rect covers, in the frame rows y0 <= y < y1, the bytes
// xb0 <= xb < xb1 of a frame row of RB = W C bytes; a chunk whose bytes lie wholly before or behind the rect's first and last byte is a
// plain copy (a test that is uniform over the workgroup), elsewhere a vector pays two divisions to learn where it lies.
#define OF_THREADS 256
#define OF_VPT 12
#define OF_CHUNK (OF_THREADS * OF_VPT)

struct OfRect { int y0, y1, xb0, xb1, RB, C; uint32_t fill; };              // clamped; y1 == 0: nothing to paint

__device__ __forceinline__ int of_head_bytes(const void* p) { return (int)((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u); }

// byte `off` of the row: the source's, or the fill's where it lies in the rect
__device__ __forceinline__ uint8_t of_byte(uint8_t v, int off, const OfRect& r) {
    const int y = off / r.RB, xb = off - y * r.RB;
    if (y < r.y0 || y >= r.y1 || xb < r.xb0 || xb >= r.xb1) return v;
    return (uint8_t)(r.fill >> (8 * (xb % r.C)));
}

// the 16 bytes at `off`
__device__ __forceinline__ uint4 of_patch(uint4 v, int off, const OfRect& r) {
    int y = off / r.RB, xb = off - y * r.RB;
    if (y >= r.y1) return v;
    const int ylast = y + (xb + 15) / r.RB;
    if (ylast < r.y0) return v;
    if (y == ylast && (xb + 16 <= r.xb0 || xb >= r.xb1)) return v;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int c = xb % r.C;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (y >= r.y0 && y < r.y1 && xb >= r.xb0 && xb < r.xb1) {
            const uint32_t sh = 8u * (i & 3);
            w[i >> 2] = (w[i >> 2] & ~(0xFFu << sh)) | (((r.fill >> (8 * c)) & 0xFFu) << sh);
        }
        ++xb;
        if (++c == r.C) c = 0;
        if (xb == r.RB) { xb = 0; ++y; }                                   // RB is a multiple of C: c is 0 here
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint4 of_load16(const uint8_t* p, bool aligned) {
    uint4 v;
    if (aligned) v = *(const uint4*)p;
    else __builtin_memcpy(&v, p, 16);                                      // alignment 1: the compiler picks the widest access the target allows
    return v;
}

__global__ __launch_bounds__(OF_THREADS) void occl_fill_kernel(urso_occl_fill_args a) {
    const int j = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int N = a.H * a.W * a.C;
    const uint8_t* __restrict__ s = a.src;
    uint8_t* __restrict__ d = a.out + (size_t)j * (size_t)N;
    OfRect r;
    {
        const int* q = a.rects + 4 * (size_t)j;
        const int y0 = max(q[0], 0), x0 = max(q[1], 0), y1 = min(q[2], a.H), x1 = min(q[3], a.W);
        const bool some = y1 > y0 && x1 > x0;
        r.RB = a.W * a.C; r.C = a.C;
        r.y0 = some ? y0 : 0; r.y1 = some ? y1 : 0; r.xb0 = x0 * a.C; r.xb1 = x1 * a.C;
        r.fill = (uint32_t)a.fill[0] | ((uint32_t)a.fill[1] << 8) | ((uint32_t)a.fill[2] << 16) | ((uint32_t)a.fill[3] << 24);
    }
    const int head = min(of_head_bytes(d), N);
    const int nv = (N - head) >> 4;
    if (chunk == 0) {                                                      // head and tail bytes, one per thread
        const int tail0 = head + (nv << 4);
        int o = -1;
        if (tid < head) o = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < N) o = tail0 + (tid - 64);
        if (o >= 0) d[o] = of_byte(s[o], o, r);
    }
    const int v0 = chunk * OF_CHUNK + tid;
    if (v0 >= nv) return;
    // the chunk's bytes against the rect's first and last: uniform over the workgroup
    const int cb0 = head + chunk * OF_CHUNK * 16, cb1 = head + min(nv, (chunk + 1) * OF_CHUNK) * 16;
    const bool touch = r.y1 > 0 && cb0 < (r.y1 - 1) * r.RB + r.xb1 && cb1 > r.y0 * r.RB + r.xb0;
    const uint8_t* sb = s + head;
    uint8_t* db = d + head;
    const bool aligned = (((uintptr_t)sb) & 15) == 0;
    uint4 v[OF_VPT];
#pragma unroll
    for (int k = 0; k < OF_VPT; ++k) { const int i = v0 + k * OF_THREADS; if (i < nv) v[k] = of_load16(sb + (size_t)i * 16, aligned); }
#pragma unroll
    for (int k = 0; k < OF_VPT; ++k) {
        const int i = v0 + k * OF_THREADS;
        if (i >= nv) continue;
        if (touch) v[k] = of_patch(v[k], head + i * 16, r);
        *(uint4*)(db + (size_t)i * 16) = v[k];                             // 16-byte aligned by construction
    }
}

// ------------------------------------------------------------------------------------------------ score
static constexpr int ST = 1024;                                            // threads per workgroup (16 waves)
static constexpr int SW = ST / 64;

// The header's order: the xor butterfly 32 .. 1 across a wave, then the wave sums from +0.0 in wave order -- by every thread alike.
__device__ __forceinline__ double os_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < SW; ++w) r = r + sh[w];
    __syncthreads();
    return r;
}

// (value, index): the larger value, a NaN winning over everything, the lower index among equals (and among NaNs)
struct OsPeak { float v; int i; };
__device__ __forceinline__ OsPeak os_peak_of(const OsPeak& a, const OsPeak& b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    bool take_b;
    if (an || bn) take_b = bn && (!an || b.i < a.i);
    else take_b = b.v > a.v || (b.v == a.v && b.i < a.i);
    return take_b ? b : a;
}
__device__ __forceinline__ OsPeak os_block_peak(OsPeak pk, OsPeak* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        OsPeak other;
        other.v = __shfl_xor(pk.v, o, 64);
        other.i = __shfl_xor(pk.i, o, 64);
        pk = os_peak_of(pk, other);
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = pk;
    __syncthreads();
    OsPeak r = sh[0];
    for (int w = 1; w < SW; ++w) r = os_peak_of(r, sh[w]);
    __syncthreads();
    return r;
}

// Calls f(first column, count) for the calling thread's groups in index order: count = 4 for a group of four columns, the ragged end
// (count = K % 4) once, by the thread whose turn it is.
template <class F>
__device__ __forceinline__ void os_walk(int K, F f) {
    const int ng = K >> 2;
    for (int g = threadIdx.x; g < ng; g += ST) f(4 * g, 4);
    const int tail = K & 3;
    if (tail && (ng % ST) == (int)threadIdx.x) f(4 * ng, tail);
}

__device__ __forceinline__ void os_load(const float* __restrict__ row, bool aligned, int c, int cnt, float (&z)[4]) {
    if (aligned && cnt == 4) {
        const f32x4_t v = *(const f32x4_t*)(row + c);
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        for (int j = 0; j < cnt; ++j) z[j] = row[c + j];
    }
}

// One head: the baseline's logits z0 against the row's z into out4 = {KL, TV, DROP, ARGMAX}.  The rows are read three times (peaks, Z,
// terms), the second and third time out of L2, and exp is computed twice rather than K doubles parked anywhere.
__device__ void os_head(const float* __restrict__ z0, const float* __restrict__ z, int K, double* out4, double* shd, OsPeak* shp) {
    const bool al0 = ((uintptr_t)z0 & 15) == 0, al = ((uintptr_t)z & 15) == 0;
    OsPeak p0 = {-INFINITY, 0x7fffffff}, p1 = {-INFINITY, 0x7fffffff};
    os_walk(K, [&](int c, int cnt) {
        float a[4], b[4];
        os_load(z0, al0, c, cnt, a);
        os_load(z, al, c, cnt, b);
        for (int j = 0; j < cnt; ++j) {
            const OsPeak ha = {a[j], c + j}, hb = {b[j], c + j};
            p0 = os_peak_of(p0, ha);
            p1 = os_peak_of(p1, hb);
        }
    });
    p0 = os_block_peak(p0, shp);
    p1 = os_block_peak(p1, shp);
    const double m0 = (double)p0.v, m1 = (double)p1.v;

    double s0 = 0.0, s1 = 0.0;
    os_walk(K, [&](int c, int cnt) {
        float a[4], b[4];
        os_load(z0, al0, c, cnt, a);
        os_load(z, al, c, cnt, b);
        for (int j = 0; j < cnt; ++j) {
            const double d0 = (double)a[j] - m0, d1 = (double)b[j] - m1;
            const double e0 = exp(d0), e1 = exp(d1);
            s0 = s0 + e0;
            s1 = s1 + e1;
        }
    });
    const double Z0 = os_block_sum(s0, shd);
    const double Z1 = os_block_sum(s1, shd);
    const double l0 = log(Z0), l1 = log(Z1);

    double kl = 0.0, tv = 0.0;
    os_walk(K, [&](int c, int cnt) {
        float a[4], b[4];
        os_load(z0, al0, c, cnt, a);
        os_load(z, al, c, cnt, b);
        for (int j = 0; j < cnt; ++j) {
            const double d0 = (double)a[j] - m0, d1 = (double)b[j] - m1;
            const double e0 = exp(d0), e1 = exp(d1);
            const double q0 = e0 / Z0, q1 = e1 / Z1;
            const double lp0 = d0 - l0, lp1 = d1 - l1;
            const double dl = lp0 - lp1;
            const double pr = q0 * dl;
            const double t = q0 == 0.0 ? 0.0 : (q1 == 0.0 ? (double)INFINITY : pr);
            const double df = q0 - q1;
            kl = kl + t;
            tv = tv + fabs(df);
        }
    });
    const double KL = os_block_sum(kl, shd);
    const double TV = os_block_sum(tv, shd);
    if (threadIdx.x != 0) return;
    const double nan = __builtin_nan("");
    if (!__builtin_isfinite(m0) || !__builtin_isfinite(m1)) { out4[0] = nan; out4[1] = nan; out4[2] = nan; out4[3] = nan; return; }
    const double dk0 = (double)z0[p0.i] - m0, dk1 = (double)z[p0.i] - m1;
    const double ek0 = exp(dk0), ek1 = exp(dk1);
    const double qk0 = ek0 / Z0, qk1 = ek1 / Z1;
    out4[0] = KL;
    out4[1] = 0.5 * TV;
    out4[2] = qk0 - qk1;
    out4[3] = (double)p1.i;
}

__global__ void __launch_bounds__(ST) occl_score_kernel(urso_occl_score_args a) {
    __shared__ double shd[SW];
    __shared__ OsPeak shp[SW];
    const int b = blockIdx.x;
    const size_t r = (size_t)a.row0 + (size_t)b;
    double* out = a.out + r * URSO_OCCL_COLS;
    if (threadIdx.x == 64) {                                               // the decoded poses: one thread of the second wave
        const double* d0 = a.dec0;
        const double* d1 = a.dec + r * URSO_DEC_COLS;
        const double q0[4] = {d0[URSO_DEC_Q_EST], d0[URSO_DEC_Q_EST + 1], d0[URSO_DEC_Q_EST + 2], d0[URSO_DEC_Q_EST + 3]};
        const double ang = ev_angle(q0, d1 + URSO_DEC_Q_EST);
        const double dx = d1[URSO_DEC_LOC_EST] - d0[URSO_DEC_LOC_EST], dy = d1[URSO_DEC_LOC_EST + 1] - d0[URSO_DEC_LOC_EST + 1],
                     dz = d1[URSO_DEC_LOC_EST + 2] - d0[URSO_DEC_LOC_EST + 2];
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const double s2 = xx + yy + zz;
        out[URSO_OCCL_D_ORI] = ang * 180 / M_PI;
        out[URSO_OCCL_D_LOC] = sqrt(s2);
    }
    if (a.ori_K > 0) os_head(a.ori_z0, a.ori_z + (size_t)b * (size_t)a.ori_ld, a.ori_K, out + URSO_OCCL_ORI_KL, shd, shp);
    if (a.loc_K > 0) os_head(a.loc_z0, a.loc_z + (size_t)b * (size_t)a.loc_ld, a.loc_K, out + URSO_OCCL_LOC_KL, shd, shp);
}

// ------------------------------------------------------------------------------------------------ splat
static constexpr int PT = 256;

__global__ void __launch_bounds__(PT) occl_splat_kernel(urso_occl_splat_args a) {
    const int idx = blockIdx.x * PT + threadIdx.x;
    if (idx >= a.h * a.w) return;
    const int y = idx / a.w, x = idx - y * a.w, fy = a.wy0 + y, fx = a.wx0 + x;
    double s[URSO_OCCL_MAX_MAPS];
#pragma unroll
    for (int m = 0; m < URSO_OCCL_MAX_MAPS; ++m) s[m] = 0.0;
    int cnt = 0;
    for (int p = 0; p < a.P; ++p) {                                        // ascending: the order of the sum
        const int* q = a.rects + 4 * (size_t)p;
        if (fy < q[0] || fy >= q[2] || fx < q[1] || fx >= q[3]) continue;
        const double* row = a.scores + (size_t)p * (size_t)a.ld;
        ++cnt;
#pragma unroll
        for (int m = 0; m < URSO_OCCL_MAX_MAPS; ++m)
            if (m < a.M) s[m] = s[m] + row[a.cols[m]];
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int m = 0; m < URSO_OCCL_MAX_MAPS; ++m)
        if (m < a.M) a.out[(size_t)m * (size_t)a.h * (size_t)a.w + idx] = cnt ? s[m] / (double)cnt : nan;
}

// ------------------------------------------------------------------------------------------------ overlay
__global__ void __launch_bounds__(PT) heat_overlay_kernel(urso_heat_overlay_args a) {
    const int idx = blockIdx.x * PT + threadIdx.x;
    if (idx >= a.h * a.w) return;
    const int y = idx / a.w, x = idx - y * a.w;
    const double v = a.map[idx];
    const double dv = v - a.lo;
    const double t = dv * a.scale;
    if (t != t) return;
    const double rt = rint(t);
    const int k = rt < 0.0 ? 0 : (rt > 255.0 ? 255 : (int)rt);
    uint8_t* px = a.img + (size_t)y * (size_t)a.ld_img + 3 * (size_t)x;
    const uint8_t* col = a.lut + 3 * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (uint8_t)((a.alpha * (int)col[c] + (256 - a.alpha) * (int)px[c] + 128) >> 8);
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int urso_occl_fill_u8(const urso_occl_fill_args* a, void* stream) {
    const char* fn = "urso_occl_fill_u8";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->src || !a->rects || !a->out) { urso_set_error("%s: null pointer (src, rects, out)", fn); return URSO_EINVAL; }
    if (a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->B > 65535) { urso_set_error("%s: B <= 65535 (got %d)", fn, a->B); return URSO_EINVAL; }
    if (a->H < 1 || a->W < 1) { urso_set_error("%s: need H, W >= 1 (got %d, %d)", fn, a->H, a->W); return URSO_EINVAL; }
    if (a->C < 1 || a->C > 4) { urso_set_error("%s: need 1 <= C <= 4 (got %d)", fn, a->C); return URSO_EINVAL; }
    const long long N = (long long)a->H * a->W * a->C;
    if (N >= (1LL << 31)) { urso_set_error("%s: H W C must stay below 2^31 (got %lld)", fn, N); return URSO_EINVAL; }
    if ((uintptr_t)a->rects & 3) { urso_set_error("%s: rects must be 4-byte aligned", fn); return URSO_EINVAL; }
    const uintptr_t s0 = (uintptr_t)a->src, o0 = (uintptr_t)a->out;
    if (s0 < o0 + (uintptr_t)a->B * (uintptr_t)N && s0 + (uintptr_t)N > o0) { urso_set_error("%s: src lies inside out", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_MOLD, 0, (double)a->n * 2.0 * (double)N);
    const unsigned chunks = (unsigned)((N >> 4) / OF_CHUNK + 1);          // a row's body has at most N / 16 vectors
    URSO_KLAUNCH(occl_fill_kernel, dim3(chunks, a->n), dim3(OF_THREADS), 0, st, *a);
    return urso_check_launch(fn);
}

static bool os_bad_head(const char* fn, const char* head, int K, int ld, const float* z0, const float* z) {
    if (K < 0) { urso_set_error("%s: %s_K must be >= 0 (got %d)", fn, head, K); return true; }
    if (K == 0) return false;
    if (!z0 || !z) { urso_set_error("%s: %s_K = %d needs both %s_z0 and %s_z", fn, head, K, head, head); return true; }
    if (ld < K) { urso_set_error("%s: %s_ld %d < %s_K %d", fn, head, ld, head, K); return true; }
    if (((uintptr_t)z0 | (uintptr_t)z) & 3) { urso_set_error("%s: %s_z0 and %s_z must be 4-byte aligned", fn, head, head); return true; }
    return false;
}

extern "C" int urso_occl_score(const urso_occl_score_args* a, void* stream) {
    const char* fn = "urso_occl_score";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->dec0 || !a->dec || !a->out) { urso_set_error("%s: null pointer (dec0, dec, out)", fn); return URSO_EINVAL; }
    if (a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (os_bad_head(fn, "ori", a->ori_K, a->ori_ld, a->ori_z0, a->ori_z) || os_bad_head(fn, "loc", a->loc_K, a->loc_ld, a->loc_z0, a->loc_z)) return URSO_EINVAL;
    if (((uintptr_t)a->dec0 | (uintptr_t)a->dec | (uintptr_t)a->out) & 7) { urso_set_error("%s: dec0, dec and out must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (8.0 * ((double)a->ori_K + (double)a->loc_K) + 8.0 * (2 * URSO_DEC_COLS + URSO_OCCL_COLS)));
    URSO_KLAUNCH(occl_score_kernel, dim3(a->n), dim3(ST), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_occl_splat(const urso_occl_splat_args* a, void* stream) {
    const char* fn = "urso_occl_splat";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->scores || !a->rects || !a->out) { urso_set_error("%s: null pointer (scores, rects, out)", fn); return URSO_EINVAL; }
    if (a->P < 0) { urso_set_error("%s: P must be >= 0 (got %d)", fn, a->P); return URSO_EINVAL; }
    if (a->M < 1 || a->M > URSO_OCCL_MAX_MAPS) { urso_set_error("%s: need 1 <= M <= %d (got %d)", fn, URSO_OCCL_MAX_MAPS, a->M); return URSO_EINVAL; }
    if (a->h < 1 || a->w < 1 || (long long)a->h * a->w >= (1LL << 31)) { urso_set_error("%s: need h, w >= 1 and h w < 2^31 (got %d, %d)", fn, a->h, a->w); return URSO_EINVAL; }
    for (int m = 0; m < a->M; ++m)
        if (a->cols[m] < 0 || a->cols[m] >= a->ld) { urso_set_error("%s: column %d (cols[%d]) outside [0, ld = %lld)", fn, a->cols[m], m, (long long)a->ld); return URSO_EINVAL; }
    if ((uintptr_t)a->rects & 3) { urso_set_error("%s: rects must be 4-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)a->scores | (uintptr_t)a->out) & 7) { urso_set_error("%s: scores and out must be 8-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const long long px = (long long)a->h * a->w;
    ProfScope ps(st, URSO_K_DECODE, 0, 8.0 * (double)a->M * (double)px + (double)a->P * (16.0 + 8.0 * a->M));
    URSO_KLAUNCH(occl_splat_kernel, dim3((unsigned)((px + PT - 1) / PT)), dim3(PT), 0, st, *a);
    return urso_check_launch(fn);
}

extern "C" int urso_heat_overlay_u8(const urso_heat_overlay_args* a, void* stream) {
    const char* fn = "urso_heat_overlay_u8";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->map || !a->lut || !a->img) { urso_set_error("%s: null pointer (map, lut, img)", fn); return URSO_EINVAL; }
    if (a->h < 1 || a->w < 1 || (long long)a->h * a->w >= (1LL << 31)) { urso_set_error("%s: need h, w >= 1 and h w < 2^31 (got %d, %d)", fn, a->h, a->w); return URSO_EINVAL; }
    if (a->alpha < 0 || a->alpha > 256) { urso_set_error("%s: need 0 <= alpha <= 256 (got %d)", fn, a->alpha); return URSO_EINVAL; }
    if (a->ld_img < 3LL * a->w) { urso_set_error("%s: ld_img %lld < 3 w = %lld", fn, (long long)a->ld_img, 3LL * a->w); return URSO_EINVAL; }
    if (!(fabs(a->lo) <= 1.7976931348623157e308) || !(fabs(a->scale) <= 1.7976931348623157e308)) { urso_set_error("%s: lo and scale must be finite", fn); return URSO_EINVAL; }
    if ((uintptr_t)a->map & 7) { urso_set_error("%s: map must be 8-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const long long px = (long long)a->h * a->w;
    ProfScope ps(st, URSO_K_MOLD, 0, (8.0 + 6.0) * (double)px);
    URSO_KLAUNCH(heat_overlay_kernel, dim3((unsigned)((px + PT - 1) / PT)), dim3(PT), 0, st, *a);
    return urso_check_launch(fn);
}
