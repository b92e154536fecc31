// The loss kernels (softmax cross-entropy, relative L2, 1-|dot|) and the block reductions they use, as device code shared by the two
// libraries: csrc/pool_loss_optim.hip launches them for the plain and the loss-scaled entry points (include/ursonet_hip.h,
// include/ursonet_loss_scale.h), csrc_ext/loss_weights.hip for the learnable-loss-weight ones (include/ursonet_ext.h).  Every kernel is
// static: each library launches its own copy.  Internal to the libraries.
#ifndef URSO_LOSS_DEV_H
#define URSO_LOSS_DEV_H

#include "common.h"
#include <math.h>

// =============================================================== block reductions (256 threads)
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* sh) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = -INFINITY;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, sh[i]);
    return r;
}

template <typename T> __device__ __forceinline__ void put_dt(void* p, size_t i, float v) { ((T*)p)[i] = Elem<T>::from_f(v); }
__device__ __forceinline__ void put_any(int dt, void* p, size_t i, float v) {
    if (dt == URSO_F32) put_dt<float>(p, i, v); else if (dt == URSO_BF16) put_dt<__bf16>(p, i, v); else put_dt<_Float16>(p, i, v);
}

// =============================================================== loss scaling
// ls: the fp32 state buffer of urso_loss_scale_update (URSO_LS_*), or NULL = no scaling: the value passes through untouched, so the entry
// points without a state keep their bits.  The factor is applied to the finished fp32 gradient, LAST, in front of the one rounding to dt.
__device__ __forceinline__ float ls_scaled(const float* __restrict__ ls, float g) { return ls ? g * ls[URSO_LS_SCALE] : g; }

// =============================================================== learnable loss weights
// s = NULL: the plain kernel, every value what it is without this struct.  Set: the kernel's weight w becomes w_eff = w * exp(-s[0]) -- that
// one fp32 product, everything after it in the plain kernel's order -- the loss P the plain formula gives under w_eff is reported as
// P + w * s[0], and ds[0] = w - P (= w (1 - L exp(-s)): the derivative of the reported loss in s) is overwritten; ds = NULL: a frozen s.
struct LossLw { const float* s; float* ds; float w; };
__device__ __forceinline__ float lw_weight(const LossLw& lw, float weight) { return lw.s ? lw.w * expf(-lw.s[0]) : weight; }
__device__ __forceinline__ void lw_report(const LossLw& lw, float P, float* __restrict__ loss) {
    if (!lw.s) { loss[0] = P; return; }
    loss[0] = P + lw.w * lw.s[0];
    if (lw.ds) lw.ds[0] = lw.w - P;
}

// =============================================================== softmax cross-entropy with soft labels
// gscale = weight / B (the host's division); under lw it is w_eff / B, B = gridDim.x
static __global__ void softmax_xent_kernel(int K, const float* __restrict__ z, const float* __restrict__ p, float gscale,
                                           int relu_mask, int dt, float* __restrict__ row_loss, void* __restrict__ dz, const float* __restrict__ ls,
                                           LossLw lw) {
    __shared__ float sh[8];
    const int b = blockIdx.x;
    if (lw.s) gscale = lw_weight(lw, 0.f) / (float)gridDim.x;
    const float* zr = z + (size_t)b * K; const float* pr = p + (size_t)b * K;
    float mx = -INFINITY;
    for (int k = threadIdx.x; k < K; k += blockDim.x) mx = fmaxf(mx, zr[k]);
    mx = block_max(mx, sh);
    float se = 0.f, spz = 0.f, sp = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) { const float zz = zr[k], pp = pr[k]; se += __expf(zz - mx); spz += pp * zz; sp += pp; }
    se = block_sum(se, sh); spz = block_sum(spz, sh); sp = block_sum(sp, sh);
    const float lse = mx + logf(se);
    if (threadIdx.x == 0) row_loss[b] = lse * sp - spz;              // -sum p*(z - lse)
    const float inv = 1.f / se;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float zz = zr[k];
        float g = (__expf(zz - mx) * inv - pr[k]) * gscale;           // TF backprop: softmax - labels
        if (relu_mask && !(zz > 0.f)) g = 0.f;
        put_any(dt, dz, (size_t)b * K + k, ls_scaled(ls, g));
    }
}
// K <= NV * blockDim (NV 4: the heads' 16^3 = 4096 orientation bins on 1024 threads; NV 16: 24^3 = 13,824 bins, 56 -> 12 us at batch 16): logits and labels are read ONCE into registers, the row maximum
// takes one block reduction and the three sums share a second one -- one memory round trip and four barriers instead of three dependent passes
// over global memory and eight barriers (18 -> 7 us for 32 x 4096; the launch is latency, not bandwidth)
template <int NV>
static __global__ __launch_bounds__(1024) void softmax_xent_reg_kernel(int K, const float* __restrict__ z, const float* __restrict__ p, float gscale,
                                                                       int relu_mask, int dt, float* __restrict__ row_loss, void* __restrict__ dz,
                                                                       const float* __restrict__ ls, LossLw lw) {
    __shared__ float sh[4][16];
    const int b = blockIdx.x, nw = (int)(blockDim.x >> 6), w = (int)(threadIdx.x >> 6);
    if (lw.s) gscale = lw_weight(lw, 0.f) / (float)gridDim.x;
    const float* zr = z + (size_t)b * K; const float* pr = p + (size_t)b * K;
    float zc[NV], pc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k = (int)threadIdx.x + i * (int)blockDim.x;
        zc[i] = k < K ? zr[k] : -INFINITY; pc[i] = k < K ? pr[k] : 0.f;
    }
    float mx = zc[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) mx = fmaxf(mx, zc[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[0][w] = mx;
    __syncthreads();
    mx = -INFINITY;
    for (int i = 0; i < nw; ++i) mx = fmaxf(mx, sh[0][i]);
    float ex[NV], se = 0.f, spz = 0.f, sp = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool in = (int)threadIdx.x + i * (int)blockDim.x < K;
        ex[i] = in ? __expf(zc[i] - mx) : 0.f;
        se += ex[i]; spz += in ? pc[i] * zc[i] : 0.f; sp += pc[i];
    }
    se = wave_sum(se); spz = wave_sum(spz); sp = wave_sum(sp);
    if ((threadIdx.x & 63) == 0) { sh[1][w] = se; sh[2][w] = spz; sh[3][w] = sp; }
    __syncthreads();
    se = spz = sp = 0.f;
    for (int i = 0; i < nw; ++i) { se += sh[1][i]; spz += sh[2][i]; sp += sh[3][i]; }
    const float lse = mx + logf(se);
    if (threadIdx.x == 0) row_loss[b] = lse * sp - spz;              // -sum p*(z - lse)
    const float inv = 1.f / se;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int k = (int)threadIdx.x + i * (int)blockDim.x;
        if (k >= K) continue;
        float g = (ex[i] * inv - pc[i]) * gscale;                    // TF backprop: softmax - labels
        if (relu_mask && !(zc[i] > 0.f)) g = 0.f;
        put_any(dt, dz, (size_t)b * K + k, ls_scaled(ls, g));
    }
}
// out = scale * sum v[0..n): the batch mean of the row losses, scale = weight / n (under lw: w_eff / n, and the report of lw_report)
static __global__ void mean_scale_kernel(int n, const float* __restrict__ v, float scale, float* __restrict__ out, LossLw lw) {
    __shared__ float sh[8];
    if (lw.s) scale = lw_weight(lw, 0.f) / (float)n;
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) lw_report(lw, s * scale, out);
}
// the launches of urso_softmax_xent_fwd_bwd[_ls|_lw] (arguments checked by the caller)
static inline void softmax_xent_launch(hipStream_t st, int B, int K, const float* logits_d, const float* labels_d, float weight, int relu_mask, int dt,
                                       float* loss_d, void* dz_d, float* row_ws_d, const float* state_d, LossLw lw) {
    if (K <= 4096) {
        int threads = ((K + 3) / 4 + 63) & ~63;
        if (threads < 64) threads = 64;
        URSO_KLAUNCH(softmax_xent_reg_kernel<4>, dim3(B), dim3(threads), 0, st, K, logits_d, labels_d, weight / (float)B, relu_mask, dt, row_ws_d, dz_d, state_d, lw);
    } else if (K <= 16384)
        URSO_KLAUNCH(softmax_xent_reg_kernel<16>, dim3(B), dim3(1024), 0, st, K, logits_d, labels_d, weight / (float)B, relu_mask, dt, row_ws_d, dz_d, state_d, lw);
    else
        URSO_KLAUNCH(softmax_xent_kernel, dim3(B), dim3(256), 0, st, K, logits_d, labels_d, weight / (float)B, relu_mask, dt, row_ws_d, dz_d, state_d, lw);
    URSO_KLAUNCH(mean_scale_kernel, dim3(1), dim3(256), 0, st, B, (const float*)row_ws_d, weight / (float)B, loss_d, lw);
}

// =============================================================== relative L2 (batch-Frobenius)
static __global__ void rel_l2_kernel(int B, int D, int ld, const float* __restrict__ gt, const float* __restrict__ pred, float weight,
                                     int dt, float* __restrict__ loss, void* __restrict__ dpred, float* __restrict__ norms, const float* __restrict__ ls,
                                     LossLw lw) {
    __shared__ float sh[8];
    weight = lw_weight(lw, weight);
    float sd = 0.f, sg = 0.f;
    for (int i = threadIdx.x; i < B * D; i += blockDim.x) {
        const int b = i / D, d = i - b * D;
        const float g = gt[i], e = g - pred[(size_t)b * ld + d];
        sd += e * e; sg += g * g;
    }
    sd = block_sum(sd, sh); sg = block_sum(sg, sh);
    const float nd = sqrtf(sd), ng = sqrtf(sg);
    if (threadIdx.x == 0) { lw_report(lw, weight * nd / ng, loss); if (norms) { norms[0] = sd; norms[1] = sg; } }
    const float c = -weight / (nd * ng);                               // d/dpred ||gt-pred||/||gt||  (NaN if pred==gt, as in TF)
    for (int i = threadIdx.x; i < B * ld; i += blockDim.x) {
        const int b = i / ld, d = i - b * ld;
        put_any(dt, dpred, i, d < D ? ls_scaled(ls, c * (gt[b * D + d] - pred[i])) : 0.f);
    }
}

// =============================================================== l2-normalise + 1-|dot|
static __global__ void absdot_kernel(int B, int D, int ld, int normalize, const float* __restrict__ gt, const float* __restrict__ x,
                                     float weight, int dt, float* __restrict__ q, float* __restrict__ loss, void* __restrict__ dx, const float* __restrict__ ls,
                                     LossLw lw) {
    __shared__ float sh[8];
    weight = lw_weight(lw, weight);
    float lsum = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float ss = 0.f;
        for (int d = 0; d < D; ++d) { const float v = x[(size_t)b * ld + d]; ss += v * v; }
        const bool clamped = !(ss > 1e-12f);
        const float rinv = normalize ? rsqrtf(fmaxf(ss, 1e-12f)) : 1.f;
        float dot = 0.f;
        for (int d = 0; d < D; ++d) { const float qq = x[(size_t)b * ld + d] * rinv; if (q) q[(size_t)b * D + d] = qq; if (gt) dot += gt[(size_t)b * D + d] * qq; }
        if (gt) {
            lsum += 1.f - fabsf(dot);
            // dL/dq = -sign(dot) * gt * weight / B ; through q = x*rinv:  dx = rinv*(dq - q*(q.dq))  (dq*rinv when clamped)
            const float sg = (dot > 0.f) ? 1.f : ((dot < 0.f) ? -1.f : 0.f);
            const float c = -sg * weight / (float)B;
            float qdq = 0.f;
            if (normalize && !clamped) for (int d = 0; d < D; ++d) qdq += (x[(size_t)b * ld + d] * rinv) * (c * gt[(size_t)b * D + d]);
            for (int d = 0; d < ld; ++d) {
                float g = 0.f;
                if (d < D) { const float dq = c * gt[(size_t)b * D + d]; g = normalize ? rinv * (dq - (clamped ? 0.f : x[(size_t)b * ld + d] * rinv * qdq)) : dq; }
                if (dx) put_any(dt, dx, (size_t)b * ld + d, ls_scaled(ls, g));
            }
        }
    }
    if (gt && loss) { lsum = block_sum(lsum, sh); if (threadIdx.x == 0) lw_report(lw, weight * lsum / (float)B, loss); }
}

#endif
