// LAMB: layer-wise trust ratios for Adam(amsgrad) with global-norm clip (liburso_opt.so; Config.LAMB): the three
// launches that stand where the plain Adam launch stands -- the tick and the moments with the per-chunk sums of w^2 and r^2, the per-tensor
// trust ratios in float64, and the update with each tensor's trust.  Rule, state and argument rules: include/ursonet_opt.h;
// ursonet_amd/lamb.py is the same rule in NumPy.  Block map, chunk, group load / store and the slot sum: csrc/lars_chunk.h, shared with
// LARS (csrc_ext/lars.hip); slot order, clip factor and skipped step: csrc/flat_stream.h.
//
// The moments and the update are HBM-bound streams (32 and 16 bytes per parameter): 256 threads per block, 16 bytes per lane and access,
// one block per chunk of 4096 elements of ONE tensor, thread t on the groups t, 256 + t, 512 + t, 768 + t: the moments pass has five
// operands times four groups in flight per thread (80 registers of data) before it computes.  r, the direction, is never stored: the
// update recomputes it from the stored m and vhat by the same statements (lamb_dir), so it has the same bits.
#include "../csrc/lars_chunk.h"
#include "../../include/ursonet_opt.h"

// ------------------------------------------------------------------------------------------------ device
// t, the running products b1^t and b2^t and kt = sqrtf(1 - p2) / (1 - p1): one thread, in a launch of its own in front of the moments, so
// that no block reads a half-written state (as adam_tick_kernel).  A skipped step does not count.
__global__ void lamb_tick_kernel(float* __restrict__ hyper, float* __restrict__ state, const float* __restrict__ normsq, int guard) {
    if (step_skipped(guard, normsq)) return;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float b1 = hyper[1], b2 = hyper[2];
    const float t = hyper[5] + 1.0f;
    const float p1 = state[0] * b1;
    const float p2 = state[1] * b2;
    const float a = 1.f - p2;
    const float b = 1.f - p1;
    const float kt = sqrtf(a) / b;
    hyper[5] = t;
    state[0] = p1; state[1] = p2; state[2] = kt;
}

// gi = g c; m = b1 m + c1 gi; v = b2 v + c2 (gi gi); vhat = max(vhat, v): every operation rounded once
__device__ __forceinline__ void lamb_moments4(const f32x4_t& g, f32x4_t& m, f32x4_t& v, f32x4_t& vhat, float c, float b1, float b2,
                                              float c1, float c2) {
    const f32x4_t gi = g * c;
    const f32x4_t m1 = m * b1;
    const f32x4_t m2 = gi * c1;
    m = m1 + m2;
    const f32x4_t gg = gi * gi;
    const f32x4_t v1 = v * b2;
    const f32x4_t v2 = gg * c2;
    v = v1 + v2;
    vhat.x = fmaxf(vhat.x, v.x); vhat.y = fmaxf(vhat.y, v.y); vhat.z = fmaxf(vhat.z, v.z); vhat.w = fmaxf(vhat.w, v.w);
}

// r = (kt m) / (sqrtf(vhat) + eps): the direction, in both passes
__device__ __forceinline__ float lamb_dir(float m, float vhat, float kt, float eps) {
    const float a = kt * m;
    const float root = sqrtf(vhat);
    const float den = root + eps;
    return a / den;
}
__device__ __forceinline__ f32x4_t lamb_dir4(const f32x4_t& m, const f32x4_t& vhat, float kt, float eps) {
    f32x4_t r;
    r.x = lamb_dir(m.x, vhat.x, kt, eps); r.y = lamb_dir(m.y, vhat.y, kt, eps); r.z = lamb_dir(m.z, vhat.z, kt, eps);
    r.w = lamb_dir(m.w, vhat.w, kt, eps);
    return r;
}

// The moments of the block's chunk, and part[block] = {sum of w^2, sum of r^2}: two slots in the order of csrc/flat_stream.h.  Elements
// past the tensor's end were read as +0; their r is SET to +0 (0 / (0 + eps) is not +0 for eps = 0 or a NaN kt), so they add nothing.
__global__ void __launch_bounds__(LT) lamb_moments_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blockmap,
                                                          const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ vhat, const float* __restrict__ hyper,
                                                          const float* __restrict__ state, const float* __restrict__ normsq, int guard,
                                                          float* __restrict__ part) {
    if (step_skipped(guard, normsq)) return;
    const LarsChunk ch = lars_chunk(tab, blockmap);
    const float b1 = hyper[1], b2 = hyper[2], eps = hyper[3], c1 = hyper[6], c2 = hyper[7], kt = state[2];
    const float c = clip_factor(hyper[4], normsq);
    const float* wp = w + ch.lo;
    const float* gp = g + ch.lo;
    float* mp = m + ch.lo;
    float* vp = v + ch.lo;
    float* hp = vhat + ch.lo;
    f32x4_t wv[LG], gv[LG], mv[LG], vv[LG], hv[LG];
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        wv[j] = lars_load(wp, e, ch.cnt);
        gv[j] = lars_load(gp, e, ch.cnt);
        mv[j] = lars_load(mp, e, ch.cnt);
        vv[j] = lars_load(vp, e, ch.cnt);
        hv[j] = lars_load(hp, e, ch.cnt);
    }
    float sw = 0.f, sr = 0.f;
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        sumsq4(sw, wv[j]);
        lamb_moments4(gv[j], mv[j], vv[j], hv[j], c, b1, b2, c1, c2);
        f32x4_t r = lamb_dir4(mv[j], hv[j], kt, eps);
        r.x = e < ch.cnt ? r.x : 0.f;                                       // past the tensor's end: nothing to add
        r.y = e + 1 < ch.cnt ? r.y : 0.f;
        r.z = e + 2 < ch.cnt ? r.z : 0.f;
        r.w = e + 3 < ch.cnt ? r.w : 0.f;
        sumsq4(sr, r);
        lars_store(mp, e, ch.cnt, mv[j]);
        lars_store(vp, e, ch.cnt, vv[j]);
        lars_store(hp, e, ch.cnt, hv[j]);
    }
    if (flat_block_sums(sw, sr)) {
        part[2 * (size_t)blockIdx.x] = sw;
        part[2 * (size_t)blockIdx.x + 1] = sr;
    }
}

// One block of two waves per tensor: wave 0 adds the tensor's w^2 slots, wave 1 its r^2 slots, each in index order in float64
// (lars_slot_sum); thread 0 finishes the tensor.  The clip factor does not appear: it is inside r.
__global__ void __launch_bounds__(128) lamb_trust_kernel(const int32_t* __restrict__ first, const int32_t* __restrict__ adapt,
                                                         const float* __restrict__ part, const float* __restrict__ normsq, double eta,
                                                         double eps, int clip_mode, int guard, float* __restrict__ trust,
                                                         double* __restrict__ stat) {
    __shared__ double sh[2];
    if (step_skipped(guard, normsq)) return;                                // the optimizer skips this step: trust and stat keep their bits
    const int t = blockIdx.x, lane = threadIdx.x & 63, which = threadIdx.x >> 6;       // which: 0 = the w^2 slots, 1 = the r^2 slots
    const int s0 = first[t], ns = first[t + 1] - s0;
    const double s = lars_slot_sum(part + 2 * (size_t)s0 + which, ns, lane);
    if (lane == 0) sh[which] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double nw = sqrt(sh[0]), nr = sqrt(sh[1]);
    double q = 1.0;
    if (adapt[t] != 0 && nw != 0.0 && nr != 0.0) {
        const double num = eta * nw;
        const double den = nr + eps;
        q = num / den;
        if (clip_mode) q = q < 1.0 ? q : 1.0;
    }
    trust[t] = (float)q;                                                    // rounded once
    stat[3 * (size_t)t] = nw; stat[3 * (size_t)t + 1] = nr; stat[3 * (size_t)t + 2] = q;
}

// step = lr * trust[tensor]; w = w - step * r over the block's chunk
__global__ void __launch_bounds__(LT) lamb_apply_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blockmap,
                                                        float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ vhat,
                                                        const float* __restrict__ trust, const float* __restrict__ hyper,
                                                        const float* __restrict__ state, const float* __restrict__ normsq, int guard) {
    if (step_skipped(guard, normsq)) return;
    const LarsChunk ch = lars_chunk(tab, blockmap);
    const float lr = hyper[0], eps = hyper[3], kt = state[2];
    const float step = lr * trust[ch.tensor];
    float* wp = w + ch.lo;
    const float* mp = m + ch.lo;
    const float* hp = vhat + ch.lo;
    f32x4_t wv[LG], mv[LG], hv[LG];
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        wv[j] = lars_load(wp, e, ch.cnt);
        mv[j] = lars_load(mp, e, ch.cnt);
        hv[j] = lars_load(hp, e, ch.cnt);
    }
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        const f32x4_t d = lamb_dir4(mv[j], hv[j], kt, eps) * step;
        wv[j] = wv[j] - d;
        lars_store(wp, e, ch.cnt, wv[j]);
    }
}

// ------------------------------------------------------------------------------------------------ launches
static double lamb_elements(int T, const int64_t* n_h) {
    double n = 0;
    for (int t = 0; t < T; ++t) n += (double)n_h[t];
    return n;
}

extern "C" int urso_lamb_moments(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                                 const float* w_d, const float* g_d, float* m_d, float* v_d, float* vhat_d, float* hyper_d, float* state_d,
                                 const float* normsq_d, float* part_d, const float* ls_state_d, void* stream) {
    const char* fn = "urso_lamb_moments";
    const int rc = lars_check_tensors(fn, T, off_h, n_h, nblocks);
    if (rc != URSO_OK) return rc;
    if (!w_d || !g_d || !m_d || !v_d || !vhat_d || !hyper_d || !state_d || !normsq_d) {
        urso_set_error("%s: null pointer (w, g, m, v, vhat, hyper, state, normsq)", fn); return URSO_EINVAL;
    }
    const void* five[5] = {w_d, g_d, m_d, v_d, vhat_d};
    for (int i = 0; i < 5; ++i) {
        if (lars_misaligned16(five[i])) { urso_set_error("%s: w, g, m, v and vhat must be 16-byte aligned", fn); return URSO_EINVAL; }
        for (int j = 0; j < i; ++j) {
            if (five[i] == five[j]) { urso_set_error("%s: w, g, m, v and vhat must be five different buffers", fn); return URSO_EINVAL; }
        }
    }
    if ((((uintptr_t)hyper_d) | ((uintptr_t)state_d) | ((uintptr_t)normsq_d) | ((uintptr_t)ls_state_d)) & 3) {
        urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL;
    }
    if (nblocks == 0) return URSO_OK;
    if (!tab_d || !blockmap_d || !part_d) { urso_set_error("%s: null pointer (tab, blockmap, part)", fn); return URSO_EINVAL; }
    if ((((uintptr_t)tab_d) | ((uintptr_t)part_d)) & 7) { urso_set_error("%s: tab and part must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)blockmap_d) & 3) { urso_set_error("%s: blockmap must be 4-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const int guard = ls_state_d ? 1 : 0;
    ProfScope ps(st, URSO_K_OPTIM, 0, lamb_elements(T, n_h) * 32);
    URSO_KLAUNCH(lamb_tick_kernel, dim3(1), dim3(64), 0, st, hyper_d, state_d, normsq_d, guard);
    URSO_KLAUNCH(lamb_moments_kernel, dim3(nblocks), dim3(LT), 0, st, tab_d, blockmap_d, w_d, g_d, m_d, v_d, vhat_d, (const float*)hyper_d,
                 (const float*)state_d, normsq_d, guard, part_d);
    return urso_check_launch(fn);
}

extern "C" int urso_lamb_trust(int T, const int32_t* first_d, const int32_t* adapt_d, int nblocks, const float* part_d, const float* normsq_d,
                               double eta, double eps, int clip_mode, float* trust_d, double* stat_d, const float* ls_state_d, void* stream) {
    const char* fn = "urso_lamb_trust";
    if (T < 0) { urso_set_error("%s: T must be >= 0 (got %d)", fn, T); return URSO_EINVAL; }
    if (nblocks < 0) { urso_set_error("%s: nblocks must be >= 0 (got %d)", fn, nblocks); return URSO_EINVAL; }
    if (!(eta > 0.0) || !(eta <= 1.7976931348623157e308)) { urso_set_error("%s: eta must be a finite number > 0", fn); return URSO_EINVAL; }
    if (!(eps >= 0.0) || !(eps <= 1.7976931348623157e308)) { urso_set_error("%s: eps must be a finite number >= 0", fn); return URSO_EINVAL; }
    if (clip_mode != 0 && clip_mode != 1) { urso_set_error("%s: clip_mode must be 0 or 1 (got %d)", fn, clip_mode); return URSO_EINVAL; }
    if (!normsq_d) { urso_set_error("%s: null pointer (normsq)", fn); return URSO_EINVAL; }
    if (T == 0) return URSO_OK;
    if (!first_d || !adapt_d || !trust_d || !stat_d || (nblocks > 0 && !part_d)) {
        urso_set_error("%s: null pointer (first, adapt, part, trust, stat)", fn); return URSO_EINVAL;
    }
    if ((((uintptr_t)part_d) | ((uintptr_t)stat_d)) & 7) { urso_set_error("%s: part and stat must be 8-byte aligned", fn); return URSO_EINVAL; }
    if ((((uintptr_t)first_d) | ((uintptr_t)adapt_d) | ((uintptr_t)trust_d) | ((uintptr_t)normsq_d) | ((uintptr_t)ls_state_d)) & 3) {
        urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)nblocks * 8 + (double)T * 36);
    URSO_KLAUNCH(lamb_trust_kernel, dim3(T), dim3(128), 0, st, first_d, adapt_d, part_d, normsq_d, eta, eps, clip_mode, ls_state_d ? 1 : 0,
                 trust_d, stat_d);
    return urso_check_launch(fn);
}

extern "C" int urso_lamb_apply(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                               float* w_d, const float* m_d, const float* vhat_d, const float* trust_d, const float* hyper_d,
                               const float* state_d, const float* normsq_d, const float* ls_state_d, void* stream) {
    const char* fn = "urso_lamb_apply";
    const int rc = lars_check_tensors(fn, T, off_h, n_h, nblocks);
    if (rc != URSO_OK) return rc;
    if (!w_d || !m_d || !vhat_d || !hyper_d || !state_d || !normsq_d) {
        urso_set_error("%s: null pointer (w, m, vhat, hyper, state, normsq)", fn); return URSO_EINVAL;
    }
    if (lars_misaligned16(w_d) || lars_misaligned16(m_d) || lars_misaligned16(vhat_d)) {
        urso_set_error("%s: w, m and vhat must be 16-byte aligned", fn); return URSO_EINVAL;
    }
    if (w_d == m_d || w_d == vhat_d || m_d == vhat_d) { urso_set_error("%s: w, m and vhat must be three different buffers", fn); return URSO_EINVAL; }
    if ((((uintptr_t)hyper_d) | ((uintptr_t)state_d) | ((uintptr_t)normsq_d) | ((uintptr_t)ls_state_d)) & 3) {
        urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL;
    }
    if (nblocks == 0) return URSO_OK;
    if (!tab_d || !blockmap_d || !trust_d) { urso_set_error("%s: null pointer (tab, blockmap, trust)", fn); return URSO_EINVAL; }
    if (((uintptr_t)tab_d) & 7) { urso_set_error("%s: tab must be 8-byte aligned", fn); return URSO_EINVAL; }
    if ((((uintptr_t)blockmap_d) | ((uintptr_t)trust_d)) & 3) { urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, lamb_elements(T, n_h) * 16);
    URSO_KLAUNCH(lamb_apply_kernel, dim3(nblocks), dim3(LT), 0, st, tab_d, blockmap_d, w_d, m_d, vhat_d, trust_d, hyper_d, state_d, normsq_d,
                 ls_state_d ? 1 : 0);
    return urso_check_launch(fn);
}
