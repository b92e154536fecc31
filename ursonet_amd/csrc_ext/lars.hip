// Layer-wise adaptive rate scaling for SGD with momentum (liburso_ext.so; Config.LARS): the host planning of the
// block map and the three launches that replace the plain SGD launch -- the per-chunk sums of w^2 and g^2, the per-tensor trust ratios in
// float64, and the update with each tensor's trust.  Rule, reduction order, tables and argument rules: include/ursonet_ext.h;
// ursonet_amd/lars.py is the same rule in NumPy.  Slot order, clip factor, skipped step and the SGD rule itself: csrc/flat_stream.h;
// the block map's device and host helpers, shared with LAMB (csrc_opt/lamb.hip): csrc/lars_chunk.h.
//
// The norms and the update are HBM-bound streams (8 and 20 bytes per parameter): 256 threads per block, 16 bytes per lane and access, one
// block per chunk of URSO_LARS_CHUNK = 4096 elements of ONE tensor, so that a block's slot pair belongs to one tensor and the result does
// not depend on how the tensors sit in the flat buffer.  Thread t of a block owns the 16-byte groups t, 256 + t, 512 + t, 768 + t of its
// chunk: four independent loads per operand in flight, consecutive lanes on consecutive addresses.  A tensor's ragged end (numel % 4
// elements) is read and written by scalars: nothing outside [offset, offset + numel) is touched, the padding between slices included.
#include "../csrc/lars_chunk.h"

// ------------------------------------------------------------------------------------------------ host planning
extern "C" int urso_lars_blocks(int T, const int64_t* n_h) {
    int64_t nb = 0;
    const int rc = lars_count("urso_lars_blocks", T, n_h, &nb);
    return rc != URSO_OK ? rc : (int)nb;
}

extern "C" int urso_lars_plan(int T, const int64_t* n_h, int nblocks, int32_t* blockmap_h, int32_t* first_h) {
    const char* fn = "urso_lars_plan";
    int64_t nb = 0;
    const int rc = lars_count(fn, T, n_h, &nb);
    if (rc != URSO_OK) return rc;
    if (!first_h || (nb > 0 && !blockmap_h)) { urso_set_error("%s: null pointer (blockmap, first)", fn); return URSO_EINVAL; }
    if (nblocks != (int)nb) { urso_set_error("%s: nblocks must be urso_lars_blocks(T, n) = %d (got %d)", fn, (int)nb, nblocks); return URSO_EINVAL; }
    int32_t b = 0;
    for (int t = 0; t < T; ++t) {
        first_h[t] = b;
        const int32_t nc = (int32_t)((n_h[t] + URSO_LARS_CHUNK - 1) / URSO_LARS_CHUNK);
        for (int32_t c = 0; c < nc; ++c, ++b) { blockmap_h[2 * b] = t; blockmap_h[2 * b + 1] = c; }
    }
    first_h[T] = b;
    return URSO_OK;
}

// ------------------------------------------------------------------------------------------------ device
// chunk, group load and store, slot sum: csrc/lars_chunk.h
// part[block] = {sum of w^2, sum of g^2} over the block's chunk, per thread in the order it reads (its groups in order): two slots in the
// order of csrc/flat_stream.h
__global__ void __launch_bounds__(LT) lars_norms_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blockmap,
                                                        const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ part) {
    const LarsChunk ch = lars_chunk(tab, blockmap);
    const float* wp = w + ch.lo;
    const float* gp = g + ch.lo;
    f32x4_t wv[LG], gv[LG];
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        wv[j] = lars_load(wp, e, ch.cnt);
        gv[j] = lars_load(gp, e, ch.cnt);
    }
    float sw = 0.f, sg = 0.f;
#pragma unroll
    for (int j = 0; j < LG; ++j) { sumsq4(sw, wv[j]); sumsq4(sg, gv[j]); }
    if (flat_block_sums(sw, sg)) {
        part[2 * (size_t)blockIdx.x] = sw;
        part[2 * (size_t)blockIdx.x + 1] = sg;
    }
}

// One block of two waves per tensor: wave 0 adds the tensor's w^2 slots, wave 1 its g^2 slots, each in index order in float64
// (lars_slot_sum, csrc/lars_chunk.h).  The two chains are independent, so they run on two SIMDs side by side.  All lanes of a wave hold the
// same sum; thread 0 finishes the tensor.
__global__ void __launch_bounds__(128) lars_trust_kernel(const int32_t* __restrict__ first, const int32_t* __restrict__ adapt,
                                                         const float* __restrict__ part, const float* __restrict__ hyper,
                                                         const float* __restrict__ normsq, double eta, double eps, int clip_mode, int guard,
                                                         float* __restrict__ trust, double* __restrict__ stat) {
    __shared__ double sh[2];
    if (step_skipped(guard, normsq)) return;                                // the optimizer skips this step: trust and stat keep their bits
    const int t = blockIdx.x, lane = threadIdx.x & 63, which = threadIdx.x >> 6;       // which: 0 = the w^2 slots, 1 = the g^2 slots
    const int s0 = first[t], ns = first[t + 1] - s0;
    const float* pp = part + 2 * (size_t)s0 + which;
    const double s = lars_slot_sum(pp, ns, lane);
    if (lane == 0) sh[which] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double nw = sqrt(sh[0]), ng = sqrt(sh[1]);
    double q = 1.0;
    if (adapt[t] != 0 && nw != 0.0 && ng != 0.0) {
        const double c = (double)clip_factor(hyper[2], normsq);
        const double prod = c * ng;
        const double den = prod + eps;
        const double num = eta * nw;
        q = num / den;
        if (clip_mode) {
            q = q / (double)hyper[0];
            q = q < 1.0 ? q : 1.0;
        }
    }
    trust[t] = (float)q;                                                    // rounded once
    stat[3 * (size_t)t] = nw; stat[3 * (size_t)t + 1] = ng; stat[3 * (size_t)t + 2] = q;
}

// step = (lr * c) * trust[tensor], then the SGD rule of csrc/flat_stream.h (sgd_one) over the block's chunk: a tensor of trust 1 moves as
// under sgd_kernel
__global__ void __launch_bounds__(LT) lars_sgd_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ blockmap,
                                                      float* __restrict__ w, const float* __restrict__ g, float* __restrict__ v,
                                                      const float* __restrict__ trust, const float* __restrict__ hyper,
                                                      const float* __restrict__ normsq, int guard) {
    if (step_skipped(guard, normsq)) return;
    const LarsChunk ch = lars_chunk(tab, blockmap);
    const float lr = hyper[0], mom = hyper[1];
    const float c = clip_factor(hyper[2], normsq);
    const float lrc = lr * c;
    const float step = lrc * trust[ch.tensor];
    float* wp = w + ch.lo;
    const float* gp = g + ch.lo;
    float* vp = v + ch.lo;
    f32x4_t wv[LG], gv[LG], vv[LG];
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        wv[j] = lars_load(wp, e, ch.cnt);
        gv[j] = lars_load(gp, e, ch.cnt);
        vv[j] = lars_load(vp, e, ch.cnt);
    }
#pragma unroll
    for (int j = 0; j < LG; ++j) {
        const int e = 4 * (j * LT + (int)threadIdx.x);
        sgd_one(wv[j], gv[j], vv[j], mom, step);
        lars_store(vp, e, ch.cnt, vv[j]);                                   // (the tensor's ragged end: scalars, the padding keeps its bits)
        lars_store(wp, e, ch.cnt, wv[j]);
    }
}

// ------------------------------------------------------------------------------------------------ launches
extern "C" int urso_lars_norms(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                               const float* w_d, const float* g_d, float* part_d, void* stream) {
    const char* fn = "urso_lars_norms";
    const int rc = lars_check_tensors(fn, T, off_h, n_h, nblocks);
    if (rc != URSO_OK) return rc;
    if (!w_d || !g_d) { urso_set_error("%s: null pointer (w, g)", fn); return URSO_EINVAL; }
    if (lars_misaligned16(w_d) || lars_misaligned16(g_d)) { urso_set_error("%s: w and g must be 16-byte aligned", fn); return URSO_EINVAL; }
    if (w_d == g_d) { urso_set_error("%s: w and g are the same buffer", fn); return URSO_EINVAL; }
    if (nblocks == 0) return URSO_OK;
    if (!tab_d || !blockmap_d || !part_d) { urso_set_error("%s: null pointer (tab, blockmap, part)", fn); return URSO_EINVAL; }
    if ((((uintptr_t)tab_d) | ((uintptr_t)part_d)) & 7) { urso_set_error("%s: tab and part must be 8-byte aligned", fn); return URSO_EINVAL; }
    if (((uintptr_t)blockmap_d) & 3) { urso_set_error("%s: blockmap must be 4-byte aligned", fn); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    double n = 0;
    for (int t = 0; t < T; ++t) n += (double)n_h[t];
    ProfScope ps(st, URSO_K_OPTIM, 0, n * 8);
    URSO_KLAUNCH(lars_norms_kernel, dim3(nblocks), dim3(LT), 0, st, tab_d, blockmap_d, w_d, g_d, part_d);
    return urso_check_launch(fn);
}

extern "C" int urso_lars_trust(int T, const int32_t* first_d, const int32_t* adapt_d, int nblocks, const float* part_d, const float* hyper_d,
                               const float* normsq_d, double eta, double eps, int clip_mode, float* trust_d, double* stat_d,
                               const float* ls_state_d, void* stream) {
    const char* fn = "urso_lars_trust";
    if (T < 0) { urso_set_error("%s: T must be >= 0 (got %d)", fn, T); return URSO_EINVAL; }
    if (nblocks < 0) { urso_set_error("%s: nblocks must be >= 0 (got %d)", fn, nblocks); return URSO_EINVAL; }
    if (!(eta > 0.0) || !(eta <= 1.7976931348623157e308)) { urso_set_error("%s: eta must be a finite number > 0", fn); return URSO_EINVAL; }
    if (!(eps >= 0.0) || !(eps <= 1.7976931348623157e308)) { urso_set_error("%s: eps must be a finite number >= 0", fn); return URSO_EINVAL; }
    if (clip_mode != 0 && clip_mode != 1) { urso_set_error("%s: clip_mode must be 0 or 1 (got %d)", fn, clip_mode); return URSO_EINVAL; }
    if (!hyper_d || !normsq_d) { urso_set_error("%s: null pointer (hyper, normsq)", fn); return URSO_EINVAL; }
    if (T == 0) return URSO_OK;
    if (!first_d || !adapt_d || !trust_d || !stat_d || (nblocks > 0 && !part_d)) {
        urso_set_error("%s: null pointer (first, adapt, part, trust, stat)", fn); return URSO_EINVAL;
    }
    if ((((uintptr_t)part_d) | ((uintptr_t)stat_d)) & 7) { urso_set_error("%s: part and stat must be 8-byte aligned", fn); return URSO_EINVAL; }
    if ((((uintptr_t)first_d) | ((uintptr_t)adapt_d) | ((uintptr_t)trust_d) | ((uintptr_t)hyper_d) | ((uintptr_t)normsq_d) |
         ((uintptr_t)ls_state_d)) & 3) {
        urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_OPTIM, 0, (double)nblocks * 8 + (double)T * 36);
    URSO_KLAUNCH(lars_trust_kernel, dim3(T), dim3(128), 0, st, first_d, adapt_d, part_d, hyper_d, normsq_d, eta, eps, clip_mode,
                 ls_state_d ? 1 : 0, trust_d, stat_d);
    return urso_check_launch(fn);
}

extern "C" int urso_lars_sgd(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                             float* w_d, const float* g_d, float* v_d, const float* trust_d, const float* hyper_d, const float* normsq_d,
                             const float* ls_state_d, void* stream) {
    const char* fn = "urso_lars_sgd";
    const int rc = lars_check_tensors(fn, T, off_h, n_h, nblocks);
    if (rc != URSO_OK) return rc;
    if (!w_d || !g_d || !v_d || !hyper_d || !normsq_d) { urso_set_error("%s: null pointer (w, g, v, hyper, normsq)", fn); return URSO_EINVAL; }
    if (lars_misaligned16(w_d) || lars_misaligned16(g_d) || lars_misaligned16(v_d)) {
        urso_set_error("%s: w, g and v must be 16-byte aligned", fn); return URSO_EINVAL;
    }
    if (w_d == g_d || w_d == v_d || g_d == (const float*)v_d) { urso_set_error("%s: w, g and v must be three different buffers", fn); return URSO_EINVAL; }
    if (nblocks == 0) return URSO_OK;
    if (!tab_d || !blockmap_d || !trust_d) { urso_set_error("%s: null pointer (tab, blockmap, trust)", fn); return URSO_EINVAL; }
    if (((uintptr_t)tab_d) & 7) { urso_set_error("%s: tab must be 8-byte aligned", fn); return URSO_EINVAL; }
    if ((((uintptr_t)blockmap_d) | ((uintptr_t)trust_d) | ((uintptr_t)hyper_d) | ((uintptr_t)normsq_d) | ((uintptr_t)ls_state_d)) & 3) {
        urso_set_error("%s: pointers must be 4-byte aligned", fn); return URSO_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    double n = 0;
    for (int t = 0; t < T; ++t) n += (double)n_h[t];
    ProfScope ps(st, URSO_K_OPTIM, 0, n * 20);
    URSO_KLAUNCH(lars_sgd_kernel, dim3(nblocks), dim3(LT), 0, st, tab_d, blockmap_d, w_d, g_d, v_d, trust_d, hyper_d, normsq_d,
                 ls_state_d ? 1 : 0);
    return urso_check_launch(fn);
}
