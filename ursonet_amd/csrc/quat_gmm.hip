// EM fit of a mixture of up to four "Gaussians on the rotation group" to an orientation PMF (pose_estimator.py:42-154,
// fit_GMM_to_orientation), batched: one workgroup per image.  Math, argument rules and output layout: include/ursonet_hip.h.
//
// One block per image keeps a batch of B < 256 images from filling the chip.  That is accepted for a decode kernel: every
// pass streams the image's PMF (or logits) and the bin map from L2, and the whole fit of a batch of 32 images at n = 64 takes
// milliseconds, against seconds to hours per image for the reference.
//
// Per image: (logits only) one max pass and one sum pass; M greedy masked arg-max passes for the initial means; then for every
// model size N = 1 .. M and every EM iteration one E/M pass (Z_k, the 10 unique entries of A_k = sum_i W_k(i) q_i q_i^T, and the
// score) and one variance pass with the new means.  Each bin is evaluated in fp32; every reduction is accumulated in fp64
// (per-thread partials, 64-lane shuffles, one LDS exchange across waves, in a fixed order: results do not depend on B).
#include "common.h"
#include <math.h>

#ifndef URSO_GMM_THREADS
#define URSO_GMM_THREADS 512
#endif
static constexpr int GT = URSO_GMM_THREADS, GW = GT / 64;
static constexpr int GMM_MAXM = 4;
static_assert(GT % 64 == 0 && GT >= 64 && GT <= 1024, "block size");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[t] = block-wide sum of v[t] (t < NV), in a fixed order.  `red` holds GW * NV doubles.  All threads must call it.
template <int NV>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* red, double* out) {
#pragma unroll
    for (int t = 0; t < NV; ++t) v[t] = wave_sum_d(v[t]);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < NV; ++t) red[w * NV + t] = v[t];
    __syncthreads();
    for (int t = threadIdx.x; t < NV; t += GT) {
        double s = 0.0;
        for (int i = 0; i < GW; ++i) s += red[i * NV + t];
        out[t] = s;
    }
    __syncthreads();
}

// PMF of bin i: the input itself, or stable_softmax (utils.py:26-28) recomputed from the logits on every pass.
struct GmmPmf {
    const float* z; int is_pmf; float mx, se;
    __device__ __forceinline__ float operator()(int i) const { return is_pmf ? z[i] : expf(z[i] - mx) / se; }
};

// d(a, b) = 2 arccos(clip(|a.b|, 0, 1)) / pi  (se3lib.angle_between_quats / 180)
__device__ __forceinline__ float qdist(const f32x4_t& q, const float* m) {
    const float c = fminf(fabsf(q.x * m[0] + q.y * m[1] + q.z * m[2] + q.w * m[3]), 1.f);
    return 2.f * acosf(c) / 3.14159265358979f;
}

// Mixture parameters of one model as the passes read them (LDS).
struct GmmState {
    float mu[GMM_MAXM][4], var[GMM_MAXM], pri[GMM_MAXM];
};

// E-step of one bin under `s` (N modes): w[k] = r_k(i) pmf(i), returns p_X(i).
template <int N>
__device__ __forceinline__ float estep(const f32x4_t& q, float p, const GmmState& s, const float (&twov)[N], const float (&nrm)[N], float (&w)[N]) {
    float pk[N], px = 0.f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float d = qdist(q, s.mu[k]);
        pk[k] = 1e-18f + expf(-(d * d) / twov[k]) / nrm[k];
        pk[k] = pk[k] * s.pri[k];
        px += pk[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) w[k] = (pk[k] / px) * p;
    return px;
}

template <int N>
__device__ __forceinline__ void mode_consts(const GmmState& s, float (&twov)[N], float (&nrm)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) { twov[k] = 2.f * s.var[k]; nrm[k] = sqrtf(6.28318530717959f * s.var[k]); }
}

// E/M pass: out[11k] = Z_k, out[11k + 1 + t] = A_k's t-th unique entry (row-major upper triangle), out[11N] = score.
template <int N>
__device__ void em_pass(int K, const GmmPmf& pmf, const f32x4_t* __restrict__ hq, const GmmState& s, double* red, double* out) {
    float twov[N], nrm[N];
    mode_consts<N>(s, twov, nrm);
    double acc[11 * N + 1];
#pragma unroll
    for (int t = 0; t < 11 * N + 1; ++t) acc[t] = 0.0;
    for (int i = threadIdx.x; i < K; i += GT) {
        const f32x4_t q = hq[i];
        const float p = pmf(i);
        float w[N];
        const float px = estep<N>(q, p, s, twov, nrm, w);
        acc[11 * N] += (double)(p * logf(px));
        const double qd[4] = {(double)q.x, (double)q.y, (double)q.z, (double)q.w};
        double qq[10];
        int t = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) qq[t++] = qd[a] * qd[b];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double wd = (double)w[k];
            acc[11 * k] += wd;
#pragma unroll
            for (int u = 0; u < 10; ++u) acc[11 * k + 1 + u] += wd * qq[u];
        }
    }
    block_sum_d<11 * N + 1>(acc, red, out);
}

// Variance pass: out[k] = sum_i W_k(i) d(q_i, newmu_k)^2, W_k from the parameters before the update.
template <int N>
__device__ void var_pass(int K, const GmmPmf& pmf, const f32x4_t* __restrict__ hq, const GmmState& s, const float (*newmu)[4],
                         double* red, double* out) {
    float twov[N], nrm[N];
    mode_consts<N>(s, twov, nrm);
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < K; i += GT) {
        const f32x4_t q = hq[i];
        float w[N];
        estep<N>(q, pmf(i), s, twov, nrm, w);
#pragma unroll
        for (int k = 0; k < N; ++k) { const float d = qdist(q, newmu[k]); acc[k] += (double)w[k] * (double)(d * d); }
    }
    block_sum_d<N>(acc, red, out);
}

// se3lib.quat_weighted_avg (se3lib.py:217-260) on a normalised A (10 unique entries): unit eigenvector of the largest
// eigenvalue by cyclic Jacobi in double, sign normalised so that the largest-magnitude component is positive.  The same
// solve as quat_wavg_kernel (pool_loss_optim.hip), kept as a copy so that that kernel's code stays as it is.
__device__ void eig_max_quat(const double* A10, float* qout) {
    double A[4][4], V[4][4];
    int t = 0;
    for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) { A[i][j] = A[j][i] = A10[t++]; }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        if (off < 1e-30) break;
        for (int p = 0; p < 3; ++p) for (int q = p + 1; q < 4; ++q) {
            if (fabs(A[p][q]) < 1e-300) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double tt = ((theta >= 0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
            for (int k = 0; k < 4; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
            for (int k = 0; k < 4; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
            for (int k = 0; k < 4; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i) if (A[i][i] > A[best][best]) best = i;
    double q[4], nrm = 0.0; int im = 0;
    for (int i = 0; i < 4; ++i) { q[i] = V[i][best]; nrm += q[i] * q[i]; if (fabs(q[i]) > fabs(q[im])) im = i; }
    nrm = 1.0 / sqrt(nrm);
    if (q[im] < 0) nrm = -nrm;
    for (int i = 0; i < 4; ++i) qout[i] = (float)(q[i] * nrm);
}

struct GmmShared {
    GmmState cur, best;
    float newmu[GMM_MAXM][4];
    float pickq[GMM_MAXM][4];
    int pick[GMM_MAXM];
    double res[11 * GMM_MAXM + 1];       // em_pass results
    double vres[GMM_MAXM];               // var_pass results
    double red[GW * (11 * GMM_MAXM + 1)];
    float redf[GW];
    int redi[GW];
    double scores[GMM_MAXM];
    int n_acc;
};

// One model size: initial state from the first N greedy picks, nit EM iterations (N = 1 stops after two, :125), returns the
// score of the last E-step (on every thread).
template <int N>
__device__ double fit_model(int K, const GmmPmf& pmf, const f32x4_t* __restrict__ hq, float var0, int nit, GmmShared& sh) {
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        for (int c = 0; c < 4; ++c) sh.cur.mu[k][c] = sh.pickq[k][c];
        sh.cur.var[k] = var0;
        sh.cur.pri[k] = 1.f / (float)N;
    }
    __syncthreads();
    double score = 0.0;
    for (int it = 0; it < nit; ++it) {
        em_pass<N>(K, pmf, hq, sh.cur, sh.red, sh.res);
        score = sh.res[11 * N];
        if (threadIdx.x < N) {
            const int k = threadIdx.x;
            const double Z = sh.res[11 * k];
            double A10[10];
            for (int u = 0; u < 10; ++u) A10[u] = sh.res[11 * k + 1 + u] / Z;       // Z = 0: NaN mean and variance, as the reference's 0/0
            eig_max_quat(A10, sh.newmu[k]);
        }
        __syncthreads();
        var_pass<N>(K, pmf, hq, sh.cur, sh.newmu, sh.red, sh.vres);
        if (threadIdx.x < N) {
            const int k = threadIdx.x;
            const double Z = sh.res[11 * k];
            for (int c = 0; c < 4; ++c) sh.cur.mu[k][c] = sh.newmu[k][c];
            sh.cur.var[k] = (float)(sh.vres[k] / Z);
            sh.cur.pri[k] = (float)Z;
        }
        __syncthreads();
        if (N == 1 && it == 1) break;
    }
    return score;
}

__global__ void __launch_bounds__(GT) quat_gmm_kernel(int K, const float* __restrict__ in, int in_is_pmf, const float* __restrict__ hquat,
                                                      float var0, int nit, int M, float* __restrict__ mean_o, float* __restrict__ var_o,
                                                      float* __restrict__ prior_o, float* __restrict__ score_o, int* __restrict__ nmodes_o) {
    __shared__ GmmShared sh;
    const int b = blockIdx.x;
    const float* z = in + (size_t)b * K;
    const f32x4_t* hq = (const f32x4_t*)hquat;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

    GmmPmf pmf{z, in_is_pmf, 0.f, 1.f};
    if (!in_is_pmf) {
        float mx = -INFINITY;
        for (int i = threadIdx.x; i < K; i += GT) mx = fmaxf(mx, z[i]);
        mx = wave_max(mx);
        if (lane == 0) sh.redf[w] = mx;
        __syncthreads();
        mx = -INFINITY;
        for (int i = 0; i < GW; ++i) mx = fmaxf(mx, sh.redf[i]);
        double se[1] = {0.0};
        for (int i = threadIdx.x; i < K; i += GT) se[0] += (double)expf(z[i] - mx);
        block_sum_d<1>(se, sh.red, sh.res);
        pmf.mx = mx; pmf.se = (float)sh.res[0];
    }

    // Initial means (:60-79): mode k = highest-PMF bin that is not a previous pick and not within d^2 < 9 var of one; ties go to
    // the lowest bin index.  No eligible bin left: the pick is -1 and the mean the zero quaternion (the reference's zeros).
    const float lim = 9.f * var0;
    for (int k = 0; k < M; ++k) {
        float bv = -INFINITY; int bi = -1;
        for (int i = threadIdx.x; i < K; i += GT) {
            const float p = pmf(i);
            if (!(p > bv)) continue;
            const f32x4_t q = hq[i];
            bool ok = true;
            for (int j = 0; j < k; ++j) {
                if (sh.pick[j] < 0) continue;
                const float d = qdist(q, sh.pickq[j]);
                if (i == sh.pick[j] || d * d < lim) { ok = false; break; }
            }
            if (ok) { bv = p; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sh.redf[w] = bv; sh.redi[w] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < GW; ++i) {
                const float ov = sh.redf[i]; const int oi = sh.redi[i];
                if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            sh.pick[k] = bi;
            const f32x4_t q = bi >= 0 ? hq[bi] : f32x4_t{0.f, 0.f, 0.f, 0.f};
            sh.pickq[k][0] = q.x; sh.pickq[k][1] = q.y; sh.pickq[k][2] = q.z; sh.pickq[k][3] = q.w;
        }
        __syncthreads();
    }

    // Model selection (:129-141): the first model is always accepted, a larger one only if score > last accepted + 0.005.
    if (threadIdx.x == 0) sh.n_acc = 0;
    __syncthreads();
    for (int N = 1; N <= M; ++N) {
        double score;
        switch (N) {
            case 1: score = fit_model<1>(K, pmf, hq, var0, nit, sh); break;
            case 2: score = fit_model<2>(K, pmf, hq, var0, nit, sh); break;
            case 3: score = fit_model<3>(K, pmf, hq, var0, nit, sh); break;
            default: score = fit_model<4>(K, pmf, hq, var0, nit, sh); break;
        }
        const bool accept = N == 1 || score > sh.scores[sh.n_acc - 1] + 0.005;
        __syncthreads();
        if (!accept) break;
        if (threadIdx.x == 0) {
            sh.scores[sh.n_acc] = score;
            sh.n_acc = N;
            sh.best = sh.cur;
        }
        __syncthreads();
    }

    // Output (:143-154): modes by prior, descending (stable: equal priors keep their order); slots past n_modes 0 / NaN score.
    if (threadIdx.x == 0) {
        const int n = sh.n_acc;
        int ord[GMM_MAXM];
        for (int k = 0; k < n; ++k) {
            int j = k;
            while (j > 0 && sh.best.pri[k] > sh.best.pri[ord[j - 1]]) { ord[j] = ord[j - 1]; --j; }
            ord[j] = k;
        }
        for (int s = 0; s < M; ++s) {
            const size_t o = (size_t)b * M + s;
            if (s < n) {
                const int k = ord[s];
                for (int c = 0; c < 4; ++c) mean_o[o * 4 + c] = sh.best.mu[k][c];
                var_o[o] = sh.best.var[k];
                prior_o[o] = sh.best.pri[k];
                score_o[o] = (float)sh.scores[s];
            } else {
                for (int c = 0; c < 4; ++c) mean_o[o * 4 + c] = 0.f;
                var_o[o] = 0.f; prior_o[o] = 0.f; score_o[o] = NAN;
            }
        }
        nmodes_o[b] = n;
    }
}

extern "C" int urso_quat_gmm_fit(int B, int K, const float* in_d, int in_is_pmf, const float* hquat_d, float var, int nr_iterations,
                                 int nr_max_modes, float* mean_d, float* var_d, float* prior_d, float* score_d, int* nmodes_d, void* stream) {
    if (!in_d || !hquat_d || !mean_d || !var_d || !prior_d || !score_d || !nmodes_d) { urso_set_error("urso_quat_gmm_fit: null pointer"); return URSO_EINVAL; }
    if (B <= 0 || K <= 0) { urso_set_error("urso_quat_gmm_fit: B and K must be positive (B=%d, K=%d)", B, K); return URSO_EINVAL; }
    if (((uintptr_t)hquat_d) & 15) { urso_set_error("urso_quat_gmm_fit: hquat must be 16-byte aligned"); return URSO_EINVAL; }
    if (!(var > 0.f) || !isfinite(var)) { urso_set_error("urso_quat_gmm_fit: var must be positive and finite (var=%g)", (double)var); return URSO_EINVAL; }
    if (nr_iterations < 1) { urso_set_error("urso_quat_gmm_fit: nr_iterations must be >= 1 (got %d)", nr_iterations); return URSO_EINVAL; }
    if (nr_max_modes < 2 || nr_max_modes > GMM_MAXM + 1) {
        urso_set_error("urso_quat_gmm_fit: nr_max_modes must be in [2, %d] (got %d)", GMM_MAXM + 1, nr_max_modes); return URSO_EINVAL;
    }
    const int M = nr_max_modes - 1;
    hipStream_t st = (hipStream_t)stream;
    // Bytes read if every model size runs (the search may stop earlier): 20 bytes per bin and pass (PMF or logit + map entry).
    const int nit1 = nr_iterations < 2 ? nr_iterations : 2;
    const double passes = (in_is_pmf ? 0 : 2) + M + 2.0 * nit1 + 2.0 * nr_iterations * (M - 1);
    ProfScope ps(st, URSO_K_DECODE, 0, passes * B * (double)K * 20 + (double)B * M * 28);
    URSO_KLAUNCH(quat_gmm_kernel, dim3(B), dim3(GT), 0, st, K, in_d, in_is_pmf, hquat_d, var, nr_iterations, M, mean_d, var_d, prior_d,
                 score_d, nmodes_d);
    return urso_check_launch("urso_quat_gmm_fit");
}
