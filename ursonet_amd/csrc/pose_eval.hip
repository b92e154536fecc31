// Batched decode and scoring of the pose heads (pose_estimator.py:321-460, evaluate): one workgroup per valid image writes one
// fp64 row of the caller's result table.  Math, argument rules and table layout: include/ursonet_hip.h.
//
// The per-image work is small (a closed-form decode, or one or two passes over at most a few thousand bins), so one 256-thread
// block per image is ample; what matters is that the whole batch is decoded and scored in one launch with no host round trip.
// Bin reductions (location first moment, encoded targets) are accumulated in fp64: per-thread partials, 64-lane shuffles, one
// LDS exchange across the 4 waves, in a fixed order.  The soft-argmax orientation is NOT recomputed here: the caller passes
// urso_quat_wavg_decode's output, so q_est is that entry point's result bit for bit.
//
// urso_pose_decode is the same decode without a ground truth (predict / submit): it shares the device routines below with
// urso_pose_eval, so both write the same loc_est / q_est bits, and adds the peak probabilities of the classification heads.
#include "common.h"
#include <math.h>
#include "pose_dev.h"

static constexpr int ET = 256, EW = ET / 64;

// out[t] = block-wide sum of v[t] (t < NV), fixed order.  `red` holds EW * NV doubles.  All threads must call it.
template <int NV>
__device__ __forceinline__ void ev_block_sum(double (&v)[NV], double* red, double* out) {
#pragma unroll
    for (int t = 0; t < NV; ++t) v[t] = ev_wave_sum(v[t]);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < NV; ++t) red[w * NV + t] = v[t];
    __syncthreads();
    for (int t = threadIdx.x; t < NV; t += ET) {
        double s = 0.0;
        for (int i = 0; i < EW; ++i) s += red[i * NV + t];
        out[t] = s;
    }
    __syncthreads();
}

// se3lib.SO32quat (se3lib.py:77-115): JPL quaternion [x, y, z, w] of a rotation matrix, all four branches.
__device__ void ev_so3_to_quat(const double (&R)[3][3], double (&q)[4]) {
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0) {
        const double Z = sqrt(tr + 1) * 2;
        q[3] = 0.25 * Z; q[0] = (R[1][2] - R[2][1]) / Z; q[1] = (R[2][0] - R[0][2]) / Z; q[2] = (R[0][1] - R[1][0]) / Z;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const double Z = sqrt(1.0 + 2 * R[0][0] - tr) * 2;
        q[3] = (R[1][2] - R[2][1]) / Z; q[0] = 0.25 * Z; q[1] = (R[0][1] + R[1][0]) / Z; q[2] = (R[0][2] + R[2][0]) / Z;
    } else if (R[1][1] > R[2][2]) {
        const double Z = sqrt(1.0 + 2 * R[1][1] - tr) * 2;
        q[3] = (R[2][0] - R[0][2]) / Z; q[0] = (R[0][1] + R[1][0]) / Z; q[1] = 0.25 * Z; q[2] = (R[1][2] + R[2][1]) / Z;
    } else {
        const double Z = sqrt(1.0 + 2 * R[2][2] - tr) * 2;
        q[3] = (R[0][1] - R[1][0]) / Z; q[0] = (R[0][2] + R[2][0]) / Z; q[1] = (R[1][2] + R[2][1]) / Z; q[2] = 0.25 * Z;
    }
}

// se3lib.euler2SO3_left (se3lib.py:38-51), degrees.
__device__ void ev_euler_to_so3(double pitch, double yaw, double roll, double (&R)[3][3]) {
    const double cp = cos(pitch * M_PI / 180), sp = sin(pitch * M_PI / 180);
    const double cy = cos(yaw * M_PI / 180), sy = sin(yaw * M_PI / 180);
    const double cr = cos(roll * M_PI / 180), sr = sin(roll * M_PI / 180);
    R[0][0] = cy * cr; R[0][1] = sp * sy * cr - cp * sr; R[0][2] = cp * sy * cr + sp * sr;
    R[1][0] = cy * sr; R[1][1] = sp * sy * sr + cp * cr; R[1][2] = cp * sy * sr - sp * cr;
    R[2][0] = -sy;     R[2][1] = sp * cy;                R[2][2] = cp * cy;
}

// pose_estimator.py:355-366: se3lib.pose_3Dto3D(P1, P2) + SO32quat(R.T) with P1 = columns (0,0,3), (0,3,0), (0,0,0) and
// P2 = [k1 | k2 | loc].  R.T is the proper rotation that best maps P1 - C1 onto P2 - C2; it is found by Horn's quaternion method
// (largest eigenvector of the 4x4 matrix built from H = sum (p1 - C1)(p2 - C2)^T), then converted with SO32quat as the reference does.
__device__ void ev_keypoints_quat(const double (&k1)[3], const double (&k2)[3], const double (&t)[3], double (&q)[4]) {
    const double P1[3][3] = {{0, 0, 3}, {0, 3, 0}, {0, 0, 0}};          // P1[j] = column j
    const double* P2[3] = {k1, k2, t};
    double C1[3], C2[3];
    for (int a = 0; a < 3; ++a) { C1[a] = (P1[0][a] + P1[1][a] + P1[2][a]) / 3; C2[a] = (P2[0][a] + P2[1][a] + P2[2][a]) / 3; }
    double S[3][3];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) {
        double s = 0.0;
        for (int j = 0; j < 3; ++j) s += (P1[j][a] - C1[a]) * (P2[j][b] - C2[b]);
        S[a][b] = s;
    }
    const double N[4][4] = {
        {S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
        {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
        {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
        {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double h[4];                                                         // Hamilton (w, x, y, z)
    ev_eig_max(N, h);
    const double w = h[0], x = h[1], y = h[2], z = h[3];
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
    ev_so3_to_quat(R, q);
}

// Block-wide maximum of row[0:K] (fmaxf: a NaN logit is dropped here and comes back through the exp sum).  All threads must call it.
__device__ __forceinline__ float ev_block_max(const float* row, int K, float* redf) {
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < K; i += ET) mx = fmaxf(mx, row[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = -INFINITY;
    for (int i = 0; i < EW; ++i) mx = fmaxf(mx, redf[i]);
    return mx;
}

// loc_est = softmax(lrow[0:K]) @ loc_map in fp64 (:380-383); returns sum_i exp(lrow[i] - max), whose reciprocal is the largest
// softmax probability.  `red` holds EW * 4 doubles, `res` 4, `redf` EW floats.  All threads must call it.
__device__ __forceinline__ double ev_loc_softmax(const float* lrow, int K, const double* loc_map, double* red, double* res, float* redf,
                                                 double (&loc_est)[3]) {
    const float mx = ev_block_max(lrow, K, redf);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < K; i += ET) {
        const double e = exp((double)lrow[i] - (double)mx);
        acc[0] += e; acc[1] += e * loc_map[3 * i]; acc[2] += e * loc_map[3 * i + 1]; acc[3] += e * loc_map[3 * i + 2];
    }
    ev_block_sum<4>(acc, red, res);
    for (int c = 0; c < 3; ++c) loc_est[c] = res[1 + c] / res[0];
    return res[0];
}

// The orientation estimate [x, y, z, w] of one row for every ori_mode (include/ursonet_hip.h); one thread.
__device__ __forceinline__ void ev_decode_ori(int ori_mode, const float* orow, const float* k2, const double (&loc_est)[3], double (&q)[4]) {
    switch (ori_mode) {
        case URSO_EVAL_ORI_EULER: {
            double R[3][3];
            ev_euler_to_so3(orow[0], orow[1], orow[2], R);
            ev_so3_to_quat(R, q);
            break;
        }
        case URSO_EVAL_ORI_ANGLE_AXIS: {                                   // :397-403
            const double v[3] = {orow[0], orow[1], orow[2]};
            const double th = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const double s = sin(th / 2);
            for (int c = 0; c < 3; ++c) q[c] = (th < 1e-6 ? 0.0 : v[c] / th) * s;
            q[3] = cos(th / 2);
            break;
        }
        case URSO_EVAL_ORI_KEYPOINTS: {
            const double k1d[3] = {orow[0], orow[1], orow[2]}, k2d[3] = {k2[0], k2[1], k2[2]};
            ev_keypoints_quat(k1d, k2d, loc_est, q);
            break;
        }
        default:                                                            // quaternion (q_out) or the soft-argmax decode
            for (int c = 0; c < 4; ++c) q[c] = orow[c];
    }
}

__global__ void __launch_bounds__(ET) pose_eval_kernel(urso_pose_eval_args a) {
    __shared__ double red[EW * 10];
    __shared__ double res[10];
    __shared__ float redf[EW];
    const int b = blockIdx.x;
    const float* lrow = a.loc + (size_t)b * a.loc_ld;

    // location: softmax(logits) @ histogram_3D_map (:380-383), and the encoded target's first moment (:386-387, no softmax)
    double loc_est[3], loc_dec[3] = {NAN, NAN, NAN};
    if (a.loc_mode == URSO_EVAL_LOC_CLASS) {
        const int K = a.loc_bins;
        ev_loc_softmax(lrow, K, a.loc_map, red, res, redf, loc_est);
        if (a.enc_loc) {
            const float* p = a.enc_loc + (size_t)b * K;
            double m[3] = {0.0, 0.0, 0.0};
            for (int i = threadIdx.x; i < K; i += ET) {
                const double pi = p[i];
                m[0] += pi * a.loc_map[3 * i]; m[1] += pi * a.loc_map[3 * i + 1]; m[2] += pi * a.loc_map[3 * i + 2];
            }
            ev_block_sum<3>(m, red, res);
            for (int c = 0; c < 3; ++c) loc_dec[c] = res[c];
        }
    } else {
        for (int c = 0; c < 3; ++c) loc_est[c] = lrow[c];
    }

    // encoded orientation target: quat_weighted_avg(ori_histogram_map, enc_ori_gt) (:429), a PMF-weighted average
    double q_enc[4] = {NAN, NAN, NAN, NAN};
    if (a.enc_ori) {
        const float* p = a.enc_ori + (size_t)b * a.ori_bins;
        const f32x4_t* hq = (const f32x4_t*)a.ori_map;
        double acc[10];
#pragma unroll
        for (int t = 0; t < 10; ++t) acc[t] = 0.0;
        for (int i = threadIdx.x; i < a.ori_bins; i += ET) {
            const f32x4_t h = hq[i];
            const double pi = p[i], v[4] = {(double)h.x, (double)h.y, (double)h.z, (double)h.w};
            int t = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = r; c < 4; ++c) acc[t++] += pi * (v[r] * v[c]);
        }
        ev_block_sum<10>(acc, red, res);
        if (threadIdx.x == 0) {
            double A[4][4];
            int t = 0;
            for (int r = 0; r < 4; ++r) for (int c = r; c < 4; ++c) { A[r][c] = A[c][r] = res[t++]; }
            ev_eig_max(A, q_enc);
        }
    }
    if (threadIdx.x != 0) return;

    // orientation
    double q[4];
    ev_decode_ori(a.ori_mode, a.ori + (size_t)b * a.ori_ld, a.ori2 ? a.ori2 + (size_t)b * a.ori_ld : nullptr, loc_est, q);
    const double* lg = a.loc_gt + (size_t)b * 3;
    const double* qg = a.q_gt + (size_t)b * 4;
    double* row = a.table + (size_t)(a.row0 + b) * URSO_EVAL_COLS;

    // multimodal (the commented block of :410-426): mode 0 if it is the only one or closer to the truth than mode 1
    double soft_err = NAN, mode = NAN;
    if (a.gmm_mean) {
        soft_err = ev_angle(q, qg) * 180 / M_PI;
        const float* mu = a.gmm_mean + (size_t)b * a.gmm_modes * 4;
        double m0[4], m1[4];
        for (int c = 0; c < 4; ++c) { m0[c] = mu[c]; m1[c] = a.gmm_modes > 1 ? mu[4 + c] : 0.0; }
        const double e0 = ev_angle(m0, qg), e1 = ev_angle(m1, qg);
        const int pick = (a.gmm_nmodes[b] <= 1 || e0 < e1) ? 0 : 1;
        for (int c = 0; c < 4; ++c) q[c] = pick ? m1[c] : m0[c];
        mode = pick;
    }

    // metrics (:432-449)
    const double ang = ev_angle(q, qg);
    const double dl[3] = {loc_est[0] - lg[0], loc_est[1] - lg[1], loc_est[2] - lg[2]};
    const double loc_err = sqrt(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
    const double ng = sqrt(lg[0] * lg[0] + lg[1] * lg[1] + lg[2] * lg[2]);
    for (int c = 0; c < 3; ++c) row[URSO_EVAL_LOC_EST + c] = loc_est[c];
    for (int c = 0; c < 4; ++c) row[URSO_EVAL_Q_EST + c] = q[c];
    row[URSO_EVAL_LOC_ERR] = loc_err;
    row[URSO_EVAL_ORI_ERR] = ang * 180 / M_PI;
    row[URSO_EVAL_ESA] = loc_err / ng + ang;
    row[URSO_EVAL_DIST] = lg[2];
    const double de[3] = {loc_dec[0] - lg[0], loc_dec[1] - lg[1], loc_dec[2] - lg[2]};
    row[URSO_EVAL_LOC_ENC_ERR] = sqrt(de[0] * de[0] + de[1] * de[1] + de[2] * de[2]);
    row[URSO_EVAL_ORI_ENC_ERR] = ev_angle(q_enc, qg) * 180 / M_PI;
    row[URSO_EVAL_ORI_ERR_SOFT] = soft_err;
    row[URSO_EVAL_MODE] = mode;
    row[URSO_EVAL_COLS - 1] = 0.0;
}

extern "C" int urso_pose_eval(const urso_pose_eval_args* a, void* stream) {
    const char* fn = "urso_pose_eval";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->loc || !a->ori || !a->loc_gt || !a->q_gt || !a->table) { urso_set_error("%s: null pointer (loc, ori, loc_gt, q_gt, table)", fn); return URSO_EINVAL; }
    if (a->B <= 0 || a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B and B > 0 (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->loc_mode != URSO_EVAL_LOC_REGRESS && a->loc_mode != URSO_EVAL_LOC_CLASS) { urso_set_error("%s: unknown loc_mode %d", fn, a->loc_mode); return URSO_EINVAL; }
    if (a->ori_mode < URSO_EVAL_ORI_QUAT || a->ori_mode > URSO_EVAL_ORI_KEYPOINTS) { urso_set_error("%s: unknown ori_mode %d", fn, a->ori_mode); return URSO_EINVAL; }
    const int soft = a->ori_mode == URSO_EVAL_ORI_SOFT, kp = a->ori_mode == URSO_EVAL_ORI_KEYPOINTS;
    const int ow = (a->ori_mode == URSO_EVAL_ORI_QUAT || soft) ? 4 : 3;
    if (a->ori_ld < ow) { urso_set_error("%s: ori_ld %d < %d values per row", fn, a->ori_ld, ow); return URSO_EINVAL; }
    if (kp && !a->ori2) { urso_set_error("%s: keypoint mode needs ori2 (k2)", fn); return URSO_EINVAL; }
    if (kp && a->loc_mode != URSO_EVAL_LOC_REGRESS) { urso_set_error("%s: keypoint mode needs a regressed location", fn); return URSO_EINVAL; }
    if (a->loc_mode == URSO_EVAL_LOC_CLASS) {
        if (!a->loc_map || a->loc_bins <= 0 || a->loc_bins != a->loc_map_rows) {
            urso_set_error("%s: location classification needs loc_map with loc_bins rows (loc_bins=%d, loc_map_rows=%d)", fn, a->loc_bins, a->loc_map_rows);
            return URSO_EINVAL;
        }
        if (a->loc_ld < a->loc_bins) { urso_set_error("%s: loc_ld %d < loc_bins %d", fn, a->loc_ld, a->loc_bins); return URSO_EINVAL; }
    } else {
        if (a->loc_ld < 3) { urso_set_error("%s: loc_ld %d < 3", fn, a->loc_ld); return URSO_EINVAL; }
        if (a->enc_loc) { urso_set_error("%s: enc_loc is defined for location classification only", fn); return URSO_EINVAL; }
    }
    if (a->enc_ori || a->gmm_mean) {
        if (!soft) { urso_set_error("%s: enc_ori and gmm_mean are defined for soft classification only", fn); return URSO_EINVAL; }
    }
    if (a->enc_ori) {
        if (!a->ori_map || a->ori_bins <= 0 || a->ori_bins != a->ori_map_rows) {
            urso_set_error("%s: enc_ori needs ori_map with ori_bins rows (ori_bins=%d, ori_map_rows=%d)", fn, a->ori_bins, a->ori_map_rows);
            return URSO_EINVAL;
        }
        if (((uintptr_t)a->ori_map) & 15) { urso_set_error("%s: ori_map must be 16-byte aligned", fn); return URSO_EINVAL; }
    }
    if (a->gmm_mean && (!a->gmm_nmodes || a->gmm_modes < 1 || a->gmm_modes > 4)) {
        urso_set_error("%s: gmm_mean needs gmm_nmodes and 1 <= gmm_modes <= 4 (got %d)", fn, a->gmm_modes); return URSO_EINVAL;
    }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const double bins = (a->loc_mode == URSO_EVAL_LOC_CLASS ? a->loc_bins * (a->enc_loc ? 32.0 : 28.0) : 12.0) + (a->enc_ori ? a->ori_bins * 20.0 : 0.0);
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (bins + 56 + URSO_EVAL_COLS * 8));
    URSO_KLAUNCH(pose_eval_kernel, dim3(a->n), dim3(ET), 0, st, *a);
    return urso_check_launch(fn);
}

// Decode without ground truth: the estimates of pose_eval_kernel (the same device routines, so the same bits) and how
// concentrated the classification heads' PMFs are.
__global__ void __launch_bounds__(ET) pose_decode_kernel(urso_pose_decode_args a) {
    __shared__ double red[EW * 4];
    __shared__ double res[4];
    __shared__ float redf[EW];
    const int b = blockIdx.x;
    const float* lrow = a.loc + (size_t)b * a.loc_ld;

    double loc_est[3], loc_peak = NAN, ori_peak = NAN;
    if (a.loc_mode == URSO_EVAL_LOC_CLASS) {
        loc_peak = 1.0 / ev_loc_softmax(lrow, a.loc_bins, a.loc_map, red, res, redf, loc_est);
    } else {
        for (int c = 0; c < 3; ++c) loc_est[c] = lrow[c];
    }
    if (a.ori_logits) {                                                     // max softmax probability = 1 / sum exp(z - max)
        const float* z = a.ori_logits + (size_t)b * a.ori_logits_ld;
        const float mx = ev_block_max(z, a.ori_bins, redf);
        double acc[1] = {0.0};
        for (int i = threadIdx.x; i < a.ori_bins; i += ET) acc[0] += exp((double)z[i] - (double)mx);
        ev_block_sum<1>(acc, red, res);
        ori_peak = 1.0 / res[0];
    }
    if (threadIdx.x != 0) return;

    const float* orow = a.ori + (size_t)b * a.ori_ld;
    double q[4];
    ev_decode_ori(a.ori_mode, orow, a.ori2 ? a.ori2 + (size_t)b * a.ori_ld : nullptr, loc_est, q);
    double lambda = NAN;
    if (a.ori_scatter) {                                                    // Rayleigh quotient of the decode's A at its q
        const float* A = a.ori_scatter + (size_t)b * 16;
        double num = 0.0, den = 0.0;
        for (int i = 0; i < 4; ++i) {
            double r = 0.0;
            for (int j = 0; j < 4; ++j) r += (double)A[i * 4 + j] * q[j];
            num += q[i] * r; den += q[i] * q[i];
        }
        lambda = num / den;
    }
    double* row = a.table + (size_t)(a.row0 + b) * URSO_DEC_COLS;
    for (int c = 0; c < 3; ++c) row[URSO_DEC_LOC_EST + c] = loc_est[c];
    for (int c = 0; c < 4; ++c) row[URSO_DEC_Q_EST + c] = q[c];
    row[URSO_DEC_LOC_PEAK] = loc_peak;
    row[URSO_DEC_ORI_PEAK] = ori_peak;
    row[URSO_DEC_ORI_LAMBDA] = lambda;
    for (int c = URSO_DEC_ORI_LAMBDA + 1; c < URSO_DEC_COLS; ++c) row[c] = 0.0;
}

extern "C" int urso_pose_decode(const urso_pose_decode_args* a, void* stream) {
    const char* fn = "urso_pose_decode";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->loc || !a->ori || !a->table) { urso_set_error("%s: null pointer (loc, ori, table)", fn); return URSO_EINVAL; }
    if (a->B <= 0 || a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B and B > 0 (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->loc_mode != URSO_EVAL_LOC_REGRESS && a->loc_mode != URSO_EVAL_LOC_CLASS) { urso_set_error("%s: unknown loc_mode %d", fn, a->loc_mode); return URSO_EINVAL; }
    if (a->ori_mode < URSO_EVAL_ORI_QUAT || a->ori_mode > URSO_EVAL_ORI_KEYPOINTS) { urso_set_error("%s: unknown ori_mode %d", fn, a->ori_mode); return URSO_EINVAL; }
    const int soft = a->ori_mode == URSO_EVAL_ORI_SOFT, kp = a->ori_mode == URSO_EVAL_ORI_KEYPOINTS;
    const int ow = (a->ori_mode == URSO_EVAL_ORI_QUAT || soft) ? 4 : 3;
    if (a->ori_ld < ow) { urso_set_error("%s: ori_ld %d < %d values per row", fn, a->ori_ld, ow); return URSO_EINVAL; }
    if (kp && !a->ori2) { urso_set_error("%s: keypoint mode needs ori2 (k2)", fn); return URSO_EINVAL; }
    if (kp && a->loc_mode != URSO_EVAL_LOC_REGRESS) { urso_set_error("%s: keypoint mode needs a regressed location", fn); return URSO_EINVAL; }
    if (a->loc_mode == URSO_EVAL_LOC_CLASS) {
        if (!a->loc_map || a->loc_bins <= 0 || a->loc_bins != a->loc_map_rows) {
            urso_set_error("%s: location classification needs loc_map with loc_bins rows (loc_bins=%d, loc_map_rows=%d)", fn, a->loc_bins, a->loc_map_rows);
            return URSO_EINVAL;
        }
        if (a->loc_ld < a->loc_bins) { urso_set_error("%s: loc_ld %d < loc_bins %d", fn, a->loc_ld, a->loc_bins); return URSO_EINVAL; }
    } else if (a->loc_ld < 3) { urso_set_error("%s: loc_ld %d < 3", fn, a->loc_ld); return URSO_EINVAL; }
    if ((a->ori_logits || a->ori_scatter) && !soft) { urso_set_error("%s: ori_logits and ori_scatter are defined for soft classification only", fn); return URSO_EINVAL; }
    if (a->ori_logits) {
        if (a->ori_bins <= 0 || a->ori_bins != a->ori_map_rows) {
            urso_set_error("%s: ori_logits needs ori_bins equal to the rows of the bin map (ori_bins=%d, ori_map_rows=%d)", fn, a->ori_bins, a->ori_map_rows);
            return URSO_EINVAL;
        }
        if (a->ori_logits_ld < a->ori_bins) { urso_set_error("%s: ori_logits_ld %d < ori_bins %d", fn, a->ori_logits_ld, a->ori_bins); return URSO_EINVAL; }
    }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    const double bins = (a->loc_mode == URSO_EVAL_LOC_CLASS ? a->loc_bins * 28.0 : 12.0) + (a->ori_logits ? a->ori_bins * 4.0 : 0.0);
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (bins + 16 + (a->ori_scatter ? 64 : 0) + URSO_DEC_COLS * 8));
    URSO_KLAUNCH(pose_decode_kernel, dim3(a->n), dim3(ET), 0, st, *a);
    return urso_check_launch(fn);
}
