// Test-time view fusion (liburso_ext.so): the per-view estimates of a batch, rotated back into the unrotated camera and fused into one
// pose per image, with the views' agreement and, given a truth, urso_pose_eval's errors.  Math, argument rules and table layout:
// include/ursonet_ext.h.
//
// The work per image is V <= 64 rows of 7 doubles and one 4x4 Jacobi, so one wave per image is ample: lane v de-rotates view v in
// registers, and every sum is taken by all 64 lanes alike, reading lane 0, 1, .. V - 1 in turn with a shuffle into ONE accumulator.
// That is the order the header promises (a butterfly would add in another one), it needs no LDS and no barrier, and it leaves every
// lane holding the same LOC_EST, S and Q_EST for the second pass (the spreads) without a broadcast.  Lanes past V take part in every
// shuffle and are never read.  The error / profiler plumbing is liburso_hip.so's (csrc/common.h), resolved when this library loads.
#include "../csrc/common.h"
#include <math.h>
#include "../csrc/pose_dev.h"
#include "../../include/ursonet_ext.h"

static constexpr int FT = 64;                                              // one wave

// The rotation angle between two orientations, 2 acos|a . b|, in the half-angle form that keeps its digits near 0 (Kahan): scale
// invariant, 0 for equal inputs, unchanged bit for bit by a sign flip of either; NaN stays NaN.
__device__ __forceinline__ double fz_angle(const double (&a)[4], const double (&b)[4]) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int c = 0; c < 4; ++c) { dot += a[c] * b[c]; na += a[c] * a[c]; nb += b[c] * b[c]; }
    na = sqrt(na); nb = sqrt(nb);
    const double s = dot < 0 ? -1.0 : 1.0;
    double dn = 0.0, dp = 0.0;
    for (int c = 0; c < 4; ++c) {
        const double x = a[c] * nb, y = s * b[c] * na;
        dn += (x - y) * (x - y); dp += (x + y) * (x + y);
    }
    return 4 * atan2(sqrt(dn), sqrt(dp));
}

__global__ void __launch_bounds__(FT) pose_fuse_kernel(urso_pose_fuse_views_args a) {
    const int b = blockIdx.x, lane = threadIdx.x, V = a.V;

    // lane v: view v's estimate in the unrotated camera
    double t[3] = {0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < V) {
        const double* row = a.est + ((size_t)lane * (size_t)a.est_view_rows + (size_t)b) * (size_t)a.est_ld;
        const double* R = a.r + lane * 9;
        const double* c = a.qr + lane * 4;
        const double tv[3] = {row[URSO_FUSE_LOC_EST], row[URSO_FUSE_LOC_EST + 1], row[URSO_FUSE_LOC_EST + 2]};
        const double qv[4] = {row[URSO_FUSE_Q_EST], row[URSO_FUSE_Q_EST + 1], row[URSO_FUSE_Q_EST + 2], row[URSO_FUSE_Q_EST + 3]};
        const bool ident = R[0] == 1.0 && R[1] == 0.0 && R[2] == 0.0 && R[3] == 0.0 && R[4] == 1.0 && R[5] == 0.0 && R[6] == 0.0 && R[7] == 0.0 && R[8] == 1.0;
        if (ident) {
            for (int j = 0; j < 3; ++j) t[j] = tv[j];
            for (int j = 0; j < 4; ++j) q[j] = qv[j];
        } else {
            for (int j = 0; j < 3; ++j) t[j] = tv[0] * R[j] + tv[1] * R[3 + j] + tv[2] * R[6 + j];
            const double x = -c[0], y = -c[1], z = -c[2], w = c[3];         // conj(qr_v)
            const double m[4] = {w * qv[0] + z * qv[1] - y * qv[2] + x * qv[3],
                                 -z * qv[0] + w * qv[1] + x * qv[2] + y * qv[3],
                                 y * qv[0] - x * qv[1] + w * qv[2] + z * qv[3],
                                 -x * qv[0] - y * qv[1] - z * qv[2] + w * qv[3]};
            const double nrm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]);
            for (int j = 0; j < 4; ++j) q[j] = m[j] / nrm;
        }
    }

    // first pass: sum_v t^_v and the upper triangle of sum_v q^_v q^_v^T, v = 0 .. V - 1
    double ls[3] = {0.0, 0.0, 0.0}, acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    double t0[3], q0[4];                                                    // view 0's, for V == 1
    for (int v = 0; v < V; ++v) {
        double tb[3], qb[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) tb[j] = __shfl(t[j], v, 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) qb[j] = __shfl(q[j], v, 64);
        if (v == 0) {
            for (int j = 0; j < 3; ++j) t0[j] = tb[j];
            for (int j = 0; j < 4; ++j) q0[j] = qb[j];
        }
        for (int j = 0; j < 3; ++j) ls[j] += tb[j];
        int k = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cc = r; cc < 4; ++cc) acc[k++] += qb[r] * qb[cc];
    }
    double loc[3], qe[4], S[4][4];
    {
        int k = 0;
        for (int r = 0; r < 4; ++r) for (int cc = r; cc < 4; ++cc) { S[r][cc] = S[cc][r] = (V == 1) ? acc[k] : acc[k] / V; ++k; }
    }
    if (V == 1) {
        for (int j = 0; j < 3; ++j) loc[j] = t0[j];
        for (int j = 0; j < 4; ++j) qe[j] = q0[j];
    } else {
        for (int j = 0; j < 3; ++j) loc[j] = ls[j] / V;
        ev_eig_max(S, qe);
    }

    // second pass: the views' deviations from the fused pose, summed in the same order
    double dl = 0.0, da = 0.0;
    if (lane < V && V > 1) {
        for (int j = 0; j < 3; ++j) dl += (t[j] - loc[j]) * (t[j] - loc[j]);
        const double ang = fz_angle(q, qe);
        da = ang * ang;
    }
    double sl = 0.0, sa = 0.0;
    for (int v = 0; v < V; ++v) { sl += __shfl(dl, v, 64); sa += __shfl(da, v, 64); }
    if (lane != 0) return;

    double lambda = 0.0;
    for (int i = 0; i < 4; ++i) {
        double rr = 0.0;
        for (int j = 0; j < 4; ++j) rr += S[i][j] * qe[j];
        lambda += qe[i] * rr;
    }
    double* row = a.table + (size_t)(a.row0 + b) * URSO_FUSE_COLS;
    for (int j = 0; j < 3; ++j) row[URSO_FUSE_LOC_EST + j] = loc[j];
    for (int j = 0; j < 4; ++j) row[URSO_FUSE_Q_EST + j] = qe[j];
    double loc_err = NAN, ori_err = NAN, esa = NAN, dist = NAN;
    if (a.loc_gt) {                                                         // urso_pose_eval's metrics, expression for expression
        const double* lg = a.loc_gt + (size_t)b * 3;
        const double* qg = a.q_gt + (size_t)b * 4;
        const double ang = ev_angle(qe, qg);
        const double d[3] = {loc[0] - lg[0], loc[1] - lg[1], loc[2] - lg[2]};
        loc_err = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double ng = sqrt(lg[0] * lg[0] + lg[1] * lg[1] + lg[2] * lg[2]);
        ori_err = ang * 180 / M_PI;
        esa = loc_err / ng + ang;
        dist = lg[2];
    }
    row[URSO_FUSE_LOC_ERR] = loc_err;
    row[URSO_FUSE_ORI_ERR] = ori_err;
    row[URSO_FUSE_ESA] = esa;
    row[URSO_FUSE_DIST] = dist;
    row[URSO_FUSE_LOC_SPREAD] = sqrt(sl / V);
    row[URSO_FUSE_ORI_SPREAD] = sqrt(sa / V) * 180 / M_PI;
    row[URSO_FUSE_VIEW_LAMBDA] = lambda;
    row[URSO_FUSE_N_VIEWS] = V;
    row[URSO_FUSE_COLS - 1] = 0.0;
}

extern "C" int urso_pose_fuse_views(const urso_pose_fuse_views_args* a, void* stream) {
    const char* fn = "urso_pose_fuse_views";
    if (!a) { urso_set_error("%s: null argument struct", fn); return URSO_EINVAL; }
    if (!a->est || !a->r || !a->qr || !a->table) { urso_set_error("%s: null pointer (est, r, qr, table)", fn); return URSO_EINVAL; }
    if (!a->loc_gt != !a->q_gt) { urso_set_error("%s: loc_gt and q_gt go together (both or neither)", fn); return URSO_EINVAL; }
    if (a->B <= 0 || a->n < 0 || a->n > a->B) { urso_set_error("%s: need 0 <= n <= B and B > 0 (B=%d, n=%d)", fn, a->B, a->n); return URSO_EINVAL; }
    if (a->row0 < 0) { urso_set_error("%s: row0 must be >= 0 (got %lld)", fn, (long long)a->row0); return URSO_EINVAL; }
    if (a->V < 1 || a->V > URSO_FUSE_MAX_VIEWS) { urso_set_error("%s: need 1 <= V <= %d (got %d)", fn, URSO_FUSE_MAX_VIEWS, a->V); return URSO_EINVAL; }
    if (a->est_ld < 7) { urso_set_error("%s: est_ld %d < 7 values per row", fn, a->est_ld); return URSO_EINVAL; }
    if (a->est_view_rows < a->B) { urso_set_error("%s: est_view_rows %lld < B %d", fn, (long long)a->est_view_rows, a->B); return URSO_EINVAL; }
    if (a->n == 0) return URSO_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_DECODE, 0, (double)a->n * (a->V * (7 + 13) * 8.0 + (a->loc_gt ? 56 : 0) + URSO_FUSE_COLS * 8));
    URSO_KLAUNCH(pose_fuse_kernel, dim3(a->n), dim3(FT), 0, st, *a);
    return urso_check_launch(fn);
}
