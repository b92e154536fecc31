// Device routines of the pose decode shared by pose_eval.hip (liburso_hip.so) and csrc_ext/pose_fuse.hip (liburso_ext.so): one wave
// sum, one eigen-solver with one sign rule, one angle with one clip convention.  Include after <hip/hip_runtime.h> and <math.h>.
#pragma once

__device__ __forceinline__ double ev_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Unit eigenvector of the largest eigenvalue of a symmetric 4x4 (cyclic Jacobi in double, the decode's solver; the sign is
// normalised so that the largest-magnitude component is positive).
__device__ void ev_eig_max(const double (&S)[4][4], double (&qout)[4]) {
    double A[4][4], V[4][4];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { A[i][j] = S[i][j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
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
    double nrm = 0.0; int im = 0;
    for (int i = 0; i < 4; ++i) { qout[i] = V[i][best]; nrm += qout[i] * qout[i]; if (fabs(qout[i]) > fabs(qout[im])) im = i; }
    nrm = 1.0 / sqrt(nrm);
    if (qout[im] < 0) nrm = -nrm;
    for (int i = 0; i < 4; ++i) qout[i] *= nrm;
}

// 2 acos(min(1, |a.b|)); NaN stays NaN (fmin would drop it).
__device__ __forceinline__ double ev_angle(const double (&a)[4], const double* b) {
    double d = fabs(a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]);
    d = d > 1.0 ? 1.0 : d;
    return 2 * acos(d);
}
