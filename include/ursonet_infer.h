/* C ABI of liburso_infer.so, the inference library (gfx950): entry points of inference features added after the surface of
 * liburso_train.so (ursonet_train.h) was pinned.  Its own surface is open: the next inference feature adds its entry points here.  It is
 * loaded behind the main library, whose error text (urso_last_error) and launch profiler it uses; it calls nothing of the other three.
 * Plain C99.  Every function returns URSO_OK or a negative URSO_E* code; the text of the last error is urso_last_error()'s.
 */
#ifndef URSONET_INFER_H
#define URSONET_INFER_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_hip.h"     /* URSO_OK / URSO_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * Split conformal prediction on a classification head's PMF (conformal(), predict / evaluate / test_and_submit with conformal=...,
 * DESIGN.md section 26; ursonet_amd/conformal.py -- weights64 / score64 / bound64 -- is the same rule in NumPy float64 / integers and the
 * written specification).  Everything below is for one row of one head: K fp32 logits z (the calibrated ones where a calibration is
 * applied), the head's bin map, and an estimate est in fp64 read from a row of the caller's table.
 *
 * Weights.  m = max z in fp32, a NaN winning.  d_i = (double) z_i - (double) m, e_i = exp(d_i), and the weight of bin i is the integer
 *   w_i = (uint64) rint(e_i * 2^URSO_CONF_SHIFT),     W = sum w_i      (K <= 2^18: W < 2^53)
 * Every sum of weights is an integer sum: exact in any order and exactly representable as a double, so the results are a function of the
 * row alone, whatever the reduction order, the grid or the use of LDS atomics.  The only step that is not an integer step is exp.
 *
 * Keys say how close bin i lies to est (the library is built with -ffp-contract=off; the parentheses give the order of the operations):
 *   URSO_CONF_ANGLE   map fp32 [K][4] (h, converted to double), est [4]:  key_i = min(1, |((e0 h0 + e1 h1) + e2 h2) + e3 h3|); a LARGER
 *                     key is closer; value(key) = ((2 acos(key)) * 180) / pi degrees.
 *   URSO_CONF_EUCLID  map fp64 [K][3], est [3], dx = h0 - e0 ..:          key_i = (dx dx + dy dy) + dz dz; a SMALLER key is closer;
 *                     value(key) = sqrt(key) metres.
 * Bins with equal keys form one group (the redundant bins of the Euler grid, sign-flipped quaternions).
 *
 * urso_conf_score (labelled data), for every valid batch row b < n: z = logits + b * ld_z, est = est + (row0 + b) * ld_est, the truth
 * ref = ref + b * ld_ref in fp64; key_ref is the key of the truth, computed as above with ref in the place of the map entry;
 * C = sum of w_i over the bins STRICTLY closer than key_ref, NEAR their number:
 *   out[row0 + b] = { SCORE = (double) C / (double) W, C, W, KEY_REF, ERR = value(key_ref), NEAR, 0, 0 }
 *
 * urso_conf_bound (any data), at the level q (a double, +inf allowed): G(v) = sum of w_i over the bins at least as close as key v, and v*
 * is the closest key of a bin with (double) G(v*) / (double) W > q -- the correctly rounded fp64 quotient compared with q:
 *   out[row0 + b] = { BOUND = value(v*), KEY = v*, MASS = G(v*) / W, COUNT = bins at least as close as v*, W, 0, 0, 0 }
 * and where no key qualifies (q >= 1): BOUND = 180 (angle) or +inf (Euclid), KEY = NaN, MASS = 1, COUNT = K.  Both kernels use the same
 * weights and the same quotient, so SCORE <= q exactly when key_ref is at least as close as v*, ties included.
 *
 * A row whose m is not finite, or whose est / ref has a component that is not finite, gets NaN in all eight columns; no other row is touched.
 *
 * Launch shape (urso_ens_add's): one workgroup of 1024 threads (16 waves) per valid row; thread t takes the groups of four columns
 * t, t + 1024, ..; a group is one 16-byte load where the row is 16-byte aligned and four 4-byte loads where it is not.  The score kernel
 * sweeps the row twice: the maximum, then the masked integer sums.  The bound kernel is a radix select over the bit pattern of the keys
 * (non-negative doubles, whose bit order is their numeric order; complemented for the angle metric): after the sweep for the maximum,
 * URSO_CONF_PASSES = 6 sweeps of URSO_CONF_DIGIT = 11 bits each, from the top (the last one takes the 9 bits that are left), each adding the
 * weights and the counts of the bins under the digits chosen so far into per-digit histograms in LDS (2048 uint64 + 2048 uint32, integer
 * LDS atomics) and descending into the first digit whose prefix sum passes q.  Seven sweeps in all; logits and map are read again on every
 * sweep (from L2 behind the first), keys are kept nowhere, whatever K is.  The results do not depend on any of this.
 *
 * No workspace, no allocation, no host synchronisation; n == 0 launches nothing.  URSO_EINVAL, with a message, before any launch: a null
 * struct or pointer; n outside [0, B]; row0 < 0; K < 1 or K > URSO_CONF_MAX_K; ld_z < K, ld_est or ld_ref below the metric's 4 / 3; an
 * unknown metric; q that is NaN or <= 0; logits off the 4-byte boundary, est / ref / out or a Euclid map off the 8-byte boundary, an
 * angle map off the 16-byte boundary.
 */
#define URSO_CONF_SHIFT 34
#define URSO_CONF_MAX_K 262144       /* 2^18 */
#define URSO_CONF_COLS 8
#define URSO_CONF_DIGIT 11
#define URSO_CONF_PASSES 6
#define URSO_CONF_ANGLE 0
#define URSO_CONF_EUCLID 1
/* the score row */
#define URSO_CONF_SCORE 0
#define URSO_CONF_C 1
#define URSO_CONF_W 2
#define URSO_CONF_KEY_REF 3
#define URSO_CONF_ERR 4
#define URSO_CONF_NEAR 5
/* the bound row */
#define URSO_CONF_BOUND 0
#define URSO_CONF_KEY 1
#define URSO_CONF_MASS 2
#define URSO_CONF_COUNT 3
#define URSO_CONF_BW 4               /* W again */
typedef struct urso_conf_score_args {
    int32_t B, n;                    /* rows of the batch, valid rows */
    int64_t row0;                    /* first row of est and out */
    int32_t K, ld_z, metric, ld_est, ld_ref, pad;
    const float* logits;             /* [B][ld_z] */
    const void* map;                 /* URSO_CONF_ANGLE: float [K][4]; URSO_CONF_EUCLID: double [K][3] */
    const double* est;               /* row r at est + r * ld_est: 4 / 3 doubles */
    const double* ref;               /* [B][ld_ref]: 4 / 3 doubles */
    double* out;                     /* [rows][URSO_CONF_COLS] */
} urso_conf_score_args;
typedef struct urso_conf_bound_args {
    int32_t B, n;
    int64_t row0;
    int32_t K, ld_z, metric, ld_est;
    double q;
    const float* logits;
    const void* map;
    const double* est;
    double* out;                     /* [rows][URSO_CONF_COLS] */
} urso_conf_bound_args;
int urso_conf_score(const urso_conf_score_args* args, void* stream);
int urso_conf_bound(const urso_conf_bound_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
