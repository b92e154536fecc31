/* C ABI of liburso_train.so, the training library (gfx950): entry points of training features added after the surfaces of liburso_hip.so
 * (ursonet_hip.h), liburso_ext.so (ursonet_ext.h) and liburso_opt.so (ursonet_opt.h) were frozen.  Its own surface is open: the next
 * training feature adds its entry points here.  It is loaded behind the main library, whose error text (urso_last_error) and launch
 * profiler it uses; it calls nothing of the other two.
 * Plain C99.  Every function returns URSO_OK or a negative URSO_E* code; the text of the last error is urso_last_error()'s.
 */
#ifndef URSONET_TRAIN_H
#define URSONET_TRAIN_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_hip.h"     /* URSO_OK / URSO_E* */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * SAM: sharpness-aware minimization (Config.SAM; ursonet_amd/sam.py is the same rule in NumPy and the written
 * specification).  The optimizer steps with the gradient taken at w + rho g / |g|: the step runs its forward and backward pass twice,
 * with the ascent between the two and the way back behind the second.
 *
 * state_d   float [URSO_SAM_STATE] = {rho, eps, normsq, scale, applied, applied_total, pending, 0}.  rho and eps are set by the host;
 *           normsq is the squared norm of g over all n elements, written by urso_sqnorm in front of the ascent.  urso_sam_ascend reads
 *           these three and writes scale, applied, applied_total and pending; urso_sam_settle writes applied_total and pending.
 *
 * Every float32 operation is rounded once (-ffp-contract=off); sqrtf and / are correctly rounded:
 *
 *   applied = isfinite(normsq) and normsq > 0
 *   s       = rho / (sqrtf(normsq) + eps)  if applied, else 0
 *   urso_sam_ascend    w0 = w (the bits);  where applied:  w = w + (s * g), the product rounded, then the sum.  s by the same statements
 *                      in every thread; one thread: scale = s, applied = 1 | 0, applied_total += applied, pending += applied.
 *                      Reads w and g, writes w0 and w: 16 bytes per parameter
 *   urso_sam_descend   w = w0 (the bits, moved as integers): 8 bytes per parameter
 *   urso_sam_settle    one thread, behind the optimizer's squared norm normsq_d[0]:  with guard = 1 and a norm that is not finite (the step
 *                      the loss-scaled optimizer skips)  applied_total -= pending;  then pending = 0
 *
 * Both streams: 256 threads per block, at most 4096 blocks with a grid stride, 16 bytes per lane and access where all buffers of the
 * launch sit alike against the 16-byte boundary (a scalar head and tail around the vectors), scalars alone otherwise.  n == 0 launches
 * nothing.  Nothing outside [0, n) is read or written.
 * URSO_EINVAL, before any launch: a null pointer; n < 0; a pointer off the 4-byte boundary; w, g, w0 (w, w0) not pairwise distinct;
 * a guard other than 0 or 1.
 */
#define URSO_SAM_STATE 8
#define URSO_SAM_RHO 0
#define URSO_SAM_EPS 1
#define URSO_SAM_NORMSQ 2
#define URSO_SAM_SCALE 3
#define URSO_SAM_APPLIED 4
#define URSO_SAM_APPLIED_TOTAL 5
#define URSO_SAM_PENDING 6
int urso_sam_ascend(int64_t n, float* w_d, const float* g_d, float* w0_d, float* state_d, void* stream);
int urso_sam_descend(int64_t n, float* w_d, const float* w0_d, void* stream);
int urso_sam_settle(float* state_d, const float* normsq_d, int guard, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * BN recalibration: pooled BatchNorm population statistics (recalibrate_bn, Config.BN_RECAL_BATCHES, DESIGN.md section 22;
 * ursonet_amd/bn_recal.py is the same rule in NumPy float64 and the written specification).  The batch-statistics forward pass leaves
 * every BN layer's float32 batch mean and (biased) batch variance on the device; these launches pool them, exactly and without a
 * momentum, into the statistics over all pixels of all batches seen (law of total variance), and write them into the statistics buffer.
 *
 * A layer (one row of the table): bmean, bvar float [N], the batch statistics over M pixels; off_mean, off_var the element offsets of
 * its moving_mean and moving_variance slices [off, off + N) in the statistics buffer stats_d, float [n_stats].  The accumulator acc_d,
 * double [n_stats], mirrors that layout: acc[off_mean + c] is channel c's running mean, acc[off_var + c] its running m2 (the sum of
 * squared deviations from the running mean).  Elements of acc and stats outside the slices are never read or written.
 *
 * t is the number of batches already added, passed by value; n = t * M pixels have been pooled before this batch.  Every float64
 * operation is rounded once (-ffp-contract=off), / is correctly rounded, in this order, per channel:
 *
 *   urso_bn_recal_add      mu_b = (double) bmean[c]   v_b = (double) bvar[c]
 *                          n1    = n + M
 *                          d     = mu_b - mean
 *                          mean' = mean + (d * M) / n1
 *                          m2'   = m2 + (v_b * M + (d * d) * ((n * M) / n1))
 *   urso_bn_recal_settle   stats[off_mean + c] = (float) mean      stats[off_var + c] = (float) (m2 / n)       n = t * M, t >= 1
 *
 * From the zero state (mean = m2 = 0, t = 0) one batch gives its own statistics back: the products with M are exact for M < 2^22.
 * A channel is one thread's, no atomics: the result does not depend on the grid.  A batch statistic that is not finite makes that
 * channel's result not finite and touches no other channel.  One launch covers every layer of the table.
 *
 * urso_bn_recal_plan validates the host table and copies it to layers_d (L rows, a synchronous copy): call it once per table.  add and
 * settle take both copies: the host one to check, the device one to run with.
 * URSO_EINVAL, before any launch or copy: L <= 0 or L > 65535; a null pointer; bmean / bvar off the 4-byte boundary, layers_d or acc_d
 * off the 8-byte one, stats_d off the 4-byte one; N <= 0; M <= 0; a negative offset; a slice that ends behind n_stats; two slices (of
 * one layer or of two) that overlap; t < 0 (add) or t < 1 (settle); t * M or (t + 1) * M above 2^53.
 */
typedef struct urso_bn_recal_layer {
    const float* bmean;     /* [N] batch mean */
    const float* bvar;      /* [N] batch variance (biased) */
    int64_t N, M;           /* channels; pixels per batch */
    int64_t off_mean;       /* offset of moving_mean [N] in the statistics buffer and of the running mean in the accumulator */
    int64_t off_var;        /* offset of moving_variance [N] and of the running m2 */
} urso_bn_recal_layer;
int urso_bn_recal_plan(int L, const urso_bn_recal_layer* layers_h, int64_t n_stats, urso_bn_recal_layer* layers_d);
int urso_bn_recal_add(int L, const urso_bn_recal_layer* layers_h, const urso_bn_recal_layer* layers_d, int64_t n_stats, double* acc_d,
                      int64_t t, void* stream);
int urso_bn_recal_settle(int L, const urso_bn_recal_layer* layers_h, const urso_bn_recal_layer* layers_d, int64_t n_stats,
                         const double* acc_d, float* stats_d, int64_t t, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * SWA: stochastic weight averaging and SWAG-diagonal (Config.SWA; ursonet_amd/swa.py is the same rule in NumPy and
 * the written specification).  Behind the optimizer, every `period` performed steps after the first `start`, the weights go into an
 * equal-weight running mean -- and, for SWAG-diagonal, their squares into a second one; a sample is mean + s * sd * z with
 * sd = sqrt(max(sq - mean^2, 0)) and z standard normal.  The exchange of the average with the weights is urso_ema_swap's (ursonet_ext.h).
 *
 * state_d   int32_t [URSO_SWA_STATE] = {period, start, ticks, models, collected, variance, 0, 0}.  period, start and variance are set by
 *           the host; urso_swa_update reads all and writes ticks, models and collected.
 * ls_state_d is the loss-scale state of ursonet_loss_scale.h or NULL.  When it is set and state[URSO_LS_LAST_SKIPPED] != 0 the optimizer
 *           skipped the step and urso_swa_update changes nothing, collected included.
 *
 *   ticks'  = min(ticks + 1, 2^31 - 1)
 *   collect = period > 0 and ticks' > start and (ticks' - start) % period == 0 and models < URSO_SWA_MAX_MODELS
 *   models' = models + 1 if collect;   collected = 1 if collect else 0
 *
 * urso_swa_update: every thread evaluates the gate.  Where it is shut no block touches w, mean or sq.  Where it is open, with m = models',
 * every float32 operation rounded once (-ffp-contract=off):
 *
 *   m == 1:  mean = w (the bits)                     sq = w * w
 *   m >  1:  r = fl32(1 / m)
 *            mean = mean + ((w - mean) * r)           sq = sq + (((w * w) - sq) * r)
 *
 * reading w and reading and writing mean: 12 bytes per parameter, 20 with sq.  A one-thread kernel behind the pass on the same stream
 * advances the state: by then every block has read it.  sq_d may be NULL: then only the mean is kept.  The state lives on the device, so
 * whether sq_d agrees with state[URSO_SWA_VARIANCE] shows only there: a NULL sq_d with variance != 0, or the reverse, touches no buffer
 * and no field but collected, which becomes URSO_SWA_REFUSED.
 *
 * urso_swag_sample: out[j] for j in [0, n) is the sample of element first + j of the flat buffer; mean_d, sq_d, out_d and z_out_d point at
 * that element.  Elements 4 i .. 4 i + 3 of the flat buffer use the four words x of Philox-4x32-10 with counter
 * (i mod 2^32, i >> 32, sample, 0) and key (seed mod 2^32, seed >> 32):
 *
 *   u = (x + 0.5) * 2^-32 (float64, exact)     (z0, z1) = sqrt(-2 log u0) * (cos, sin)(2 pi u1)     (z2, z3) likewise from u2, u3
 *
 * in float64, rounded to float32 at the end; then in float32, each operation rounded once, sqrtf correctly rounded:
 *
 *   d = sq - (mean * mean)     sd = sqrtf(d > 0 ? d : 0)     out = mean + ((s * sd) * z)
 *
 * z_out_d, when not NULL, receives z.  The values depend on first + j alone, not on the grid, the alignment or how a range is cut into
 * launches.  s is the host's fl32(sqrt(var_scale)).
 *
 * Both streams: 256 threads per block, at most 4096 blocks with a grid stride, 16 bytes per lane and access where all buffers of the
 * launch sit alike against the 16-byte boundary (a scalar head and tail around the vectors), scalars alone otherwise.  n == 0 launches
 * nothing.  Nothing outside [0, n) is read or written.
 * URSO_EINVAL, before any launch: a null pointer (sq_d of the update and z_out_d may be NULL); n < 0; a pointer off the 4-byte boundary;
 * w, mean, sq (out or z_out and any other buffer) being one buffer or overlapping within n elements; first negative or no multiple of 4;
 * s negative or not finite; sample < 0.
 */
#define URSO_SWA_STATE 8
#define URSO_SWA_PERIOD 0
#define URSO_SWA_START 1
#define URSO_SWA_TICKS 2
#define URSO_SWA_MODELS 3
#define URSO_SWA_COLLECTED 4
#define URSO_SWA_VARIANCE 5
#define URSO_SWA_MAX_MODELS 16777216
#define URSO_SWA_REFUSED (-1)
int urso_swa_update(int64_t n, const float* w_d, float* mean_d, float* sq_d, int32_t* state_d, const float* ls_state_d, void* stream);
int urso_swag_sample(int64_t n, int64_t first, const float* mean_d, const float* sq_d, float* out_d, float* z_out_d, float s, uint64_t seed,
                     int sample, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * Ensemble inference: the Bayesian model average of a classification head (predict / evaluate / test_and_submit with members=...,
 * DESIGN.md section 24; ursonet_amd/ensemble.py, add64 / settle64, is the same rule in NumPy float64 and the written specification).
 * The network runs once per member (weight set) over the dataset; urso_ens_add folds a member's softmax over one batch of logit rows into
 * fp64 accumulators, urso_ens_settle turns accumulated rows into log-probabilities that urso_quat_wavg_decode, urso_quat_gmm_fit,
 * urso_pose_decode and urso_pose_eval take in the place of logits, and into the uncertainty columns.  The average is the mean of the
 * members' PMFs, decoded once -- not a mean of decoded poses.
 *
 * urso_ens_add, for every valid batch row b < n, r = row0 + b, z = logits + b * ld (K fp32 values); all arithmetic fp64, each operation
 * rounded once (-ffp-contract=off), exp and log the device library's:
 *
 *   m   = max_i z_i, a NaN winning                 d_i = (double) z_i - (double) m              e_i = exp(d_i)
 *   Z   = sum_i e_i                                S   = sum_i (e_i == 0 ? 0 : e_i * (-d_i))    (a vanished term adds exactly 0, also for d_i = -inf)
 *   p_i = e_i / Z                                  H   = log(Z) + S / Z      the member's entropy in nats; both terms >= 0: no cancellation
 *   first != 0:  acc[r][i]  = p_i                  stat[r] = {H, 1, 0, 0}      overwrites: the buffers need no clearing and may hold NaN
 *   first == 0:  acc[r][i] += p_i                  stat[r][0] += H             stat[r][1] += 1
 *
 * A NaN or +inf logit makes the whole row NaN (m = +inf gives d = NaN).  Rows past n, columns past K and the padding between rows are
 * never read or written.
 *
 * urso_ens_settle, for every b < n, r = row0 + b, over M members:
 *
 *   pbar_i     = acc[r][i] / (double) M
 *   logp[b][i] = (float) log(pbar_i);  pbar_i == 0 gives -FLT_MAX, not -inf, so that z - max stays finite in every downstream kernel;
 *                softmax(logp) is pbar up to fp32 rounding.  logp is [n][K]: the rows of this launch only
 *   Hbar       = -sum_i (pbar_i == 0 ? 0 : pbar_i * log(pbar_i))
 *   table[r]   = { H_MEAN = Hbar,  H_MEMBERS = stat[r][0] / M,  MI = max(Hbar - H_MEMBERS, 0) with a NaN staying NaN (the mutual information
 *                  between the prediction and the member, BALD: the epistemic part),  PEAK = max_i pbar_i (a NaN winning),
 *                  ARGMAX = the lowest index of the peak,  N_MEMBERS = stat[r][1] (the caller checks that it equals M),  0,  0 }
 *
 * Launch shape and reduction order, which are part of the result: one workgroup of 1024 threads (16 waves) per valid row.  Columns are
 * dealt by their index alone: thread t owns the groups of four columns g = t, 1024 + t, 2048 + t, ... (columns 4 g .. 4 g + 3), and the
 * ragged end K % 4 is the group behind the last whole one.  A thread adds its terms to its running sum in column order; the threads' sums
 * are added by the xor shuffle 32, 16, .. 1 across a wave, then the 16 wave sums in wave order (the order urso_lars_norms documents).
 * A group is one 16-byte load (store) where the row's first element sits on a 16-byte boundary and four 4-byte (8-byte) ones where it
 * does not -- the same columns on the same thread, so every output is a function of the row's inputs alone: the same bits on a repeated
 * launch, and for the same row whatever B, n, row0, ld, the alignment and its position in the batch.  The logits are read three times (max,
 * sums, write; the second and third time from L2) and exp is computed twice: no e_i is kept.
 *
 * No allocation, no workspace, no host synchronisation.  n == 0 launches nothing.
 * URSO_EINVAL, with a message, before any launch: a null struct or pointer; B <= 0, n outside [0, B] (settle: n < 0); row0 < 0; K < 1;
 * ld < K; M outside [1, URSO_ENS_MAX_MEMBERS]; logits / logp off the 4-byte boundary; acc / stat / table off the 8-byte one.
 */
#define URSO_ENS_MAX_MEMBERS 64
#define URSO_ENS_STAT 4
#define URSO_ENS_COLS 8
#define URSO_ENS_H_MEAN 0
#define URSO_ENS_H_MEMBERS 1
#define URSO_ENS_MI 2
#define URSO_ENS_PEAK 3
#define URSO_ENS_ARGMAX 4
#define URSO_ENS_N_MEMBERS 5
typedef struct urso_ens_add_args {
    int32_t B, n;                    /* rows of logits, valid rows (0 <= n <= B) */
    int64_t row0;                    /* accumulator row of batch row 0 */
    int32_t K, ld;                   /* bins; floats between rows of logits (ld >= K) */
    int32_t first, pad;              /* != 0: this is the first member (overwrite) */
    const float* logits;             /* [B][ld] */
    double* acc;                     /* [rows][K] */
    double* stat;                    /* [rows][URSO_ENS_STAT] */
} urso_ens_add_args;
typedef struct urso_ens_settle_args {
    int32_t n;                       /* rows of this launch */
    int64_t row0;                    /* accumulator / table row of row 0 */
    int32_t K, M;                    /* bins; members added */
    const double* acc;               /* [rows][K] */
    const double* stat;              /* [rows][URSO_ENS_STAT] */
    float* logp;                     /* [n][K] */
    double* table;                   /* [rows][URSO_ENS_COLS] */
} urso_ens_settle_args;
int urso_ens_add(const urso_ens_add_args* args, void* stream);
int urso_ens_settle(const urso_ens_settle_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * Temperature scaling of the classification heads (calibrate(), predict / evaluate / test_and_submit with calibration=..., DESIGN.md
 * section 25; ursonet_amd/calibrate.py, stats64 / reduce64 / scale32, is the same rule in NumPy float64 and the written specification).
 * One scalar beta = 1 / T per head is fitted on held-out labelled data by minimising the head's own cross-entropy, and the head's logits
 * are multiplied by it before every decode.  For a row of K fp32 logits z with the fp32 encoded target y (the PMF the training loss
 * uses, which may be un-normalised)
 *
 *   CE(beta) = sy lse(beta) - beta yz      dCE/dbeta = sy m1(beta) - yz      d2CE/dbeta2 = sy var(beta) >= 0
 *   sy = sum_i y_i    yz = sum_i y_i z_i    lse = log sum_i exp(beta z_i)    m1 = E_p[z]    var = Var_p[z]    p = softmax(beta z)
 *
 * urso_temp_stats, for every valid batch row b < n, z = logits + b * ld_z, y = target + b * ld_y, over the J inverse temperatures beta_j
 * passed by value; all arithmetic fp64, each operation rounded once (-ffp-contract=off), exp and log the device library's:
 *
 *   sweep 1   m  = max_i z_i (fp32, a NaN winning)       sy = sum_i (double) y_i       yz = sum_i (y_i == 0 ? 0 : (double) y_i * (double) z_i)
 *   sweep 2   d_i = (double) z_i - (double) m            e_ij = exp(beta_j * d_i)
 *             Z_j = sum_i e_ij        A_j = sum_i (e_ij == 0 ? 0 : e_ij * d_i)        Q_j = sum_i (e_ij == 0 ? 0 : e_ij * (d_i * d_i))
 *             (a vanished term adds exactly 0, also for d_i = -inf; a bin the target gives no weight adds nothing to yz, also at z_i = -inf)
 *   close     r_j = A_j / Z_j         LSE_j = log(Z_j) + beta_j * m         M1_j = m + r_j         VAR_j = Q_j / Z_j - r_j * r_j
 *             poison = 0 * (double) m  (0 for a finite m, NaN otherwise)      SY = sy + poison       YZ = yz + poison
 *   out[row0 + b] = { SY, YZ, LSE_0, M1_0, VAR_0, .. LSE_(J-1), M1_(J-1), VAR_(J-1) }: 2 + 3 J of the row's URSO_TEMP_COLS doubles; the
 *             columns behind them are not written
 *
 * A NaN or +inf logit, or a row of -inf alone, makes every written column of that row NaN and touches no other row.  The logits are read
 * once per sweep for all J temperatures (the second time out of L2); the 3 J accumulators live in registers.  Rows >= n, rows of out
 * outside [row0, row0 + n) and the padding behind K are never read or written.
 *
 * urso_temp_reduce, over rows 0 .. N - 1 of such a table, for j < J:
 *
 *   CE_rj = SY_r * LSE_rj - beta_j * YZ_r        g_rj = SY_r * M1_rj - YZ_r        h_rj = SY_r * VAR_rj       (products first, then the difference)
 *   totals[j] = { sum_r CE_rj,  sum_r g_rj,  sum_r h_rj,  the number of rows r where one of SY, YZ, LSE_j, M1_j, VAR_j is not finite }
 *
 * One workgroup of 1024 threads: thread t adds rows t, t + 1024, .. in that order, then the order below.  Rows that are not finite are
 * added like the others: the count says why a total is not finite.
 *
 * urso_temp_scale, for b < n and i < K:  out[b][i] = (float) ((double) in[b][i] * beta) -- the product is exact in fp64, so this is the
 * correctly rounded fp32 product; beta == 1 gives the input's bits back, NaN and +-inf pass through.  in == out is allowed.
 *
 * Launch shape and reduction order of urso_temp_stats are urso_ens_add's and part of the result: one workgroup of 1024 threads (16 waves)
 * per valid row; thread t owns the groups of four columns g = t, 1024 + t, .. and the ragged end K % 4 is the group behind the last whole
 * one; a thread adds its terms in column order; the threads' sums are added by the xor shuffle 32, 16, .. 1 across a wave, then the 16
 * wave sums in wave order.  A group is one 16-byte load where the row's first element sits on a 16-byte boundary and four 4-byte loads
 * where it does not (logits and target each by their own alignment) -- the same columns on the same thread, so every output is a function
 * of the row alone: the same bits on a repeated launch and whatever B, n, row0, the strides, the alignment, J's other temperatures and the
 * row's position in the batch.  urso_temp_scale deals the same groups over a grid of (n, ceil((K / 4 + 1) / 1024)) workgroups, 16-byte
 * loads and stores under the same rule.
 *
 * No allocation, no workspace, no host synchronisation.  n == 0 launches nothing.
 * URSO_EINVAL, with a message, before any launch: a null struct or pointer; J outside [1, URSO_TEMP_MAX_J]; K < 1; a row stride < K;
 * n outside [0, B]; row0 < 0; N < 1; a beta that is not finite and > 0; logits / target / in / out off the 4-byte boundary; the fp64
 * tables off the 8-byte one.
 */
#define URSO_TEMP_MAX_J 8
#define URSO_TEMP_COLS 26            /* 2 + 3 * URSO_TEMP_MAX_J */
#define URSO_TEMP_SY 0
#define URSO_TEMP_YZ 1
#define URSO_TEMP_LSE 2              /* + 3 j */
#define URSO_TEMP_M1 3               /* + 3 j */
#define URSO_TEMP_VAR 4              /* + 3 j */
#define URSO_TEMP_TOTALS 4           /* {CE, g, h, rows that are not finite} */
typedef struct urso_temp_stats_args {
    int32_t B, n;                    /* rows of logits and target, valid rows (0 <= n <= B) */
    int64_t row0;                    /* table row of batch row 0 */
    int32_t K, ld_z, ld_y, J;        /* bins; floats between rows of logits and of target (>= K); temperatures (1 .. 8) */
    double beta[URSO_TEMP_MAX_J];    /* the first J are used */
    const float* logits;             /* [B][ld_z] */
    const float* target;             /* [B][ld_y] */
    double* out;                     /* [rows][URSO_TEMP_COLS] */
} urso_temp_stats_args;
typedef struct urso_temp_reduce_args {
    int64_t N;                       /* rows 0 .. N - 1 */
    int32_t J, pad;
    double beta[URSO_TEMP_MAX_J];    /* the temperatures the rows were written with */
    const double* rows;              /* [N][URSO_TEMP_COLS] */
    double* totals;                  /* [URSO_TEMP_MAX_J][URSO_TEMP_TOTALS]; rows j < J are written */
} urso_temp_reduce_args;
typedef struct urso_temp_scale_args {
    int32_t B, n;                    /* rows, valid rows (0 <= n <= B) */
    int32_t K, ld_in, ld_out, pad;   /* bins; floats between rows (>= K) */
    double beta;
    const float* in;                 /* [B][ld_in] */
    float* out;                      /* [B][ld_out] */
} urso_temp_scale_args;
int urso_temp_stats(const urso_temp_stats_args* args, void* stream);
int urso_temp_reduce(const urso_temp_reduce_args* args, void* stream);
int urso_temp_scale(const urso_temp_scale_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif
