/* ursonet_ext.h -- the C ABI of liburso_ext.so, the extension library next to liburso_hip.so (gfx950).  Plain C99.
 *
 * liburso_hip.so's surface is frozen at the entry points of ursonet_hip.h; what is added after that lives here, in a library of its
 * own.  The extension reuses the main library's status codes, its error text (a failure here is read with urso_last_error()) and its
 * launch profiler, so liburso_hip.so must be loaded first with its symbols visible to later loads: link both and name liburso_hip.so
 * in front, or dlopen it with RTLD_GLOBAL before this one (ursonet_amd/hip.py does the latter on first use).  Every entry point
 * returns URSO_OK or a negative URSO_E* code of ursonet_hip.h.
 */
#ifndef URSONET_EXT_H
#define URSONET_EXT_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_hip.h"     /* URSO_OK / URSO_E*, and the URSO_EVAL_* columns the table below shares */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Test-time view fusion (ursonet_amd/views.py): the network saw V rotated views of every image of a batch (view v
 * = the frame re-rendered through a camera rotated by R_v, as utils.rotate_cam does, utils.py:30-86) and urso_pose_decode /
 * urso_pose_eval wrote one estimate per view and image.  This entry point rotates every estimate back into the unrotated camera and
 * fuses the V estimates of an image into one pose plus how well the views agree.  One launch per batch, one wave per valid image
 * b < n writes row row0 + b of the fp64 table [rows][URSO_FUSE_COLS]; rows past n are not touched.  No workspace, no allocation, no host
 * synchronisation; n = 0 launches nothing.  All arithmetic is fp64, compiled without contraction.
 *
 * Inputs (device pointers):
 *   est     fp64: the row of view v and batch row b is at est + (v * est_view_rows + b) * est_ld, with LOC_EST in columns 0..2 and
 *           Q_EST ([x, y, z, w]) in columns 3..6 -- where urso_pose_decode and urso_pose_eval both write them.  est_ld >= 7,
 *           est_view_rows >= B.
 *   r       fp64 [V][9]: the view rotations R_v, row-major.    qr  fp64 [V][4]: SO32quat(R_v) (se3lib.py:77-115).
 *   loc_gt  fp64 [B][3], q_gt fp64 [B][4]: the truth, optional; both or neither.
 *   1 <= V <= URSO_FUSE_MAX_VIEWS.
 *
 * De-rotation, the inverse of the pose update t' = t R^T, q' = quat_mult(SO32quat(R), q) of utils.py:53-56:
 *   t^_v[j] = sum_i t_v[i] R_v[i][j]                                        (t_v R_v)
 *   q^_v    = quat_mult(conj(qr_v), q_v) / |.|   with conj(q) = [-x, -y, -z, w] and se3lib.quat_mult's formula (se3lib.py:164-179):
 *             quat_mult(a, b) = [ aw bx + az by - ay bz + ax bw,  -az bx + aw by + ax bz + ay bw,
 *                                 ay bx - ax by + aw bz + az bw,  -ax bx - ay by - az bz + aw bw ]
 *   A view whose r is exactly the identity matrix is passed through with no arithmetic: t^ = t, q^ = q.
 *
 * Fusion (every sum runs over v = 0 .. V - 1 in that order, in one accumulator: the result is a function of the inputs alone):
 *   LOC_EST = (1/V) sum_v t^_v
 *   S       = (1/V) sum_v q^_v q^_v^T
 *   Q_EST   = unit eigenvector of S's largest eigenvalue by the decode's solver (cyclic Jacobi), largest-magnitude component
 *             positive: q and -q inputs fuse identically, bit for bit.
 *   V == 1:   LOC_EST = t^_0 and Q_EST = q^_0 with no division and no eigen-solve, so one identity view reproduces the input bits.
 *
 * Agreement columns:
 *   LOC_SPREAD  = sqrt((1/V) sum_v ||t^_v - LOC_EST||^2)
 *   ORI_SPREAD  = sqrt((1/V) sum_v angle(q^_v, Q_EST)^2) * 180/pi, angle = the rotation angle 2 acos|a . b| between two orientations,
 *                 evaluated as 4 atan2(|a |b| - s b |a||, |a |b| + s b |a||), s = sign(a . b): the same angle, but accurate near 0,
 *                 where acos turns one ulp of the dot product into 1.7e-6 degrees.  Views that agree exactly give exactly 0.
 *   VIEW_LAMBDA = Q_EST^T S Q_EST: 1 when all views agree, 1/4 when they are spread uniformly.
 *   N_VIEWS     = V
 *   V == 1: both spreads are 0.
 *
 * With a truth, by urso_pose_eval's formulas and its clip convention (the same device routine, so the same bits for the same
 * estimate): LOC_ERR = ||LOC_EST - loc_gt||, ORI_ERR = 2 acos(min(1, |Q_EST . q_gt|)) * 180/pi, ESA = LOC_ERR / ||loc_gt|| +
 * 2 acos(min(1, |Q_EST . q_gt|)), DIST = loc_gt[2].  Without one the four are NaN.
 *
 * Columns 0..10 sit at URSO_EVAL_*'s positions; column 15 is 0.  A NaN input gives NaN in everything it feeds: no view is dropped.
 *
 * Bad arguments return URSO_EINVAL before any launch: a null struct, a null est / r / qr / table, exactly one of loc_gt / q_gt, B <= 0,
 * n outside [0, B], row0 < 0, V outside [1, URSO_FUSE_MAX_VIEWS], est_ld < 7, est_view_rows < B.
 */
enum { URSO_FUSE_LOC_EST = 0, URSO_FUSE_Q_EST = 3, URSO_FUSE_LOC_ERR = 7, URSO_FUSE_ORI_ERR = 8, URSO_FUSE_ESA = 9, URSO_FUSE_DIST = 10,
       URSO_FUSE_LOC_SPREAD = 11, URSO_FUSE_ORI_SPREAD = 12, URSO_FUSE_VIEW_LAMBDA = 13, URSO_FUSE_N_VIEWS = 14, URSO_FUSE_COLS = 16 };
enum { URSO_FUSE_MAX_VIEWS = 64 };
typedef struct urso_pose_fuse_views_args {
    int32_t B, n;                    /* rows of a view's block of est and of loc_gt / q_gt, valid rows (0 <= n <= B) */
    int64_t row0;                    /* table row of batch row 0 */
    int32_t V;                       /* views */
    int32_t est_ld;                  /* doubles between rows of est */
    int64_t est_view_rows;           /* rows between the blocks of consecutive views */
    const double* est;
    const double* r;
    const double* qr;
    const double* loc_gt;            /* optional, with q_gt */
    const double* q_gt;
    double* table;
} urso_pose_fuse_views_args;
int urso_pose_fuse_views(const urso_pose_fuse_views_args* args, void* stream);

/*
 * Learnable loss weights (Config.LEARNABLE_LOSS_WEIGHTS; after Kendall & Cipolla, and net.py:648-654 + the
 * commented-out `loss / exp(weight) + weight` of net.py:709-760).  Each entry point is the plain loss of ursonet_hip.h with the same
 * leading arguments, plus s_d, ds_d and ls_state_d in front of the stream; the kernels are the plain ones (one device code).
 *   s_d         fp32[1], device: the trainable log-variance s of this loss (a slot of the flat parameter buffer).  Required.
 *   ds_d        fp32[1], device: OVERWRITTEN (never accumulated) with d(reported loss)/ds; NULL = s is frozen, nothing is written.
 *   ls_state_d  the loss-scale state of ursonet_loss_scale.h or NULL: as in the *_ls forms, the finished fp32 head gradient is multiplied
 *               by state[URSO_LS_SCALE] last, in front of its one rounding to dt.  ds_d is never scaled.
 * With w = weight and L the batch-mean loss without its weight:
 *   w_eff          = w * expf(-s)                  that one fp32 product
 *   P              = the plain entry point's loss under weight w_eff, in its order of operations (= w_eff L)
 *   head gradient  = the plain entry point's under weight w_eff, in its order of operations
 *   loss_d[0]      = P + w * s                     (= w (L exp(-s) + s); may be negative)
 *   ds_d[0]        = w - P                         (= w (1 - L exp(-s)), from the P that is reported)
 * At s = 0, w_eff = w exactly: the head gradient, norms_d / q_d and the loss have the bits of the plain form (ls_state_d NULL) or of the
 * *_ls form (ls_state_d set).  Bad arguments (those of the plain form, or a null s_d) return URSO_EINVAL before any launch.
 */
int urso_softmax_xent_fwd_bwd_lw(int B, int K, const float* logits_d, const float* labels_d, float weight, int relu_mask, int dt,
                                 float* loss_d, void* dz_d, float* row_ws_d, const float* s_d, float* ds_d, const float* ls_state_d,
                                 void* stream);
int urso_rel_l2_fwd_bwd_lw(int B, int D, int ld, const float* gt_d, const float* pred_d, float weight, int dt, float* loss_d,
                           void* dpred_d, float* norms_d, const float* s_d, float* ds_d, const float* ls_state_d, void* stream);
int urso_absdot_fwd_bwd_lw(int B, int D, int ld, int normalize, const float* gt_d, const float* x_d, float weight, int dt, float* q_d,
                           float* loss_d, void* dx_d, const float* s_d, float* ds_d, const float* ls_state_d, void* stream);

/*
 * Exponential moving average of the weights (Config.WEIGHT_EMA; ursonet_amd/weight_ema.py is the same rule in NumPy
 * float32).  The reference has none.  The state is ONE fp32 buffer of URSO_EMA_FIELDS floats in device memory:
 *   URSO_EMA_DECAY       the configured decay, in (0, 1)
 *   URSO_EMA_WARMUP      0 or 1: with 1 the decay follows the TensorFlow num_updates schedule below
 *   URSO_EMA_UPDATES     t, the updates done so far; saturates at 2^24, where an fp32 counter stops
 *   URSO_EMA_NEXT_DECAY  d, the decay the next update will use
 *   4..7                 reserved, zero
 *
 * urso_ema_update, one streaming launch and a one-thread launch behind it on the same stream.  For every i < n, with d read from the state:
 *   c      = 1.0f - d
 *   ema[i] = ema[i] + c * (w[i] - ema[i])
 * three fp32 operations, each rounded once, compiled without contraction: the result is a function of the inputs alone.  Nothing is
 * guarded: a NaN in w reaches ema.  Where w[i] == ema[i] the difference is exactly 0 and ema[i] keeps its bits (a frozen layer's average
 * is its weights).  Then, after every block has read d, the state advances:
 *   t          = min(t + 1, 2^24)
 *   NEXT_DECAY = decay                                               (warm-up off)
 *   NEXT_DECAY = min(decay, fl32((1.0f + t) / (10.0f + t)))          (warm-up on, with the new t; the quotient of the two fp32 sums is
 *                                                                     correctly rounded, whatever the compiler's fp32 division mode)
 * ls_state_d is the loss-scale state of ursonet_loss_scale.h or NULL.  When it is set and state[URSO_LS_LAST_SKIPPED] != 0 the optimizer
 * skipped this step: ema keeps its bits and the state is not advanced (call it behind urso_loss_scale_update).
 *
 * urso_ema_swap exchanges the bit patterns of two fp32 buffers in place, NaN payloads included (they move as 32-bit integers).
 *
 * Both: no allocation, no synchronisation; n == 0 launches nothing and advances nothing.  Bad arguments return URSO_EINVAL before any
 * launch: a null w / ema / state (a / b), n < 0, a pointer that is not 4-byte aligned, a == b.  Buffers that are 16-byte aligned, or
 * misaligned alike, are moved 16 bytes per access; the two buffers must not overlap unless they are the same (update only).
 */
enum { URSO_EMA_DECAY = 0, URSO_EMA_WARMUP = 1, URSO_EMA_UPDATES = 2, URSO_EMA_NEXT_DECAY = 3, URSO_EMA_FIELDS = 8 };
int urso_ema_update(int64_t n, const float* w_d, float* ema_d, float* state_d, const float* ls_state_d, void* stream);
int urso_ema_swap(int64_t n, float* a_d, float* b_d, void* stream);

/*
 * Gradient accumulation over k micro-batches (Config.GRAD_ACCUM_STEPS; ursonet_amd/grad_accum.py is the same rule in
 * NumPy float32).  The reference has none.  With g what a backward pass left in the flat gradient buffer and acc a second buffer of n floats:
 *
 * urso_grad_accum, one streaming launch behind the backward pass of a micro-step that does not close.  For every i < n:
 *   first != 0:  acc[i] = g[i]                 the bits, NaN payloads included (they move as 32-bit integers)
 *   first == 0:  acc[i] = acc[i] + g[i]        one fp32 add, rounded once
 *
 * urso_grad_accum_close, one streaming launch in front of the optimizer of the closing micro-step.  For every i < n:
 *   g[i] = (acc[i] + g[i]) * c                 one fp32 add and one fp32 multiply, each rounded once; acc is only read
 * c is fl32(1 / k), computed by the caller.  Compiled without contraction: every value is a function of the inputs alone.  Nothing is
 * guarded: a non-finite value in either buffer reaches g.
 *
 * The grid.  Both launch B = urso_grad_accum_parts(n) = min(4096, ceil(ceil(n / 4) / 256)) blocks of 256 threads (0 for n <= 0), a function
 * of n alone.  When g and acc sit alike against the 16-byte boundary, head = min(n, ((16 - address % 16) % 16) / 4) leading elements and the
 * (n - head) % 4 trailing ones are scalars and the nvec = (n - head) / 4 groups of four between them are vectors; otherwise every element is
 * a scalar (head = n, nvec = 0).  Thread t of the grid (t = 256 block + thread) handles the vectors t, t + 256 B, t + 512 B, ... and then
 * the scalars t, t + 256 B, ... of the list [head elements, tail elements]: every element is read and written by exactly one thread, once.
 *
 * The slots.  The close launch also writes sqpart[b], b < B: the sum of squares of the values block b stored.  Every square v * v is
 * rounded once and added to the thread's running sum (from 0.0f) in the order the thread stores: its vectors in order, x y z w each, then its
 * scalars.  The 64 lanes of a wave are added by the xor shuffle (offsets 32, 16, 8, 4, 2, 1), the four wave sums in wave order from 0.0f:
 * the order of the urso_param_batch_run_sq slots, so urso_sqnorm_final over the B slots yields the squared norm of the closed gradient
 * without a pass over it.  A non-finite stored value makes its slot non-finite.
 *
 * All: no allocation, no synchronisation; n == 0 launches nothing (and wants nparts == 0).  Bad arguments return URSO_EINVAL before any
 * launch: a null g / acc / sqpart, n < 0, a pointer that is not 4-byte aligned, g == acc, nparts != urso_grad_accum_parts(n).  The two
 * buffers must not overlap.
 */
int urso_grad_accum(int64_t n, const float* g_d, float* acc_d, int first, void* stream);
int urso_grad_accum_parts(int64_t n);
int urso_grad_accum_close(int64_t n, float* g_d, const float* acc_d, float c, float* sqpart_d, int nparts, void* stream);

/*
 * Layer-wise adaptive rate scaling for SGD with momentum (Config.LARS; ursonet_amd/lars.py is the same rule in
 * NumPy).  The reference has none.  Five entry points (the library exports 14 with them): two on the host that plan the grid and three
 * launches that take the place of urso_sgd_momentum_clip[_ls] behind the global norm.
 *
 * The tensors.  T tensors lie in the flat fp32 buffers w, g and v: tensor t is the n[t] floats from element off[t].  Each has an adapt
 * flag; a tensor that does not adapt has trust 1 and moves exactly as under urso_sgd_momentum_clip.  Floats that belong to no tensor
 * (the padding between slices) are neither read nor written.
 *
 * The rule.  With lr = hyper[0], mom = hyper[1], clip = hyper[2] and, in fp32 as urso_sgd_momentum_clip computes it,
 *   norm = sqrtf(normsq[0]);  c = (clip > 0 && norm >= clip) ? clip / norm : 1
 * per tensor, in fp64 (+ * / sqrt and comparisons only, compiled without contraction):
 *   nw = sqrt(sum of w^2), ng = sqrt(sum of g^2)                      the sums: "The order" below
 *   q = 1                                     if the tensor does not adapt, or nw == 0, or ng == 0 (fresh zeros, a frozen layer)
 *   q = eta * nw / ((double)c * ng + eps)     otherwise
 *   q = min(q / (double)lr, 1)                with clip_mode = 1 (LARC's "clip": the tensor's rate never exceeds the global one)
 *   trust = (float)q                          rounded once
 * per element of the tensor, in fp32, every operation rounded once:
 *   step = (lr * c) * trust;  v[i] = mom * v[i] - step * g[i];  w[i] = w[i] + v[i]
 *
 * The order.  Tensor t is cut into ceil(n[t] / URSO_LARS_CHUNK) chunks, the last one short; one block of 256 threads owns one chunk and
 * writes one slot pair part[block] = {sum of w^2, sum of g^2}, fp32.  Thread i of the block owns the 16-byte groups i, 256 + i, 512 + i,
 * 768 + i of the chunk.  Every square is rounded once and added to the thread's running sum (from 0.0f) in the order the thread reads:
 * its groups in order, x y z w each.  The 64 lanes of a wave are added by the xor shuffle (offsets 32, 16, 8, 4, 2, 1), the four wave
 * sums in wave order from 0.0f: the order of urso_grad_accum_close's slots.  Elements past the tensor's end contribute nothing.  A
 * tensor's slots are then added in index order in fp64 (from 0.0).  Every result is a function of the inputs alone.
 *
 * Host planning (no GPU needed):
 *   urso_lars_blocks   NB = the sum over t of ceil(n_h[t] / URSO_LARS_CHUNK), a function of the sizes alone; 0 for T == 0.  A negative
 *                      return is an error code (T < 0, a null n_h with T > 0, a negative size, NB above 2^31 - 1).
 *   urso_lars_plan     fills blockmap_h[NB][2], one (tensor, chunk) pair per block, tensors in index order and chunks in order within a
 *                      tensor, and first_h[T + 1], each tensor's first slot (first_h[T] = NB).  nblocks must be urso_lars_blocks(T, n_h).
 *
 * Device tables (the caller uploads them once per plan): tab_d int64 [T][2] = {off[t], n[t]}, the same values as off_h / n_h;
 * blockmap_d and first_d as urso_lars_plan filled them; adapt_d int32 [T], nonzero = adapts.  The launches check the host tables and
 * trust the device tables to hold the same.
 *
 * Launches, in this order on one stream; no allocation, no synchronisation:
 *   urso_lars_norms    NB blocks of 256 threads.  Reads w and g once (8 bytes per parameter) and writes part_d[NB][2].
 *   urso_lars_trust    T blocks of two waves: block t adds the slots first[t] .. first[t + 1] - 1 of tensor t in index order (one wave
 *                      the w^2 slots, the other the g^2 slots) and writes trust_d[t] (fp32) and stat_d[t][3] = {nw, ng, q} (fp64), for
 *                      every tensor, adapting or not.  With ls_state_d set and a non-finite normsq[0] it writes nothing.  nblocks is NB,
 *                      the slot pairs part_d holds.
 *   urso_lars_sgd      NB blocks of 256 threads over the same block map: each reads trust_d[tensor], recomputes c and applies the
 *                      update with 16-byte accesses (20 bytes per parameter); a tensor's last n % 4 elements move as scalars.  With
 *                      ls_state_d set (the loss-scaled form) a non-finite normsq[0] changes nothing: w and v keep their bits.
 * T == 0 (and so NB == 0) launches nothing.
 *
 * Bad arguments return URSO_EINVAL with a message before any launch: a null pointer; T < 0; a negative size; an offset that is negative
 * or not a multiple of 4 floats; w, g or v not 16-byte aligned; tab, part or stat not 8-byte aligned; two non-empty tensors that overlap;
 * nblocks != urso_lars_blocks(T, n_h); w, g and v not pairwise distinct; eta not a finite number > 0, eps not a finite number >= 0,
 * clip_mode outside {0, 1}.
 */
#define URSO_LARS_CHUNK 4096
int urso_lars_blocks(int T, const int64_t* n_h);
int urso_lars_plan(int T, const int64_t* n_h, int nblocks, int32_t* blockmap_h, int32_t* first_h);
int urso_lars_norms(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                    const float* w_d, const float* g_d, float* part_d, void* stream);
int urso_lars_trust(int T, const int32_t* first_d, const int32_t* adapt_d, int nblocks, const float* part_d, const float* hyper_d,
                    const float* normsq_d, double eta, double eps, int clip_mode, float* trust_d, double* stat_d,
                    const float* ls_state_d, void* stream);
int urso_lars_sgd(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                  float* w_d, const float* g_d, float* v_d, const float* trust_d, const float* hyper_d, const float* normsq_d,
                  const float* ls_state_d, void* stream);

#ifdef __cplusplus
}
#endif

#endif
