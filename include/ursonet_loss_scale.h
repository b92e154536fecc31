/* ursonet_loss_scale.h -- the loss-scaling extension of the C ABI of liburso_hip.so (10 entry points).  Included by ursonet_hip.h, behind
 * the types it uses (urso_param_desc); include that header, not this one.  Plain C99. */
#ifndef URSONET_LOSS_SCALE_H
#define URSONET_LOSS_SCALE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Loss scaling for 16-bit training (Config.LOSS_SCALE).  The reference has none (Keras floatx('float16') has none): the
 * gradient of a near-uniform 13,824-bin soft classification at batch 32 is ~2e-6 per logit, below fp16's smallest normal (6.1e-5).
 * The state is ONE fp32 buffer of URSO_LS_FIELDS floats in device memory, indexed by the URSO_LS_* constants; scale is a power of two and
 * inv_scale = 1 / scale exactly.  A step under loss scaling is:
 *   the *_ls losses         : as the plain entry points, but the finished fp32 gradient is multiplied by state[URSO_LS_SCALE] LAST, immediately
 *                             in front of its one rounding to dt; loss_d keeps the unscaled loss, bit for bit.  state_d = NULL is the plain form
 *                             (the plain entry points forward with NULL).
 *   the backward pass       : unchanged (linear in the head gradients)
 *   the *_ls finalisations  : urso_param_batch_run_ls (FINALIZE phases; sqpart_d may be NULL = no norm slots), urso_param_grad_finalize_ls
 *                             (likewise) and urso_bn_backward_ls (its gbeta / ggamma slices; dbeta / dgamma / dz stay in scaled units)
 *                             multiply the raw fp32 gradient by state[URSO_LS_INV_SCALE] BEFORE the weight-decay term, the folded-BN gamma /
 *                             beta derivation and the squared-norm slots: the gradient buffer, the norm and the clip are in true units
 *   the *_ls optimizers     : no-ops when normsq_d[0] is not finite (an overflow of the scaled pass): w, v, m, vhat and Adam's t keep their bits
 *   urso_loss_scale_update  : one thread, after the optimizer.  Non-finite norm: scale = max(scale / 2, min), good_steps = 0,
 *                             skipped_total += 1, last_step_skipped = 1.  Finite: last_step_skipped = 0, good_steps += 1, and when it reaches
 *                             growth_interval: scale = min(2 scale, max), good_steps = 0.  growth_interval <= 0 is a STATIC scale: skips are
 *                             recorded, the scale never moves.  (ursonet_amd/loss_scale.py next_state is the same rule in Python.)
 */
enum { URSO_LS_SCALE = 0, URSO_LS_INV_SCALE = 1, URSO_LS_GOOD_STEPS = 2, URSO_LS_GROWTH_INTERVAL = 3, URSO_LS_MIN = 4, URSO_LS_MAX = 5,
       URSO_LS_SKIPPED_TOTAL = 6, URSO_LS_LAST_SKIPPED = 7, URSO_LS_FIELDS = 8 };
int urso_softmax_xent_fwd_bwd_ls(int B, int K, const float* logits_d, const float* labels_d, float weight, int relu_mask, int dt,
                                 float* loss_d, void* dz_d, float* row_ws_d, const float* state_d, void* stream);
int urso_rel_l2_fwd_bwd_ls(int B, int D, int ld, const float* gt_d, const float* pred_d, float weight,
                           int dt, float* loss_d, void* dpred_d, float* norms_d, const float* state_d, void* stream);
int urso_absdot_fwd_bwd_ls(int B, int D, int ld, int normalize, const float* gt_d, const float* x_d,
                           float weight, int dt, float* q_d, float* loss_d, void* dx_d, const float* state_d, void* stream);
int urso_mse_fwd_bwd_ls(int B, int D, int ld, const float* gt_d, const float* pred_d, float weight,
                        int dt, float* loss_d, void* dpred_d, const float* state_d, void* stream);
int urso_param_batch_run_ls(int phase, int dt, const urso_param_desc* descs_d, const int32_t* blockmap_d, int nblocks, float* sqpart_d,
                            const float* state_d, void* stream);
int urso_param_grad_finalize_ls(int K, int N, int ldn, const float* dw_raw_d, const float* colsum_d,
                                const float* w_d, const float* b_d, const float* gamma_d, const float* mean_d,
                                const float* var_d, float eps, float weight_decay, int trainable, int bn_trainable,
                                float* gw_d, float* gb_d, float* ggamma_d, float* gbeta_d,
                                float* ws_d, size_t ws_bytes, float* sqpart_d, const float* state_d, void* stream);
int urso_bn_backward_ls(int M, int N, int dt, const void* g_d, const void* z_d, const float* mean_d, const float* var_d,
                        const float* gamma_d, float eps, void* ws_d, size_t ws_bytes, float* dbeta_d, float* dgamma_d,
                        int bn_trainable, float* gbeta_d, float* ggamma_d, void* dz_d, const float* state_d, void* stream);
int urso_sgd_momentum_clip_ls(size_t n, float* w_d, const float* g_d, float* v_d,
                              const float* hyper_d, const float* normsq_d, const float* state_d, void* stream);
int urso_adam_amsgrad_clip_ls(size_t n, float* w_d, const float* g_d, float* m_d, float* v_d, float* vhat_d,
                              float* hyper_d, const float* normsq_d, const float* state_d, void* stream);
int urso_loss_scale_update(float* state_d, const float* normsq_d, void* stream);

#ifdef __cplusplus
}
#endif

#endif
