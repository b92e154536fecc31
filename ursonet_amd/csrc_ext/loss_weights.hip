// Learnable loss weights (liburso_ext.so; Config.LEARNABLE_LOSS_WEIGHTS): the three loss entry points whose weight is
// w * exp(-s) with s a trainable fp32 scalar in device memory.  The kernels are the main library's own (csrc/loss_dev.h): with s they
// replace the weight by that one product, report P + w s and overwrite ds = w - P.  Math and argument rules: include/ursonet_ext.h.
#include "../csrc/loss_dev.h"
#include "../../include/ursonet_ext.h"

extern "C" int urso_softmax_xent_fwd_bwd_lw(int B, int K, const float* logits_d, const float* labels_d, float weight, int relu_mask, int dt,
                                            float* loss_d, void* dz_d, float* row_ws_d, const float* s_d, float* ds_d, const float* ls_state_d,
                                            void* stream) {
    if (!logits_d || !labels_d || !loss_d || !dz_d || !row_ws_d || !s_d || B <= 0 || K <= 0) { urso_set_error("urso_softmax_xent_fwd_bwd_lw: bad argument"); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_LOSS, 0, (double)B * K * (8 + dt_size(dt)));
    softmax_xent_launch(st, B, K, logits_d, labels_d, weight, relu_mask, dt, loss_d, dz_d, row_ws_d, ls_state_d, LossLw{s_d, ds_d, weight});
    return urso_check_launch("urso_softmax_xent_fwd_bwd_lw");
}

extern "C" int urso_rel_l2_fwd_bwd_lw(int B, int D, int ld, const float* gt_d, const float* pred_d, float weight, int dt, float* loss_d,
                                      void* dpred_d, float* norms_d, const float* s_d, float* ds_d, const float* ls_state_d, void* stream) {
    if (!gt_d || !pred_d || !loss_d || !dpred_d || !s_d || B <= 0 || D <= 0 || ld < D) { urso_set_error("urso_rel_l2_fwd_bwd_lw: bad argument"); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_LOSS, 0, 0);
    URSO_KLAUNCH(rel_l2_kernel, dim3(1), dim3(256), 0, st, B, D, ld, gt_d, pred_d, weight, dt, loss_d, dpred_d, norms_d, ls_state_d, LossLw{s_d, ds_d, weight});
    return urso_check_launch("urso_rel_l2_fwd_bwd_lw");
}

extern "C" int urso_absdot_fwd_bwd_lw(int B, int D, int ld, int normalize, const float* gt_d, const float* x_d, float weight, int dt, float* q_d,
                                      float* loss_d, void* dx_d, const float* s_d, float* ds_d, const float* ls_state_d, void* stream) {
    if (!gt_d || !x_d || !loss_d || !dx_d || !s_d || B <= 0 || D <= 0 || ld < D) { urso_set_error("urso_absdot_fwd_bwd_lw: bad argument"); return URSO_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, URSO_K_LOSS, 0, 0);
    URSO_KLAUNCH(absdot_kernel, dim3(1), dim3(256), 0, st, B, D, ld, normalize, gt_d, x_d, weight, dt, q_d, loss_d, dx_d, ls_state_d, LossLw{s_d, ds_d, weight});
    return urso_check_launch("urso_absdot_fwd_bwd_lw");
}
