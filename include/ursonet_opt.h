/* C ABI of liburso_opt.so, the optimizer library (gfx950): entry points added after the surfaces of liburso_hip.so (ursonet_hip.h) and
 * liburso_ext.so (ursonet_ext.h) were frozen.  It is loaded behind the main library, whose error text (urso_last_error) and launch
 * profiler it uses; it shares the block map of urso_lars_blocks / urso_lars_plan (ursonet_ext.h) but calls nothing of liburso_ext.so.
 * Plain C99.  Every function returns URSO_OK or a negative URSO_E* code; the text of the last error is urso_last_error()'s.
 */
#ifndef URSONET_OPT_H
#define URSONET_OPT_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_ext.h"     /* URSO_LARS_CHUNK and the block map's host functions; URSO_OK / URSO_E* through ursonet_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * LAMB: layer-wise trust ratios for Adam(amsgrad) with global-norm clip (Config.LAMB; ursonet_amd/lamb.py is the
 * same rule in NumPy and the written specification).  Three launches that stand where the plain Adam launch stands.
 *
 * hyper_d   float [8] = {lr, b1, b2, eps, clip, t, c1, c2}: the layout of the plain Adam launch; the tick advances t
 * state_d   float [URSO_LAMB_STATE] = {p1, p2, kt}: the running products b1^t and b2^t and kt = sqrtf(1 - p2) / (1 - p1), {1, 1, 0}
 *           before the first step.  Products, not powf: * - / and sqrtf are rounded correctly and so have a bit-exact host counterpart
 * normsq_d  float [1]: the squared global norm of g
 * tab_d, blockmap_d, first_d, adapt_d, off_h, n_h, nblocks: the tables of urso_lars_norms / _trust / _sgd, as urso_lars_plan filled them
 *
 * Every float32 operation is rounded once (-ffp-contract=off).  With c the clip factor of the plain launches:
 *
 *   tick (one thread, a launch of its own in front):  t = t + 1;  p1 = p1 * b1;  p2 = p2 * b2;  kt = sqrtf(1 - p2) / (1 - p1)
 *   per element:  gi = g * c;  m = b1 * m + c1 * gi;  v = b2 * v + c2 * (gi * gi);  vhat = max(vhat, v)
 *                 r = (kt * m) / (sqrtf(vhat) + eps)
 *   per tensor, float64:  nw = sqrt(sum w^2), nr = sqrt(sum r^2) from float32 slots in the order of urso_lars_norms, w before the step
 *                 q = 1 if the tensor does not adapt or nw == 0 or nr == 0, else eta * nw / (nr + eps_trust);  q = min(q, 1) with clip_mode
 *                 trust = (float)q
 *   per element:  w = w - (lr * trust) * r,  r recomputed from the stored m and vhat by the same statements
 *
 *   urso_lamb_moments  the tick, then NB blocks of 256 threads: reads w, g, m, v, vhat (16 bytes per lane and access, a tensor's last
 *                      n % 4 elements by scalars), writes m, v, vhat and part_d[NB][2] = {sum w^2, sum r^2}: 32 bytes per parameter
 *   urso_lamb_trust    T blocks of two waves: trust_d[T] and stat_d[T][3] = (nw, nr, q), float64
 *   urso_lamb_apply    NB blocks over the same map: reads w, m, vhat and trust_d[tensor], writes w: 16 bytes per parameter
 *
 * ls_state_d: NULL, or the loss-scale state (ursonet_loss_scale.h), which marks the launch as part of a scaled step: a step whose
 * normsq is not finite then changes nothing -- w, m, v, vhat, t, the state, the slots, trust and stat keep their bits.
 * T == 0 or nblocks == 0 launches nothing.  Nothing outside a tensor's [offset, offset + n) is read or written.
 * URSO_EINVAL: a null pointer; w, g, m, v, vhat not 16-byte aligned or not pairwise distinct; tab, part or stat not 8-byte aligned; any
 * other pointer not 4-byte aligned; an offset that is not a non-negative multiple of 4; a negative size; overlapping tensors;
 * nblocks != urso_lars_blocks(T, n_h); eta not a finite number > 0, eps not a finite number >= 0, clip_mode not 0 or 1.
 */
#define URSO_LAMB_STATE 3
int urso_lamb_moments(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                      const float* w_d, const float* g_d, float* m_d, float* v_d, float* vhat_d, float* hyper_d, float* state_d,
                      const float* normsq_d, float* part_d, const float* ls_state_d, void* stream);
int urso_lamb_trust(int T, const int32_t* first_d, const int32_t* adapt_d, int nblocks, const float* part_d, const float* normsq_d,
                    double eta, double eps, int clip_mode, float* trust_d, double* stat_d, const float* ls_state_d, void* stream);
int urso_lamb_apply(int T, const int64_t* off_h, const int64_t* n_h, const int64_t* tab_d, const int32_t* blockmap_d, int nblocks,
                    float* w_d, const float* m_d, const float* vhat_d, const float* trust_d, const float* hyper_d, const float* state_d,
                    const float* normsq_d, const float* ls_state_d, void* stream);

#ifdef __cplusplus
}
#endif

#endif
