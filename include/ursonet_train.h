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

#ifdef __cplusplus
}
#endif

#endif
