/* C ABI of liburso_feat.so, the feature library (gfx950): feature-space statistics of the bottleneck features, for fit_domain(),
 * predict / evaluate with domain=... and domain_gap() (ursonet_amd/domain.py).  The surface of liburso_infer.so
 * (ursonet_infer.h) is pinned to conformal's two names, so these three have a library of their own.  It is loaded behind the main library,
 * whose error text (urso_last_error) and launch profiler it uses; it calls nothing of the other four.
 * Plain C99.  Every function returns URSO_OK or a negative URSO_E* code; the text of the last error is urso_last_error()'s.
 */
#ifndef URSONET_FEAT_H
#define URSONET_FEAT_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_hip.h"     /* URSO_OK / URSO_E*, URSO_F32 / URSO_BF16 / URSO_F16 */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * ursonet_amd/domain.py -- pool64 / gram_add64 / maha64 -- is the same rule in NumPy float64 and the written specification; the kernels
 * equal it bit for bit (no transcendental function is involved, the library is built with -ffp-contract=off, and every sum below has one
 * stated order).  All tables are fp64.
 *
 * Features.  act is the bottleneck_layer output [B][h][w][C] in the engine's dtype; grid (gh, gw) divides (h, w); D = gh * gw * C,
 * 1 <= D <= URSO_FEAT_MAX_D.  Feature ((gy * gw) + gx) * C + c is the fp64 mean of channel c over the cell (gy, gx) of (h / gh) x (w / gw)
 * pixels: the sum starts at +0.0 and runs over the cell's pixels in row-major ascending order in fp64 (the conversion from bf16 / fp16 /
 * fp32 is exact), then one IEEE division by the pixel count.  Non-finite values pass through.
 *
 * urso_feat_pool, for every valid batch row b < n: out[(row0 + b) * ld + f] = feature f of act[b], f < D.  Batch rows >= n are not read,
 * columns >= D and other rows are not written.  Launch shape: one thread per (b, cell, c), c fastest, so a wave reads 64 consecutive
 * channels of one pixel; each thread walks its cell's pixels.
 *
 * urso_feat_gram_add, for the valid rows r = 0 .. n - 1 ascending, x_r = x + (row0 + r) * ld_x, with the centre c [D]:
 *   d = x_r - c                                  (one rounding per component)
 *   s_i = s_i + d_i                              (i < D)
 *   G_ij = G_ij + d_i * d_j   for j >= i         (the product is rounded, then the sum is rounded; G at g + i * ld_g + j)
 * which is the NumPy statement `for r: d = X[r] - c; s += d; G += triu(outer(d, d))`, bit for bit, across any number of calls.  Only the
 * upper triangle of G including the diagonal is read or written: neither the strict lower triangle nor the padding (columns >= D) is read
 * or written.  NaN propagates.  Launch shape: one workgroup of 256 threads per 32 x 32 tile of the upper triangle (T (T + 1) / 2 workgroups,
 * T = ceil(D / 32)); a thread keeps a 2 x 2 register tile of G; the batch's d rows of the tile's 32 rows and 32 columns are staged in LDS 32
 * batch rows at a time (16 KiB) and every thread runs over them in ascending order, so each element of G and s is read once and written
 * once per call.  The pass is bound by streaming the accumulator: 8 D (D + 1) bytes per call (4 D (D + 1) read, as many written), beside
 * 8 n D bytes of x per tile row and column.  The workgroups of the diagonal tiles add s.
 *
 * urso_feat_maha, for every valid batch row b < n: x = x + b * ld_x (the batch's feature rows, [B][ld_x]), mean [D], and W lower
 * triangular, stored TRANSPOSED for coalesced reads: W_ij at wt + j * ld_w + i (j <= i); entries above the diagonal (j > i) are never read:
 *   d = x - mean
 *   y_i = sum_{j = 0 .. i} W_ij d_j               (j ascending from +0.0; each term is acc = acc + W_ij * d_j: two roundings)
 *   out[row0 + b] = { SCORE = sum_i y_i y_i, DIST2 = sum_i d_i d_i  (both i ascending from +0.0, product rounded, then the sum),
 *                     ZMAX = max_i |y_i|, ZARG = the lowest index that attains it (a NaN counts as the largest; the first one wins) }
 * A row of x with a component that is not finite gets NaN in all four columns; no other row is touched.  Launch shape: one workgroup of 256
 * threads per URSO_FEAT_MAHA_ROWS = 8 batch rows; the workgroup walks i in tiles of 256 (one i per thread) and, inside, j in tiles of 64 whose
 * d values of the 8 rows sit in LDS, so one load of a W element serves 8 rows and W is read ceil(n / 8) times per launch, not n times
 * (4 D (D + 1) bytes each time); a thread's loads of W run 16 elements ahead of their terms; behind every i tile one thread per row adds
 * the tile's y_i^2 and another its d_i^2 from LDS in ascending order.
 *
 * None of the three uses a workspace, allocates or synchronises the host; n == 0 launches nothing.  URSO_EINVAL, with a message, before
 * any launch: a null struct or pointer; n outside [0, B]; row0 < 0; h, w, C < 1; a grid that does not divide (h, w); D outside
 * [1, URSO_FEAT_MAX_D]; an unknown dtype; ld, ld_x < D, ld_g < D, ld_w < D; act off its element's boundary, any fp64 pointer off the 8-byte
 * boundary.
 */
#define URSO_FEAT_MAX_D 4096
#define URSO_FEAT_COLS 4
#define URSO_FEAT_MAHA_ROWS 8
#define URSO_FEAT_SCORE 0
#define URSO_FEAT_DIST2 1
#define URSO_FEAT_ZMAX 2
#define URSO_FEAT_ZARG 3
typedef struct urso_feat_pool_args {
    int32_t B, n;                    /* rows of the batch, valid rows */
    int64_t row0;                    /* first row of out */
    int32_t h, w, C, gh, gw, dtype;  /* dtype: URSO_F32 / URSO_BF16 / URSO_F16 */
    int64_t ld;                      /* doubles between rows of out, >= D */
    const void* act;                 /* [B][h][w][C] */
    double* out;                     /* [rows][ld] */
} urso_feat_pool_args;
typedef struct urso_feat_gram_args {
    int32_t B, n;
    int64_t row0;                    /* first row of x */
    int32_t D, pad;
    int64_t ld_x, ld_g;
    const double* x;                 /* [rows][ld_x] */
    const double* centre;            /* [D] */
    double* s;                       /* [D] */
    double* g;                       /* [D][ld_g], the upper triangle */
} urso_feat_gram_args;
typedef struct urso_feat_maha_args {
    int32_t B, n;
    int64_t row0;                    /* first row of out */
    int32_t D, pad;
    int64_t ld_x, ld_w;
    const double* x;                 /* [B][ld_x] */
    const double* mean;              /* [D] */
    const double* wt;                /* W transposed: W_ij at wt[j * ld_w + i], j <= i */
    double* out;                     /* [rows][URSO_FEAT_COLS] */
} urso_feat_maha_args;
int urso_feat_pool(const urso_feat_pool_args* args, void* stream);
int urso_feat_gram_add(const urso_feat_gram_args* args, void* stream);
int urso_feat_maha(const urso_feat_maha_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
