/* C ABI of liburso_explain.so, the explanation library (gfx950): occlusion-sensitivity maps of the pose heads, for explain()
 * (ursonet_amd/explain.py).  The surfaces of the other six libraries are pinned or belong to other subjects, so these
 * four have a library of their own.  It is loaded behind the main library, whose error text (urso_last_error) and launch profiler it
 * uses; it calls nothing of the other five.
 * Plain C99.  Every function returns URSO_OK or a negative URSO_E* code; the text of the last error is urso_last_error()'s.
 */
#ifndef URSONET_EXPLAIN_H
#define URSONET_EXPLAIN_H

#include <stddef.h>
#include <stdint.h>
#include "ursonet_hip.h"     /* URSO_OK / URSO_E*, URSO_DEC_* */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * ursonet_amd/explain.py -- occlude_host / score64 / splat64 / overlay_host -- is the same rule in NumPy and the written specification.
 * All four run on the given stream, use no workspace, allocate nothing and never synchronise the host.  The library is built with
 * -ffp-contract=off: every fp64 operation below is rounded once.  A rect is four int32 (y0, x0, y1, x1), half open, in pixels of the frame.
 *
 * urso_occl_fill_u8.  src is one uint8 frame [H][W][C], C in 1 .. 4; out is a batch [B][H][W][C]; rects is [n][4] on the device.  Row
 * j < n of out becomes src with the pixels of rect j -- clamped to the frame: y0, x0 raised to 0, y1 lowered to H, x1 to W -- replaced by
 * fill[0 .. C - 1]; a rect with y1 <= y0 or x1 <= x0 (before or behind the clamp) gives a plain copy.  Rows >= n are not touched.  src must
 * not overlap out.  Launch shape: a grid over (chunk, row) of 256 threads; a row is a flat array of H W C bytes that is copied as
 * urso_frames_gather_u8 copies a frame -- a bytewise head up to the first 16-byte boundary of the destination, a body of aligned 16-byte
 * stores (the loads are aligned where source and destination agree mod 16, alignment-1 accesses elsewhere), a bytewise tail, 12 vectors
 * per thread in flight -- and a vector some byte of which lies in the rect has those bytes replaced between its load and its store.
 * It is byte for byte explain.occlude_host(frame, rects, fill).
 *
 * urso_occl_score.  One workgroup of 1024 threads per valid batch row b < n compares table row r = row0 + b with the baseline and
 * writes out[r][0 .. URSO_OCCL_COLS).  dec0 points at the baseline's row of a DEC table (URSO_DEC_COLS doubles, as urso_pose_decode wrote
 * them), dec at a DEC table whose row r is the batch row's.  All arithmetic is fp64:
 *   D_ORI  = (2 acos(min(1, |q0 . q|))) * 180 / pi, the dot product summed x, y, z, w in that order (ev_angle of csrc/pose_dev.h, the
 *            convention urso_pose_eval scores with); q0, q the two Q_EST
 *   D_LOC  = sqrt(dx dx + dy dy + dz dz), d = LOC_EST - LOC_EST0, summed in that order
 * and, per classification head that is given (ori: columns URSO_OCCL_ORI_KL .., loc: URSO_OCCL_LOC_KL ..; K >= 1 with both pointers
 * gives the head, K == 0 leaves it out and its four columns keep what they held), with z0 fp32 [K] the baseline's logits and z fp32
 * [B][ld] the batch's (row b), m = the row's maximum, d_k = (double)z_k - m, e_k = exp(d_k), Z = sum_k e_k, p_k = e_k / Z,
 * lp_k = d_k - log(Z) (each for z0 and for z):
 *   KL     = sum_k t_k,  t_k = 0 where p0_k == 0, +inf where p0_k > 0 and p_k == 0, else p0_k * (lp0_k - lp_k)
 *   TV     = 0.5 * sum_k |p0_k - p_k|
 *   DROP   = p0[k0] - p[k0], k0 the first argmax of z0
 *   ARGMAX = the first argmax of z, as a double
 * A NaN in either row makes the head's four columns NaN (so does a row whose maximum is not finite: d is inf - inf).  K = 1 gives
 * 0, 0, 0, 0.  Two identical rows give KL == 0 and TV == 0 exactly: every term is a difference of equal numbers.
 * Order of the sums Z, KL and TV (one order, so a row gives the same bits at any position and in any batch size): columns are dealt to
 * threads in groups of four -- thread t owns the groups t, 1024 + t, 2048 + t, ... and the ragged end K % 4 belongs to the group behind
 * the last whole one -- a thread adds its terms from +0.0 in ascending column order; the 64 lanes of a wave are added by the xor
 * butterfly with offsets 32, 16, 8, 4, 2, 1 (v = v + v[lane ^ o]); the 16 wave sums are added from +0.0 in wave order.  Where a row's
 * first logit sits on a 16-byte boundary a group is one 16-byte load, elsewhere four 4-byte loads: the sums do not depend on it.
 *
 * urso_occl_splat.  scores is fp64 [P][ld]; cols[0 .. M) are the columns used, M in 1 .. URSO_OCCL_MAX_MAPS; rects is [P][4] on the
 * device; the window has its origin at frame pixel (wy0, wx0) and h x w pixels; out is fp64 [M][h][w].  One thread per window pixel
 * (y, x), a gather without atomics: over the patches p = 0 .. P - 1 ascending whose rect holds the frame pixel (wy0 + y, wx0 + x)
 * (y0 <= . < y1 and x0 <= . < x1, the rect as it is: no clamp), s_m = s_m + scores[p][cols[m]] from +0.0 and a count; out[m][y][x] =
 * s_m / count, NaN where the count is 0.  Non-finite scores pass through.  Bit for bit explain.splat64, whatever the grid.
 *
 * urso_heat_overlay_u8.  map is fp64 [h][w]; img is uint8 [h][w][3] with ld_img bytes between rows, modified in place; lut is uint8
 * [256][3]; alpha in 0 .. 256; lo and scale are fp64 (the host computes scale = 255 / (hi - lo)).  Per pixel, v = map[y][x]:
 *   t = (v - lo) * scale (two roundings); a NaN t (so a NaN v) leaves the pixel as it is
 *   idx = min(255, max(0, rint(t)))  (rint: to nearest, ties to even)
 *   px_c = (alpha * lut[idx][c] + (256 - alpha) * px_c + 128) >> 8, c = 0, 1, 2, in integers
 * One thread per pixel.  Byte for byte explain.overlay_host.
 *
 * URSO_EINVAL, with a message, before any HIP call: a null struct or pointer; n outside [0, B]; row0 < 0; H, W < 1; C outside 1 .. 4;
 * H W C at or above 2^31; B above 65535 (fill); src inside out; rects off the 4-byte boundary; a head with K < 0, ld < K, one pointer of the two
 * missing or a pointer off the 4-byte boundary; any fp64 pointer off the 8-byte boundary; P < 0; M outside 1 .. URSO_OCCL_MAX_MAPS; a
 * column outside [0, ld); h, w < 1 (h w at or above 2^31); alpha outside 0 .. 256; ld_img < 3 w; lo or scale not finite.  n == 0
 * launches nothing.
 */
#define URSO_OCCL_COLS 10
#define URSO_OCCL_MAX_MAPS 8
#define URSO_OCCL_D_ORI 0
#define URSO_OCCL_D_LOC 1
#define URSO_OCCL_ORI_KL 2
#define URSO_OCCL_ORI_TV 3
#define URSO_OCCL_ORI_DROP 4
#define URSO_OCCL_ORI_ARGMAX 5
#define URSO_OCCL_LOC_KL 6
#define URSO_OCCL_LOC_TV 7
#define URSO_OCCL_LOC_DROP 8
#define URSO_OCCL_LOC_ARGMAX 9
typedef struct urso_occl_fill_args {
    int32_t B, n;                    /* rows of out, rows to make */
    int32_t H, W, C;
    uint8_t fill[4];                 /* fill[0 .. C) replaces a pixel */
    const uint8_t* src;              /* [H][W][C] */
    const int32_t* rects;            /* [n][4] */
    uint8_t* out;                    /* [B][H][W][C] */
} urso_occl_fill_args;
typedef struct urso_occl_score_args {
    int32_t B, n;                    /* rows of the batch, valid rows */
    int64_t row0;                    /* first row of dec and out */
    int32_t ori_K, ori_ld, loc_K, loc_ld;  /* K == 0: the head is absent */
    const double* dec0;              /* the baseline's DEC row */
    const double* dec;               /* [rows][URSO_DEC_COLS] */
    const float* ori_z0;             /* [ori_K] */
    const float* ori_z;              /* [B][ori_ld] */
    const float* loc_z0;             /* [loc_K] */
    const float* loc_z;              /* [B][loc_ld] */
    double* out;                     /* [rows][URSO_OCCL_COLS] */
} urso_occl_score_args;
typedef struct urso_occl_splat_args {
    int32_t P, M;                    /* patches, maps */
    int32_t wy0, wx0, h, w;          /* the window */
    int32_t cols[URSO_OCCL_MAX_MAPS];
    int64_t ld;                      /* doubles between rows of scores */
    const double* scores;            /* [P][ld] */
    const int32_t* rects;            /* [P][4] */
    double* out;                     /* [M][h][w] */
} urso_occl_splat_args;
typedef struct urso_heat_overlay_args {
    int32_t h, w, alpha, pad;
    int64_t ld_img;                  /* bytes between rows of img, >= 3 w */
    double lo, scale;
    const double* map;               /* [h][w] */
    const uint8_t* lut;              /* [256][3] */
    uint8_t* img;                    /* [h][ld_img] */
} urso_heat_overlay_args;
int urso_occl_fill_u8(const urso_occl_fill_args* args, void* stream);
int urso_occl_score(const urso_occl_score_args* args, void* stream);
int urso_occl_splat(const urso_occl_splat_args* args, void* stream);
int urso_heat_overlay_u8(const urso_heat_overlay_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
