/* michigan_hip/editing/stroke_orient.h -- part of the C ABI of libmichigan_hip (michigan_hip.h includes it): the stroke route of the interactive demo (mg_stroke.hip).
 * Reference: ui_util/cal_orient_stroke.py:85-121, 133-149 (orient.stroke_to_orient: the drawn stroke mask under the 32
 * difference-of-Gaussians filters, first arg-max, the RGB-coded orientation picture) and models/pix2pix_model.py:431-464
 * (inpainting_stroke_orient: the input of the frozen stroke in-painting net and what is made of its output).
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind mg_last_error(); arguments are
 * validated before the device is touched; all work is enqueued on `stream` (a hipStream_t) and nothing synchronises. */
#ifndef MICHIGAN_HIP_EDITING_STROKE_ORIENT_H
#define MICHIGAN_HIP_EDITING_STROKE_ORIENT_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MG_STROKE_FILTERS 32               /* bank [32][17][17], rgb_table [32][3] */
#define MG_STROKE_RADIUS 8                 /* a filter is bank[k][-8 .. 8][-8 .. 8] */
#define MG_STROKE_TILE_H 16                /* output pixels one workgroup owns; a tile without a stroke pixel is not filtered */
#define MG_STROKE_TILE_W 16                /* (tests sit on these edges) */

/* stroke [n][h][w] u8 (non-zero = stroke), bank fp32 [32][17][17] (ops.dog_bank), rgb_table u8 [32][3] from the host
 * (ops.stroke_rgb_table: the kernel evaluates no sin or cos).  In float64, with s = stroke != 0:
 *   resp_k[y,x] = sum_ij bank[k][i][j] s[y+i-8, x+j-8]      (correlation; s is 0 outside the image)
 *   conf        = max_k max(resp_k, 0),   idx = the first k that attains conf (0 when every response is <= 0)
 *   where s:      rgb_u8 = rgb_table[idx]
 *   where not s:  rgb_u8 = (0, 0, 0), idx = 0, conf = 0
 * rgb_u8 [n][h][w][3] u8; idx [n][h][w] u8 and conf [n][h][w] fp32 may each be NULL (not written).  The sums are accumulated in fp32
 * in a fixed order (s is 0 or 1, so every product is exact).  One launch, no intermediate in device memory, no atomics: two runs
 * are bit-identical.  Any h, w >= 1; n h w < 2^31. */
int mg_stroke_orient(const uint8_t* stroke, const float* bank, const uint8_t* rgb_table, uint8_t* rgb_u8, uint8_t* idx, float* conf,
                     int32_t n, int32_t h, int32_t w, void* stream);

/* The in-painting net's input, assembled in its own layout (pix2pix_model.py:443-447; 408-411 without strokes).
 * orient_rgb, noise, stroke fp32 [n][3][h][w]; hole, stroke_mask fp32 [n][1][h][w]; stroke and stroke_mask are given together or are
 * both NULL.  ytab int32 [ho], xtab int32 [wo]: the source row / column of each output row / column (ops.interp_nearest_table;
 * NULL = identity, which needs ho == h / wo == w).  inp [n][ho][wo][8] in dtype (MG_F32 / MG_BF16), at p = (ytab[y], xtab[x]):
 *   channels 0-2 = orient_rgb (1 - hole) + noise (hole - stroke_mask) + stroke stroke_mask      (with strokes)
 *                = orient_rgb (1 - hole) + noise hole                                             (without)
 *   channel  3   = hole,   channel 4 = stroke_mask (0 without strokes),   channels 5-7 = 0
 * evaluated in fp32 operation by operation, left to right as written, nothing contracted into a fused multiply-add, and rounded
 * once to dtype. */
int mg_stroke_compose(const float* orient_rgb, const float* noise, const float* hole, const float* stroke, const float* stroke_mask,
                      const int32_t* ytab, const int32_t* xtab, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ho, int32_t wo,
                      void* inp, void* stream);

/* What becomes of the net's output (pix2pix_model.py:450-463).  net_out fp32 [n][3][ho][wo]; ytab int32 [h], xtab int32 [w]: the row /
 * column of net_out each output row / column reads (NULL = identity); hole, mask fp32 [n][1][h][w]; orient_rgb fp32 [n][3][h][w].
 *   out_rgb [n][3][h][w] fp32 = net_out[ytab[y], xtab[x]] hole + orient_rgb (1 - hole)
 *   orient2 [n][2][h][w] fp32 = ((out_rgb[1] - 0.5) 2 mask, (out_rgb[0] - 0.5) 2 mask)
 * in fp32 operation by operation, as mg_stroke_compose. */
int mg_inpaint_finish(const float* net_out, const int32_t* ytab, const int32_t* xtab, const float* hole, const float* orient_rgb,
                      const float* mask, int32_t n, int32_t h, int32_t w, int32_t ho, int32_t wo, float* out_rgb, float* orient2,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
