/* michigan_hip/preprocess/dense_orient.h -- part of the C ABI of libmichigan_hip (michigan_hip.h includes it): the second half of dense hair-orientation
 * extraction (mg_orient_smooth.hip).  Reference: cal_orientation.py:101-109 -- the flow field of the arg-max orientation, two
 * cv2.GaussianBlur(sigma 4) calls, atan2 and the quantisation to the uint8 map the data set stores.  The first half (gray image,
 * 32 difference-of-Gaussians filters, first arg-max; cal_orientation.py:60-80) is mg_gabor_argmax_fwd of michigan_hip.h with the bank
 * of ops.dog_bank().
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind mg_last_error(); arguments are
 * validated before the device is touched; all work is enqueued on `stream` (a hipStream_t) and nothing synchronises. */
#ifndef MICHIGAN_HIP_PREPROCESS_DENSE_ORIENT_H
#define MICHIGAN_HIP_PREPROCESS_DENSE_ORIENT_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MG_ORIENT_RADIUS 16                /* taps[33] = taps[-16 .. 16] */
#define MG_ORIENT_TILE_H 32                /* output pixels one workgroup owns (tests sit on these edges) */
#define MG_ORIENT_TILE_W 32

/* conf [n][h][w] fp32 and idx [n][h][w] u8 (< 32; the low five bits are used) as mg_gabor_argmax_fwd wrote them, mask [n][h][w] u8.
 * trig: 32 x {cos, sin} of the angle an index stands for; taps: 33 weights of the separable smoothing window.  Both tables come from
 * the host (ops.orient_trig_table, ops.gaussian_taps): the kernel evaluates no sin, cos or exp.
 * With refl = reflect-101 (-i -> i, h-1+i -> h-1-i), in float64, rounded once at the outputs:
 *   m[p]    = mask[p] != 0
 *   fx[p]   = m[p] ? trig[idx[p]][0] conf[p] : 0,   fy[p] = m[p] ? trig[idx[p]][1] conf[p] : 0     (conf is not read as a number where m = 0)
 *   bx[y,x] = sum_j taps[j+16] sum_i taps[i+16] fx[refl(y+j), refl(x+i)],   by likewise
 *   theta   = 0.5 atan2(by, bx), + pi where that is negative
 *   angle     [n][h][w] fp32 = theta                                    (NULL: not written)
 *   orient_u8 [n][h][w] u8   = trunc(min(theta 255 / pi m, 255))
 * h, w >= 17: one reflection reaches every tap.  One launch, no intermediate in device memory, no atomics: two runs are
 * bit-identical.  n h w < 2^31. */
int mg_orient_smooth(const float* conf, const uint8_t* idx, const uint8_t* mask, const float* trig, const float* taps,
                     uint8_t* orient_u8, float* angle, int32_t n, int32_t h, int32_t w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
