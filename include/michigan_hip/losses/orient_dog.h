/* michigan_hip/losses/orient_dog.h -- the LOSS EXTENSION group of libmichigan_hip (mg_orient_dog.hip): the tail of the orientation
 * loss behind the filter-bank arg-max when the bank is the difference-of-Gaussians bank (--orient_filter dog; reference:
 * models/networks/loss.py:320-349 and the DoG branch of 352-385).  The filter launch itself is the existing arg-max entry point of
 * michigan_hip.h, which takes any 32 x 17 x 17 bank.
 *
 * The group carries the prefix mgl_ and is NOT part of the versioned symbol table of michigan_hip.h: MG_ABI_VERSION does not count
 * it, michigan_amd/_cabi.py binds it in a table of its own (_LOSS_PROTOS), and the contract emulator under oracle/ does not know it
 * (tests/orient_dog_fixtures.py carries the float64 contract and an emulator subclass).
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind mg_last_error; arguments are
 * validated before the device is touched; all work is enqueued on `stream` (a hipStream_t), nothing synchronises and nothing is read
 * back. */
#ifndef MICHIGAN_HIP_LOSSES_ORIENT_DOG_H
#define MICHIGAN_HIP_LOSSES_ORIENT_DOG_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGL_ORIENT_DOG_BLOCKS 1024         /* at most this many workgroups; the row stride of the workspace */
#define MGL_ORIENT_DOG_WS_ROWS 7           /* ws: float [7][1024] = block maxima, then the six partial-sum rows */
#define MGL_ORIENT_DOG_OUT 8               /* out: float [8], see below */

/* Forward.  conf_raw float [N][HW]: R, the clamped maximum response (>= 0); idx u8 [N][HW]: its arg-max, the angle is a = idx pi / 32;
 * label float, label_ch planes of HW per sample, samples label_nstride elements apart: 2 planes = (sin 2t, cos 2t), 1 plane = the
 * 0..255 angle map v, read as t = v / 255 pi; hair float [N][HW] with samples hair_nstride elements apart (plane 1 of the one-hot
 * label, no copy): m.
 *   c1 = R m,   M = max of c1 over ALL N HW pixels (the batch, not the sample),   q = c1 / M,   c = q <= 0 ? 0 : q
 *   out[0] orient      = sum(|sin 2a c m - l0 m| + |cos 2a c m - l1 m|) / (2 N HW)
 *   out[1] confidence  = sum |c m - m| / (sum m + 1e-5)
 *   out[2] sum m       out[3] M       out[4] the number of pixels with c1 == M
 *   out[5] A = sum (sign(d0) sin 2a + sign(d1) cos 2a) m c1,  d0, d1 the two differences of out[0]
 *   out[6] B = sum sign(c m - m) m c1                          out[7] 0
 * q is one IEEE division, so c == 1 exactly where c1 == M and c < 1 elsewhere.  M == 0 (no hair pixel with a positive response in
 * the whole batch) makes q = 0 / 0: out[0], out[1], out[5] and out[6] are NaN then, as in the reference.  A NaN in c1 is not a maximum.
 * out[2..6] are what the backward needs: the incoming gradients are not known in the forward.
 * Three launches: workgroup maxima into ws row 0 (a float maximum is order-free); a partial pass in which every workgroup first joins
 * the maxima to M and then leaves six fp32 sums in ws rows 1..6 (a thread's own strided sum from +0, the wave tree, the four waves left
 * to right); one workgroup that adds each row in double (thread t takes blocks t, t + 256, .. ascending, then a halving tree).  No
 * atomics: two runs are bit-identical.  ws holds MGL_ORIENT_DOG_WS_ROWS * MGL_ORIENT_DOG_BLOCKS floats, out MGL_ORIENT_DOG_OUT.
 * label_ch 1 or 2, N >= 1, 1 <= HW < 2^31; for N > 1 the sample strides are at least label_ch HW and HW. */
int mgl_orient_dog_fwd(const float* conf_raw, const uint8_t* idx, const float* label, int32_t label_ch, int64_t label_nstride,
                       const float* hair, int64_t hair_nstride, int32_t N, int64_t HW, float* out, float* ws, void* stream);

/* Backward to R.  g_orient, g_conf: one float each on the device, the gradients of out[0] and out[1]; either may be NULL (= 0).
 * fwd_out: the forward's out.  With g_o = g_orient / (2 N HW) and g_c = g_conf / (out[2] + 1e-5):
 *   dL/dc_i    = g_o (sign(d0) sin 2a + sign(d1) cos 2a) m_i + g_c sign(c_i m_i - m_i) m_i              (sign(0) = 0)
 *   dconf_i    = (c_i > 0 ? dL/dc_i m_i / M : 0) + (c1_i == M ? -((g_o A + g_c B) / M^2) / out[4] m_i : 0)
 * The second term is the path through the maximum, split evenly among ties (torch.max's backward).  Evaluated per pixel in double
 * in the order written and rounded to float once.  The clamp of R at 0 is the caller's.  One launch. */
int mgl_orient_dog_bwd(const float* conf_raw, const uint8_t* idx, const float* label, int32_t label_ch, int64_t label_nstride,
                       const float* hair, int64_t hair_nstride, const float* g_orient, const float* g_conf, const float* fwd_out,
                       int32_t N, int64_t HW, float* dconf, void* stream);

#ifdef __cplusplus
}
#endif
#endif
