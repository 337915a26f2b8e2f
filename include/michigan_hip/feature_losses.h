/* michigan_hip/feature_losses.h -- part of the C ABI of libmichigan_hip (michigan_hip.h includes it): the style and content terms of the generator objective as
 * fused VGG feature-moment kernels (mg_feat_moments.hip).  Reference: StyleContentLoss, models/networks/loss.py:624-711, called at
 * models/pix2pix_model.py:309-319.
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind mg_last_error(); arguments are
 * validated before the device is touched; all work is enqueued on `stream` (a hipStream_t) and nothing synchronises. */
#ifndef MICHIGAN_HIP_FEATURE_LOSSES_H
#define MICHIGAN_HIP_FEATURE_LOSSES_H

#include "../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MG_FEAT_STYLE   1                  /* `flags` bit 0 */
#define MG_FEAT_CONTENT 2                  /* `flags` bit 1 */

/* One VGG tap.  x (fake features, gets the gradient), s (style features), t (content features): NHWC [N][P][C] in `dtype` (MG_F32 /
 * MG_BF16), 16-byte aligned, as VGG19.forward produces them before the NCHW view.  A lane owns 16 bytes of channels: C % 8 == 0 for
 * bf16, C % 4 == 0 for fp32.  mask_x, mask_s, mask_t (l below): fp32 planes [P] per sample at the FEATURE's resolution, at a sample
 * stride >= P; a NULL mask is the unmasked form (mask_x and mask_s are given together or not at all).
 *
 * Unmasked moments per (n, c) (calc_mean_std, loss.py:624-632; torch.var is unbiased), P >= 2:
 *   mu = sum_p x / P,   sigma = sqrt(sum_p (x - mu)^2 / (P - 1) + 1e-5)
 * Masked moments under m (calc_mean_std_mask, loss.py:634-654; the mask VALUE multiplies, exactly as written there):
 *   S = sum_p m + 1e-5,   mu = sum_p m x / S,   r_p = (m_p x_p - mu) m_p,   sigma = sqrt(sum_p r_p^2 / S + 1e-5)
 *   (an empty mask gives mu = 0, sigma = sqrt(1e-5), no NaN)
 * bit 0  out[0] = style   = (1 / (N C)) sum_{n,c} [(mu_x - mu_s)^2 + (sigma_x - sigma_s)^2], x under mask_x and s under mask_s
 *                           (calc_style_loss, loss.py:679-694: two nn.MSELoss over [N, C, 1, 1])
 * bit 1  out[1] = content = mean (x - t)^2 over N P C unmasked (loss.py:667-668), or, under l = mask_t,
 *                           sum (l (x - t))^2 / (C sum_{n,p} l + 1e-5) (loss.py:669-677)
 * out: 2 floats, 0 for a term not selected; a term not selected costs nothing, reads nothing and its operands may be NULL.
 * coef: 4 N C floats, 16-byte aligned: {a, b, mu_x, 2 / den} of (n, c) -- what the backward reads; it reduces nothing.  With
 *   gm = 2 (mu_x - mu_s) / (N C), gs = 2 (sigma_x - sigma_s) / (N C), T = sum_p r_p m_p:
 *   a = gm / S - gs T / (sigma_x S^2), b = gs / (sigma_x S);  unmasked a = gm / P, b = gs / (sigma_x (P - 1));
 *   den = N P C unmasked, C sum_{n,p} l + 1e-5 masked.
 * ws: mg_feat_moment_workspace(N, P, C) bytes, 16-byte aligned, contents undefined on entry.
 *
 * fwd, two launches.  Launch 1 reads x, s and (bit 1) t once each: a workgroup owns a pixel chunk of one sample and writes fp32 chunk
 * partials taken about a per-(chunk, n, c) pivot (the chunk's first pixel with a non-zero mask), the mask power sums in double.
 * Launch 2 un-shifts and sums the partials in a fixed order in fp64, writes coef and both outputs.  No float atomics: loss and gradient
 * are bit-reproducible and do not depend on which other bit is set.  Features at pixels whose mask is 0 are NOT read (x where
 * mask_x == 0 and, with bit 1, l == 0; s where mask_s == 0; t where l == 0): a NaN there reaches no result.
 * bwd, one launch, dx in the feature's dtype and layout (every element written):
 *   dx = g_style[0] (m a + m^3 b (m x - mu_x)) + g_content[0] 2 l^2 (x - t) / den        (unmasked: m = l = 1)
 * exactly 0 where both masks are 0.  g_*: device scalars, a NULL pointer = 0.  s, t and the masks get no gradient.
 * N <= 65535, P < 2^31. */
typedef struct mg_feat_moment_desc {
    const void* x;
    const void* s;
    const void* t;
    const float* mask_x;
    const float* mask_s;
    const float* mask_t;
    int64_t mask_x_nstride, mask_s_nstride, mask_t_nstride;
    int64_t P;
    int32_t dtype, N, C, flags;
    float* out;
    float* coef;
    void* ws;
} mg_feat_moment_desc;

/* bytes of `ws` for either dtype; 0 for a geometry the entry points refuse */
int64_t mg_feat_moment_workspace(int32_t N, int64_t P, int32_t C);
int mg_feat_moment_loss_fwd(const mg_feat_moment_desc* d, void* stream);
int mg_feat_moment_loss_bwd(const mg_feat_moment_desc* d, const float* g_style, const float* g_content, void* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
