/* michigan_hip/evaluation/quality.h -- the QUALITY EXTENSION group of libmichigan_hip (mg_quality.hip): what an evaluation pass
 * measures on the device.  PSNR and SSIM ingredients of two u8 image batches in one pass, and the agreement of two orientation maps.
 * Neither exists in the reference, which stops at writing pictures.
 *
 * The group carries the prefix mgq_ and is NOT part of the versioned symbol table of michigan_hip.h: MG_ABI_VERSION does not count
 * it, michigan_amd/_cabi.py binds it in a table of its own (_QUALITY_PROTOS), and the contract emulator under oracle/ does not know
 * it (tests/quality_fixtures.py carries the contracts and an emulator subclass).
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind the library's last-error
 * call; arguments are validated before the device is touched; all work is enqueued on `stream` (a hipStream_t) and nothing
 * synchronises.  The workspace query returns bytes and carries no status (0 for a geometry the entry point would refuse). */
#ifndef MICHIGAN_HIP_EVALUATION_QUALITY_H
#define MICHIGAN_HIP_EVALUATION_QUALITY_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGQ_TILE 16                        /* a workgroup owns a 16 x 16 tile of one sample (tests sit on these edges) */
#define MGQ_MIN_K 3                        /* the window has k taps, k odd, MGQ_MIN_K <= k <= MGQ_MAX_K */
#define MGQ_MAX_K 15
#define MGQ_MAX_C 4                        /* 1 <= c <= 4 channels */
#define MGQ_WS_SLOTS 6                     /* 8-byte slots a workgroup leaves per channel in the workspace */
#define MGQ_INT_TERMS 4                    /* out_int  [n][c][4] = {sse, sse_mask, mask_count, valid_mask_count} */
#define MGQ_SSIM_TERMS 2                   /* out_ssim [n][c][2] = {ssim_sum, ssim_sum_mask} */
#define MGQ_ORIENT_PERIOD 255              /* an orientation map codes the angle as v / 255 * pi */

/* PSNR and SSIM ingredients.  a, b u8 [n][h][w][c] (NHWC, dense) on the device; mask u8 [n][h][w] on the device or NULL (non-zero =
 * in; NULL = every pixel in); window k doubles in HOST memory, read before the call returns and passed by value into the launch;
 * ws the workspace, at least the companion query's bytes, 8-byte aligned; out_int uint64 [n][c][4], out_ssim double [n][c][2].
 * Per sample and channel, with r = k / 2 and the VALID region r <= y < h - r, r <= x < w - r (where the window lies inside the
 * image; there is no padding rule):
 *   sse               sum over all h w pixels of (a - b)^2, an exact integer
 *   sse_mask          the same over the pixels with mask != 0
 *   mask_count        the number of pixels with mask != 0 (h w without a mask); the same for every channel
 *   valid_mask_count  the number of VALID pixels with mask != 0 ((h - 2r)(w - 2r) without a mask)
 *   ssim_sum          sum over the valid region of ssim(y, x)
 *   ssim_sum_mask     the same over the valid pixels whose own (centre) mask byte is non-zero
 * ssim is Wang et al. 2004 in the scikit-image convention, in double throughout.  With W the separable window (x first, then y):
 *   mu_a = W * a, mu_b = W * b, E_aa = W * (a a), E_bb = W * (b b), E_ab = W * (a b)
 *   var_a = E_aa - mu_a mu_a, var_b = E_bb - mu_b mu_b, cov = E_ab - mu_a mu_b        (population form)
 *   C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
 *   ssim = ((2 mu_a) mu_b + C1) (2 cov + C2) / ((mu_a mu_a + mu_b mu_b + C1) (var_a + var_b + C2))
 * Each moment is accumulated from +0 in ascending tap order with one fused multiply-add per tap; everything after the moments is
 * evaluated exactly as spelt above, one rounding per operation, nothing contracted.  For a == b numerator and denominator are then
 * the same bits, the map is exactly 1.0 everywhere and ssim_sum is the count.
 * The sums are fixed-order: a workgroup adds its 256 pixels (mg_reduce.h: the wave tree, the four waves left to right) and leaves
 * its partials in ws; a second launch adds the partials of a (sample, channel): thread t of 256 takes tiles t, t + 256, ... in
 * ascending order, then the same join.  No float atomics: two runs are bit-identical.
 * 1 <= c <= 4, k odd in [3, 15], h, w >= k, n h w c < 2^31.  Two launches. */
int64_t mgq_quality_workspace(int32_t n, int32_t h, int32_t w, int32_t c);
int mgq_image_quality_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const double* window, int32_t k, void* ws,
                         uint64_t* out_int, double* out_ssim, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);

/* Agreement of two orientation maps.  a, b, mask u8 [n][h][w] on the device (mask required); out uint64 [n][2] = {sum, count}:
 *   over the pixels with mask != 0:  d = |a - b|,  sum += min(d, 255 - d),  count += 1
 * The coding has period 255 (0 and 255 are the same angle), so the mean error in degrees is sum / count * 180 / 255.  Integers
 * only: out is cleared on the stream and the workgroups add their sums with 64-bit integer atomics, which is exact in any order.
 * n h w < 2^31.  One memset node and one launch. */
int mgq_orient_distance_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, uint64_t* out, int32_t n, int32_t h, int32_t w,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
