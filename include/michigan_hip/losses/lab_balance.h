/* michigan_hip/losses/lab_balance.h -- the COLOUR-BALANCE EXTENSION group of libmichigan_hip (mg_color_loss.hip, mg_hair_lab.hip): the
 * Lab colour loss and the hair-average Lab loss under --balance_Lab (reference: models/networks/loss.py:484-531 and 578-620), in which a
 * colour that is rare among hair colours weighs more.  The passes are the colour pass and the hair-Lab pass of michigan_hip.h with one
 * more operand; everything said there about layouts, the Lab route, the reduction order and sign(0) = 0 holds here unchanged, and the
 * terms the table does not touch (rgb, background) ride along bit for bit.
 *
 * The group carries the prefix mgc_ and is NOT part of the versioned symbol table of michigan_hip.h: MG_ABI_VERSION does not count it,
 * michigan_amd/_cabi.py binds it in a table of its own (_COLOR_PROTOS), and the contract emulator under oracle/ does not know it
 * (tests/lab_balance_fixtures.py carries the float64 contract and an emulator subclass).
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind the last-error call; arguments
 * are validated before the device is touched; all work is enqueued on `stream` (a hipStream_t), nothing synchronises and nothing is
 * read back.
 *
 * THE TABLE.  `table`: float [256][256] on the device, S[ka][kb], rows index a, columns index b.  The bin of a Lab coordinate v is
 *   k(v) = (int) min(max(v + 128.f, 0.f), 255.f)                 evaluated in fp32; a NaN gives bin 0
 * The library reads S as the caller wrote it, all 65536 entries.  The reference forms its weights from a histogram of hair colours
 * (counts -> fp32, zeros -> 1, max / count, capped at --Lab_weight_th) and samples them with grid_sample(mode='nearest'), which under
 * today's default align_corners=False maps bin 255 to the position 255.5, rounds it to 256 and reads the zero padding: S[255][..] =
 * S[..][255] = 0.  (The torch the reference was written for, align_corners=True, read w[255][..] there; this package follows the
 * reference as it runs today.)  ops.lab_weight_table builds that S; nothing here calls grid_sample. */
#ifndef MICHIGAN_HIP_LOSSES_LAB_BALANCE_H
#define MICHIGAN_HIP_LOSSES_LAB_BALANCE_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGC_TABLE_BINS 256                 /* the table is float [256][256] */
#define MGC_HAIR_STATS 8                   /* floats per sample of the balanced hair pass's `stats`: da, db, 1 / S_f, 1 / S_r, w_n, 0, 0, 0 */

/* The colour pass, balanced.  Arguments, `out`, `ws` and launches as the colour pass of michigan_hip.h; `flags` must contain lab (1).
 * hair: float [N][HW], samples hair_nstride >= HW elements apart (plane 1 of the one-hot label, no copy); its VALUE multiplies.
 * Per pixel, from the TARGET image's (a_r, b_r):
 *   w = S[k(a_r)][k(b_r)] * hair,   w = 1 where w == 0             (outside the hair; a zero of the table)
 *   out[0] lab = sum w (|da| + |db|) / (2 N HW)                    out[1], out[2]: rgb and background, unchanged
 * The (a_r, b_r) are the ones the differences are taken of: one evaluation per pixel.  Two launches. */
int mgc_color_loss_balanced_fwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                const float* hair, int64_t hair_nstride, const float* table,
                                int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, float* out, float* ws, void* stream);

/* Backward to img: the Lab part of a pixel's gradient is the unbalanced one times w (the scalar d mean / d element is multiplied by w
 * first, so w == 1 reproduces the unbalanced bits and a power of two scales them exactly); where the generated pixel equals the target
 * the Lab part is exactly 0.  g_lab, g_rgb, g_back: one float each on the device, any may be NULL (= 0).  One launch. */
int mgc_color_loss_balanced_bwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                const float* hair, int64_t hair_nstride, const float* table,
                                const float* g_lab, const float* g_rgb, const float* g_back,
                                int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream);

/* The hair-Lab pass, balanced.  Arguments, `out`, `ws` and launches as the hair-Lab pass of michigan_hip.h; `flags` must contain
 * hairAvgLab (1).  One weight per sample from the REFERENCE image's mean hair colour (the mean as the unbalanced pass forms it, in
 * double, rounded to fp32 once, then binned as above):
 *   w_n = S[k(mean a_ref)][k(mean b_ref)]                           NO zero-to-one replacement: a zero of the table gives weight 0
 *   out[0] hairAvgLab = sum_n w_n (|da_n| + |db_n|) / (2 N)        out[1]: background, unchanged
 * stats: float [N][MGC_HAIR_STATS], written here for the backward: da_n, db_n, 1 / S_f, 1 / S_r, w_n and three zeros. */
int mgc_hair_lab_balanced_fwd(const void* img, const float* ref, int64_t ref_nstride, const float* hair_tag, int64_t hair_tag_nstride,
                              const float* hair_ref, int64_t hair_ref_nstride, const float* tgt, int64_t tgt_nstride,
                              const float* back, int64_t back_nstride, const float* table, int32_t dtype, int32_t N, int32_t H, int32_t W,
                              int32_t C, int32_t flags, float* out, float* stats, float* ws, void* stream);

/* Backward to img: the unbalanced one with the per-sample scale multiplied by w_n, which it reads from the forward's `stats` -- so it
 * takes no table.  One launch. */
int mgc_hair_lab_balanced_bwd(const void* img, const float* hair_tag, int64_t hair_tag_nstride, const float* tgt, int64_t tgt_nstride,
                              const float* back, int64_t back_nstride, const float* stats, const float* g_hair, const float* g_back,
                              int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
