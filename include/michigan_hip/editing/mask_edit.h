/* michigan_hip/editing/mask_edit.h -- the EDITING EXTENSION group of libmichigan_hip (mg_mask_edit.hip): what turns the pen record
 * of the interactive demo into the two u8 masks the stroke route takes.  Reference: demo.py:431-435 (make_mask: cv2.line per recorded
 * segment), demo.py:323-324 and 471-472 (cv2.dilate with a 50 x 50 / 20 x 20 MORPH_ELLIPSE element).
 *
 * The group carries the prefix mge_ and is NOT part of the versioned symbol table of michigan_hip.h: MG_ABI_VERSION does not count
 * it, michigan_amd/_cabi.py binds it in a table of its own (_EDIT_PROTOS), and the contract emulator under oracle/ does not know it
 * (tests/mask_edit_fixtures.py carries the contracts and an emulator subclass).  It moves into the main table, under the main
 * prefix, with the change that next owns that emulator.
 *
 * Conventions as in michigan_hip.h: every call returns MG_OK or an MG_ERR_* code with a message behind mg_last_error; arguments are
 * validated before the device is touched; all work is enqueued on `stream` (a hipStream_t) and nothing synchronises. */
#ifndef MICHIGAN_HIP_EDITING_MASK_EDIT_H
#define MICHIGAN_HIP_EDITING_MASK_EDIT_H

#include "../../michigan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGE_BRUSH_TILE 16                  /* a workgroup owns a 16 x 16 tile of one sample's canvas (tests sit on these edges) */
#define MGE_BRUSH_CHUNK 256                /* segments staged through LDS at a time */
#define MGE_BRUSH_MAX_THICKNESS 255
#define MGE_BRUSH_MAX_COORD 8191           /* |x|, |y| of an end point; h, w <= MGE_BRUSH_MAX_COORD + 1 */
#define MGE_MORPH_TILE 16                  /* output pixels per workgroup, each axis */
#define MGE_MORPH_MAX_K 64                 /* the element is at most 64 x 64 */
#define MGE_MORPH_DILATE 0
#define MGE_MORPH_ERODE 1

/* The brush.  canvas u8 [n][h][w], updated in place; segs int32 [s][8] on the device = {sample, x0, y0, x1, y1, thickness, value, 0}.
 * The segments are applied IN ORDER: a pixel ends with the value of the last segment that covers it and is not written when none
 * does.  Segment (a, b, t) covers pixel p when p is within t / 2 of the closed segment a-b -- a capsule, decided in integers only:
 * with d = b - a, q = p - a, L2 = d.d, dot = q.d,
 *   L2 == 0 or dot <= 0:   4 (q.q) <= t^2
 *   dot >= L2:             4 |p - b|^2 <= t^2
 *   otherwise:             4 cross^2 <= t^2 L2,   cross = q.x d.y - q.y d.x     (int64)
 * This is the package's OWN brush definition.  cv2.line draws a thick line as a filled polygon with round caps whose edge rule
 * cannot be pinned without OpenCV, and no machine of this project has it; a stroke drawn here and one drawn by the reference's
 * demo may differ along the rim.
 * Ranges: 1 <= thickness <= 255, |x|, |y| <= 8191, 0 <= value <= 255, 0 <= sample < n, 1 <= h, w <= 8192: every product above
 * then fits int64.  n, h, w and s are checked here.  The segment list lives in device memory, which this call does not read back:
 * the caller that holds the list on the host checks the per-segment ranges before it uploads (michigan_amd.inputs.brush_u8 does,
 * and raises before anything is launched), and the kernel skips a segment outside them.
 * s == 0 returns MG_OK without a launch (segs may then be NULL).  One launch: a workgroup stages the list through LDS in chunks of
 * 256, keeps (in order) the segments of its sample whose bounding box, widened by the pen, meets its tile, and each thread reads no
 * canvas pixel and writes only its own: in place is race-free and two runs are bit-identical. */
int mge_brush_u8(uint8_t* canvas, const int32_t* segs, int32_t s, int32_t n, int32_t h, int32_t w, void* stream);

/* Grey-level dilation (op 0) or erosion (op 1) with an arbitrary element.  src, dst u8 [n][h][w], elem u8 [kh][kw] on the device
 * (non-zero = the tap is in), anchor (ay, ax):
 *   dst[n][y][x] = max (op 0) / min (op 1) over the taps (i, j) with elem[i][j] != 0 and (y + i - ay, x + j - ax) inside the image
 *                  of src[n][y + i - ay][x + j - ax];   0 (op 0) / 255 (op 1) when no tap falls inside
 * -- cv2.dilate / cv2.erode with their default border.  Nothing is assumed of the element (not convex, not symmetric, possibly
 * empty) nor of the input (any grey level).  1 <= kh, kw <= 64, the anchor inside the element, src and dst must not overlap,
 * n h w < 2^31.  One launch: a workgroup loads its 16 x 16 tile with the halo and one 64-bit tap mask per element row into LDS, builds
 * the row-wise window maxima (minima) of the patch over 2, 4 .. 64 columns there, and reads two bytes per run of consecutive taps; for
 * dilation a tile whose halo is all zero stores zeros and leaves. */
int mge_morph_u8(const uint8_t* src, const uint8_t* elem, int32_t kh, int32_t kw, int32_t ay, int32_t ax, int32_t op, uint8_t* dst,
                 int32_t n, int32_t h, int32_t w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
