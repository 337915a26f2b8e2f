// mg_mask_edit.hip -- the editing extension group (include/michigan_hip/editing/mask_edit.h): from the demo's pen record to the two
// u8 masks of the stroke route.
//
// mge_brush_u8   demo.py:431-435 (make_mask): the reference calls cv2.line once per recorded segment on the host.  Here a workgroup
//                owns a 16 x 16 tile of one sample.  The segment list goes through LDS in chunks of 256: a thread reads one
//                segment, tests its pen-widened bounding box against the tile, and the survivors are compacted IN ORDER (a wave
//                ballot, the four wave counts joined through LDS).  Every thread then walks the survivors for its own pixel and
//                remembers the value of the last one that covers it: a canvas pixel is never read and is written at most once, by
//                its own thread, so in place is race-free.  The capsule test is integer arithmetic only (the header states it).
// mge_morph_u8   demo.py:323-324, 471-472 (cv2.dilate with an elliptical element), as grey-level dilation / erosion with any
//                element up to 64 x 64: the tile with its halo sits in LDS as bytes (outside the image: the identity of the
//                operation, which is cv2's default border), the element as one 64-bit tap mask per row (a wave ballot over the
//                row's bytes), and beside the patch its row-wise window maxima (minima) over 2, 4 .. 64 columns, each level
//                from the one below.  A run of consecutive taps in an element row is then two overlapping windows: a thread
//                reads two bytes a run, not one a tap, and nothing is assumed of the element (any number of runs a row).  The
//                masks are wave-uniform, so finding the runs is scalar work.  A dilation tile whose halo is all zero leaves
//                after storing zeros: a stroke covers a few percent of the canvas.
#include "mg_common.h"
#include "michigan_hip/editing/mask_edit.h"

namespace {

constexpr int NTHREADS = 256, NWAVES = NTHREADS / 64;
constexpr int BT = MGE_BRUSH_TILE, BCHUNK = MGE_BRUSH_CHUNK;
static_assert(BT * BT == NTHREADS && BCHUNK == NTHREADS, "one thread per pixel of the tile and per segment of a chunk");

__global__ __launch_bounds__(NTHREADS) void brush_kernel(uint8_t* __restrict__ canvas, const int32_t* __restrict__ segs, int S, int H, int W,
                                                         int tiles_x, int tiles_y)
{
    __shared__ int32_t kept[BCHUNK * 6];                               // {ax, ay, dx, dy, t^2, value} of the chunk's survivors, in list order
    __shared__ int wave_count[NWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t_ = blockIdx.x;
    const int tx = t_ % tiles_x; t_ /= tiles_x;
    const int ty = t_ % tiles_y;
    const int n = t_ / tiles_y;
    const int x0 = tx * BT, y0 = ty * BT;
    const int x = x0 + (tid % BT), y = y0 + (tid / BT);
    int last = -1;                                                     // the value of the last segment that covers (x, y)

    for (int base = 0; base < S; base += BCHUNK) {
        const int s = base + tid;
        bool take = false;
        int ax = 0, ay = 0, bx = 0, by = 0, t = 0, val = 0;
        if (s < S) {
            const int32_t* g = segs + (size_t)s * 8;
            const int sn = g[0];
            ax = g[1]; ay = g[2]; bx = g[3]; by = g[4]; t = g[5]; val = g[6];
            const int c = MGE_BRUSH_MAX_COORD;
            const bool ok = sn == n && t >= 1 && t <= MGE_BRUSH_MAX_THICKNESS && (unsigned)val <= 255u &&
                            ax >= -c && ax <= c && ay >= -c && ay <= c && bx >= -c && bx <= c && by >= -c && by <= c;   // outside the ranges: skipped, the products below stay in int64
            const int r = (t + 1) >> 1;                                // a covered pixel is within t / 2 of the segment, so inside its box widened by ceil(t / 2)
            take = ok && min(ax, bx) - r <= x0 + BT - 1 && max(ax, bx) + r >= x0 && min(ay, by) - r <= y0 + BT - 1 && max(ay, by) + r >= y0;
        }
        const unsigned long long votes = __ballot(take);
        if (lane == 0) wave_count[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) {
            const int c = wave_count[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (take) {
            int32_t* k = kept + (before + __popcll(votes & ((1ull << lane) - 1ull))) * 6;
            k[0] = ax; k[1] = ay; k[2] = bx - ax; k[3] = by - ay; k[4] = t * t; k[5] = val;
        }
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const int32_t* k = kept + i * 6;                           // the same address in every lane: a broadcast
            const int dx = k[2], dy = k[3];
            const int qx = x - k[0], qy = y - k[1];                    // |q|, |d| <= 16382: q.q, d.d and q.d stay below 2^30
            const int64_t t2 = k[4];
            const int L2 = dx * dx + dy * dy, dot = qx * dx + qy * dy;
            bool covered;
            if (L2 == 0 || dot <= 0) {
                covered = 4 * (int64_t)(qx * qx + qy * qy) <= t2;
            } else if (dot >= L2) {
                const int ex = qx - dx, ey = qy - dy;
                covered = 4 * (int64_t)(ex * ex + ey * ey) <= t2;
            } else {
                const int64_t cross = (int64_t)qx * dy - (int64_t)qy * dx;     // |cross| < 2^30, 4 cross^2 < 2^62
                covered = 4 * cross * cross <= t2 * (int64_t)L2;
            }
            if (covered) last = k[5];
        }
        __syncthreads();                                               // the next chunk overwrites kept and wave_count
    }
    if (last >= 0 && x < W && y < H) canvas[((size_t)n * H + y) * W + x] = (uint8_t)last;
}

constexpr int MT = MGE_MORPH_TILE, MK = MGE_MORPH_MAX_K;
constexpr int MPH = MT + MK - 1;                                       // 79 patch rows at most
constexpr int MPS = 80;                                                // patch row stride in bytes: the four tile rows of a wave fall in disjoint banks (20 dwords apart)
constexpr int MLEV = 7;                                                // windows of 1, 2, 4 .. 64 columns
static_assert(MT * MT == NTHREADS && MPS >= MPH && MPS % 4 == 0 && MK == 64 && (1 << (MLEV - 1)) == MK, "a row's taps are one 64-bit mask");

template <int OP>
__global__ __launch_bounds__(NTHREADS) void morph_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ elem, int kh, int kw,
                                                         int ay, int ax, uint8_t* __restrict__ dst, int H, int W, int tiles_x, int tiles_y)
{
    // lev[k][r][c] = the maximum (minimum) of patch row r over columns c .. c + 2^k - 1; lev[0] is the patch itself.  43.2 KiB
    __shared__ uint8_t lev[MLEV][MPH * MPS];
    __shared__ unsigned long long taps[MK];
    constexpr int IDENT = OP == MGE_MORPH_DILATE ? 0 : 255;            // what a tap outside the image contributes: nothing
    auto join = [](int a, int b) { return OP == MGE_MORPH_DILATE ? max(a, b) : min(a, b); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t_ = blockIdx.x;
    const int tx = t_ % tiles_x; t_ /= tiles_x;
    const int ty = t_ % tiles_y;
    const int n = t_ / tiles_y;
    const int x0 = tx * MT, y0 = ty * MT;
    const size_t plane = (size_t)n * H * W;
    const int ph = MT + kh - 1, pw = MT + kw - 1;

    int seen = 0;
    for (int i = tid; i < ph * pw; i += NTHREADS) {
        const int r = i / pw, c = i - r * pw;
        const int y = y0 + r - ay, x = x0 + c - ax;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        const int v = in ? src[plane + (size_t)y * W + x] : IDENT;
        lev[0][r * MPS + c] = (uint8_t)v;
        seen |= v;
    }
    for (int i = wave; i < kh; i += NWAVES) {                          // kh <= 64 rows, kw <= 64 bytes each: a lane per byte
        const unsigned long long m = __ballot(lane < kw && elem[i * kw + lane] != 0);
        if (lane == 0) taps[i] = m;
    }
    const int any = __syncthreads_or(seen);                            // also the barrier behind the patch and taps
    const int px = tid % MT, py = tid / MT;
    const int x = x0 + px, y = y0 + py;
    const bool inside = x < W && y < H;
    if (OP == MGE_MORPH_DILATE && !any) {                              // the whole workgroup agrees: the maximum of zeros
        if (inside) dst[plane + (size_t)y * W + x] = 0;
        return;
    }
    // A run of L consecutive taps of an element row is two overlapping windows of 2^k <= L columns, so a pixel costs two reads a run
    // instead of one a tap (one dependent read a tap: 91 us at 1 x 512^2 with the 50 x 50 ellipse, profiles/edit_session.txt).  No run is
    // longer than kw: the levels up to floor(log2 kw), each from the one below; level k is defined where its window ends inside the patch.
    const int top = 31 - __builtin_clz(kw);
    for (int k = 1; k <= top; ++k) {
        const int half = 1 << (k - 1), wk = pw - (1 << k) + 1;         // 2^k <= kw <= pw: wk >= 1
        for (int i = tid; i < ph * wk; i += NTHREADS) {
            const int r = i / wk, c = i - r * wk;
            lev[k][r * MPS + c] = (uint8_t)join(lev[k - 1][r * MPS + c], lev[k - 1][r * MPS + c + half]);    // c + half <= pw - 2^(k-1): defined
        }
        __syncthreads();
    }
    int v = IDENT;
    const int p = py * MPS + px;                                       // tap (i, j) of this pixel is patch row py + i, column px + j
    for (int i = 0; i < kh; ++i) {
        const unsigned long long m = taps[i];
        unsigned long long bits = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);            // the same in every lane: finding the runs is scalar work
        while (bits) {                                                 // run by run: [j0, j1) are consecutive taps of this row
            const int j0 = __builtin_ctzll(bits);
            const unsigned long long gaps = ~(bits >> j0);             // a full row from bit 0 leaves no gap: the run is all 64
            const int j1 = j0 + (gaps ? __builtin_ctzll(gaps) : 64);
            bits = j1 >= 64 ? 0ull : bits & (~0ull << j1);
            const int k = 31 - __builtin_clz(j1 - j0);                 // 2^k <= j1 - j0 <= kw: k <= top
            const uint8_t* row = lev[k] + p + i * MPS;
            v = join(v, join(row[j0], row[j1 - (1 << k)]));            // [j0, j0 + 2^k) and [j1 - 2^k, j1) cover the run and nothing else
        }
    }
    if (inside) dst[plane + (size_t)y * W + x] = (uint8_t)v;
}

}  // namespace

extern "C" int mge_brush_u8(uint8_t* canvas, const int32_t* segs, int32_t s, int32_t n, int32_t h, int32_t w, void* stream)
{
    MG_CHECK_ARG(canvas, "mge_brush_u8: null canvas");
    MG_CHECK_ARG(s >= 0 && s < (1 << 27), "mge_brush_u8: bad segment count s=%d", s);
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1 && h <= MGE_BRUSH_MAX_COORD + 1 && w <= MGE_BRUSH_MAX_COORD + 1,
                 "mge_brush_u8: bad geometry n=%d h=%d w=%d (h, w in [1, %d])", n, h, w, MGE_BRUSH_MAX_COORD + 1);
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "mge_brush_u8: n h w = %lld does not fit 31 bits", (long long)n * h * w);
    if (s == 0) return MG_OK;                                          // nothing drawn: no launch
    MG_CHECK_ARG(segs, "mge_brush_u8: null segment list");
    const int64_t tx = (w + BT - 1) / BT, ty = (h + BT - 1) / BT;
    hipLaunchKernelGGL(brush_kernel, dim3((unsigned)(n * tx * ty)), dim3(NTHREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       canvas, segs, s, h, w, (int)tx, (int)ty);
    MG_CHECK_LAUNCH("mge_brush_u8");
    return MG_OK;
}

extern "C" int mge_morph_u8(const uint8_t* src, const uint8_t* elem, int32_t kh, int32_t kw, int32_t ay, int32_t ax, int32_t op, uint8_t* dst,
                            int32_t n, int32_t h, int32_t w, void* stream)
{
    MG_CHECK_ARG(src && elem && dst, "mge_morph_u8: null pointer");
    MG_CHECK_ARG(op == MGE_MORPH_DILATE || op == MGE_MORPH_ERODE, "mge_morph_u8: bad op %d (0 dilates, 1 erodes)", op);
    MG_CHECK_ARG(kh >= 1 && kw >= 1 && kh <= MK && kw <= MK, "mge_morph_u8: bad element %d x %d (1 .. %d each way)", kh, kw, MK);
    MG_CHECK_ARG(ay >= 0 && ay < kh && ax >= 0 && ax < kw, "mge_morph_u8: anchor (%d, %d) outside the %d x %d element", ay, ax, kh, kw);
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1, "mge_morph_u8: bad geometry n=%d h=%d w=%d", n, h, w);
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "mge_morph_u8: n h w = %lld does not fit 31 bits", (long long)n * h * w);
    const int64_t bytes = (int64_t)n * h * w;
    MG_CHECK_ARG(src + bytes <= dst || dst + bytes <= src, "mge_morph_u8: src and dst overlap (not an in-place operation)");
    const int64_t tx = (w + MT - 1) / MT, ty = (h + MT - 1) / MT;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (op == MGE_MORPH_DILATE)
        hipLaunchKernelGGL(morph_kernel<MGE_MORPH_DILATE>, dim3((unsigned)(n * tx * ty)), dim3(NTHREADS), 0, st, src, elem, kh, kw, ay, ax, dst, h, w, (int)tx, (int)ty);
    else
        hipLaunchKernelGGL(morph_kernel<MGE_MORPH_ERODE>, dim3((unsigned)(n * tx * ty)), dim3(NTHREADS), 0, st, src, elem, kh, kw, ay, ax, dst, h, w, (int)tx, (int)ty);
    MG_CHECK_LAUNCH("mge_morph_u8");
    return MG_OK;
}
