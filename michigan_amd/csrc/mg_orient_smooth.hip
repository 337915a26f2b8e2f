// mg_orient_smooth.hip -- second half of dense hair-orientation extraction (reference: cal_orientation.py:101-109).
//
// The reference turns the arg-max filter index and its confidence into a flow field (two [H,W] fp32 maps), smooths each with
// cv2.GaussianBlur(sigma 4: 33 taps, BORDER_REFLECT_101), takes 0.5 atan2, and quantises to the uint8 map the data set stores --
// on the CPU, seven full-size intermediates.  Here one launch does it: a workgroup owns a 32 x 32 output tile, forms the flow
// of the (32+32) x (32+32) haloed patch while loading it into LDS, runs the row pass into a second LDS image and the column pass
// out of it, and writes one byte (and optionally one float) per pixel.  Both passes slide a register window, so an LDS value is
// read once per pass and not once per tap:
//   row pass     lane = patch row (64 rows = one wave), a wave owns 8 output columns: 40 ds_read_b64 for 8 outputs;
//   column pass  lane = output column x 2 row groups, a thread owns 4 output rows:     36 ds_read_b64 for 4 outputs.
// Row strides of 65 and 33 float2 keep every access conflict-free: a row-pass lane step is 130 (66) dwords = 2 mod 64, a
// column-pass wave half reads 32 consecutive float2.
// sin / cos / exp are tables from the host (include/michigan_hip/preprocess/dense_orient.h).
#include "mg_common.h"
#include "michigan_hip/preprocess/dense_orient.h"

namespace {

constexpr int R = MG_ORIENT_RADIUS, NT = 2 * R + 1;                 // 33 taps
constexpr int TH = MG_ORIENT_TILE_H, TW = MG_ORIENT_TILE_W;         // output tile
constexpr int PH = TH + 2 * R, PW = TW + 2 * R;                     // 64 x 64 haloed patch
constexpr int FS = PW + 1, RS = TW + 1;                             // LDS row strides in float2 (odd: see above)
constexpr int NTHREADS = 256, NWAVES = NTHREADS / 64;
constexpr int RC = TW / NWAVES;                                     // row pass: output columns per wave (8)
constexpr int CR = TH * TW / NTHREADS;                              // column pass: output rows per thread (4)
constexpr int LP = PH * PW / NTHREADS;                              // load: patch pixels per thread (16)
static_assert(PW == 64 && NTHREADS % PW == 0 && LP * NTHREADS == PH * PW, "the load maps a thread to one patch column");
static_assert(PH == 64, "the row pass maps one patch row to one lane of a wave");
static_assert(TW == 32 && NTHREADS == 8 * TW && CR * 8 == TH, "the column pass maps a wave half to one row group of 32 columns");

__device__ __forceinline__ int refl101(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);            // only positions of a partial tile that no output reads are clamped (h, w >= 17)
}

__global__ __launch_bounds__(NTHREADS) void orient_smooth_kernel(const float* __restrict__ conf, const uint8_t* __restrict__ idx,
                                                                 const uint8_t* __restrict__ mask, const float* __restrict__ trig,
                                                                 const float* __restrict__ taps, uint8_t* __restrict__ orient_u8,
                                                                 float* __restrict__ angle, int H, int W, int tiles_x, int tiles_y)
{
    __shared__ float2 flow[PH * FS];                   // 33,280 B
    __shared__ float2 rows[PH * RS];                   // 16,896 B
    __shared__ float2 trg[32];                         // the host's {cos, sin} table
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = blockIdx.x;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int n = t / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t plane = (size_t)n * H * W;

    float tp[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) tp[k] = taps[k];

    // the flow of the haloed patch, formed on the way in.  A thread owns patch column tid % 64 and every 4th patch row: its 16 x 3
    // loads do not depend on each other (the mask selects afterwards, it does not branch around them) and are all in flight together
    if (tid < 32) trg[tid] = make_float2(trig[2 * tid], trig[2 * tid + 1]);
    {
        const int px = tid & (PW - 1), py0 = tid / PW;
        const size_t col = plane + refl101(x0 + px - R, W);
        float c[LP];
        uint8_t k[LP], m[LP];
#pragma unroll
        for (int j = 0; j < LP; ++j) {
            const size_t o = col + (size_t)refl101(y0 + py0 + j * (NTHREADS / PW) - R, H) * W;
            m[j] = mask[o];
            k[j] = idx[o];
            c[j] = conf[o];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LP; ++j) {
            const float2 t = trg[k[j] & 31];
            flow[(py0 + j * (NTHREADS / PW)) * FS + px] = m[j] != 0 ? make_float2(t.x * c[j], t.y * c[j]) : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();

    // row pass: rows[r][c] = sum_i taps[i] flow[r][c + i]
    {
        const int c0 = wave * RC;
        float2 acc[RC];
#pragma unroll
        for (int o = 0; o < RC; ++o) acc[o] = make_float2(0.f, 0.f);
#pragma unroll
        for (int k = 0; k < RC + NT - 1; ++k) {
            const float2 v = flow[lane * FS + c0 + k];
#pragma unroll
            for (int o = 0; o < RC; ++o)
                if (k - o >= 0 && k - o < NT) {
                    acc[o].x = fmaf(tp[k - o], v.x, acc[o].x);
                    acc[o].y = fmaf(tp[k - o], v.y, acc[o].y);
                }
        }
#pragma unroll
        for (int o = 0; o < RC; ++o) rows[lane * RS + c0 + o] = acc[o];
    }
    __syncthreads();

    // column pass: b[y][x] = sum_j taps[j] rows[y + j][x], then the angle and its byte
    const int x = tid & (TW - 1), r0 = (tid / TW) * CR;
    float2 acc[CR];
#pragma unroll
    for (int o = 0; o < CR; ++o) acc[o] = make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < CR + NT - 1; ++k) {
        const float2 v = rows[(r0 + k) * RS + x];
#pragma unroll
        for (int o = 0; o < CR; ++o)
            if (k - o >= 0 && k - o < NT) {
                acc[o].x = fmaf(tp[k - o], v.x, acc[o].x);
                acc[o].y = fmaf(tp[k - o], v.y, acc[o].y);
            }
    }
    const float PI = 3.14159265358979323846f;
#pragma unroll
    for (int o = 0; o < CR; ++o) {
        const int gy = y0 + r0 + o, gx = x0 + x;
        if (gy >= H || gx >= W) continue;
        const size_t p = plane + (size_t)gy * W + gx;
        float th = 0.5f * atan2f(acc[o].y, acc[o].x);
        if (th < 0.f) th += PI;
        if (angle) angle[p] = th;
        const float level = mask[p] != 0 ? th * 255.f / PI : 0.f;          // the reference's order: (theta * 255) / pi, then the mask
        orient_u8[p] = (uint8_t)fminf(level, 255.f);
    }
}

}  // namespace

extern "C" int mg_orient_smooth(const float* conf, const uint8_t* idx, const uint8_t* mask, const float* trig, const float* taps,
                                uint8_t* orient_u8, float* angle, int32_t n, int32_t h, int32_t w, void* stream)
{
    MG_CHECK_ARG(conf && idx && mask && trig && taps && orient_u8, "mg_orient_smooth: null pointer");
    MG_CHECK_ARG(n > 0 && h >= NT / 2 + 1 && w >= NT / 2 + 1, "mg_orient_smooth: bad geometry n=%d h=%d w=%d (h, w >= %d: one reflection must reach every tap)", n, h, w, NT / 2 + 1);
    const int64_t tx = (w + TW - 1) / TW, ty = (h + TH - 1) / TH;
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31) && n * tx * ty < (1ll << 31), "mg_orient_smooth: n h w = %lld does not fit 31 bits", (long long)n * h * w);
    hipLaunchKernelGGL(orient_smooth_kernel, dim3((unsigned)(n * tx * ty)), dim3(NTHREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       conf, idx, mask, trig, taps, orient_u8, angle, h, w, (int)tx, (int)ty);
    MG_CHECK_LAUNCH("mg_orient_smooth");
    return MG_OK;
}
