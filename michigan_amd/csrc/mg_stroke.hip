// mg_stroke.hip -- the stroke route of the interactive demo (include/michigan_hip/editing/stroke_orient.h).
//
// mg_stroke_orient   ui_util/cal_orient_stroke.py:85-121, 133-149: the reference runs 32 F.conv2d calls over the whole canvas,
//                    concatenates, clamps, takes arg-max and max, builds (sin 2a, cos 2a), multiplies by the mask three times and
//                    converts to bytes on the host.  A stroke covers a few percent of the canvas and every pixel outside it is
//                    black by definition, so here a workgroup owns a 16 x 16 tile, loads its (16+16)^2 patch of the mask, and
//                    leaves at once (writing zeros) when the tile holds no stroke pixel.  Otherwise a thread owns one pixel:
//                    the bank sits in LDS tap-major, so the 32 weights of a tap are eight 16-byte reads that every lane of a
//                    wave shares (a broadcast), and the 32 sums stay in registers.  The mask is 0 or 1, so a product is exact
//                    and a sum is a plain chain of fp32 additions, one chain per tap row, the 17 row sums added in order.
//                    Waves of an active tile without a stroke pixel skip the filter loop too.
// mg_stroke_compose  models/pix2pix_model.py:443-447 (408-411 without strokes): five NCHW fp32 maps -> the net's NHWC8 input at
// mg_inpaint_finish  its 256 x 256 working size, and :450-463: the net's output back at the crop size, blended, and the
//                    2-channel orientation.  Streaming kernels, one thread per output pixel; the arithmetic is the reference's
//                    operation by operation (no contraction), so the fp32 results are the torch expressions' bit for bit.
#include <algorithm>
#include "mg_common.h"
#include "mg_launch.h"
#include "michigan_hip/editing/stroke_orient.h"

namespace {

constexpr int NF = MG_STROKE_FILTERS, KR = MG_STROKE_RADIUS, KS = 2 * KR + 1, NTAP = KS * KS;   // 32 filters of 17 x 17 = 289 taps
constexpr int TH = MG_STROKE_TILE_H, TW = MG_STROKE_TILE_W;                                     // one thread per pixel of the tile
constexpr int PH = TH + 2 * KR, PW = TW + 2 * KR;                                               // 32 x 32 patch
constexpr int PS = PW + 16;                                // patch row stride: two tile rows (one 32-lane group) fall in disjoint banks
constexpr int NTHREADS = TH * TW;
static_assert(NTHREADS == 256 && TW == 16 && PS % 32 == 16, "a 32-lane group reads two patch rows of 16 pixels");
static_assert(NF == 32, "a tap's weights are eight float4");

__global__ __launch_bounds__(NTHREADS) void stroke_orient_kernel(const uint8_t* __restrict__ stroke, const float* __restrict__ bank,
                                                                 const uint8_t* __restrict__ rgb_table, uint8_t* __restrict__ rgb_u8,
                                                                 uint8_t* __restrict__ idx, float* __restrict__ conf,
                                                                 int H, int W, int tiles_x, int tiles_y)
{
    __shared__ float patch[PH * PS];                                   // 6 KiB
    __shared__ __attribute__((aligned(16))) float wts[NTAP * NF];      // tap-major: wts[tap][filter], 36.1 KiB
    const int tid = threadIdx.x;
    int t = blockIdx.x;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int n = t / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t plane = (size_t)n * H * W;

    for (int i = tid; i < PH * PW; i += NTHREADS) {
        const int py = i / PW, px = i - py * PW;
        const int y = y0 + py - KR, x = x0 + px - KR;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;            // zero outside the image
        patch[py * PS + px] = in && stroke[plane + (size_t)y * W + x] != 0 ? 1.f : 0.f;
    }
    const int py = tid / TW, px = tid - py * TW;
    const int y = y0 + py, x = x0 + px;
    const bool inside = y < H && x < W;
    const size_t p = plane + (size_t)(inside ? y : 0) * W + (inside ? x : 0);
    const bool on = inside && stroke[p] != 0;
    const int any = __syncthreads_or(on);                              // also the barrier behind the patch
    if (!any) {                                                        // the whole workgroup agrees: nothing to filter
        if (inside) {
            rgb_u8[3 * p] = 0; rgb_u8[3 * p + 1] = 0; rgb_u8[3 * p + 2] = 0;
            if (idx) idx[p] = 0;
            if (conf) conf[p] = 0.f;
        }
        return;
    }
    for (int i = tid; i < NF * NTAP; i += NTHREADS) {                  // bank[f][tap] -> wts[tap][f]
        const int f = i / NTAP, k = i - f * NTAP;
        wts[k * NF + f] = bank[i];
    }
    __syncthreads();

    float best = 0.f;
    int bi = 0;
    if (on) {
        float acc[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = 0.f;
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
            float row[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) row[f] = 0.f;
            const float* pr = patch + (py + ky) * PS + px;
            const f32x4_t* wr = reinterpret_cast<const f32x4_t*>(wts + ky * KS * NF);
#pragma unroll 4                                          // the reads of the next taps are in flight behind the FMAs of this one: a lone wave per SIMD has nothing else to hide them
            for (int kx = 0; kx < KS; ++kx) {
                const float s = pr[kx];
#pragma unroll
                for (int q = 0; q < NF / 4; ++q) {
                    const f32x4_t b = wr[kx * (NF / 4) + q];
#pragma unroll
                    for (int j = 0; j < 4; ++j) row[4 * q + j] = fmaf(b[j], s, row[4 * q + j]);      // s is 0 or 1: row += b or row
                }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) acc[f] += row[f];
        }
        best = -1.f;
#pragma unroll
        for (int f = 0; f < NF; ++f) {                                 // clamp, then the FIRST arg-max
            const float v = fmaxf(acc[f], 0.f);
            if (v > best) { best = v; bi = f; }
        }
    }
    if (inside) {
        uint8_t r = 0, g = 0, b = 0;
        if (on) { r = rgb_table[3 * bi]; g = rgb_table[3 * bi + 1]; b = rgb_table[3 * bi + 2]; }
        rgb_u8[3 * p] = r; rgb_u8[3 * p + 1] = g; rgb_u8[3 * p + 2] = b;
        if (idx) idx[p] = (uint8_t)bi;
        if (conf) conf[p] = best;
    }
}

// ---- the two glue kernels: the reference's fp32 expressions, one operation at a time -------------------------------------------------
__device__ __forceinline__ int table_at(const int32_t* tab, int i, int n)
{
    return tab ? min(max(tab[i], 0), n - 1) : i;           // a table from ops.interp_nearest_table is in range; a stray entry must not leave the map
}

template <typename T>
__global__ __launch_bounds__(256) void stroke_compose_kernel(const float* __restrict__ orient_rgb, const float* __restrict__ noise,
                                                             const float* __restrict__ hole, const float* __restrict__ stroke,
                                                             const float* __restrict__ stroke_mask, const int32_t* __restrict__ ytab,
                                                             const int32_t* __restrict__ xtab, int N, int H, int W, int Ho, int Wo,
                                                             T* __restrict__ inp)
{
#pragma clang fp contract(off)
    const int64_t total = (int64_t)N * Ho * Wo;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const unsigned u = (unsigned)o;                                  // total < 2^31: 32-bit divisions
        const int x = (int)(u % (unsigned)Wo);
        const int y = (int)((u / (unsigned)Wo) % (unsigned)Ho);
        const int n = (int)(u / ((unsigned)Wo * (unsigned)Ho));
        const size_t hw = (size_t)H * W;
        const size_t q = (size_t)table_at(ytab, y, H) * W + table_at(xtab, x, W);
        const float hl = hole[n * hw + q];
        const float sm = stroke_mask ? stroke_mask[n * hw + q] : 0.f;
        const float keep = 1.f - hl;
        float v[8];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t pc = ((size_t)n * 3 + c) * hw + q;
            const float a = orient_rgb[pc] * keep;
            if (stroke_mask) {
                const float b = noise[pc] * (hl - sm);
                const float d = stroke[pc] * sm;
                v[c] = (a + b) + d;
            } else {
                v[c] = a + noise[pc] * hl;
            }
        }
        v[3] = hl; v[4] = sm; v[5] = 0.f; v[6] = 0.f; v[7] = 0.f;
        T* dst = inp + (size_t)o * 8;
        ET<T>::store4(dst, f32x4_t{v[0], v[1], v[2], v[3]});
        ET<T>::store4(dst + 4, f32x4_t{v[4], v[5], v[6], v[7]});
    }
}

__global__ __launch_bounds__(256) void inpaint_finish_kernel(const float* __restrict__ net_out, const int32_t* __restrict__ ytab,
                                                             const int32_t* __restrict__ xtab, const float* __restrict__ hole,
                                                             const float* __restrict__ orient_rgb, const float* __restrict__ mask,
                                                             int N, int H, int W, int Ho, int Wo, float* __restrict__ out_rgb,
                                                             float* __restrict__ orient2)
{
#pragma clang fp contract(off)
    const int64_t total = (int64_t)N * H * W;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const unsigned u = (unsigned)o;                                  // total < 2^31: 32-bit divisions
        const int x = (int)(u % (unsigned)W);
        const int y = (int)((u / (unsigned)W) % (unsigned)H);
        const int n = (int)(u / ((unsigned)W * (unsigned)H));
        const size_t hw = (size_t)H * W, hwo = (size_t)Ho * Wo;
        const size_t q = (size_t)y * W + x;
        const size_t qs = (size_t)table_at(ytab, y, Ho) * Wo + table_at(xtab, x, Wo);
        const float hl = hole[n * hw + q], m = mask[n * hw + q];
        const float keep = 1.f - hl;
        float out[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t pc = ((size_t)n * 3 + c) * hw + q;
            const float a = net_out[((size_t)n * 3 + c) * hwo + qs] * hl;
            const float b = orient_rgb[pc] * keep;
            out[c] = a + b;
            out_rgb[pc] = out[c];
        }
        orient2[((size_t)n * 2 + 0) * hw + q] = ((out[1] - 0.5f) * 2.f) * m;
        orient2[((size_t)n * 2 + 1) * hw + q] = ((out[0] - 0.5f) * 2.f) * m;
    }
}

inline unsigned stream_grid(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 8192); }

}  // namespace

extern "C" int mg_stroke_orient(const uint8_t* stroke, const float* bank, const uint8_t* rgb_table, uint8_t* rgb_u8, uint8_t* idx, float* conf,
                                int32_t n, int32_t h, int32_t w, void* stream)
{
    MG_CHECK_ARG(stroke && bank && rgb_table && rgb_u8, "mg_stroke_orient: null pointer");
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1, "mg_stroke_orient: bad geometry n=%d h=%d w=%d", n, h, w);
    const int64_t tx = (w + TW - 1) / TW, ty = (h + TH - 1) / TH;
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "mg_stroke_orient: n h w = %lld does not fit 31 bits", (long long)n * h * w);
    hipLaunchKernelGGL(stroke_orient_kernel, dim3((unsigned)(n * tx * ty)), dim3(NTHREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       stroke, bank, rgb_table, rgb_u8, idx, conf, h, w, (int)tx, (int)ty);
    MG_CHECK_LAUNCH("mg_stroke_orient");
    return MG_OK;
}

extern "C" int mg_stroke_compose(const float* orient_rgb, const float* noise, const float* hole, const float* stroke, const float* stroke_mask,
                                 const int32_t* ytab, const int32_t* xtab, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t ho, int32_t wo,
                                 void* inp, void* stream)
{
    MG_CHECK_ARG(orient_rgb && noise && hole && inp, "mg_stroke_compose: null pointer");
    MG_CHECK_ARG((stroke == nullptr) == (stroke_mask == nullptr), "mg_stroke_compose: stroke and stroke_mask are given together or not at all");
    MG_CHECK_ARG(dtype == MG_F32 || dtype == MG_BF16, "mg_stroke_compose: bad dtype");
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1 && ho >= 1 && wo >= 1, "mg_stroke_compose: bad geometry n=%d h=%d w=%d ho=%d wo=%d", n, h, w, ho, wo);
    MG_CHECK_ARG((ytab || ho == h) && (xtab || wo == w), "mg_stroke_compose: a null table is the identity and needs ho == h / wo == w (%d x %d -> %d x %d)", h, w, ho, wo);
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31) && (int64_t)n * ho * wo < (1ll << 31), "mg_stroke_compose: the maps do not fit 31 bits");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(stroke_compose_kernel<T>, dim3(stream_grid((int64_t)n * ho * wo)), dim3(256), 0, st,
                           orient_rgb, noise, hole, stroke, stroke_mask, ytab, xtab, n, h, w, ho, wo, (T*)inp); });
    MG_CHECK_LAUNCH("mg_stroke_compose");
    return MG_OK;
}

extern "C" int mg_inpaint_finish(const float* net_out, const int32_t* ytab, const int32_t* xtab, const float* hole, const float* orient_rgb,
                                 const float* mask, int32_t n, int32_t h, int32_t w, int32_t ho, int32_t wo, float* out_rgb, float* orient2,
                                 void* stream)
{
    MG_CHECK_ARG(net_out && hole && orient_rgb && mask && out_rgb && orient2, "mg_inpaint_finish: null pointer");
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1 && ho >= 1 && wo >= 1, "mg_inpaint_finish: bad geometry n=%d h=%d w=%d ho=%d wo=%d", n, h, w, ho, wo);
    MG_CHECK_ARG((ytab || ho == h) && (xtab || wo == w), "mg_inpaint_finish: a null table is the identity and needs ho == h / wo == w (%d x %d <- %d x %d)", h, w, ho, wo);
    MG_CHECK_ARG((int64_t)n * h * w < (1ll << 31) && (int64_t)n * ho * wo < (1ll << 31), "mg_inpaint_finish: the maps do not fit 31 bits");
    hipLaunchKernelGGL(inpaint_finish_kernel, dim3(stream_grid((int64_t)n * h * w)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       net_out, ytab, xtab, hole, orient_rgb, mask, n, h, w, ho, wo, out_rgb, orient2);
    MG_CHECK_LAUNCH("mg_inpaint_finish");
    return MG_OK;
}
