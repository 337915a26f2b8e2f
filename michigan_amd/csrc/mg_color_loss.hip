// mg_color_loss.hip -- the image-space L1 terms of the generator objective as one fused pass (reference:
// models/networks/loss.py:388-400 RGBBackgroundL1Loss, :403-532 LabColorLoss, models/pix2pix_model.py:317-336).
//
// The three terms read the same two images: the generated one (NHWC, RGB in channels 0..2, what the generator's last
// convolution wrote) and the target (NCHW fp32, what the loader gives).  Per pixel and image: rgb01 = (x + 1) / 2, XYZ by the
// row-normalised sRGB matrix, f(t) = cbrt(t) above 0.008856 and 7.787 t + 0.137931 below, a = 500 (f(X) - f(Y)),
// b = 200 (f(Y) - f(Z)) -- L never enters the loss and is not computed.
//   color_loss_partial_kernel   per-workgroup partial sums of |da| + |db|, sum_c |dx_c| and sum_c |dx_c * m| into the workspace
//   color_loss_final_kernel     sums the partials in a fixed order in double, scales to the three means (no float atomics:
//                               the result is bit-reproducible from run to run)
//   color_loss_bwd_kernel       dimg = g_lab dlab + g_rgb drgb + g_back dback in the image's dtype and layout, padding channels zero
// The eager spelling is ~40 launches per call, six of them boolean-mask index assignments that synchronise the host; the
// data is ~50 MB per step at 8 x 512^2, so one coalesced read of each operand is all there is to do here.
//
// --balance_Lab (loss.py:484-507) is the same pass with one more operand, the compile-time parameter `Balanced` of the three bodies
// below: the Lab term of a pixel is weighted by w = S[ka][kb] * m, w = 1 where that is 0, with (ka, kb) the bin of the TARGET pixel's
// (a, b) (cl_bin), S the [256][256] fp32 table of michigan_hip/losses/lab_balance.h and m the hair plane.  The gather is 4 bytes per
// pixel from a 256 KiB table that stays in L2.  The unbalanced kernels keep their signatures and their code: their bodies are the
// Balanced = false instantiation, in which the weight does not exist.
#include "michigan_hip/losses/lab_balance.h"
#include "mg_common.h"
#include "mg_launch.h"
#include "mg_lab.h"
#include "mg_reduce.h"

// No fused multiply-add contraction in this file: a - b of two products that are equal must be exactly 0 (sign(0) = 0 where the
// generated pixel equals the target), and a contracted fma(x, y, -round(x * y)) would leave the product's rounding error instead.
#pragma clang fp contract(off)

namespace {

constexpr int CL_BLOCKS = 1024;                                   // rows of the workspace: ws[term * CL_BLOCKS + block]

// bin of one Lab coordinate: trunc(clamp(v + 128, 0, 255)) in fp32 (loss.py:496-499); a NaN lands in bin 0, so the index is always in the table
__device__ __forceinline__ int cl_bin(float v)
{
    float t = v + 128.f;
    t = t > 0.f ? t : 0.f;
    t = t < 255.f ? t : 255.f;
    return (int)t;
}

// the weight of a pixel's Lab term from the target's (a, b): S[ka][kb] * m, and 1 where that is 0 (loss.py:503-505)
__device__ __forceinline__ float cl_weight(const float* __restrict__ table, float ar, float br, float m)
{
    const float w = table[cl_bin(ar) * 256 + cl_bin(br)] * m;
    return w == 0.f ? 1.f : w;
}

template <typename T, bool Balanced>
__device__ __forceinline__ void color_loss_partial_body(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                        const float* __restrict__ back, int64_t back_nstride,
                                                        const float* __restrict__ hair, int64_t hair_nstride, const float* __restrict__ table,
                                                        int N, int64_t HW, int C, int flags, float* __restrict__ ws)
{
    __shared__ float red[3][4];
    float s[3] = {0.f, 0.f, 0.f};                                 // lab, rgb, background
    const int64_t total = (int64_t)N * HW;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / HW);
        const int64_t pix = i - (int64_t)n * HW;
        const float* __restrict__ rp = real + (int64_t)n * real_nstride + pix;
        float xf[3], xr[3];
        cl_load_rgb(img + i * C, C, xf);
        xr[0] = rp[0]; xr[1] = rp[HW]; xr[2] = rp[2 * HW];
        if (flags & 1) {
            float af, bf, ar, br;
            cl_ab(xf, af, bf);
            cl_ab(xr, ar, br);
            if constexpr (Balanced) s[0] += cl_weight(table, ar, br, hair[(int64_t)n * hair_nstride + pix]) * (fabsf(af - ar) + fabsf(bf - br));
            else s[0] += fabsf(af - ar) + fabsf(bf - br);
        }
        if (flags & 2) s[1] += fabsf(xf[0] - xr[0]) + fabsf(xf[1] - xr[1]) + fabsf(xf[2] - xr[2]);
        if (flags & 4) {
            const float m = back[(int64_t)n * back_nstride + pix];
            s[2] += fabsf(xf[0] * m - xr[0] * m) + fabsf(xf[1] * m - xr[1] * m) + fabsf(xf[2] * m - xr[2] * m);
        }
    }
    const float t = mg_block_sum_to<MgJoin::LeftToRight>(s, red);
    if (threadIdx.x < 3) ws[threadIdx.x * CL_BLOCKS + blockIdx.x] = t;
}

template <typename T>
__global__ __launch_bounds__(256) void color_loss_partial_kernel(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                                 const float* __restrict__ back, int64_t back_nstride, int N, int64_t HW, int C,
                                                                 int flags, float* __restrict__ ws)
{
    color_loss_partial_body<T, false>(img, real, real_nstride, back, back_nstride, nullptr, 0, nullptr, N, HW, C, flags, ws);
}

template <typename T>
__global__ __launch_bounds__(256) void color_loss_balanced_partial_kernel(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                                          const float* __restrict__ back, int64_t back_nstride,
                                                                          const float* __restrict__ hair, int64_t hair_nstride,
                                                                          const float* __restrict__ table, int N, int64_t HW, int C, int flags,
                                                                          float* __restrict__ ws)
{
    color_loss_partial_body<T, true>(img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, N, HW, C, flags, ws);
}

__global__ __launch_bounds__(256) void color_loss_final_kernel(const float* __restrict__ ws, int nblk, double inv_lab, double inv_rgb, float* __restrict__ out)
{
    __shared__ double red[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256)
        for (int q = 0; q < 3; ++q) s[q] += (double)ws[q * CL_BLOCKS + i];
    mg_tree_sum_f64(s, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(red[0][0] * inv_lab);                      // nn.L1Loss over Lab channels 1: -> N*2*H*W elements
        out[1] = (float)(red[1][0] * inv_rgb);                      // nn.L1Loss over N*3*H*W
        out[2] = (float)(red[2][0] * inv_rgb);                      // NOT divided by sum(m) (loss.py:393-400)
    }
}

template <typename T, bool Balanced>
__device__ __forceinline__ void color_loss_bwd_body(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                    const float* __restrict__ back, int64_t back_nstride,
                                                    const float* __restrict__ hair, int64_t hair_nstride, const float* __restrict__ table,
                                                    const float* __restrict__ g_lab, const float* __restrict__ g_rgb,
                                                    const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                    T* __restrict__ dimg)
{
    const int64_t total = (int64_t)N * HW;
    // d mean / d element, and the /2 of rgb01 for the Lab chain
    const float gl = (flags & 1) && g_lab ? g_lab[0] * (float)(0.5 / (2.0 * (double)total)) : 0.f;
    const float gr = (flags & 2) && g_rgb ? g_rgb[0] * (float)(1.0 / (3.0 * (double)total)) : 0.f;
    const float gb = (flags & 4) && g_back ? g_back[0] * (float)(1.0 / (3.0 * (double)total)) : 0.f;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / HW);
        const int64_t pix = i - (int64_t)n * HW;
        const float* __restrict__ rp = real + (int64_t)n * real_nstride + pix;
        float xf[3], xr[3], d[3] = {0.f, 0.f, 0.f};
        cl_load_rgb(img + i * C, C, xf);
        xr[0] = rp[0]; xr[1] = rp[HW]; xr[2] = rp[2 * HW];
        if (flags & 1) {
            float xyz[3], ar, br;
            cl_xyz(xf, xyz);
            cl_ab(xr, ar, br);
            float g = gl;
            if constexpr (Balanced) g = gl * cl_weight(table, ar, br, hair[(int64_t)n * hair_nstride + pix]);
            const float fx = cl_f(xyz[0]), fy = cl_f(xyz[1]), fz = cl_f(xyz[2]);
            const float sa = 500.f * cl_sign(500.f * (fx - fy) - ar), sb = 200.f * cl_sign(200.f * (fy - fz) - br);
            // dL/dX, dL/dY, dL/dZ, then through the matrix rows
            const float dX = g * sa * cl_df(xyz[0]), dY = g * (sb - sa) * cl_df(xyz[1]), dZ = -g * sb * cl_df(xyz[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = dX * cl_m(0, c) + dY * cl_m(1, c) + dZ * cl_m(2, c);
        }
        if (flags & 2) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += gr * cl_sign(xf[c] - xr[c]);
        }
        if (flags & 4) {
            const float m = back[(int64_t)n * back_nstride + pix];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += gb * m * cl_sign(xf[c] * m - xr[c] * m);
        }
        cl_store_rgb_grad(dimg + i * C, C, d);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void color_loss_bwd_kernel(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                             const float* __restrict__ back, int64_t back_nstride,
                                                             const float* __restrict__ g_lab, const float* __restrict__ g_rgb,
                                                             const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                             T* __restrict__ dimg)
{
    color_loss_bwd_body<T, false>(img, real, real_nstride, back, back_nstride, nullptr, 0, nullptr, g_lab, g_rgb, g_back, N, HW, C, flags, dimg);
}

template <typename T>
__global__ __launch_bounds__(256) void color_loss_balanced_bwd_kernel(const T* __restrict__ img, const float* __restrict__ real, int64_t real_nstride,
                                                                      const float* __restrict__ back, int64_t back_nstride,
                                                                      const float* __restrict__ hair, int64_t hair_nstride,
                                                                      const float* __restrict__ table,
                                                                      const float* __restrict__ g_lab, const float* __restrict__ g_rgb,
                                                                      const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                                      T* __restrict__ dimg)
{
    color_loss_bwd_body<T, true>(img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, g_lab, g_rgb, g_back, N, HW, C, flags, dimg);
}

}  // namespace

#define MG_COLOR_CHECK(name) \
    MG_CHECK_ARG(dtype == MG_F32 || dtype == MG_BF16, name ": bad dtype"); \
    MG_CHECK_ARG(N > 0 && H > 0 && W > 0 && C >= 3, name ": bad geometry N=%d H=%d W=%d C=%d", N, H, W, C); \
    MG_CHECK_ARG(flags >= 1 && flags <= 7, name ": flags must select at least one of lab (1), rgb (2), background (4)"); \
    MG_CHECK_ARG(real_nstride >= 3 * (int64_t)H * W, name ": the target image needs three dense planes per sample"); \
    MG_CHECK_ARG(!(flags & 4) || (back && back_nstride >= (int64_t)H * W), name ": the background term needs the label plane")

extern "C" int mg_color_loss_fwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                 int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, float* out, float* ws, void* stream)
{
    MG_CHECK_ARG(img && real && out && ws, "mg_color_loss_fwd: null pointer");
    MG_COLOR_CHECK("mg_color_loss_fwd");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int grid = mg_ew_grid((int64_t)N * HW, CL_BLOCKS);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(color_loss_partial_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)img, real, real_nstride, back, back_nstride, N, HW, C, flags, ws); });
    MG_CHECK_LAUNCH("mg_color_loss_fwd");
    const double cnt = (double)N * (double)HW;
    hipLaunchKernelGGL(color_loss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, grid, 1.0 / (2.0 * cnt), 1.0 / (3.0 * cnt), out);
    MG_CHECK_LAUNCH("mg_color_loss_fwd(final)");
    return MG_OK;
}

extern "C" int mg_color_loss_bwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                 const float* g_lab, const float* g_rgb, const float* g_back,
                                 int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream)
{
    MG_CHECK_ARG(img && real && dimg, "mg_color_loss_bwd: null pointer");
    MG_COLOR_CHECK("mg_color_loss_bwd");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int grid = mg_ew_grid((int64_t)N * HW, 4096);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(color_loss_bwd_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)img, real, real_nstride, back, back_nstride, g_lab, g_rgb, g_back, N, HW, C, flags, (T*)dimg); });
    MG_CHECK_LAUNCH("mg_color_loss_bwd");
    return MG_OK;
}

// ---- the balanced entry points (michigan_hip/losses/lab_balance.h): the same launches with the hair plane and the table ----------------
#define MGC_COLOR_CHECK(name) \
    MG_CHECK_ARG(flags & 1, name ": flags must contain lab (1): the table weights the Lab term"); \
    MG_COLOR_CHECK(name); \
    MG_CHECK_ARG(hair && hair_nstride >= (int64_t)H * W, name ": the balanced Lab term needs the hair plane"); \
    MG_CHECK_ARG(table, name ": null pointer (table)")

extern "C" int mgc_color_loss_balanced_fwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                           const float* hair, int64_t hair_nstride, const float* table,
                                           int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, float* out, float* ws, void* stream)
{
    MG_CHECK_ARG(img && real && out && ws, "mgc_color_loss_balanced_fwd: null pointer");
    MGC_COLOR_CHECK("mgc_color_loss_balanced_fwd");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int grid = mg_ew_grid((int64_t)N * HW, CL_BLOCKS);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(color_loss_balanced_partial_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, N, HW, C, flags, ws); });
    MG_CHECK_LAUNCH("mgc_color_loss_balanced_fwd");
    const double cnt = (double)N * (double)HW;
    hipLaunchKernelGGL(color_loss_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, grid, 1.0 / (2.0 * cnt), 1.0 / (3.0 * cnt), out);
    MG_CHECK_LAUNCH("mgc_color_loss_balanced_fwd(final)");
    return MG_OK;
}

extern "C" int mgc_color_loss_balanced_bwd(const void* img, const float* real, int64_t real_nstride, const float* back, int64_t back_nstride,
                                           const float* hair, int64_t hair_nstride, const float* table,
                                           const float* g_lab, const float* g_rgb, const float* g_back,
                                           int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream)
{
    MG_CHECK_ARG(img && real && dimg, "mgc_color_loss_balanced_bwd: null pointer");
    MGC_COLOR_CHECK("mgc_color_loss_balanced_bwd");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int grid = mg_ew_grid((int64_t)N * HW, 4096);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(color_loss_balanced_bwd_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)img, real, real_nstride, back, back_nstride, hair, hair_nstride, table, g_lab, g_rgb, g_back, N, HW, C, flags, (T*)dimg); });
    MG_CHECK_LAUNCH("mgc_color_loss_balanced_bwd");
    return MG_OK;
}
