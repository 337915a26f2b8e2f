// mg_hair_lab.hip -- the two image-space terms of the unpaired training stage (curr_step = 2) as one fused pass (reference:
// models/networks/loss.py:534-621 HairAvgLabLoss, :388-400 RGBBackgroundL1Loss, called at models/pix2pix_model.py:352-363).
//
// hairAvgLab compares the MEAN Lab (a, b) colour of the generated hair inside the target's hair mask with the mean colour of the
// reference image's hair inside the reference's mask, one pair of means per sample -- a per-sample reduction the colour pass
// (mg_color_loss.hip) does not have; background is that pass's bit 2, computed here beside it so that the generated image is read
// once forward and once backward for the whole step-2 objective.
//   hair_lab_partial_kernel   2-D grid (blocks of a sample, sample): per-workgroup partial sums of m_f, m_f a, m_f b, m_r, m_r a,
//                             m_r b and sum_c |x_c m_b - t_c m_b| into the workspace; a workgroup never crosses a sample boundary
//   hair_lab_final_kernel     one wave per sample sums its partials in a fixed order in double (no float atomics: bit-reproducible),
//                             forms da, db, writes them and 1 / S_f to `stats` for the backward, then the two means
//   hair_lab_bwd_kernel       dimg in the image's dtype and layout, padding channels zero; reads `stats`, reduces nothing
// What is provably zero is not read: img only where m_f != 0 (bit 0) or m_b != 0 (bit 1), ref only where m_r != 0, tgt only where
// m_b != 0 -- with a one-hot label every pixel takes exactly one of the two branches.
//
// --balance_Lab (loss.py:578-600, 614-618) changes the per-sample tail alone: the final kernel looks the sample's weight w_n up in the
// [256][256] fp32 table of michigan_hip/losses/lab_balance.h at the bin of the REFERENCE image's mean hair colour (the mean rounded to
// fp32, + 128.f, clamped, truncated; no zero-to-one replacement, so a zero of the table gives weight 0), sums w_n (|da_n| + |db_n|)
// and leaves w_n in a `stats` row of MGC_HAIR_STATS floats; the backward multiplies its per-sample scale by it.  `Balanced` is a
// compile-time parameter of the two bodies; the unbalanced kernels keep their signatures and their code.
#include "michigan_hip/losses/lab_balance.h"
#include "mg_common.h"
#include "mg_launch.h"
#include "mg_lab.h"
#include "mg_reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int HL_BLOCKS = 1024;                                   // forward workgroups over all samples (when N <= HL_BLOCKS)
constexpr int HL_TERMS = 7;                                       // ws[(term * N + n) * bps + block]

inline int hl_bps(int64_t HW, int N, int cap)
{
    const int64_t need = (HW + 255) / 256, room = cap / N > 0 ? cap / N : 1;
    return (int)(need < room ? need : room);
}

template <typename T>
__global__ __launch_bounds__(256) void hair_lab_partial_kernel(const T* __restrict__ img, const float* __restrict__ ref, int64_t ref_nstride,
                                                               const float* __restrict__ mf, int64_t mf_nstride,
                                                               const float* __restrict__ mr, int64_t mr_nstride,
                                                               const float* __restrict__ tgt, int64_t tgt_nstride,
                                                               const float* __restrict__ back, int64_t back_nstride,
                                                               int N, int64_t HW, int C, int flags, float* __restrict__ ws)
{
    __shared__ float red[HL_TERMS][4];
    float s[HL_TERMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int n = blockIdx.y;
    const T* __restrict__ ip = img + (int64_t)n * HW * C;
    for (int64_t pix = blockIdx.x * 256LL + threadIdx.x; pix < HW; pix += (int64_t)gridDim.x * 256) {
        const float vf = (flags & 1) ? mf[(int64_t)n * mf_nstride + pix] : 0.f;
        const float vr = (flags & 1) ? mr[(int64_t)n * mr_nstride + pix] : 0.f;
        const float vb = (flags & 2) ? back[(int64_t)n * back_nstride + pix] : 0.f;
        float xf[3];
        if (vf != 0.f || vb != 0.f) cl_load_rgb(ip + pix * C, C, xf);
        if (vf != 0.f) {
            float a, b;
            cl_ab(xf, a, b);
            s[0] += vf; s[1] += vf * a; s[2] += vf * b;
        }
        if (vr != 0.f) {
            const float* __restrict__ rp = ref + (int64_t)n * ref_nstride + pix;
            const float xr[3] = {rp[0], rp[HW], rp[2 * HW]};
            float a, b;
            cl_ab(xr, a, b);
            s[3] += vr; s[4] += vr * a; s[5] += vr * b;
        }
        if (vb != 0.f) {
            const float* __restrict__ tp = tgt + (int64_t)n * tgt_nstride + pix;
            s[6] += fabsf(xf[0] * vb - tp[0] * vb) + fabsf(xf[1] * vb - tp[HW] * vb) + fabsf(xf[2] * vb - tp[2 * HW] * vb);
        }
    }
    const float t = mg_block_sum_to<MgJoin::LeftToRight>(s, red);
    if (threadIdx.x < HL_TERMS) ws[((int64_t)threadIdx.x * N + n) * gridDim.x + blockIdx.x] = t;
}

// bin of one mean Lab coordinate: the double mean rounded to fp32, then trunc(clamp(v + 128, 0, 255)) in fp32 (loss.py:590-594)
__device__ __forceinline__ int hl_bin(double mean)
{
    float t = (float)mean + 128.f;
    t = t > 0.f ? t : 0.f;
    t = t < 255.f ? t : 255.f;
    return (int)t;
}

// one workgroup; wave w owns samples w, w + 4, ...: lanes stride over the sample's partials, a fixed shuffle tree joins them
template <bool Balanced>
__device__ __forceinline__ void hair_lab_final_body(const float* __restrict__ ws, const float* __restrict__ table, int N, int bps, int flags,
                                                    double inv_hair, double inv_back, float* __restrict__ stats, float* __restrict__ out)
{
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double hair = 0.0, bg = 0.0;
    for (int n = wave; n < N; n += 4) {
        double s[HL_TERMS];
#pragma unroll
        for (int q = 0; q < HL_TERMS; ++q) {
            double t = 0.0;
            for (int i = lane; i < bps; i += 64) t += (double)ws[((int64_t)q * N + n) * bps + i];
            s[q] = mg_wave_sum(t);
        }
        if (lane == 0) {
            if (flags & 1) {
                const double sf = s[0] == 0.0 ? 1.0 : s[0], sr = s[3] == 0.0 ? 1.0 : s[3];      // mask_sum[mask_sum == 0] = 1 (loss.py:575)
                const double da = s[1] / sf - s[4] / sr, db = s[2] / sf - s[5] / sr;
                const f32x4_t v = {(float)da, (float)db, (float)(1.0 / sf), (float)(1.0 / sr)};
                if constexpr (Balanced) {
                    const float w = table[hl_bin(s[4] / sr) * 256 + hl_bin(s[5] / sr)];
                    hair += (double)w * (fabs(da) + fabs(db));
                    const f32x4_t v1 = {w, 0.f, 0.f, 0.f};
                    ET<float>::store4(stats + MGC_HAIR_STATS * (int64_t)n, v);
                    ET<float>::store4(stats + MGC_HAIR_STATS * (int64_t)n + 4, v1);
                } else {
                    hair += fabs(da) + fabs(db);
                    ET<float>::store4(stats + 4 * (int64_t)n, v);
                }
            }
            bg += s[6];
        }
    }
    if (lane == 0) { red[0][wave] = hair; red[1][wave] = bg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (float)(mg_join<MgJoin::LeftToRight>(red[0]) * inv_hair);                  // nn.L1Loss over [N, 2, 1, 1]
        out[1] = (float)(mg_join<MgJoin::LeftToRight>(red[1]) * inv_back);                  // mean over N*3*H*W, not divided by sum(m_b)
    }
}

__global__ __launch_bounds__(256) void hair_lab_final_kernel(const float* __restrict__ ws, int N, int bps, int flags, double inv_hair, double inv_back,
                                                             float* __restrict__ stats, float* __restrict__ out)
{
    hair_lab_final_body<false>(ws, nullptr, N, bps, flags, inv_hair, inv_back, stats, out);
}

__global__ __launch_bounds__(256) void hair_lab_balanced_final_kernel(const float* __restrict__ ws, const float* __restrict__ table, int N, int bps,
                                                                      int flags, double inv_hair, double inv_back, float* __restrict__ stats,
                                                                      float* __restrict__ out)
{
    hair_lab_final_body<true>(ws, table, N, bps, flags, inv_hair, inv_back, stats, out);
}

template <typename T, bool Balanced>
__device__ __forceinline__ void hair_lab_bwd_body(const T* __restrict__ img, const float* __restrict__ mf, int64_t mf_nstride,
                                                  const float* __restrict__ tgt, int64_t tgt_nstride,
                                                  const float* __restrict__ back, int64_t back_nstride,
                                                  const float* __restrict__ stats, const float* __restrict__ g_hair,
                                                  const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                  T* __restrict__ dimg)
{
    const int n = blockIdx.y;
    const bool hair = (flags & 1) && g_hair, bgt = (flags & 2) && g_back;
    float sa = 0.f, sb = 0.f, gl = 0.f;
    if (hair) {
        const f32x4_t st = ET<float>::load4(stats + (Balanced ? MGC_HAIR_STATS : 4) * (int64_t)n);
        sa = 500.f * cl_sign(st[0]);
        sb = 200.f * cl_sign(st[1]);
        gl = g_hair[0] * (float)(0.5 / (2.0 * (double)N)) * st[2];    // d mean / d element, the /2 of rgb01, 1 / S_f
        if constexpr (Balanced) gl = gl * stats[MGC_HAIR_STATS * (int64_t)n + 4];           // ... and the sample's weight
    }
    const float gb = bgt ? g_back[0] * (float)(1.0 / (3.0 * (double)N * (double)HW)) : 0.f;
    const T* __restrict__ ip = img + (int64_t)n * HW * C;
    T* __restrict__ op = dimg + (int64_t)n * HW * C;
    for (int64_t pix = blockIdx.x * 256LL + threadIdx.x; pix < HW; pix += (int64_t)gridDim.x * 256) {
        const float vf = hair ? mf[(int64_t)n * mf_nstride + pix] : 0.f;
        const float vb = bgt ? back[(int64_t)n * back_nstride + pix] : 0.f;
        float xf[3], d[3] = {0.f, 0.f, 0.f};
        if (vf != 0.f || vb != 0.f) cl_load_rgb(ip + pix * C, C, xf);
        if (vf != 0.f) {
            float xyz[3];
            cl_xyz(xf, xyz);
            const float g = gl * vf;
            // dL/dX, dL/dY, dL/dZ, then through the matrix rows
            const float dX = g * sa * cl_df(xyz[0]), dY = g * (sb - sa) * cl_df(xyz[1]), dZ = -g * sb * cl_df(xyz[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = dX * cl_m(0, c) + dY * cl_m(1, c) + dZ * cl_m(2, c);
        }
        if (vb != 0.f) {
            const float* __restrict__ tp = tgt + (int64_t)n * tgt_nstride + pix;
            const float xr[3] = {tp[0], tp[HW], tp[2 * HW]};
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += gb * vb * cl_sign(xf[c] * vb - xr[c] * vb);
        }
        cl_store_rgb_grad(op + pix * C, C, d);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void hair_lab_bwd_kernel(const T* __restrict__ img, const float* __restrict__ mf, int64_t mf_nstride,
                                                           const float* __restrict__ tgt, int64_t tgt_nstride,
                                                           const float* __restrict__ back, int64_t back_nstride,
                                                           const float* __restrict__ stats, const float* __restrict__ g_hair,
                                                           const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                           T* __restrict__ dimg)
{
    hair_lab_bwd_body<T, false>(img, mf, mf_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back, N, HW, C, flags, dimg);
}

template <typename T>
__global__ __launch_bounds__(256) void hair_lab_balanced_bwd_kernel(const T* __restrict__ img, const float* __restrict__ mf, int64_t mf_nstride,
                                                                    const float* __restrict__ tgt, int64_t tgt_nstride,
                                                                    const float* __restrict__ back, int64_t back_nstride,
                                                                    const float* __restrict__ stats, const float* __restrict__ g_hair,
                                                                    const float* __restrict__ g_back, int N, int64_t HW, int C, int flags,
                                                                    T* __restrict__ dimg)
{
    hair_lab_bwd_body<T, true>(img, mf, mf_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back, N, HW, C, flags, dimg);
}

}  // namespace

#define MG_HAIR_CHECK(name) \
    MG_CHECK_ARG(dtype == MG_F32 || dtype == MG_BF16, name ": bad dtype"); \
    MG_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && C >= 3, name ": bad geometry N=%d H=%d W=%d C=%d", N, H, W, C); \
    MG_CHECK_ARG(flags >= 1 && flags <= 3, name ": flags must select at least one of hairAvgLab (1), background (2)"); \
    MG_CHECK_ARG(!(flags & 1) || (hair_tag && hair_tag_nstride >= (int64_t)H * W), name ": the hairAvgLab term needs the tag hair plane"); \
    MG_CHECK_ARG(!(flags & 2) || (tgt && tgt_nstride >= 3 * (int64_t)H * W), name ": the background term needs three dense planes per sample of the target image"); \
    MG_CHECK_ARG(!(flags & 2) || (back && back_nstride >= (int64_t)H * W), name ": the background term needs the label plane")

extern "C" int mg_hair_lab_fwd(const void* img, const float* ref, int64_t ref_nstride, const float* hair_tag, int64_t hair_tag_nstride,
                               const float* hair_ref, int64_t hair_ref_nstride, const float* tgt, int64_t tgt_nstride,
                               const float* back, int64_t back_nstride, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                               int32_t flags, float* out, float* stats, float* ws, void* stream)
{
    MG_CHECK_ARG(img && out, "mg_hair_lab_fwd: null pointer");
    MG_HAIR_CHECK("mg_hair_lab_fwd");
    MG_CHECK_ARG(!(flags & 1) || stats, "mg_hair_lab_fwd: null pointer (stats)");
    MG_CHECK_ARG(!(flags & 1) || (ref && ref_nstride >= 3 * (int64_t)H * W), "mg_hair_lab_fwd: the hairAvgLab term needs three dense planes per sample of the reference image");
    MG_CHECK_ARG(!(flags & 1) || (hair_ref && hair_ref_nstride >= (int64_t)H * W), "mg_hair_lab_fwd: the hairAvgLab term needs the reference hair plane");
    MG_CHECK_ARG(ws, "mg_hair_lab_fwd: null pointer (ws)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int bps = hl_bps(HW, N, HL_BLOCKS);
    const dim3 grid(bps, N);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(hair_lab_partial_kernel<T>, grid, dim3(256), 0, st, (const T*)img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride, back, back_nstride, N, HW, C, flags, ws); });
    MG_CHECK_LAUNCH("mg_hair_lab_fwd");
    hipLaunchKernelGGL(hair_lab_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, N, bps, flags, 1.0 / (2.0 * (double)N), 1.0 / (3.0 * (double)N * (double)HW), stats, out);
    MG_CHECK_LAUNCH("mg_hair_lab_fwd(final)");
    return MG_OK;
}

extern "C" int mg_hair_lab_bwd(const void* img, const float* hair_tag, int64_t hair_tag_nstride, const float* tgt, int64_t tgt_nstride,
                               const float* back, int64_t back_nstride, const float* stats, const float* g_hair, const float* g_back,
                               int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream)
{
    MG_CHECK_ARG(img && dimg, "mg_hair_lab_bwd: null pointer");
    MG_HAIR_CHECK("mg_hair_lab_bwd");
    MG_CHECK_ARG(!(flags & 1) || stats, "mg_hair_lab_bwd: null pointer (stats)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const dim3 grid(hl_bps(HW, N, 4096), N);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(hair_lab_bwd_kernel<T>, grid, dim3(256), 0, st, (const T*)img, hair_tag, hair_tag_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back, N, HW, C, flags, (T*)dimg); });
    MG_CHECK_LAUNCH("mg_hair_lab_bwd");
    return MG_OK;
}

// ---- the balanced entry points (michigan_hip/losses/lab_balance.h): the same partial pass, the weighted tail -----------------------------
#define MGC_HAIR_CHECK(name) \
    MG_CHECK_ARG(flags & 1, name ": flags must contain hairAvgLab (1): the table weights that term"); \
    MG_HAIR_CHECK(name); \
    MG_CHECK_ARG(stats, name ": null pointer (stats)")

extern "C" int mgc_hair_lab_balanced_fwd(const void* img, const float* ref, int64_t ref_nstride, const float* hair_tag, int64_t hair_tag_nstride,
                                         const float* hair_ref, int64_t hair_ref_nstride, const float* tgt, int64_t tgt_nstride,
                                         const float* back, int64_t back_nstride, const float* table, int32_t dtype, int32_t N, int32_t H, int32_t W,
                                         int32_t C, int32_t flags, float* out, float* stats, float* ws, void* stream)
{
    MG_CHECK_ARG(img && out && ws && table, "mgc_hair_lab_balanced_fwd: null pointer");
    MGC_HAIR_CHECK("mgc_hair_lab_balanced_fwd");
    MG_CHECK_ARG(ref && ref_nstride >= 3 * (int64_t)H * W, "mgc_hair_lab_balanced_fwd: the hairAvgLab term needs three dense planes per sample of the reference image");
    MG_CHECK_ARG(hair_ref && hair_ref_nstride >= (int64_t)H * W, "mgc_hair_lab_balanced_fwd: the hairAvgLab term needs the reference hair plane");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int bps = hl_bps(HW, N, HL_BLOCKS);
    const dim3 grid(bps, N);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(hair_lab_partial_kernel<T>, grid, dim3(256), 0, st, (const T*)img, ref, ref_nstride, hair_tag, hair_tag_nstride, hair_ref, hair_ref_nstride, tgt, tgt_nstride, back, back_nstride, N, HW, C, flags, ws); });
    MG_CHECK_LAUNCH("mgc_hair_lab_balanced_fwd");
    hipLaunchKernelGGL(hair_lab_balanced_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, table, N, bps, flags, 1.0 / (2.0 * (double)N), 1.0 / (3.0 * (double)N * (double)HW), stats, out);
    MG_CHECK_LAUNCH("mgc_hair_lab_balanced_fwd(final)");
    return MG_OK;
}

extern "C" int mgc_hair_lab_balanced_bwd(const void* img, const float* hair_tag, int64_t hair_tag_nstride, const float* tgt, int64_t tgt_nstride,
                                         const float* back, int64_t back_nstride, const float* stats, const float* g_hair, const float* g_back,
                                         int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flags, void* dimg, void* stream)
{
    MG_CHECK_ARG(img && dimg, "mgc_hair_lab_balanced_bwd: null pointer");
    MGC_HAIR_CHECK("mgc_hair_lab_balanced_bwd");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const dim3 grid(hl_bps(HW, N, 4096), N);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(hair_lab_balanced_bwd_kernel<T>, grid, dim3(256), 0, st, (const T*)img, hair_tag, hair_tag_nstride, tgt, tgt_nstride, back, back_nstride, stats, g_hair, g_back, N, HW, C, flags, (T*)dimg); });
    MG_CHECK_LAUNCH("mgc_hair_lab_balanced_bwd");
    return MG_OK;
}
