// mg_orient_dog.hip -- the tail of the orientation loss behind the arg-max kernel when the filter bank is the difference-of-Gaussians
// bank (reference: loss.py:320-349 calOrientationDoG, 352-385 forward, the branch 'gabor' not in opt.orient_filter).  The loss
// extension group, prefix mgl_ (include/michigan_hip/losses/orient_dog.h).
//
// Not the Gabor tail of mg_glue.hip with another constant: the confidence is the response normalised by its maximum over the WHOLE
// batch, the confidence term is an L1 against 1, and the gradient has a second path through that maximum.  With R the clamped maximum
// response, m the hair plane, a = idx * pi / 32 and (l0, l1) the label planes:
//   c1 = R m,   M = max c1 (all samples),   q = c1 / M (one IEEE division),   c = q <= 0 ? 0 : q   (NaN stays NaN: M == 0 gives NaN)
//   orient     = sum(|sin 2a c m - l0 m| + |cos 2a c m - l1 m|) / (2 N HW)
//   confidence = sum |c m - m| / (sum m + 1e-5)
// Forward, three launches, no read-back, no atomics:
//   dog_max_kernel      block maxima of c1 into ws row 0 (a float maximum is order-free)
//   dog_partial_kernel  every workgroup joins the <= 1024 block maxima to M, then accumulates six fp32 terms per thread over a
//                       grid-stride loop and leaves the workgroup's sums (mg_reduce.h: wave tree, four waves left to right) in ws rows 1..6
//   dog_final_kernel    one workgroup: M again from row 0, the six rows in double (thread t takes blocks t, t + 256, ..; halving tree)
// Backward, one launch: per pixel in double from the scalars of the forward's `out`, rounded to fp32 once.
// HBM traffic per pixel: R 4 + idx 1 + label 4 (or 8) + hair 4 bytes read in each pass; the backward writes 4.
#include "mg_common.h"
#include "mg_launch.h"
#include "mg_reduce.h"
#include "michigan_hip/losses/orient_dog.h"

namespace {

constexpr int DOG_BLOCKS = MGL_ORIENT_DOG_BLOCKS;                // rows of the workspace: ws[row * DOG_BLOCKS + block]
constexpr int DOG_TERMS = 6;                                     // |d0| + |d1|, |c m - m|, m, [c1 == M], A, B (rows 1..6)

__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// the workgroup's maximum of v for every thread (256 threads; red is re-usable after the call)
__device__ __forceinline__ float block_max_all(float v, float (&red)[4])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// M from the nblk <= 1024 block maxima.  c1 >= 0 or NaN (fmaxf drops a NaN operand), so 0 is the identity
__device__ __forceinline__ float join_maxima(const float* __restrict__ ws, int nblk, float (&red)[4])
{
    float v = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) v = fmaxf(v, ws[i]);
    return block_max_all(v, red);
}

struct DogPixel { float c1, c, m, f0, f1, d0, d1, e; };          // e = c m - m

__device__ __forceinline__ DogPixel dog_pixel(float R, int idx, const float* __restrict__ label, int label_ch, int64_t HW, int64_t pix,
                                              float m, float M)
{
    DogPixel p;
    p.m = m;
    p.c1 = R * m;
    const float q = __fdiv_rn(p.c1, M);
    p.c = q <= 0.f ? 0.f : q;
    const float ang = (float)idx * (float)(M_PI / 32.0);
    p.f0 = sinf(2.f * ang);
    p.f1 = cosf(2.f * ang);
    float l0, l1;
    if (label_ch == 2) { l0 = label[pix]; l1 = label[HW + pix]; }
    else { const float lab = label[pix] / 255.f * (float)M_PI; l0 = sinf(2.f * lab); l1 = cosf(2.f * lab); }
    p.d0 = p.f0 * p.c * m - l0 * m;
    p.d1 = p.f1 * p.c * m - l1 * m;
    p.e = p.c * m - m;
    return p;
}

__global__ __launch_bounds__(256) void dog_max_kernel(const float* __restrict__ conf_raw, const float* __restrict__ hair, int64_t hair_nstride,
                                                      int N, int64_t HW, float* __restrict__ ws)
{
    __shared__ float red[4];
    const int64_t total = (int64_t)N * HW;
    float v = 0.f;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / HW);
        const int64_t pix = i - (int64_t)n * HW;
        v = fmaxf(v, conf_raw[i] * hair[(int64_t)n * hair_nstride + pix]);
    }
    v = block_max_all(v, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void dog_partial_kernel(const float* __restrict__ conf_raw, const uint8_t* __restrict__ idx,
                                                          const float* __restrict__ label, int label_ch, int64_t label_nstride,
                                                          const float* __restrict__ hair, int64_t hair_nstride, int N, int64_t HW,
                                                          float* __restrict__ ws)
{
    __shared__ float redm[4];
    __shared__ float red[DOG_TERMS][4];
    const float M = join_maxima(ws, (int)gridDim.x, redm);       // the same grid as dog_max_kernel
    float s[DOG_TERMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t total = (int64_t)N * HW;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / HW);
        const int64_t pix = i - (int64_t)n * HW;
        const DogPixel p = dog_pixel(conf_raw[i], idx[i], label + (int64_t)n * label_nstride, label_ch, HW, pix,
                                     hair[(int64_t)n * hair_nstride + pix], M);
        s[0] += fabsf(p.d0) + fabsf(p.d1);
        s[1] += fabsf(p.e);
        s[2] += p.m;
        s[3] += p.c1 == M ? 1.f : 0.f;
        s[4] += (sgnf(p.d0) * p.f0 + sgnf(p.d1) * p.f1) * p.m * p.c1;
        s[5] += sgnf(p.e) * p.m * p.c1;
    }
    const float t = mg_block_sum_to<MgJoin::LeftToRight>(s, red);
    if (threadIdx.x < DOG_TERMS) ws[(threadIdx.x + 1) * DOG_BLOCKS + blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void dog_final_kernel(const float* __restrict__ ws, int nblk, double count, float* __restrict__ out)
{
#pragma clang fp contract(off)                                      // the doubles below are the contract's operations, one rounding each
    __shared__ float redm[4];
    __shared__ double red[DOG_TERMS][256];
    const float M = join_maxima(ws, nblk, redm);
    double s[DOG_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256)
        for (int q = 0; q < DOG_TERMS; ++q) s[q] += (double)ws[(q + 1) * DOG_BLOCKS + i];
    mg_tree_sum_f64(s, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(red[0][0] / count);                        // F.l1_loss over N*2*H*W elements
        out[1] = (float)(red[1][0] / (red[2][0] + 1e-5));           // sum |c m - m| / (sum m + 1e-5)
        out[2] = (float)red[2][0];
        out[3] = M;
        out[4] = (float)red[3][0];
        out[5] = (float)red[4][0];
        out[6] = (float)red[5][0];
        out[7] = 0.f;
    }
}

__global__ __launch_bounds__(256) void dog_bwd_kernel(const float* __restrict__ conf_raw, const uint8_t* __restrict__ idx,
                                                      const float* __restrict__ label, int label_ch, int64_t label_nstride,
                                                      const float* __restrict__ hair, int64_t hair_nstride, const float* __restrict__ g_orient,
                                                      const float* __restrict__ g_conf, const float* __restrict__ fwd_out, int N, int64_t HW,
                                                      float* __restrict__ dconf)
{
#pragma clang fp contract(off)                                      // evaluated in double in the order the header states, rounded once
    const int64_t total = (int64_t)N * HW;
    const float M = fwd_out[3];
    const double Md = (double)M;
    const double g_or = g_orient ? (double)g_orient[0] / (2.0 * (double)total) : 0.0;
    const double g_cf = g_conf ? (double)g_conf[0] / ((double)fwd_out[2] + 1e-5) : 0.0;
    // the path through the maximum: -(sum_j dL/dc_j c1_j) / M^2, split evenly among the pixels that attain M
    const double tie = -((g_or * (double)fwd_out[5] + g_cf * (double)fwd_out[6]) / (Md * Md)) / (double)fwd_out[4];
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i / HW);
        const int64_t pix = i - (int64_t)n * HW;
        const DogPixel p = dog_pixel(conf_raw[i], idx[i], label + (int64_t)n * label_nstride, label_ch, HW, pix,
                                     hair[(int64_t)n * hair_nstride + pix], M);
        const double md = (double)p.m;
        const double dc = g_or * (double)(sgnf(p.d0) * p.f0 + sgnf(p.d1) * p.f1) * md + g_cf * (double)sgnf(p.e) * md;
        double d = p.c > 0.f ? dc * md / Md : 0.0;
        if (p.c1 == M) d += tie * md;
        dconf[i] = (float)d;
    }
}

bool dog_args_ok(int32_t label_ch, int64_t label_nstride, int64_t hair_nstride, int32_t N, int64_t HW)
{
    return (label_ch == 1 || label_ch == 2) && N > 0 && HW > 0 && HW < (1ll << 31) &&
           (N == 1 || (label_nstride >= (int64_t)label_ch * HW && hair_nstride >= HW));      // a stride is not read for one sample
}

}  // namespace

extern "C" int mgl_orient_dog_fwd(const float* conf_raw, const uint8_t* idx, const float* label, int32_t label_ch, int64_t label_nstride,
                                  const float* hair, int64_t hair_nstride, int32_t N, int64_t HW, float* out, float* ws, void* stream)
{
    MG_CHECK_ARG(conf_raw && idx && label && hair && out && ws, "mgl_orient_dog_fwd: null pointer");
    MG_CHECK_ARG(dog_args_ok(label_ch, label_nstride, hair_nstride, N, HW), "mgl_orient_dog_fwd: bad geometry");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int grid = mg_ew_grid((int64_t)N * HW, DOG_BLOCKS);
    hipLaunchKernelGGL(dog_max_kernel, dim3(grid), dim3(256), 0, st, conf_raw, hair, hair_nstride, N, HW, ws);
    MG_CHECK_LAUNCH("mgl_orient_dog_fwd(max)");
    hipLaunchKernelGGL(dog_partial_kernel, dim3(grid), dim3(256), 0, st, conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, N, HW, ws);
    MG_CHECK_LAUNCH("mgl_orient_dog_fwd");
    hipLaunchKernelGGL(dog_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, grid, 2.0 * (double)N * (double)HW, out);
    MG_CHECK_LAUNCH("mgl_orient_dog_fwd(final)");
    return MG_OK;
}

extern "C" int mgl_orient_dog_bwd(const float* conf_raw, const uint8_t* idx, const float* label, int32_t label_ch, int64_t label_nstride,
                                  const float* hair, int64_t hair_nstride, const float* g_orient, const float* g_conf, const float* fwd_out,
                                  int32_t N, int64_t HW, float* dconf, void* stream)
{
    MG_CHECK_ARG(conf_raw && idx && label && hair && fwd_out && dconf, "mgl_orient_dog_bwd: null pointer");
    MG_CHECK_ARG(dog_args_ok(label_ch, label_nstride, hair_nstride, N, HW), "mgl_orient_dog_bwd: bad geometry");
    hipLaunchKernelGGL(dog_bwd_kernel, dim3(mg_ew_grid((int64_t)N * HW, 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       conf_raw, idx, label, label_ch, label_nstride, hair, hair_nstride, g_orient, g_conf, fwd_out, N, HW, dconf);
    MG_CHECK_LAUNCH("mgl_orient_dog_bwd");
    return MG_OK;
}
