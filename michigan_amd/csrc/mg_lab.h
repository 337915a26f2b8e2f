// mg_lab.h -- RGB in [-1, 1] -> CIE Lab (a, b) as the reference spells it (models/networks/loss.py:409-482, :540-570), shared by the
// image-space loss passes (mg_color_loss.hip, mg_hair_lab.hip).  Per pixel: rgb01 = (x + 1) / 2, XYZ by the row-normalised sRGB matrix,
// f(t) = cbrt(t) above 0.008856 and 7.787 t + 0.137931 below, a = 500 (f(X) - f(Y)), b = 200 (f(Y) - f(Z)); L never enters a loss and is
// not computed.
#pragma once
#include "mg_common.h"

// No fused multiply-add contraction in these functions (nor, from here on, in the file that includes this header): a - b of two
// products that are equal must be exactly 0, and the two users must compute bit-identical (a, b) for the same pixel.
#pragma clang fp contract(off)

namespace {

constexpr float CL_KNEE = 0.008856f, CL_LIN = 7.787f, CL_OFF = 0.137931f;
// loss.py:409 (an fp32 tensor there, hence the f suffixes), each row divided by its row sum (rgb2xyz, loss.py:446-464)
constexpr float CL_M[3][3] = {{0.412453f, 0.357580f, 0.180423f}, {0.212671f, 0.715160f, 0.072169f}, {0.019334f, 0.119193f, 0.950227f}};
constexpr float cl_m(int r, int c) { return (float)((double)CL_M[r][c] / ((double)CL_M[r][0] + (double)CL_M[r][1] + (double)CL_M[r][2])); }

__device__ __forceinline__ float cl_f(float t) { return t > CL_KNEE ? cbrtf(t) : CL_LIN * t + CL_OFF; }
__device__ __forceinline__ float cl_df(float t) { if (t > CL_KNEE) { const float c = cbrtf(t); return 1.f / (3.f * c * c); } return CL_LIN; }
__device__ __forceinline__ float cl_sign(float u) { return u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ void cl_xyz(const float x[3], float xyz[3])
{
    const float r = (x[0] + 1.f) * 0.5f, g = (x[1] + 1.f) * 0.5f, b = (x[2] + 1.f) * 0.5f;
    xyz[0] = cl_m(0, 0) * r + cl_m(0, 1) * g + cl_m(0, 2) * b;
    xyz[1] = cl_m(1, 0) * r + cl_m(1, 1) * g + cl_m(1, 2) * b;
    xyz[2] = cl_m(2, 0) * r + cl_m(2, 1) * g + cl_m(2, 2) * b;
}

__device__ __forceinline__ void cl_ab(const float x[3], float& a, float& b)
{
    float xyz[3];
    cl_xyz(x, xyz);
    const float fx = cl_f(xyz[0]), fy = cl_f(xyz[1]), fz = cl_f(xyz[2]);
    a = 500.f * (fx - fy);
    b = 200.f * (fy - fz);
}

// RGB of one generated pixel: one 8- or 16-byte load when the pixel is quad-aligned (the generator's padded output), else three scalars
template <typename T>
__device__ __forceinline__ void cl_load_rgb(const T* __restrict__ p, int C, float x[3])
{
    if ((C & 3) == 0) { const f32x4_t v = ET<T>::load4(p); x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; }
    else { x[0] = ET<T>::load1(p); x[1] = ET<T>::load1(p + 1); x[2] = ET<T>::load1(p + 2); }
}

// the gradient of one generated pixel: d in channels 0..2, zero in the padding channels; quads when the pixel is quad-aligned
template <typename T>
__device__ __forceinline__ void cl_store_rgb_grad(T* __restrict__ o, int C, const float d[3])
{
    if ((C & 3) == 0) {
        const f32x4_t v = {d[0], d[1], d[2], 0.f}, z = {0.f, 0.f, 0.f, 0.f};
        ET<T>::store4(o, v);
        for (int c = 4; c < C; c += 4) ET<T>::store4(o + c, z);
    } else {
        ET<T>::store1(o, d[0]); ET<T>::store1(o + 1, d[1]); ET<T>::store1(o + 2, d[2]);
        for (int c = 3; c < C; ++c) ET<T>::store1(o + c, 0.f);
    }
}

}  // namespace
