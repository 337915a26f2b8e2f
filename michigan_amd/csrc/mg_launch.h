// Host-side launch helpers shared by the streaming kernel files (include after mg_common.h): the dtype dispatch, the block size
// and grid of a grid-stride pass, a runtime flag as a template argument, and the activation's slope factor.  Prefixed: mg_conv_common.h and mg_inputs.hip keep an
// NTHR / ew_grid of their own.
#pragma once
#include "mg_common.h"
#include <type_traits>

constexpr int MG_NTHR = 256;
// blocks of MG_NTHR threads for n work items, at least one and at most `cap` (the kernel strides over the rest)
static inline int mg_ew_grid(int64_t n, int cap) { int64_t b = (n + MG_NTHR - 1) / MG_NTHR; return (int)(b > cap ? cap : (b < 1 ? 1 : b)); }

#define MG_GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// f(tag) with tag::type = uint16_t (MG_BF16) or float (anything else: the entry point has checked dtype).  A call site is
//     mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type; hipLaunchKernelGGL(kern<T>, ..., (const T*)x, ...); });
// so the argument list of a launch exists once.  The bf16 branch comes first: kernels are emitted in order of first use.
template <typename T> struct mg_dtype_tag { using type = T; };
template <typename F> static inline auto mg_by_dtype(int dtype, F&& f)
{
    if (dtype == MG_BF16) return f(mg_dtype_tag<uint16_t>{});
    return f(mg_dtype_tag<float>{});
}

// f(std::true_type) or f(std::false_type): a runtime flag as a template argument (the true branch first, like mg_by_dtype)
template <typename F> static inline void mg_by_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// derivative factor of NONE / RELU / LRELU through the output: y > 0 ? 1 : mg_neg_slope(act, slope)
__host__ __device__ static __forceinline__ float mg_neg_slope(int act, float slope)
{
    return act == MG_ACT_NONE ? 1.f : (act == MG_ACT_RELU ? 0.f : slope);
}
__device__ __forceinline__ float mg_act_factor(float y, float neg) { return y > 0.f ? 1.f : neg; }
