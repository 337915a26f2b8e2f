// mg_reduce.h -- the fixed-order sums behind every scalar loss and norm.  The summation ORDER is part
// of the contract: a loss is bit-reproducible from run to run, and the spectral-norm scalars are bit-identical on every rank of a
// data-parallel job.  A kernel's sum is a thread's own sequential (strided) sum, then these, and nothing here reorders:
//   mg_wave_sum        64 lanes -> lane 0, the tree o = 32, 16, ..., 1:  v[l] += v[l ^ o]
//   mg_join            the NW wave sums of a workgroup, MgJoin::LeftToRight ((w0 + w1) + w2) + w3 ... or MgJoin::Pairwise
//                      (w0 + w1) + (w2 + w3) (mg_feat_moments.hip, four waves)
//   mg_put_wave_sums   K terms: lane 0 of every wave leaves its wave sums in LDS (no barrier: for a caller that joins by hand)
//   mg_block_sum_to    K terms: thread q < K gets the workgroup's sum of term q (one barrier); one term: thread 0 gets it
//   mg_block_sum_all   one term: every thread gets the workgroup's sum (two barriers; the scratch is re-usable after the call)
//   mg_tree_sum_f64    K terms (or one) over NT = 256 or 1024 threads in double: red[q][t] += red[q][t + o], o = NT / 2, ..., 1
// LeftToRight is spelt w0 + w1 + ... here and was `t = 0; t += w0; ...` in places: the same bits.  Every per-thread accumulator
// starts at +0, and a sum that starts at +0 is never -0 (round to nearest: x + y is -0 only for x = y = -0), so no wave sum is -0
// and 0 + w0 is w0.
#pragma once
#include "mg_common.h"

enum class MgJoin { LeftToRight, Pairwise };

// sum over the wave; defined for lane 0 only (the other lanes end with the same terms in another order)
template <typename T>
__device__ __forceinline__ T mg_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <MgJoin J, int NW, typename T>
__device__ __forceinline__ T mg_join(const T (&w)[NW])
{
    if constexpr (J == MgJoin::Pairwise) {
        static_assert(NW == 4, "the pairwise join is defined for four waves");
        return (w[0] + w[1]) + (w[2] + w[3]);
    } else {
        T t = w[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) t += w[i];
        return t;
    }
}

// lane 0 of every wave leaves the wave's sum of term q in red[q][wave]; the caller's barrier comes before a join
template <int K, int NW, typename T>
__device__ __forceinline__ void mg_put_wave_sums(const T (&v)[K], T (&red)[K][NW])
{
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const T s = mg_wave_sum(v[q]);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s;
    }
}

// thread q < K returns the workgroup's sum of term q, the others 0 (NW waves; one barrier, after the wave sums are in red)
template <MgJoin J, int K, int NW, typename T>
__device__ __forceinline__ T mg_block_sum_to(const T (&v)[K], T (&red)[K][NW])
{
    mg_put_wave_sums(v, red);
    __syncthreads();
    return (int)threadIdx.x < K ? mg_join<J>(red[threadIdx.x]) : T(0);
}

template <MgJoin J, int NW, typename T>
__device__ __forceinline__ T mg_block_sum_to(T v, T (&red)[NW]) { const T one[1] = {v}; return mg_block_sum_to<J>(one, reinterpret_cast<T (&)[1][NW]>(red)); }

// every thread returns the workgroup's sum.  The leading barrier lets a second call re-use red
template <MgJoin J, int NW, typename T>
__device__ __forceinline__ T mg_block_sum_all(T v, T (&red)[NW])
{
    v = mg_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return mg_join<J>(red);
}

// thread t of NT brings s[q]; red[q][0] is the sum of term q when this returns (after a barrier: any thread may read it)
template <int NT, int K>
__device__ __forceinline__ void mg_tree_sum_f64(const double (&s)[K], double (&red)[K][NT])
{
    static_assert(NT == 256 || NT == 1024, "one halving tree per workgroup size in use");
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < K; ++q) red[q][t] = s[q];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int q = 0; q < K; ++q) red[q][t] += red[q][t + o];
        }
        __syncthreads();
    }
}

template <int NT>      // one term: red[0] is the sum
__device__ __forceinline__ void mg_tree_sum_f64(double s, double (&red)[NT]) { const double one[1] = {s}; mg_tree_sum_f64(one, reinterpret_cast<double (&)[1][NT]>(red)); }
