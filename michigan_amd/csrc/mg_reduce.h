// mg_reduce.h -- the fixed-order sums behind every scalar loss and norm, and behind the per-channel (column) sums of the
// normalisation statistics, the norm backward reduction and the style moments.  The summation ORDER is part
// of the contract: a loss is bit-reproducible from run to run, and the spectral-norm scalars are bit-identical on every rank of a
// data-parallel job.  A kernel's sum is a thread's own sequential (strided) sum, then these, and nothing here reorders:
//   mg_wave_sum        64 lanes -> lane 0, the tree o = 32, 16, ..., 1:  v[l] += v[l ^ o]
//   mg_join            the NW wave sums of a workgroup, MgJoin::LeftToRight ((w0 + w1) + w2) + w3 ... or MgJoin::Pairwise
//                      (w0 + w1) + (w2 + w3) (mg_feat_moments.hip, four waves)
//   mg_put_wave_sums   K terms: lane 0 of every wave leaves its wave sums in LDS (no barrier: for a caller that joins by hand)
//   mg_block_sum_to    K terms: thread q < K gets the workgroup's sum of term q (one barrier); one term: thread 0 gets it
//   mg_block_sum_all   one term: every thread gets the workgroup's sum (two barriers; the scratch is re-usable after the call)
//   mg_tree_sum_f64    K terms (or one) over NT = 256 or 1024 threads in double: red[q][t] += red[q][t + o], o = NT / 2, ..., 1
// Column sums (NHWC: one sum per channel over pixels), `rows` thread rows of cv threads, thread tr * cv + tq owns W channels:
//   a thread's own sum   pixels p0 + tr, p0 + tr + rows, ... of the workgroup's chunk, sequentially from +0 (the kernel's loop)
//   mg_row_join          K terms: row 0 gets own + row 1 + row 2 + ... + row rows-1 per channel, read from LDS in ascending row
//                        order after one barrier (mg_rows_put / mg_rows_fold are its two halves, for a caller that places the barrier)
//   mg_chunk_sum_f64     thread row k of 8 adds chunk partials k, k + 8, ... of one column in double, ascending
//   mg_chunk_rows_join   8 rows x 32 columns: row 0 gets own + row 1 + ... + row 7 in double (one barrier)
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

// ---- column sums ----
// K terms of W channels each, v[q] -> the W sums of term q: this thread's sums -> red[thread][K][W]; the caller's barrier comes
// before a fold
template <int K, int W>
__device__ __forceinline__ void mg_rows_put(float* const (&v)[K], float* red)
{
#pragma unroll
    for (int q = 0; q < K; ++q)
#pragma unroll
        for (int j = 0; j < W; ++j) red[(threadIdx.x * K + q) * W + j] = v[q][j];
}

// for a thread of row 0 (threadIdx.x < cv): v[q][j] += rows 1 .. rows-1 of the same term and channel, ascending
template <int K, int W>
__device__ __forceinline__ void mg_rows_fold(float* const (&v)[K], const float* red, int cv, int rows)
{
    for (int r = 1; r < rows; ++r) {
#pragma unroll
        for (int q = 0; q < K; ++q)
#pragma unroll
            for (int j = 0; j < W; ++j) v[q][j] += red[((threadIdx.x + r * cv) * K + q) * W + j];
    }
}

// `row0`: this thread is one of row 0 whose sums are wanted.  red holds K * W floats per thread
template <int K, int W>
__device__ __forceinline__ void mg_row_join(float* const (&v)[K], float* red, int cv, int rows, bool row0)
{
    mg_rows_put<K, W>(v, red);
    __syncthreads();
    if (row0) mg_rows_fold<K, W>(v, red, cv, rows);
}

// a + this thread's share of column p[0] of the [nchunks][C2] partials: chunks k, k + 8, ... in fp64, fixed order.
// Eight independent loads in flight per thread (the trip count is a runtime value: without the explicit batch the loop was a
// chain of ~64 dependent L2 round trips, 10.6 us per launch, 99 launches per step); same summation order as the plain loop
__device__ __forceinline__ double mg_chunk_sum_f64(double a, const float* p, int k, int nchunks, int C2)
{
    for (; k + 56 < nchunks; k += 64) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(k + 8 * j) * C2];
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (double)v[j];
    }
    for (; k < nchunks; k += 8) a += (double)p[(size_t)k * C2];
    return a;
}

// 256 threads as 8 rows x 32 columns: thread (row k, column cl) brings a; a thread of row 0 returns its column's sum, the others a
__device__ __forceinline__ double mg_chunk_rows_join(double a, double (&red)[256])
{
    red[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x < 32) {
#pragma unroll
        for (int r = 1; r < 8; ++r) a += red[r * 32 + threadIdx.x];
    }
    return a;
}
