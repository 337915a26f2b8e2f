// mg_norm.hip -- per-channel statistics and normalisation forward/backward
// (sync-BN inside SPADE, InstanceNorm2d in the discriminator / appearance encoder).
//
// All kernels are HBM-bound streaming passes over NHWC activations: a thread
// owns one quad (4 consecutive channels) so a pixel row of C channels is read
// by C/4 consecutive lanes as 8 B (bf16) / 16 B (f32) vector loads; the
// reduction over pixels is two-stage and deterministic:
//   stage 1  grid (chunks, G): register accumulation over the block's pixel
//            chunk, LDS tree across the thread rows -> partial[g][chunk][2][C]
//   stage 2  fp64 sum over chunks in a fixed order -> sums[g][2][C]
// Forward statistics (sum x, sum x^2) are conditioned like a two-pass variance: stage 1 accumulates the SHIFTED values x - k[g][c] with
// the pivot k = x[g][pixel 0][c] (a sample of the channel: sum (x-k)^2 ~ n (var + (mean-k)^2) carries no mean^2 / var cancellation into
// the fp32 partials), stage 2 adds the partials in fp64, un-shifts in fp64 (sum x = s + n k, sum x^2 = ss + 2 k s + n k^2) and hands FP64
// sums to the cross-rank all-reduce and to finalize: nothing between the per-thread partials and var = E[x^2] - E[x]^2 is rounded to
// fp32 (the one-pass fp32 sums were; sync_batchnorm/batchnorm.py:128-145 is that formula, batchnorm_reimpl.py:18-74 the
// two-pass yardstick).  `shift = 0` (plain column sums of gradients: ops.channel_sums for bias gradients) keeps k = 0: for ZERO-mean data a
// sample pivot makes the partial sums grow like n |k| instead of sqrt(n) sigma.  Per-thread fp64 accumulation (no pivot needed) was
// measured too: same results, stats_stage1_vec 17.8 -> 21.7 us per launch (+0.24 ms per step), not kept.
#include "mg_common.h"
#include "mg_launch.h"
#include "mg_options.h"
#include "mg_reduce.h"


namespace {

struct StatGeom { int tpr; int rpb; int nchunks; int64_t chunk; };

static inline StatGeom stat_geom(int G, int64_t P, int C)
{
    StatGeom g;
    const int c4 = C / 4;
    g.tpr = c4 < MG_NTHR ? c4 : MG_NTHR;
    g.rpb = MG_NTHR / g.tpr;
    // enough stage-1 blocks to fill 256 CUs a few times over (G groups share the budget), but at
    // least 16 rows per thread and at most 512 partials per group for the stage-2 tree.
    int64_t want = (1536 + G - 1) / G;
    const int64_t cap = (P + (int64_t)g.rpb * 16 - 1) / ((int64_t)g.rpb * 16);
    if (want > cap) want = cap;
    if (want > 512) want = 512;
    if (want < 1) want = 1;
    g.chunk = (P + want - 1) / want;
    g.nchunks = (int)((P + g.chunk - 1) / g.chunk);
    return g;
}

// blocks of `rows` channel-resident thread rows with `pix` pixels in flight each, at most 4096 over the G groups
static inline int pix_grid(int64_t P, int rows, int pix, int G)
{
    int64_t b = (P + (int64_t)rows * pix - 1) / ((int64_t)rows * pix);
    const int64_t cap = (4096 + G - 1) / G;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

// element offset of channel c of the half-resolution source pixel that full-resolution pixel q of [N, H, W] reads through a
// nearest 2x upsample
__device__ __forceinline__ size_t up_src_offset(int q, int H, int W, int C, int c)
{
    const int n = q / (H * W), rem = q - n * (H * W);
    const int yy = rem / W, xx = rem - yy * W;
    return ((size_t)(n * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1)) * C + c;
}

// sums of one channel -> mean / rstd (fp64 inside) and the optional running-statistics update of channel c: the one copy of this
// arithmetic, so mg_channel_stats_finalize is bit-identical to mg_channel_stats + mg_norm_finalize by construction.  at() is the
// channel's index into mean / rstd, a callable so that it is formed at the stores, where each caller had it: both kernels keep
// their instructions
template <typename Index>
__device__ __forceinline__ void finalize_channel(double s, double ss, double count, float eps, float momentum,
                                                 float* running_mean, float* running_var, int c,
                                                 float* mean, float* rstd, Index&& at)
{
    const double m = s / count;
    double var = ss / count - m * m;
    if (var < 0.0) var = 0.0;
    mean[at()] = (float)m;
    rstd[at()] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double unbiased = var * (count / (count > 1.0 ? count - 1.0 : 1.0));
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
}

// dxhat = (dh * act'(h)) * (1 + gamma) of one element, and its first product dpre, which d[gamma | beta] take.  The quad kernels
// go through mg_act_grad_from_out (any activation, h = 1 where there is none); the channel-resident ones know NONE / RELU / LRELU
// as neg = mg_neg_slope(act, slope), and a missing h or g1 is a factor 1 that is not multiplied
struct DxHat { float dpre, dxh; };
__device__ __forceinline__ DxHat dxhat_quad(float dv, float hv, float gv, int act, float slope)
{
    const float dpre = dv * mg_act_grad_from_out(hv, act, slope);
    return {dpre, dpre * gv};
}
__device__ __forceinline__ DxHat dxhat_vec(float dv, float hv, float gv, float neg, bool has_h, bool has_g1)
{
    const float dpre = has_h ? dv * mg_act_factor(hv, neg) : dv;
    return {dpre, has_g1 ? dpre * gv : dpre};
}

// the end of every stage-1 kernel: the row join of mg_reduce.h, then row 0 stores its W channels from c of partial[g][chunk][2][C]
// (grid (chunks, G))
template <int W>
__device__ __forceinline__ void join_to_partial(float (&s)[W], float (&ss)[W], float* red, int cv, int rows, bool row0, float* __restrict__ partial, int C, int c)
{
    float* const terms[2] = {s, ss};
    mg_row_join<2, W>(terms, red, cv, rows, row0);
    if (row0) {
        float* dst = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C + c;
#pragma unroll
        for (int j = 0; j < W; ++j) { dst[j] = s[j]; dst[C + j] = ss[j]; }
    }
}

// quad thread (tq, tr) of tpr x rpb and the pixels [p0, p1) of the workgroup's chunk
struct QuadChunk { int tq, tr; bool active; int64_t p0, p1; };
__device__ __forceinline__ QuadChunk quad_chunk(int64_t P, int tpr, int rpb, int64_t chunk)
{
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    return {tid % tpr, tid / tpr, tid < tpr * rpb, p0, (p0 + chunk < P) ? p0 + chunk : P};
}

// stage 1 of the plain statistics (sum x, sum x^2) for any C % 4 == 0
template <typename T>
__global__ __launch_bounds__(MG_NTHR) void stats_stage1_quad(const T* __restrict__ x, float* __restrict__ partial, int64_t P, int C,
                                                             int tpr, int rpb, int64_t chunk, int shift)
{
    __shared__ float red[MG_NTHR * 8];
    const int g = blockIdx.y, c4 = C / 4;
    const auto [tq, tr, active, p0, p1] = quad_chunk(P, tpr, rpb, chunk);
    for (int qd0 = 0; qd0 < c4; qd0 += tpr) {         // uniform trip count (one trip unless C > 1024)
        const int qd = qd0 + tq;
        const bool qv = active && qd < c4;
        const int c = (qd < c4 ? qd : 0) * 4;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4_t kv = {0.f, 0.f, 0.f, 0.f};
        if (shift) kv = ET<T>::load4(x + (size_t)g * P * C + c);     // pivot = the group's first pixel
        if (qv) {
            for (int64_t p = p0 + tr; p < p1; p += rpb) {
                const f32x4_t xv = ET<T>::load4(x + ((size_t)g * P + p) * C + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float t = xv[j] - kv[j]; s[j] += t; ss[j] += t * t; }
            }
        }
        join_to_partial(s, ss, red, tpr, rpb, qv && tr == 0, partial, C, c);
        __syncthreads();                                 // red is free for the next channel trip
    }
}

// stage 1 of the norm backward reduction (sum dxhat, sum dxhat * xhat, optional d[gamma|beta] output) for any C % 4 == 0 and any
// activation; `up`: x is the half-resolution source of a nearest 2x upsample (G == 1)
template <typename T, bool HAS_H>
__global__ __launch_bounds__(MG_NTHR) void bwd_stage1_quad(
    const T* __restrict__ x, const T* __restrict__ dh, const T* __restrict__ h, const T* __restrict__ g1,
    const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ dgb,
    float* __restrict__ partial, int64_t P, int C, int tpr, int rpb, int64_t chunk, int act, float slope, int up, int H, int W)
{
    __shared__ float red[MG_NTHR * 8];
    const int g = blockIdx.y, c4 = C / 4;
    const auto [tq, tr, active, p0, p1] = quad_chunk(P, tpr, rpb, chunk);
    const int Cr2 = 2 * ((C + 31) / 32) * 32;
    for (int qd0 = 0; qd0 < c4; qd0 += tpr) {         // uniform trip count (one trip unless C > 1024)
        const int qd = qd0 + tq;
        const bool qv = active && qd < c4;
        const int c = (qd < c4 ? qd : 0) * 4;
        float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4_t mu, rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) { mu[j] = mean[(size_t)g * C + c + j]; rs[j] = rstd[(size_t)g * C + c + j]; }
        if (qv) {
            for (int64_t p = p0 + tr; p < p1; p += rpb) {
                const size_t o = ((size_t)g * P + p) * C + c;
                size_t ox = o;
                if (up) ox = up_src_offset((int)p, H, W, C, c);
                const f32x4_t xv = ET<T>::load4(x + ox);
                const f32x4_t dv = ET<T>::load4(dh + o);
                f32x4_t hv = {1.f, 1.f, 1.f, 1.f};              // h only matters through the sign of the activation's output
                if constexpr (HAS_H) hv = ET<T>::load4(h + o);
                f32x4_t gv = {1.f, 1.f, 1.f, 1.f};
                if (g1) gv = ET<T>::load4(g1 + o);
                f32x4_t dgam, dbet;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const DxHat d = dxhat_quad(dv[j], hv[j], gv[j], act, slope);
                    const float xh = (xv[j] - mu[j]) * rs[j];
                    s[j] += d.dxh; ss[j] += d.dxh * xh;
                    dgam[j] = d.dpre * xh; dbet[j] = d.dpre;
                }
                if (dgb) {
                    const size_t ob = ((size_t)g * P + p) * Cr2 + (size_t)(c >> 5) * 64 + (c & 31);
                    ET<T>::store4(dgb + ob, dgam);
                    ET<T>::store4(dgb + ob + 32, dbet);
                }
            }
        }
        join_to_partial(s, ss, red, tpr, rpb, qv && tr == 0, partial, C, c);
        __syncthreads();                                 // red is free for the next channel trip
    }
}

// stage 2: one 256-thread block per 32 consecutive outputs; 8 thread rows split the chunks,
// fp64 accumulation, fixed order (deterministic).
__global__ __launch_bounds__(256) void reduce_stage2(const float* __restrict__ partial, float* __restrict__ sums, int nchunks, int C2)
{
    __shared__ double red[256];
    const int cl = threadIdx.x & 31, kk = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + cl;
    const int g = blockIdx.y;
    double a = 0.0;
    if (i < C2) a = mg_chunk_sum_f64(a, partial + (size_t)g * nchunks * C2 + i, kk, nchunks, C2);
    a = mg_chunk_rows_join(a, red);
    if (kk == 0 && i < C2) sums[(size_t)g * C2 + i] = (float)a;
}

template <typename T>
__global__ void norm_act_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t nquads, int64_t P, int C,
                                    const float* __restrict__ mean, const float* __restrict__ rstd, int act, float slope,
                                    const T* __restrict__ resid)
{
    const int c4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nquads; i += (int64_t)gridDim.x * blockDim.x) {
        const int qd = (int)(i % c4);
        const int64_t pix = i / c4;
        const int g = (int)(pix / P);
        const int c = qd * 4;
        const f32x4_t xv = ET<T>::load4(x + i * 4);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = mg_act((xv[j] - mean[(size_t)g * C + c + j]) * rstd[(size_t)g * C + c + j], act, slope);
        if (resid) {
            const f32x4_t rv = ET<T>::load4(resid + i * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += rv[j];
        }
        ET<T>::store4(y + i * 4, o);
    }
}

template <typename T>
__global__ void norm_bwd_apply_kernel(const T* __restrict__ dh, const T* __restrict__ h, const T* __restrict__ x,
                                      const T* __restrict__ g1, T* __restrict__ dx, int64_t nquads, int64_t P, int C,
                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                      const float* __restrict__ s1, const float* __restrict__ s2, int sgs, float sscale, int act, float slope)
{
    const int c4 = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nquads; i += (int64_t)gridDim.x * blockDim.x) {
        const int qd = (int)(i % c4);
        const int64_t pix = i / c4;
        const int g = (int)(pix / P);
        const size_t sc = (size_t)g * C + qd * 4, ss = (size_t)g * sgs + qd * 4;
        const f32x4_t dv = ET<T>::load4(dh + i * 4);
        f32x4_t hv = {1.f, 1.f, 1.f, 1.f};
        if (h) hv = ET<T>::load4(h + i * 4);
        const f32x4_t xv = ET<T>::load4(x + i * 4);
        f32x4_t gv = {1.f, 1.f, 1.f, 1.f};
        if (g1) gv = ET<T>::load4(g1 + i * 4);
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float r = rstd[sc + j];
            const float xh = (xv[j] - mean[sc + j]) * r;
            const float dxh = dxhat_quad(dv[j], hv[j], gv[j], act, slope).dxh;
            o[j] = r * (dxh - s1[ss + j] * sscale - xh * (s2[ss + j] * sscale));
        }
        ET<T>::store4(dx + i * 4, o);
    }
}


// ---------------------------------------------------------------------------------------------
// Channel-resident 16-byte variants (the common geometries: C a multiple of VEC = 16 B / sizeof(T) and C / VEC a
// divisor of 256).  A thread keeps ONE group of VEC channels for the whole launch, so the per-channel constants
// are loaded once, the pixel loop has no integer division, every access is a full 16-byte vector and PIX
// independent pixels are in flight per thread.  The quad kernels above (8-byte accesses, div/mod and 16 scalar
// parameter loads per quad) ran at 2.0-2.5 TB/s on [8,512,512,128] bf16; these run at 4-5 TB/s (tools/bench_pointwise.py).
template <typename T> static inline bool vec_geom_ok(int C)
{
    constexpr int VEC = EV<T>::VEC;
    if (C % VEC) return false;
    const int cv = C / VEC;
    return cv <= MG_NTHR && MG_NTHR % cv == 0;
}
// this (T, C, act) takes the channel-resident kernel: TANH stays on the quad kernels
template <typename T> static inline bool takes_vec(int C, int act) { return act != MG_ACT_TANH && vec_geom_ok<T>(C); }
template <typename T> static inline int vec_rows(int C) { return MG_NTHR / (C / EV<T>::VEC); }

// channel-resident thread (tq, tr) of cv x rows: channels c .. c + VEC - 1 for the whole launch
struct ChanThread { int cv, rows, tq, tr, c; };
template <int VEC> __device__ __forceinline__ ChanThread chan_thread(int C)
{
    const int cv = C / VEC, tq = threadIdx.x % cv;
    const int tr = threadIdx.x / cv;
    return {cv, MG_NTHR / cv, tq, tr, tq * VEC};
}
// its channels' mean / rstd (of one group: the caller offsets the pointers) into registers
template <int VEC> __device__ __forceinline__ void chan_stats(const float* __restrict__ mean, const float* __restrict__ rstd, float (&m)[VEC], float (&r)[VEC])
{
#pragma unroll
    for (int j = 0; j < VEC; ++j) { m[j] = mean[j]; r[j] = rstd[j]; }
}

template <typename T, int PIX>
__global__ __launch_bounds__(MG_NTHR) void norm_bwd_apply_vec(const T* __restrict__ dh, const T* __restrict__ h, const T* __restrict__ x,
                                                         const T* __restrict__ g1, T* __restrict__ dx, int64_t P, int C,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ s1, const float* __restrict__ s2, int sgs, float sscale, float neg)
{
    constexpr int VEC = EV<T>::VEC;
    const auto [cv, rows, tq, tr, c] = chan_thread<VEC>(C);
    const int g = blockIdx.y;
    float m[VEC], r[VEC], c1[VEC], c2[VEC];
    chan_stats(mean + (size_t)g * C + c, rstd + (size_t)g * C + c, m, r);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const size_t k = (size_t)g * sgs + c + j;
        c1[j] = r[j] * (s1[k] * sscale); c2[j] = r[j] * r[j] * (s2[k] * sscale);
    }
    const size_t base = (size_t)g * P * C + c;
    const int64_t step = (int64_t)gridDim.x * rows;
    for (int64_t p0 = (int64_t)blockIdx.x * rows + tr; p0 < P; p0 += step * PIX) {
        float dv[PIX][VEC], hv[PIX][VEC], xv[PIX][VEC], gv[PIX][VEC];
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = p0 + k * step;
            if (p < P) {
                const size_t o = base + (size_t)p * C;
                EV<T>::load(dh + o, dv[k]); EV<T>::load(x + o, xv[k]);
                if (h) EV<T>::load(h + o, hv[k]);
                if (g1) EV<T>::load(g1 + o, gv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = p0 + k * step;
            if (p < P) {
                float o4[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float dxh = dxhat_vec(dv[k][j], hv[k][j], gv[k][j], neg, h != nullptr, g1 != nullptr).dxh;
                    o4[j] = r[j] * dxh - c1[j] - c2[j] * (xv[k][j] - m[j]);
                }
                EV<T>::store(dx + base + (size_t)p * C, o4);
            }
        }
    }
}

template <typename T, int PIX>
__global__ __launch_bounds__(MG_NTHR) void norm_act_fwd_vec(const T* __restrict__ x, T* __restrict__ y, int64_t P, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       float neg, bool relu, const T* __restrict__ resid)
{
    constexpr int VEC = EV<T>::VEC;
    const auto [cv, rows, tq, tr, c] = chan_thread<VEC>(C);
    const int g = blockIdx.y;
    float m[VEC], r[VEC];
    chan_stats(mean + (size_t)g * C + c, rstd + (size_t)g * C + c, m, r);
    const size_t base = (size_t)g * P * C + c;
    const int64_t step = (int64_t)gridDim.x * rows;
    for (int64_t p0 = (int64_t)blockIdx.x * rows + tr; p0 < P; p0 += step * PIX) {
        float xv[PIX][VEC], rv[PIX][VEC];
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = p0 + k * step;
            if (p < P) { EV<T>::load(x + base + (size_t)p * C, xv[k]); if (resid) EV<T>::load(resid + base + (size_t)p * C, rv[k]); }
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = p0 + k * step;
            if (p < P) {
                float o4[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float v = (xv[k][j] - m[j]) * r[j];
                    const float t = v > 0.f ? v : v * neg;
                    o4[j] = relu ? fmaxf(v, 0.f) : t;
                    if (resid) o4[j] += rv[k][j];
                }
                EV<T>::store(y + base + (size_t)p * C, o4);
            }
        }
    }
}

// stage 1 of the plain statistics (sum x, sum x^2) with the same chunking / partial layout as stats_stage1_quad
template <typename T, int PIX>
__global__ __launch_bounds__(MG_NTHR) void stats_stage1_vec(const T* __restrict__ x, float* __restrict__ partial, int64_t P, int C, int64_t chunk, int shift)
{
    constexpr int VEC = EV<T>::VEC;
    __shared__ float red[MG_NTHR * 2 * VEC];
    const auto [cv, rows, tq, tr, c] = chan_thread<VEC>(C);
    const int g = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = (p0 + chunk < P) ? p0 + chunk : P;
    float s[VEC], ss[VEC], kv[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s[j] = 0.f; ss[j] = 0.f; }
    const size_t base = (size_t)g * P * C + c;
    if (shift) EV<T>::load(x + base, kv);                                // pivot of the shifted sums: the group's first pixel
    else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) kv[j] = 0.f;
    }
    for (int64_t pp = p0 + tr; pp < p1; pp += (int64_t)rows * PIX) {
        float xv[PIX][VEC];
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = pp + (int64_t)k * rows;
            if (p < p1) EV<T>::load(x + base + (size_t)p * C, xv[k]);
            else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) xv[k][j] = kv[j];           // contributes (k - k) = 0
            }
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k)
#pragma unroll
            for (int j = 0; j < VEC; ++j) { const float t = xv[k][j] - kv[j]; s[j] += t; ss[j] += t * t; }
    }
    join_to_partial(s, ss, red, cv, rows, tr == 0, partial, C, c);
}

// stage 1 of the norm backward reduction (sum dxhat, sum dxhat * xhat, optional d[gamma|beta] output), 16-byte variant of
// bwd_stage1_quad: a thread keeps VEC channels (mean / rstd loaded once), PIX pixels in flight, every access a full 16-byte
// vector -- the quad kernel moved its four input streams in 8-byte pieces at 4.4 TB/s and was the largest non-MFMA kernel of the step.
// Same chunking and partial layout; `act` is NONE / RELU / LRELU only (neg = 1 / 0 / slope), TANH stays on the quad kernel.
template <typename T, int PIX, bool HAS_H, bool UP>
__global__ __launch_bounds__(MG_NTHR) void bwd_stage1_vec(const T* __restrict__ x, const T* __restrict__ dh, const T* __restrict__ h, const T* __restrict__ g1,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, T* __restrict__ dgb,
                                                     float* __restrict__ partial, int64_t P, int C, int64_t chunk, float neg, int H, int W)
{
    constexpr int VEC = EV<T>::VEC;
    __shared__ float red[MG_NTHR * 2 * VEC];
    const auto [cv, rows, tq, tr, c] = chan_thread<VEC>(C);
    const int g = blockIdx.y;
    const int Cr2 = 2 * ((C + 31) / 32) * 32;
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = (p0 + chunk < P) ? p0 + chunk : P;
    float mu[VEC], rs[VEC], s[VEC], ss[VEC];
    chan_stats(mean + (size_t)g * C + c, rstd + (size_t)g * C + c, mu, rs);
#pragma unroll
    for (int j = 0; j < VEC; ++j) { s[j] = 0.f; ss[j] = 0.f; }
    const size_t base = (size_t)g * P * C + c;
    const size_t gbase = (size_t)g * P * Cr2 + (size_t)(c >> 5) * 64 + (c & 31);
    for (int64_t pp = p0 + tr; pp < p1; pp += (int64_t)rows * PIX) {
        float xv[PIX][VEC], dv[PIX][VEC], hv[PIX][VEC], gv[PIX][VEC];
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = pp + (int64_t)k * rows;
            if (p < p1) {
                size_t ox = base + (size_t)p * C;
                if (UP) ox = up_src_offset((int)p, H, W, C, c);       // x is the half-resolution source of a nearest 2x upsample (G == 1)
                EV<T>::load(x + ox, xv[k]);
                EV<T>::load(dh + base + (size_t)p * C, dv[k]);
                if (HAS_H) EV<T>::load(h + base + (size_t)p * C, hv[k]);
                if (g1) EV<T>::load(g1 + base + (size_t)p * C, gv[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < PIX; ++k) {
            const int64_t p = pp + (int64_t)k * rows;
            if (p < p1) {
                float dgam[VEC], dbet[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const DxHat d = dxhat_vec(dv[k][j], hv[k][j], gv[k][j], neg, HAS_H, g1 != nullptr);
                    const float xh = (xv[k][j] - mu[j]) * rs[j];
                    s[j] += d.dxh; ss[j] += d.dxh * xh;
                    dgam[j] = d.dpre * xh; dbet[j] = d.dpre;
                }
                if (dgb) {
                    EV<T>::store(dgb + gbase + (size_t)p * Cr2, dgam);
                    EV<T>::store(dgb + gbase + (size_t)p * Cr2 + 32, dbet);
                }
            }
        }
    }
    join_to_partial(s, ss, red, cv, rows, tr == 0, partial, C, c);
}

// sums[g][2][C] (+ element count) -> mean / rstd (fp64 inside), optional running-statistics update (G == 1):
// replaces a dozen [C]-sized eager ops per normalisation layer.
__global__ void norm_finalize_kernel(const double* __restrict__ sums, int G, int C, double count, float eps, float momentum,
                                     float* __restrict__ running_mean, float* __restrict__ running_var,
                                     float* __restrict__ mean, float* __restrict__ rstd)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * C) return;
    const int g = i / C, c = i - g * C;
    const double s = sums[((size_t)g * 2) * C + c], ss = sums[((size_t)g * 2 + 1) * C + c];
    finalize_channel(s, ss, count, eps, momentum, running_mean, running_var, c, mean, rstd, [&] { return i; });
}

// Input gradient of batch norm for up to TWO consumers that normalise the same x (SPADE norm_0 / norm_s of a block with a learned
// shortcut, architecture.py:68-70,79), optionally through a nearest 2x upsample of x (generator.py:166-207):
//   dx[src] = sum over branches b and over the (1 | 2x2) full-resolution pixels q of  rstd * (dxhat_b[q] - s1_b - xhat[src] * s2_b),
//   dxhat_b = dh_b * act_b'(h_b) * g1_b,  s1_b / s2_b = sums_b[0 / 1] * inv_count.
// One pass instead of two applies + autograd's add of their results + the upsample's 2x2 adjoint: x is read once at its own
// resolution and dx written once at its own resolution.  Channel-resident threads like norm_bwd_apply_vec.
template <typename T, int NB, bool UP>
__global__ __launch_bounds__(MG_NTHR) void norm_bwd_apply2_vec(const mg_norm_apply2_desc d, float neg0, float neg1)
{
    constexpr int VEC = EV<T>::VEC;
    const int C = d.C;
    const auto [cv, rows, tq, tr, c] = chan_thread<VEC>(C);
    const T* dh0 = (const T*)d.dh[0]; const T* h0 = (const T*)d.h[0]; const T* g0 = (const T*)d.g1[0];
    const T* dh1 = (const T*)d.dh[1]; const T* h1 = (const T*)d.h[1]; const T* g1 = (const T*)d.g1[1];
    const T* x = (const T*)d.x; T* dx = (T*)d.dx;
    constexpr int Q = UP ? 4 : 1;
    float m[VEC], r[VEC], k1[VEC], k2[VEC];
    chan_stats(d.mean + c, d.rstd + c, m, r);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        float s1 = d.sums[0][c + j], s2 = d.sums[0][C + c + j];
        if (NB == 2) { s1 += d.sums[1][c + j]; s2 += d.sums[1][C + c + j]; }
        k1[j] = (float)Q * r[j] * s1 * d.inv_count;
        k2[j] = (float)Q * r[j] * r[j] * s2 * d.inv_count;
    }
    const int W = d.W, H = d.H, W2 = W >> 1, H2 = H >> 1;
    const int64_t Pout = UP ? d.P / 4 : d.P;                       // pixels of x / dx
    const int64_t step = (int64_t)gridDim.x * rows;
    for (int64_t po = (int64_t)blockIdx.x * rows + tr; po < Pout; po += step) {
        int64_t pf[Q];
        if (UP) {
            const int pp = (int)po, n = pp / (H2 * W2), rem = pp - n * (H2 * W2);
            const int y2 = rem / W2, x2 = rem - y2 * W2;
            const int64_t base = ((int64_t)n * H + 2 * y2) * W + 2 * x2;
            pf[0] = base; if (Q > 1) { pf[1 % Q] = base + 1; pf[2 % Q] = base + W; pf[3 % Q] = base + W + 1; }
        } else pf[0] = po;
        float xv[VEC], acc[VEC];
        EV<T>::load(x + (size_t)po * C + c, xv);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const size_t o = (size_t)pf[q] * C + c;
            float dv[VEC], hv[VEC], gv[VEC];
            EV<T>::load(dh0 + o, dv);
            if (h0) EV<T>::load(h0 + o, hv);
            if (g0) EV<T>::load(g0 + o, gv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += dxhat_vec(dv[j], hv[j], gv[j], neg0, h0 != nullptr, g0 != nullptr).dxh;
            if (NB == 2) {
                EV<T>::load(dh1 + o, dv);
                if (h1) EV<T>::load(h1 + o, hv);
                if (g1) EV<T>::load(g1 + o, gv);
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] += dxhat_vec(dv[j], hv[j], gv[j], neg1, h1 != nullptr, g1 != nullptr).dxh;
            }
        }
        float o4[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o4[j] = r[j] * acc[j] - k1[j] - k2[j] * (xv[j] - m[j]);
        EV<T>::store(dx + (size_t)po * C + c, o4);
    }
}

// Stage 2 of the forward statistics: a block owns 16 channels; lanes 0..15 of each thread row sum the channels' shifted partial sums,
// lanes 16..31 their shifted partial sums of squares (fp64, fixed order), then lanes 0..15 un-shift with the pivot x[g][0][c] (0 without `shift`) in fp64
// and write sums[g][2][C] (fp64; x sum_scale: the statistics of a nearest 2x upsample from its source, x 4, exact).
// FIN: the same lanes also run norm_finalize_kernel's arithmetic on those fp64 sums -- statistics that need no cross-rank reduction in
// between (instance norm; batch norm on one GPU) finish in two launches, bit-identical to mg_channel_stats + mg_norm_finalize.
template <typename T, bool FIN>
__global__ __launch_bounds__(256) void stats_stage2(const float* __restrict__ partial, const T* __restrict__ x, int64_t P, double* __restrict__ sums,
                                                    int nchunks, int C, int shift, double sum_scale, double count, float eps, float momentum,
                                                    float* __restrict__ running_mean, float* __restrict__ running_var,
                                                    float* __restrict__ mean, float* __restrict__ rstd)
{
    __shared__ double red[256];
    __shared__ double fin[32];
    const int cl = threadIdx.x & 31, kk = threadIdx.x >> 5;
    const int c = blockIdx.x * 16 + (cl & 15);
    const int g = blockIdx.y;
    const int C2 = 2 * C;
    const int i = (cl >> 4) * C + c;                            // column of the [sum | sum of squares] vector
    double a = 0.0;
    if (c < C) a = mg_chunk_sum_f64(a, partial + (size_t)g * nchunks * C2 + i, kk, nchunks, C2);
    a = mg_chunk_rows_join(a, red);
    if (kk == 0) fin[cl] = a;
    __syncthreads();
    if (threadIdx.x < 16 && c < C) {
        const double kv = shift ? (double)ET<T>::load1(x + (size_t)g * P * C + c) : 0.0;
        const double sh = fin[threadIdx.x], ssh = fin[16 + threadIdx.x], n = (double)P;
        const double s = (sh + n * kv) * sum_scale;
        const double ss = (ssh + 2.0 * kv * sh + n * kv * kv) * sum_scale;
        sums[(size_t)g * C2 + c] = s;
        sums[(size_t)g * C2 + C + c] = ss;
        if (FIN) finalize_channel(s, ss, count, eps, momentum, running_mean, running_var, c, mean, rstd, [&] { return (size_t)g * C + c; });
    }
}

// forward statistics: stage 1 (shifted fp32 partial sums) + stage 2 (fp64 sums [+ finalize])
template <typename T, bool FIN>
int run_stats(const void* x, int G, int64_t P, int C, int shift, double* sums, void* partial, double sum_scale, double count, float eps, float momentum,
              float* running_mean, float* running_var, float* mean, float* rstd, hipStream_t st)
{
    const StatGeom sg = stat_geom(G, P, C);
    dim3 grid(sg.nchunks, G);
    if (vec_geom_ok<T>(C))
        hipLaunchKernelGGL((stats_stage1_vec<T, 4>), grid, dim3(MG_NTHR), 0, st, (const T*)x, (float*)partial, P, C, sg.chunk, shift);
    else
        hipLaunchKernelGGL(stats_stage1_quad<T>, grid, dim3(MG_NTHR), 0, st, (const T*)x, (float*)partial, P, C, sg.tpr, sg.rpb, sg.chunk, shift);
    MG_CHECK_LAUNCH("channel statistics (stage 1)");
    hipLaunchKernelGGL((stats_stage2<T, FIN>), dim3((C + 15) / 16, G), dim3(256), 0, st, (const float*)partial, (const T*)x, P, sums, sg.nchunks, C, shift,
                       sum_scale, count, eps, momentum, running_mean, running_var, mean, rstd);
    MG_CHECK_LAUNCH("channel statistics (stage 2)");
    return MG_OK;
}

// norm backward reduction (sum dxhat, sum dxhat * xhat [+ d[gamma|beta]]): these sums cancel by themselves (no pivot helps);
// fp32 per-thread partials over >= 16 values, fp64 across chunks.
template <typename T>
int run_reduce(const void* x, const void* dh, const void* h, const void* g1, const float* mean, const float* rstd,
               void* dgb, int G, int64_t P, int C, float* sums, void* partial, int act, float slope, hipStream_t st,
               int up, int H, int W)
{
    const StatGeom sg = stat_geom(G, P, C);
    dim3 grid(sg.nchunks, G);
    if (mg_opt(MG_OPT_NORM_BWD_VEC) && takes_vec<T>(C, act)) {
        // (d[gamma|beta] rows are 32-channel blocks; a thread's VEC channels start at a multiple of VEC and stay inside one block)
        const float neg = mg_neg_slope(act, slope);
        mg_by_bool(h != nullptr && act != MG_ACT_NONE, [&](auto hh) { mg_by_bool(up != 0, [&](auto upf) {
            hipLaunchKernelGGL((bwd_stage1_vec<T, 2, hh.value, upf.value>), grid, dim3(MG_NTHR), 0, st, (const T*)x, (const T*)dh, (const T*)h,
                               (const T*)g1, mean, rstd, (T*)dgb, (float*)partial, P, C, sg.chunk, neg, H, W); }); });
    } else
        mg_by_bool(h != nullptr, [&](auto hh) {
            hipLaunchKernelGGL((bwd_stage1_quad<T, hh.value>), grid, dim3(MG_NTHR), 0, st, (const T*)x, (const T*)dh, (const T*)h, (const T*)g1,
                               mean, rstd, (T*)dgb, (float*)partial, P, C, sg.tpr, sg.rpb, sg.chunk, act, slope, up, H, W); });
    MG_CHECK_LAUNCH("reduce_stage1");
    dim3 grid2((2 * C + 31) / 32, G);
    hipLaunchKernelGGL(reduce_stage2, grid2, dim3(256), 0, st, (const float*)partial, sums, sg.nchunks, 2 * C);
    MG_CHECK_LAUNCH("reduce_stage2");
    return MG_OK;
}

}  // namespace

#define MG_CHECK_NORM_GEOM(name) \
    MG_CHECK_ARG(dtype == MG_F32 || dtype == MG_BF16, "%s: bad dtype %d", name, dtype); \
    MG_CHECK_ARG(G > 0 && P > 0 && C > 0 && (C % 4) == 0 && C <= 4096, "%s: bad geometry G=%d P=%ld C=%d (C must be a multiple of 4, <= 4096)", name, G, (long)P, C)

extern "C" int64_t mg_stats_workspace(int32_t G, int64_t P, int32_t C)
{
    if (G <= 0 || P <= 0 || C <= 0) return 0;
    const StatGeom sg = stat_geom(G, P, C);
    return (int64_t)G * sg.nchunks * 2 * C * (int64_t)sizeof(float);
}

extern "C" int mg_channel_stats(const void* x, int32_t dtype, int32_t G, int64_t P, int32_t C, int32_t shift,
                                double* sums, void* partial, void* stream)
{
    MG_CHECK_NORM_GEOM("mg_channel_stats");
    MG_CHECK_ARG(x && sums && partial, "mg_channel_stats: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        return run_stats<T, false>(x, G, P, C, shift != 0, sums, partial, 1.0, 1.0, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, st); });
}

extern "C" int mg_channel_stats_finalize(const void* x, int32_t dtype, int32_t G, int64_t P, int32_t C, float sum_scale, double count,
                                         float eps, float momentum, float* running_mean, float* running_var,
                                         double* sums, float* mean, float* rstd, void* partial, void* stream)
{
    MG_CHECK_NORM_GEOM("mg_channel_stats_finalize");
    MG_CHECK_ARG(x && sums && mean && rstd && partial, "mg_channel_stats_finalize: null pointer");
    MG_CHECK_ARG(count > 0 && sum_scale > 0.f, "mg_channel_stats_finalize: bad count / scale");
    MG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr) && (running_mean == nullptr || G == 1),
                 "mg_channel_stats_finalize: running statistics need both buffers and G == 1");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        return run_stats<T, true>(x, G, P, C, 1, sums, partial, (double)sum_scale, count, eps, momentum, running_mean, running_var, mean, rstd, st); });
}

extern "C" int mg_norm_act_fwd(const void* x, void* y, int32_t dtype, int32_t G, int64_t P, int32_t C,
                               const float* mean, const float* rstd, int32_t act, float slope, const void* resid, void* stream)
{
    MG_CHECK_NORM_GEOM("mg_norm_act_fwd");
    MG_CHECK_ARG(x && y && mean && rstd, "mg_norm_act_fwd: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nq = (int64_t)G * P * (C / 4);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (takes_vec<T>(C, act)) {
            hipLaunchKernelGGL((norm_act_fwd_vec<T, 4>), dim3(pix_grid(P, vec_rows<T>(C), 4, G), G), dim3(MG_NTHR), 0, st,
                               (const T*)x, (T*)y, P, C, mean, rstd, mg_neg_slope(act, slope), act == MG_ACT_RELU, (const T*)resid);
        } else
            hipLaunchKernelGGL(norm_act_fwd_kernel<T>, dim3(mg_ew_grid(nq, 8192)), dim3(MG_NTHR), 0, st,
                               (const T*)x, (T*)y, nq, P, C, mean, rstd, act, slope, (const T*)resid);
    });
    MG_CHECK_LAUNCH("mg_norm_act_fwd");
    return MG_OK;
}

// what mg_norm_bwd_reduce and mg_norm_bwd_reduce_up check and launch; up: P = N * H * W pixels read x through a nearest 2x upsample
static int norm_bwd_reduce(const char* name, const void* dh, const void* h, const void* x, const void* g1,
                           int32_t dtype, int32_t G, int64_t P, int32_t C, const float* mean, const float* rstd, int32_t act, float slope,
                           void* dgb, float* sums, void* partial, void* stream, int up, int32_t N, int32_t H, int32_t W)
{
    MG_CHECK_NORM_GEOM(name);
    MG_CHECK_ARG(dh && (h || act == MG_ACT_NONE) && x && mean && rstd && sums && partial, "%s: null pointer", name);
    MG_CHECK_ARG(dgb == nullptr || G == 1, "%s: dgb output requires G == 1", name);
    if (up) MG_CHECK_ARG(N > 0 && H > 0 && W > 0 && (H % 2) == 0 && (W % 2) == 0 && P < (1L << 31), "%s: H, W must be even", name);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        return run_reduce<T>(x, dh, h, g1, mean, rstd, dgb, G, P, C, sums, partial, act, slope, st, up, H, W); });
}

extern "C" int mg_norm_bwd_reduce(const void* dh, const void* h, const void* x, const void* g1,
                                  int32_t dtype, int32_t G, int64_t P, int32_t C,
                                  const float* mean, const float* rstd, int32_t act, float slope,
                                  void* dgb, float* sums, void* partial, void* stream)
{
    return norm_bwd_reduce("mg_norm_bwd_reduce", dh, h, x, g1, dtype, G, P, C, mean, rstd, act, slope, dgb, sums, partial, stream, 0, 0, 0, 0);
}

extern "C" int mg_norm_bwd_reduce_up(const void* dh, const void* h, const void* x, const void* g1,
                                     int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                                     const float* mean, const float* rstd, int32_t act, float slope,
                                     void* dgb, float* sums, void* partial, void* stream)
{
    return norm_bwd_reduce("mg_norm_bwd_reduce_up", dh, h, x, g1, dtype, 1, (int64_t)N * H * W, C, mean, rstd, act, slope, dgb, sums, partial, stream, 1, N, H, W);
}

template <typename T>
static int launch_apply2(const mg_norm_apply2_desc& d, hipStream_t st)
{
    const int rows = vec_rows<T>(d.C);
    const bool two = d.dh[1] != nullptr;
    const int64_t pout = d.up ? d.P / 4 : d.P;
    const float n0 = mg_neg_slope(d.act[0], d.slope[0]), n1 = mg_neg_slope(d.act[1], d.slope[1]);
    const dim3 grid(pix_grid(pout, rows, 1, 1)), blk(MG_NTHR);
    mg_by_bool(d.up != 0, [&](auto up) { mg_by_bool(two, [&](auto nb2) {
        hipLaunchKernelGGL((norm_bwd_apply2_vec<T, nb2.value ? 2 : 1, up.value>), grid, blk, 0, st, d, n0, n1); }); });
    return 0;
}

extern "C" int mg_norm_apply2_supported(int32_t dtype, int32_t C)
{
    return dtype == MG_BF16 ? vec_geom_ok<uint16_t>(C) : (dtype == MG_F32 ? vec_geom_ok<float>(C) : 0);
}

extern "C" int mg_norm_bwd_apply2(const mg_norm_apply2_desc* d, void* stream)
{
    MG_CHECK_ARG(d != nullptr, "mg_norm_bwd_apply2: null descriptor");
    MG_CHECK_ARG(d->dtype == MG_F32 || d->dtype == MG_BF16, "mg_norm_bwd_apply2: bad dtype");
    MG_CHECK_ARG(d->dh[0] && d->sums[0] && d->x && d->mean && d->rstd && d->dx, "mg_norm_bwd_apply2: null pointer");
    MG_CHECK_ARG((d->dh[1] == nullptr) == (d->sums[1] == nullptr), "mg_norm_bwd_apply2: the second branch needs dh and sums");
    for (int b = 0; b < 2; ++b)
        MG_CHECK_ARG(d->act[b] != MG_ACT_TANH && (d->h[b] || d->act[b] == MG_ACT_NONE || !d->dh[b]), "mg_norm_bwd_apply2: activation needs its output h");
    MG_CHECK_ARG(d->C > 0 && d->P > 0 && d->P < (1L << 31) && mg_norm_apply2_supported(d->dtype, d->C), "mg_norm_bwd_apply2: unsupported geometry C=%d", d->C);
    MG_CHECK_ARG(!d->up || (d->H > 0 && d->W > 0 && (d->H % 2) == 0 && (d->W % 2) == 0 && d->P % ((int64_t)d->H * d->W) == 0),
                 "mg_norm_bwd_apply2: up needs even H, W and P = N*H*W");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    mg_by_dtype(d->dtype, [&](auto t) { launch_apply2<typename decltype(t)::type>(*d, st); });
    MG_CHECK_LAUNCH("mg_norm_bwd_apply2");
    return MG_OK;
}

extern "C" int mg_norm_bwd_apply(const void* dh, const void* h, const void* x, const void* g1,
                                 int32_t dtype, int32_t G, int64_t P, int32_t C,
                                 const float* mean, const float* rstd, const float* s1, const float* s2,
                                 int32_t sum_gstride, float sum_scale, int32_t act, float slope, void* dx, void* stream)
{
    MG_CHECK_NORM_GEOM("mg_norm_bwd_apply");
    MG_CHECK_ARG(sum_gstride >= C, "mg_norm_bwd_apply: sum_gstride < C");
    const int sgs = sum_gstride; const float sscale = sum_scale;
    MG_CHECK_ARG(dh && (h || act == MG_ACT_NONE) && x && mean && rstd && s1 && s2 && dx, "mg_norm_bwd_apply: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t nq = (int64_t)G * P * (C / 4);
    mg_by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (takes_vec<T>(C, act)) {
            hipLaunchKernelGGL((norm_bwd_apply_vec<T, 2>), dim3(pix_grid(P, vec_rows<T>(C), 2, G), G), dim3(MG_NTHR), 0, st,
                               (const T*)dh, (const T*)h, (const T*)x, (const T*)g1, (T*)dx,
                               P, C, mean, rstd, s1, s2, sgs, sscale, mg_neg_slope(act, slope));
        } else
            hipLaunchKernelGGL(norm_bwd_apply_kernel<T>, dim3(mg_ew_grid(nq, 8192)), dim3(MG_NTHR), 0, st,
                               (const T*)dh, (const T*)h, (const T*)x, (const T*)g1, (T*)dx,
                               nq, P, C, mean, rstd, s1, s2, sgs, sscale, act, slope);
    });
    MG_CHECK_LAUNCH("mg_norm_bwd_apply");
    return MG_OK;
}

extern "C" int mg_norm_finalize(const double* sums, int32_t G, int32_t C, double count, float eps, float momentum,
                                float* running_mean, float* running_var, float* mean, float* rstd, void* stream)
{
    MG_CHECK_ARG(sums && mean && rstd, "mg_norm_finalize: null pointer");
    MG_CHECK_ARG(G > 0 && C > 0 && count > 0, "mg_norm_finalize: bad geometry");
    MG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr) && (running_mean == nullptr || G == 1),
                 "mg_norm_finalize: running statistics need both buffers and G == 1");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(norm_finalize_kernel, dim3((G * C + 255) / 256), dim3(256), 0, st, sums, G, C, count, eps, momentum,
                       running_mean, running_var, mean, rstd);
    MG_CHECK_LAUNCH("mg_norm_finalize");
    return MG_OK;
}
