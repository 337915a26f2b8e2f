// mg_feat_moments.hip -- the style and content terms of the generator objective on one VGG tap (reference: StyleContentLoss,
// models/networks/loss.py:624-711, called at models/pix2pix_model.py:309-319; contract: include/michigan_hip/feature_losses.h).
//
// Style compares the per-(sample, channel) mean and standard deviation of the fake features with the style features', optionally
// under hair masks whose VALUE multiplies; content is a (masked) mean squared error against the content features.  The reference
// spells this as a dozen full-tensor passes and ~25 [N, C] ops per tap; the arithmetic needs one read of each feature map.
//   feat_moment_partial_kernel  3-D grid (pixel chunk, channel tile, sample): a lane owns 16 bytes of channels, a workgroup row a
//                               pixel; fp32 sums of m y, m^3 y, m^4 y, m^4 y^2 (y = x - pivot) for x and s, sum (l (x - t))^2, and
//                               the chunk's mask power sums in double, into the workspace.  The pivot of a chunk is its first pixel
//                               with a non-zero mask: what is masked out is never read
//   feat_moment_final_kernel    a workgroup per (16 channels, sample), 16 lanes over the chunks: un-shifts and adds the chunk partials in a fixed order in
//                               fp64, writes coef {a, b, mu_x, 2 / den}; the workgroup that arrives last adds the workgroups' sums
//                               (fixed order, no float atomics: bit-reproducible) and writes the two outputs
//   feat_moment_bwd_kernel      dx in the features' dtype and layout from x, t, the masks and coef; reduces nothing
#include "mg_common.h"
#include "mg_launch.h"
#include "mg_reduce.h"
#include "michigan_hip/feature_losses.h"
#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int FM_TILE = 256;                // channel vectors of a workgroup at most (wider feature maps take several channel tiles)
constexpr int FM_PLANES = 10;               // part[((n * nchunks + ck) * FM_PLANES + plane) * C + c]: x {A1, A3, A4y, A4, k}, s the same
constexpr int FM_MSUMS = 9;                 // msum[(n * nchunks + ck) * FM_MSUMS + i]: sum m^1..4 of mask_x, of mask_s, sum l
constexpr int FM_PIX = 4;                   // pixels in flight per thread
constexpr int FM_BLOCKS = 2048;             // forward workgroups aimed at
constexpr int FM_MAX_CHUNKS = 256;          // per sample: the final kernel gives a thread one chunk's mask sums
constexpr int FM_MIN_CHUNK = 128;           // pixels: the chunk partials (10 floats per channel) stay a few percent of what the chunk reads
constexpr int FM_FC = 16;                   // channels of a final workgroup (x 16 chunk lanes)

struct FmGeom { int vec, cv, tile_cv, ctiles, rows, nchunks; int64_t chunk; };

inline FmGeom fm_geom(int dtype, int N, int64_t P, int C)
{
    FmGeom g;
    g.vec = dtype == MG_BF16 ? 8 : 4;
    g.cv = C / g.vec;
    g.tile_cv = g.cv < FM_TILE ? g.cv : FM_TILE;
    g.ctiles = (g.cv + FM_TILE - 1) / FM_TILE;
    g.rows = FM_TILE / g.tile_cv;
    int64_t want = FM_BLOCKS / ((int64_t)N * g.ctiles);
    want = want < 1 ? 1 : (want > FM_MAX_CHUNKS ? FM_MAX_CHUNKS : want);
    const int64_t least = (int64_t)g.rows * FM_PIX > FM_MIN_CHUNK ? (int64_t)g.rows * FM_PIX : FM_MIN_CHUNK;   // pixels of a chunk at least
    const int64_t most = (P + least - 1) / least;
    const int64_t cps = want < most ? want : most;
    g.chunk = (P + cps - 1) / cps;
    g.chunk = (g.chunk + g.rows - 1) / g.rows * g.rows;
    g.nchunks = (int)((P + g.chunk - 1) / g.chunk);
    return g;
}

// workspace: [msum: double][bsum: double, one per final workgroup][counter, 16 bytes][part: float][qsum: float]
struct FmLayout { int64_t msum, bsum, cnt, part, qsum, bytes; };

inline FmLayout fm_layout(const FmGeom& g, int N, int C)
{
    FmLayout l;
    l.msum = 0;
    l.bsum = l.msum + (int64_t)N * g.nchunks * FM_MSUMS * 8;
    l.cnt = l.bsum + (int64_t)N * ((C + FM_FC - 1) / FM_FC) * 8;
    l.cnt = (l.cnt + 15) / 16 * 16;
    l.part = l.cnt + 16;
    l.qsum = l.part + (int64_t)N * g.nchunks * FM_PLANES * C * 4;
    l.bytes = l.qsum + (int64_t)N * g.nchunks * g.ctiles * 4;
    l.bytes = (l.bytes + 15) / 16 * 16;
    return l;
}

struct FmArgs {
    const void *x, *s, *t;
    const float *mx, *ms, *ml;
    int64_t sx, ss, sl, P, chunk;
    int N, C, cv, tile_cv, rows, nchunks, ctiles, flags;
    double *msum, *bsum;
    unsigned* cnt;
    float *part, *qsum, *coef, *out;
};

// MASKED: at least one mask pointer is given (a NULL one among them reads as 1).  Unmasked, sum m y = sum m^3 y = sum m^4 y: only
// planes A1 and A4 are formed and the final kernel reads those.
template <typename T, bool MASKED>
__global__ __launch_bounds__(256) void feat_moment_partial_kernel(const FmArgs a)
{
    constexpr int VEC = EV<T>::VEC;
    __shared__ float red[3][256 * VEC];
    __shared__ double mred[FM_MSUMS][4];
    __shared__ float qred[4];
    __shared__ int piv[2];
    const int tid = threadIdx.x, ck = blockIdx.x, ct = blockIdx.y, n = blockIdx.z;
    const int tq = tid % a.tile_cv, tr = tid / a.tile_cv;
    const int cvec = ct * FM_TILE + tq;
    const bool active = tr < a.rows && cvec < a.cv;
    const int c = cvec * VEC;
    const bool style = (a.flags & MG_FEAT_STYLE) != 0, content = (a.flags & MG_FEAT_CONTENT) != 0;
    const int64_t p0 = (int64_t)ck * a.chunk;
    const int64_t p1 = p0 + a.chunk < a.P ? p0 + a.chunk : a.P;
    const float* __restrict__ mx = a.mx ? a.mx + (int64_t)n * a.sx : nullptr;
    const float* __restrict__ ms = a.ms ? a.ms + (int64_t)n * a.ss : nullptr;
    const float* __restrict__ ml = a.ml ? a.ml + (int64_t)n * a.sl : nullptr;
    if (tid == 0 && ck == 0 && ct == 0 && n == 0) *a.cnt = 0u;           // the final kernel's arrival counter

    // ---- the chunk's masks: power sums in double and the first non-zero pixel of mask_x / mask_s (the pivots) ----
    if (tid < 2) piv[tid] = INT_MAX;
    __syncthreads();
    double md[FM_MSUMS];
    {
#pragma unroll
        for (int i = 0; i < FM_MSUMS; ++i) md[i] = 0.0;
        int fx = INT_MAX, fs = INT_MAX;
        for (int64_t p = p0 + tid; p < p1; p += 256) {
            if (style) {
                const double m = mx ? (double)mx[p] : 1.0, v = ms ? (double)ms[p] : 1.0;
                if (m != 0.0 && fx == INT_MAX) fx = (int)(p - p0);
                if (v != 0.0 && fs == INT_MAX) fs = (int)(p - p0);
                const double m2 = m * m, v2 = v * v;
                md[0] += m; md[1] += m2; md[2] += m2 * m; md[3] += m2 * m2;
                md[4] += v; md[5] += v2; md[6] += v2 * v; md[7] += v2 * v2;
            }
            if (content) md[8] += ml ? (double)ml[p] : 1.0;
        }
        if (fx != INT_MAX) atomicMin(&piv[0], fx);
        if (fs != INT_MAX) atomicMin(&piv[1], fs);
    }
    const double msum = mg_block_sum_to<MgJoin::Pairwise>(md, mred);        // its barrier also orders the pivots
    if (ct == 0 && tid < FM_MSUMS) a.msum[((int64_t)n * a.nchunks + ck) * FM_MSUMS + tid] = msum;
    const int px = piv[0], ps = piv[1];

    const T* __restrict__ xb = (const T*)a.x + (int64_t)n * a.P * a.C + c;
    const T* __restrict__ sb = (const T*)a.s + (int64_t)n * a.P * a.C + c;
    const T* __restrict__ tb = (const T*)a.t + (int64_t)n * a.P * a.C + c;
    float kx[VEC], ks[VEC], acc[8][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        kx[j] = 0.f; ks[j] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q][j] = 0.f;
    }
    float qs = 0.f;
    if (active) {
        if (style && px != INT_MAX) EV<T>::load(xb + (p0 + px) * a.C, kx);
        if (style && ps != INT_MAX) EV<T>::load(sb + (p0 + ps) * a.C, ks);
        for (int64_t pp = p0 + tr; pp < p1; pp += (int64_t)a.rows * FM_PIX) {
            uint4 rx[FM_PIX], rs[FM_PIX], rt[FM_PIX];
            float vm[FM_PIX], vs[FM_PIX], vl[FM_PIX];
#pragma unroll
            for (int k = 0; k < FM_PIX; ++k) {
                const int64_t p = pp + (int64_t)k * a.rows;
                const bool ok = p < p1;
                vm[k] = (ok && style) ? (mx ? mx[p] : 1.f) : 0.f;
                vs[k] = (ok && style) ? (ms ? ms[p] : 1.f) : 0.f;
                vl[k] = (ok && content) ? (ml ? ml[p] : 1.f) : 0.f;
                if (vm[k] != 0.f || vl[k] != 0.f) rx[k] = EV<T>::raw(xb + p * a.C);
                if (vs[k] != 0.f) rs[k] = EV<T>::raw(sb + p * a.C);
                if (vl[k] != 0.f) rt[k] = EV<T>::raw(tb + p * a.C);
            }
#pragma unroll
            for (int k = 0; k < FM_PIX; ++k) {
                float xv[VEC], ov[VEC];
                if (vm[k] != 0.f || vl[k] != 0.f) EV<T>::decode(rx[k], xv);
                if (vm[k] != 0.f) {
                    const float m = vm[k], m2 = m * m, m3 = m2 * m, m4 = m2 * m2;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float y = xv[j] - kx[j];
                        if (MASKED) {
                            const float my = m4 * y;
                            acc[0][j] += m * y; acc[1][j] += m3 * y; acc[2][j] += my; acc[3][j] += my * y;
                        } else { acc[0][j] += y; acc[3][j] += y * y; }
                    }
                }
                if (vs[k] != 0.f) {
                    EV<T>::decode(rs[k], ov);
                    const float m = vs[k], m2 = m * m, m3 = m2 * m, m4 = m2 * m2;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const float y = ov[j] - ks[j];
                        if (MASKED) {
                            const float my = m4 * y;
                            acc[4][j] += m * y; acc[5][j] += m3 * y; acc[6][j] += my; acc[7][j] += my * y;
                        } else { acc[4][j] += y; acc[7][j] += y * y; }
                    }
                }
                if (vl[k] != 0.f) {
                    EV<T>::decode(rt[k], ov);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) { const float d = vl[k] * (xv[j] - ov[j]); qs += d * d; }
                }
            }
        }
    }

    // ---- the rows of the workgroup, in a fixed order ----
    if (style) {
        float* __restrict__ dst = a.part + ((int64_t)n * a.nchunks + ck) * FM_PLANES * a.C + c;
        const bool wr = active && tr == 0;
        auto put = [&](int slot, float (&v)[VEC]) { float* const t[1] = {v}; mg_rows_put<1, VEC>(t, red[slot]); };
        auto fold = [&](int slot, float (&v)[VEC], int plane) {                 // the row join of mg_reduce.h, one term per LDS slot
            if (!wr) return;
            float* const t[1] = {v};
            mg_rows_fold<1, VEC>(t, red[slot], a.tile_cv, a.rows);
#pragma unroll
            for (int j = 0; j < VEC; ++j) dst[(int64_t)plane * a.C + j] = v[j];
        };
        const bool lds = a.rows > 1;                                      // uniform
        if (MASKED) {
            if (lds) { __syncthreads(); put(0, acc[0]); put(1, acc[1]); put(2, acc[2]); __syncthreads(); }
            fold(0, acc[0], 0); fold(1, acc[1], 1); fold(2, acc[2], 2);
            if (lds) { __syncthreads(); put(0, acc[3]); put(1, acc[4]); put(2, acc[5]); __syncthreads(); }
            fold(0, acc[3], 3); fold(1, acc[4], 5); fold(2, acc[5], 6);
            if (lds) { __syncthreads(); put(0, acc[6]); put(1, acc[7]); __syncthreads(); }
            fold(0, acc[6], 7); fold(1, acc[7], 8);
        } else {
            if (lds) { __syncthreads(); put(0, acc[0]); put(1, acc[3]); put(2, acc[4]); __syncthreads(); }
            fold(0, acc[0], 0); fold(1, acc[3], 3); fold(2, acc[4], 5);
            if (lds) { __syncthreads(); put(0, acc[7]); __syncthreads(); }
            fold(0, acc[7], 8);
        }
        if (wr) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) { dst[4 * (int64_t)a.C + j] = kx[j]; dst[9 * (int64_t)a.C + j] = ks[j]; }
        }
    }
    if (content) {
        const float q = mg_block_sum_to<MgJoin::Pairwise>(qs, qred);
        if (tid == 0) a.qsum[((int64_t)n * a.nchunks + ck) * a.ctiles + ct] = q;
    }
}

__global__ __launch_bounds__(256) void feat_moment_final_kernel(const FmArgs a, int style_masked, int content_masked)
{
    __shared__ double red[6][FM_FC][FM_FC];
    __shared__ double mred[FM_MSUMS][4];
    __shared__ double scratch[4];
    __shared__ int last;
    const int tid = threadIdx.x, cl = tid % FM_FC, kl = tid / FM_FC, n = blockIdx.y;   // 16 channels x 16 chunk lanes
    const int c = blockIdx.x * FM_FC + cl;
    const bool style = (a.flags & MG_FEAT_STYLE) != 0, content = (a.flags & MG_FEAT_CONTENT) != 0;
    const double P = (double)a.P;

    // the sample's mask power sums (one chunk per thread: nchunks <= 256) and sum l over ALL samples (every workgroup adds the
    // chunks in the same order)
    double tm[FM_MSUMS];
#pragma unroll
    for (int i = 0; i < 8; ++i) tm[i] = (style && tid < a.nchunks) ? a.msum[((int64_t)n * a.nchunks + tid) * FM_MSUMS + i] : 0.0;
    tm[8] = 0.0;
    if (content && content_masked)
        for (int64_t i = tid; i < (int64_t)a.N * a.nchunks; i += 256) tm[8] += a.msum[i * FM_MSUMS + 8];
    mg_put_wave_sums(tm, mred);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FM_MSUMS; ++i) tm[i] = mg_join<MgJoin::Pairwise>(mred[i]);      // every thread needs all nine
    double two_over_den = 0.0, den = 1.0;
    if (content) {
        den = content_masked ? (double)a.C * tm[8] + 1e-5 : (double)a.N * P * (double)a.C;
        two_over_den = 2.0 / den;
    }

    double e = 0.0;
    if (style) {
        double sx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};               // sum m x, sum m^3 x, sum m^4 x^2 of x; of s
        if (c < a.C) {
            for (int ck = kl; ck < a.nchunks; ck += FM_FC) {
                const float* __restrict__ src = a.part + ((int64_t)n * a.nchunks + ck) * FM_PLANES * a.C + c;
                const double* __restrict__ m = a.msum + ((int64_t)n * a.nchunks + ck) * FM_MSUMS;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const double a1 = (double)src[(5 * h + 0) * (int64_t)a.C], a4 = (double)src[(5 * h + 3) * (int64_t)a.C];
                    const double a3 = style_masked ? (double)src[(5 * h + 1) * (int64_t)a.C] : a1;
                    const double a4y = style_masked ? (double)src[(5 * h + 2) * (int64_t)a.C] : a1;
                    const double k = (double)src[(5 * h + 4) * (int64_t)a.C];
                    sx[3 * h + 0] += a1 + k * m[4 * h + 0];
                    sx[3 * h + 1] += a3 + k * m[4 * h + 2];
                    sx[3 * h + 2] += a4 + 2.0 * k * a4y + k * k * m[4 * h + 3];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) red[q][kl][cl] = sx[q];
        __syncthreads();
        if (kl == 0 && c < a.C) {
            double t[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                t[q] = red[q][0][cl];
                for (int k = 1; k < FM_FC; ++k) t[q] += red[q][k][cl];         // fixed order
            }
            double mu[2], sg[2], S[2], T = 0.0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                S[h] = style_masked ? tm[4 * h] + 1e-5 : P;
                mu[h] = t[3 * h] / S[h];
                double r = t[3 * h + 2] - 2.0 * mu[h] * t[3 * h + 1] + mu[h] * mu[h] * tm[4 * h + 1];
                r = r > 0.0 ? r : 0.0;
                sg[h] = sqrt(r / (style_masked ? S[h] : P - 1.0) + 1e-5);
                if (h == 0) T = t[1] - mu[0] * tm[1];
            }
            const double inv_nc = 1.0 / ((double)a.N * (double)a.C);
            const double dm = mu[0] - mu[1], ds = sg[0] - sg[1];
            const double gm = 2.0 * dm * inv_nc, gs = 2.0 * ds * inv_nc;
            e = dm * dm + ds * ds;
            const double ca = style_masked ? gm / S[0] - gs * T / (sg[0] * S[0] * S[0]) : gm / P;
            const double cb = style_masked ? gs / (sg[0] * S[0]) : gs / (sg[0] * (P - 1.0));
            const f32x4_t v = {(float)ca, (float)cb, (float)mu[0], (float)two_over_den};
            ET<float>::store4(a.coef + 4 * ((int64_t)n * a.C + c), v);
        }
    } else if (kl == 0 && c < a.C) {
        const f32x4_t v = {0.f, 0.f, 0.f, (float)two_over_den};
        ET<float>::store4(a.coef + 4 * ((int64_t)n * a.C + c), v);
    }
    e = mg_block_sum_all<MgJoin::Pairwise>(e, scratch);                   // the chunk lanes 1..15 hold 0

    // ---- arrival: the workgroup's sum is published, the last workgroup to arrive adds them all ----
    const int nblocks = gridDim.x * gridDim.y;
    if (tid == 0) {
        a.bsum[(int64_t)n * gridDim.x + blockIdx.x] = e;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(a.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = ticket == (unsigned)(nblocks - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    double st = 0.0, q = 0.0;
    if (style) for (int i = tid; i < nblocks; i += 256) st += a.bsum[i];
    if (content) for (int64_t i = tid; i < (int64_t)a.N * a.nchunks * a.ctiles; i += 256) q += (double)a.qsum[i];
    st = mg_block_sum_all<MgJoin::Pairwise>(st, scratch);
    q = mg_block_sum_all<MgJoin::Pairwise>(q, scratch);
    if (tid == 0) {
        a.out[0] = style ? (float)(st / ((double)a.N * (double)a.C)) : 0.f;
        a.out[1] = content ? (float)(q / den) : 0.f;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void feat_moment_bwd_kernel(const FmArgs a, const float* __restrict__ g_style, const float* __restrict__ g_content,
                                                              T* __restrict__ dx)
{
    constexpr int VEC = EV<T>::VEC;
    const int tid = threadIdx.x, ct = blockIdx.y, n = blockIdx.z;
    const int tq = tid % a.tile_cv, tr = tid / a.tile_cv;
    const int cvec = ct * FM_TILE + tq;
    if (!(tr < a.rows && cvec < a.cv)) return;
    const int c = cvec * VEC;
    const bool style = (a.flags & MG_FEAT_STYLE) && g_style, content = (a.flags & MG_FEAT_CONTENT) && g_content;
    const float* __restrict__ mx = a.mx ? a.mx + (int64_t)n * a.sx : nullptr;
    const float* __restrict__ ml = a.ml ? a.ml + (int64_t)n * a.sl : nullptr;
    float ca[VEC], cb[VEC], mu[VEC], gc = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { ca[j] = 0.f; cb[j] = 0.f; mu[j] = 0.f; }
    if (style || content) {
        const float gs = style ? g_style[0] : 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const f32x4_t v = ET<float>::load4(a.coef + 4 * ((int64_t)n * a.C + c + j));
            ca[j] = gs * v[0]; cb[j] = gs * v[1]; mu[j] = v[2];
            if (content) gc = g_content[0] * v[3];
        }
    }
    const T* __restrict__ xb = (const T*)a.x + (int64_t)n * a.P * a.C + c;
    const T* __restrict__ tb = (const T*)a.t + (int64_t)n * a.P * a.C + c;
    T* __restrict__ ob = dx + (int64_t)n * a.P * a.C + c;
    const int64_t step = (int64_t)gridDim.x * a.rows;
    for (int64_t pp = (int64_t)blockIdx.x * a.rows + tr; pp < a.P; pp += step * FM_PIX) {
        uint4 rx[FM_PIX], rt[FM_PIX];
        float vm[FM_PIX], vl[FM_PIX];
#pragma unroll
        for (int k = 0; k < FM_PIX; ++k) {
            const int64_t p = pp + k * step;
            const bool ok = p < a.P;
            vm[k] = (ok && style) ? (mx ? mx[p] : 1.f) : 0.f;
            vl[k] = (ok && content) ? (ml ? ml[p] : 1.f) : 0.f;
            if (vm[k] != 0.f || vl[k] != 0.f) rx[k] = EV<T>::raw(xb + p * a.C);
            if (vl[k] != 0.f) rt[k] = EV<T>::raw(tb + p * a.C);
        }
#pragma unroll
        for (int k = 0; k < FM_PIX; ++k) {
            const int64_t p = pp + k * step;
            if (p >= a.P) continue;
            float xv[VEC], tv[VEC], o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = 0.f;
            if (vm[k] != 0.f || vl[k] != 0.f) EV<T>::decode(rx[k], xv);
            if (vm[k] != 0.f) {
                const float m = vm[k], m3 = m * m * m;
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = m * ca[j] + m3 * cb[j] * (m * xv[j] - mu[j]);
            }
            if (vl[k] != 0.f) {
                EV<T>::decode(rt[k], tv);
                const float g = gc * (vl[k] * vl[k]);
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] += g * (xv[j] - tv[j]);
            }
            EV<T>::store(ob + p * a.C, o);
        }
    }
}

inline bool fm_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// everything both entry points check; fills the kernel arguments
int fm_check(const char* name, const mg_feat_moment_desc* d, FmArgs& a, FmGeom& g)
{
    MG_CHECK_ARG(d, "%s: null pointer (descriptor)", name);
    MG_CHECK_ARG(d->dtype == MG_F32 || d->dtype == MG_BF16, "%s: bad dtype", name);
    const int vec = d->dtype == MG_BF16 ? 8 : 4;
    MG_CHECK_ARG(d->N > 0 && d->N <= 65535 && d->P > 0 && d->P < ((int64_t)1 << 31) && d->C > 0,
                 "%s: bad geometry N=%d P=%lld C=%d", name, d->N, (long long)d->P, d->C);
    MG_CHECK_ARG(d->C % vec == 0, "%s: a lane owns 16 bytes of channels: C=%d is not a multiple of %d", name, d->C, vec);
    MG_CHECK_ARG(d->flags >= 1 && d->flags <= 3, "%s: flags must select at least one of style (1), content (2)", name);
    MG_CHECK_ARG(d->x && d->coef, "%s: null pointer", name);
    MG_CHECK_ARG(fm_aligned(d->x) && fm_aligned(d->coef), "%s: x and coef must be 16-byte aligned", name);
    if (d->flags & MG_FEAT_STYLE) {
        MG_CHECK_ARG(!d->mask_x || d->mask_x_nstride >= d->P, "%s: a style mask plane has a sample stride below P", name);
        MG_CHECK_ARG(d->mask_x || d->P >= 2, "%s: the unbiased variance needs P >= 2", name);
    }
    if (d->flags & MG_FEAT_CONTENT) {
        MG_CHECK_ARG(d->t && fm_aligned(d->t), "%s: the content term needs the content features (16-byte aligned)", name);
        MG_CHECK_ARG(!d->mask_t || d->mask_t_nstride >= d->P, "%s: the content mask plane has a sample stride below P", name);
    }
    g = fm_geom(d->dtype, d->N, d->P, d->C);
    const bool st = d->flags & MG_FEAT_STYLE, co = d->flags & MG_FEAT_CONTENT;
    a = FmArgs{};
    a.x = d->x; a.s = st ? d->s : nullptr; a.t = co ? d->t : nullptr;
    a.mx = st ? d->mask_x : nullptr; a.ms = st ? d->mask_s : nullptr; a.ml = co ? d->mask_t : nullptr;
    a.sx = d->mask_x_nstride; a.ss = d->mask_s_nstride; a.sl = d->mask_t_nstride;
    a.P = d->P; a.chunk = g.chunk;
    a.N = d->N; a.C = d->C; a.cv = g.cv; a.tile_cv = g.tile_cv; a.rows = g.rows; a.nchunks = g.nchunks; a.ctiles = g.ctiles; a.flags = d->flags;
    a.coef = d->coef; a.out = d->out;
    return MG_OK;
}

}  // namespace

extern "C" int64_t mg_feat_moment_workspace(int32_t N, int64_t P, int32_t C)
{
    if (N <= 0 || N > 65535 || P <= 0 || P >= ((int64_t)1 << 31) || C <= 0 || C % 4) return 0;
    const int64_t f32 = fm_layout(fm_geom(MG_F32, N, P, C), N, C).bytes;
    const int64_t bf16 = C % 8 ? 0 : fm_layout(fm_geom(MG_BF16, N, P, C), N, C).bytes;
    return f32 > bf16 ? f32 : bf16;
}

extern "C" int mg_feat_moment_loss_fwd(const mg_feat_moment_desc* d, void* stream)
{
    FmArgs a;
    FmGeom g;
    if (int rc = fm_check("mg_feat_moment_loss_fwd", d, a, g)) return rc;
    MG_CHECK_ARG(d->out && d->ws, "mg_feat_moment_loss_fwd: null pointer (out / ws)");
    MG_CHECK_ARG(fm_aligned(d->ws), "mg_feat_moment_loss_fwd: ws must be 16-byte aligned");
    if (d->flags & MG_FEAT_STYLE) {
        MG_CHECK_ARG(d->s && fm_aligned(d->s), "mg_feat_moment_loss_fwd: the style term needs the style features (16-byte aligned)");
        MG_CHECK_ARG((d->mask_x != nullptr) == (d->mask_s != nullptr), "mg_feat_moment_loss_fwd: mask_x and mask_s are given together or not at all");
        MG_CHECK_ARG(!d->mask_s || d->mask_s_nstride >= d->P, "mg_feat_moment_loss_fwd: a style mask plane has a sample stride below P");
    }
    const FmLayout l = fm_layout(g, d->N, d->C);
    char* ws = static_cast<char*>(d->ws);
    a.msum = reinterpret_cast<double*>(ws + l.msum); a.bsum = reinterpret_cast<double*>(ws + l.bsum);
    a.cnt = reinterpret_cast<unsigned*>(ws + l.cnt);
    a.part = reinterpret_cast<float*>(ws + l.part); a.qsum = reinterpret_cast<float*>(ws + l.qsum);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool masked = a.mx || a.ml;
    const dim3 grid(g.nchunks, g.ctiles, d->N);
    mg_by_dtype(d->dtype, [&](auto t) { using T = typename decltype(t)::type;
        if (masked) hipLaunchKernelGGL((feat_moment_partial_kernel<T, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((feat_moment_partial_kernel<T, false>), grid, dim3(256), 0, st, a); });
    MG_CHECK_LAUNCH("mg_feat_moment_loss_fwd");
    hipLaunchKernelGGL(feat_moment_final_kernel, dim3((d->C + FM_FC - 1) / FM_FC, d->N), dim3(256), 0, st, a, a.mx != nullptr, a.ml != nullptr);
    MG_CHECK_LAUNCH("mg_feat_moment_loss_fwd(final)");
    return MG_OK;
}

extern "C" int mg_feat_moment_loss_bwd(const mg_feat_moment_desc* d, const float* g_style, const float* g_content, void* dx, void* stream)
{
    FmArgs a;
    FmGeom g;
    if (int rc = fm_check("mg_feat_moment_loss_bwd", d, a, g)) return rc;
    MG_CHECK_ARG(dx && fm_aligned(dx), "mg_feat_moment_loss_bwd: null pointer (dx; 16-byte aligned)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t gx = (d->P + (int64_t)g.rows * FM_PIX - 1) / ((int64_t)g.rows * FM_PIX);
    const int64_t cap = 8192 / ((int64_t)d->N * g.ctiles);
    gx = gx > cap ? (cap < 1 ? 1 : cap) : gx;
    const dim3 grid((unsigned)gx, g.ctiles, d->N);
    mg_by_dtype(d->dtype, [&](auto t) { using T = typename decltype(t)::type;
        hipLaunchKernelGGL(feat_moment_bwd_kernel<T>, grid, dim3(256), 0, st, a, g_style, g_content, (T*)dx); });
    MG_CHECK_LAUNCH("mg_feat_moment_loss_bwd");
    return MG_OK;
}
