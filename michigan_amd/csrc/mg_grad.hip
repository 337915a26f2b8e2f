// mg_grad.hip -- batched "drain" of the GEMM-order weight-gradient arena into the reference-layout gradient arena.
//
// Before: every conv backward zero-filled a scratch buffer, ran its wgrad kernel (fp32 atomics, GEMM order
// [taps][rows][cols]), launched an unpack kernel into a fresh reference-layout tensor, for spectral-normed layers a dot
// + the sigma-backward kernel, and autograd then added the result into the flat gradient arena: ~375 launches of
// 5-10 us per training step (fills 95, unpack 74, dot + sn_bwd 48, adds 158; 2.9 ms of a 75 ms step, rocprofv3
// profiles/r02a_kernel_stats.csv).  Now the wgrad kernels accumulate straight into a persistent GEMM-order arena that
// stays resident (optim.FlatAdam.gemm) and two (three with spectral norm) launches per optimiser step move everything:
//   grad_sn_dot_kernel   spectral-normed slots only:  per-tile partials of s = sum(g * W_sn); grad_sn_finish_kernel adds them in a
//                        fixed order (bit-identical on every rank of a data-parallel job)
//   grad_drain_kernel    every slot:  dst[co][ci][t] += SN ? (g - s u[co] v[ci*T+t]) / sigma : g ;  gemm <- 0 ;  biases
// (reference: torch.autograd of nn.Conv2d weights + torch.nn.utils.spectral_norm, architecture.py:31-42,
//  normalization.py:28-29,94-99; optimiser arenas pix2pix_model.py:137-145).
//
// Tiling: a workgroup owns (slot, tensor, CO_PER output channels, 64 input channels, all T taps).  The GEMM image is
// read tap by tap as 256-byte rows (coalesced; with swapped roles as 16-byte pieces, the CO_PER channels of one input
// channel), transposed through LDS (pitch T|1) and written / read-modify-written as contiguous 64*T-float runs of the
// reference tensor.  For T <= 16 the CO_PER tiles go through LDS TOGETHER (17 KB): every thread issues all its loads before
// the first LDS write, there is one barrier pair per workgroup, and the accesses are 16 bytes wide wherever the rows are
// 16-byte aligned (4-byte fallback: a 3-channel layer has runs of 27 floats).  The first version handled the channels one
// after the other with 4-byte accesses and two barriers each.  7x7 windows (4 x 64 x 49 floats = 50 KB) stay on that path.
// HBM-bound: ~16 B per gradient element (+4 B of W_sn for spectral-normed layers); no MFMA.
#include "mg_common.h"
#include "mg_reduce.h"

namespace {

constexpr int CO_PER = 4;                 // output channels per workgroup
constexpr int MAXT = 49;                  // 7x7 is the largest window on the path

struct Tile { int slot, which, co0, ci0, bias; };

__device__ __forceinline__ Tile decode(const mg_grad_slot* __restrict__ tab, const int32_t* __restrict__ block_slot, int b)
{
    Tile t;
    t.slot = block_slot[b];
    const mg_grad_slot& s = tab[t.slot];
    int rel = b - (int)s.first_block;
    const int ci_blocks = (s.cin + 63) >> 6, co_groups = (s.cout + CO_PER - 1) / CO_PER;
    const int per_tensor = ci_blocks * co_groups;
    const int ntens = s.dst1 ? 2 : 1;
    t.bias = rel >= per_tensor * ntens;
    t.which = t.bias ? 0 : rel / per_tensor;
    rel -= t.which * per_tensor;
    t.co0 = (rel / ci_blocks) * CO_PER;
    t.ci0 = (rel % ci_blocks) << 6;
    return t;
}

// GEMM row of output channel co (plain: co; fused SPADE pair: [32 gamma | 32 beta] blocks)
__device__ __forceinline__ int gemm_row(int co, int which, bool two) { return two ? 64 * (co >> 5) + (co & 31) + 32 * which : co; }

// load the tile's [T][64] GEMM values of channel `co` into LDS as lds[ci_local * pitch + t]; optionally zero the source
template <bool ZERO>
__device__ __forceinline__ void load_tile(const mg_grad_slot& s, int which, int co, int ci0, float* lds, int pitch)
{
    const int T = s.taps, r = gemm_row(co, which, s.dst1 != nullptr);
    const int c = threadIdx.x & 63, ci = ci0 + c;
    for (int t = threadIdx.x >> 6; t < T; t += 4) {
        float v = 0.f;
        if (ci < s.cin) {
            float* p = s.swapped ? s.gemm + ((size_t)t * s.cols + ci) * s.rows + r      // swapped roles: [T][cin][rows]
                                 : s.gemm + ((size_t)t * s.rows + r) * s.cols + ci;
            v = *p;
            if (ZERO) *p = 0.f;
        }
        lds[c * pitch + t] = v;
    }
}

constexpr int JOINT_MAXT = 16;            // windows whose CO_PER tiles share the LDS buffer
constexpr int LDS_FLOATS = CO_PER * 64 * (JOINT_MAXT + 1) > 64 * (MAXT + 1) ? CO_PER * 64 * (JOINT_MAXT + 1) : 64 * (MAXT + 1);

// T <= 16: the tile's GEMM values of channels co0 .. co0 + CO_PER - 1 into LDS as lds[(k * 64 + ci_local) * pitch + t]; optionally
// zero the source.  Elements of channels past cout / input channels past cin that a 16-byte piece carries along are padding of
// the GEMM image (inside its rows x cols extent): they land in LDS cells nobody reads, and zeroing them changes nothing.
template <bool ZERO>
__device__ __forceinline__ void load_tiles(const mg_grad_slot& s, int which, int co0, int ci0, float* lds, int pitch)
{
    const int T = s.taps, tid = threadIdx.x;
    const bool two = s.dst1 != nullptr;
    const int r0 = gemm_row(co0, which, two);                    // co0 % 4 == 0: the CO_PER channels are rows r0 .. r0 + 3
    const bool aligned = ((uintptr_t)s.gemm & 15) == 0;
    if (s.swapped && aligned && (s.rows & 3) == 0) {             // [T][cin][rows]: one 16-byte piece = the four channels of (t, ci)
        float4 v[4];
        float* p[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = tid + m * 256, t = i >> 6, c = i & 63;
            p[m] = (t < T && ci0 + c < s.cin) ? s.gemm + ((size_t)t * s.cols + ci0 + c) * s.rows + r0 : nullptr;
            v[m] = p[m] ? *reinterpret_cast<const float4*>(p[m]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = tid + m * 256, t = i >> 6, c = i & 63;
            if (t >= T) break;
            if (ZERO && p[m]) *reinterpret_cast<float4*>(p[m]) = make_float4(0.f, 0.f, 0.f, 0.f);
            lds[(0 * 64 + c) * pitch + t] = v[m].x; lds[(1 * 64 + c) * pitch + t] = v[m].y;
            lds[(2 * 64 + c) * pitch + t] = v[m].z; lds[(3 * 64 + c) * pitch + t] = v[m].w;
        }
        return;
    }
    if (!s.swapped && aligned && (s.cols & 3) == 0) {            // [T][rows][cols]: 16 pieces per 64-column row, rows j = (t, k)
        float4 v[4];
        float* p[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = tid + m * 256, j = i >> 4, c = (i & 15) * 4, k = j & 3, t = j >> 2;
            p[m] = (t < T && co0 + k < s.cout && ci0 + c < s.cin) ? s.gemm + ((size_t)t * s.rows + r0 + k) * s.cols + ci0 + c : nullptr;
            v[m] = p[m] ? *reinterpret_cast<const float4*>(p[m]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int i = tid + m * 256, j = i >> 4, c = (i & 15) * 4, k = j & 3, t = j >> 2;
            if (t >= T) break;
            if (ZERO && p[m]) *reinterpret_cast<float4*>(p[m]) = make_float4(0.f, 0.f, 0.f, 0.f);
            float* l = lds + (k * 64 + c) * pitch + t;
            l[0] = v[m].x; l[pitch] = v[m].y; l[2 * pitch] = v[m].z; l[3 * pitch] = v[m].w;
        }
        return;
    }
    float v[JOINT_MAXT];                                         // 4-byte accesses: rows j = (t, k), one column per lane
    float* p[JOINT_MAXT];
    const int c = tid & 63, ci = ci0 + c;
#pragma unroll
    for (int m = 0; m < JOINT_MAXT; ++m) {
        const int j = (tid >> 6) + m * 4, k = j & 3, t = j >> 2;
        p[m] = nullptr;
        if (t < T && co0 + k < s.cout && ci < s.cin)
            p[m] = s.swapped ? s.gemm + ((size_t)t * s.cols + ci) * s.rows + r0 + k : s.gemm + ((size_t)t * s.rows + r0 + k) * s.cols + ci;
        v[m] = p[m] ? *p[m] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < JOINT_MAXT; ++m) {
        const int j = (tid >> 6) + m * 4, k = j & 3, t = j >> 2;
        if (t >= T) break;
        if (ZERO && p[m]) *p[m] = 0.f;
        lds[(k * 64 + c) * pitch + t] = v[m];
    }
}

__global__ __launch_bounds__(256) void grad_sn_dot_kernel(const mg_grad_slot* __restrict__ tab, const int32_t* __restrict__ block_slot,
                                                          double* __restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ double red[4];
    const Tile tl = decode(tab, block_slot, blockIdx.x);
    const mg_grad_slot& s = tab[tl.slot];
    if (tl.bias || !s.w_sn) { if (threadIdx.x == 0) partial[blockIdx.x] = 0.0; return; }
    const int T = s.taps, pitch = T | 1;
    const int ncol = min(64, s.cin - tl.ci0), run = ncol * T;
    // element e of the contiguous run <-> (column c = e / T, tap t = e % T), walked without divisions in the loop
    const int c0 = (int)threadIdx.x / T, t0 = (int)threadIdx.x - c0 * T, dc = 256 / T, dt = 256 - dc * T;
    double acc = 0.0;
    // The sum keeps its order in both branches: thread i adds the products of elements i, i + 256, ... of a channel in fp32, the
    // channels' sums in double, then the block and the slot in a fixed order -- the bits every rank must agree on (and the bits of
    // the version with one barrier pair per channel).  Hence W_sn is read as coalesced 4-byte loads here, all of them in flight
    // before the first product.
    if (T <= JOINT_MAXT) {
        float wv[CO_PER][4];                                     // <= ceil(64 * 16 / 256) = 4 elements per thread and channel
#pragma unroll
        for (int k = 0; k < CO_PER; ++k) {
            const float* w = s.w_sn + ((size_t)min(tl.co0 + k, s.cout - 1) * s.cin + tl.ci0) * T;
#pragma unroll
            for (int m = 0; m < 4; ++m) { const int e = threadIdx.x + m * 256; wv[k][m] = e < run ? w[e] : 0.f; }
        }
        load_tiles<false>(s, 0, tl.co0, tl.ci0, lds, pitch);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CO_PER; ++k) {
            if (tl.co0 + k >= s.cout) break;
            const float* l = lds + k * 64 * pitch;
            float part = 0.f;
            int c = c0, t = t0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if ((int)threadIdx.x + m * 256 < run) part += l[c * pitch + t] * wv[k][m];
                c += dc; t += dt;
                if (t >= T) { t -= T; ++c; }
            }
            acc += (double)part;
        }
    } else {
        for (int k = 0; k < CO_PER && tl.co0 + k < s.cout; ++k) {
            const int co = tl.co0 + k;
            __syncthreads();
            load_tile<false>(s, 0, co, tl.ci0, lds, pitch);
            __syncthreads();
            const float* w = s.w_sn + ((size_t)co * s.cin + tl.ci0) * T;
            float part = 0.f;                                    // <= ceil(64 * 49 / 256) = 13 products per thread and channel
            for (int e = threadIdx.x, c = c0, t = t0; e < run; e += 256) {
                part += lds[c * pitch + t] * w[e];
                c += dc; t += dt;
                if (t >= T) { t -= T; ++c; }
            }
            acc += (double)part;
        }
    }
    const double t = mg_block_sum_to<MgJoin::LeftToRight>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// s[slot] = sum of the slot's per-workgroup partials in a FIXED order (one workgroup per slot): the value every rank of a
// data-parallel job computes from the same all-reduced gradients must be bit-identical, or the replicas' weights drift apart
__global__ __launch_bounds__(256) void grad_sn_finish_kernel(const mg_grad_slot* __restrict__ tab, const double* __restrict__ partial, int nblocks_total,
                                                             const int32_t* __restrict__ block_slot)
{
    __shared__ double red[256];
    const mg_grad_slot& s = tab[blockIdx.x];
    if (!s.w_sn) return;
    const int b0 = (int)s.first_block;
    double acc = 0.0;
    for (int b = b0 + threadIdx.x; b < nblocks_total && block_slot[b] == (int)blockIdx.x; b += 256) acc += partial[b];
    mg_tree_sum_f64(acc, red);
    if (threadIdx.x == 0) *s.s = red[0];
}

__global__ __launch_bounds__(256) void grad_drain_kernel(const mg_grad_slot* __restrict__ tab, const int32_t* __restrict__ block_slot)
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const Tile tl = decode(tab, block_slot, blockIdx.x);
    const mg_grad_slot& s = tab[tl.slot];
    if (tl.bias) {
        if (!s.dbias_gemm) return;
        const bool two = s.dbias1 != nullptr;
        for (int co = threadIdx.x; co < s.cout; co += 256) {
            for (int which = 0; which < (two ? 2 : 1); ++which) {
                float* p = s.dbias_gemm + gemm_row(co, which, two);
                (which ? s.dbias1 : s.dbias0)[co] += *p;
                *p = 0.f;
            }
        }
        return;
    }
    const int T = s.taps, pitch = T | 1;
    const int ncol = min(64, s.cin - tl.ci0), run = ncol * T;
    const bool sn = s.w_sn != nullptr;
    float sv = 0.f, inv_sigma = 1.f;
    if (sn) { sv = (float)*s.s; inv_sigma = 1.f / *s.sigma; }
    float* const dst = tl.which ? s.dst1 : s.dst0;
    const float* vv = sn ? s.v + (size_t)tl.ci0 * T : nullptr;
    if (T <= JOINT_MAXT) {
        load_tiles<true>(s, tl.which, tl.co0, tl.ci0, lds, pitch);
        __syncthreads();
        const int nk = min(CO_PER, s.cout - tl.co0);
        // every run starts on a 16-byte boundary and is a whole number of 16-byte pieces
        if (((s.cin * T) & 3) == 0 && (((uintptr_t)dst | (uintptr_t)s.v) & 15) == 0) {
            const int q_per = 16 * T;                            // pieces of a full 64 * T run; <= 1024 pieces per workgroup
            float4 dq[4], vq[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int i = threadIdx.x + m * 256, k = i / q_per, e = (i - k * q_per) * 4;
                dq[m] = vq[m] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < nk && e < run) {
                    dq[m] = *reinterpret_cast<const float4*>(dst + ((size_t)(tl.co0 + k) * s.cin + tl.ci0) * T + e);
                    if (sn) vq[m] = *reinterpret_cast<const float4*>(vv + e);
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int i = threadIdx.x + m * 256, k = i / q_per, e = (i - k * q_per) * 4;
                if (k < nk && e < run) {
                    const float su = sn ? sv * s.u[tl.co0 + k] : 0.f;
                    int c = e / T, t = e - c * T;
                    float d4[4] = {dq[m].x, dq[m].y, dq[m].z, dq[m].w};
                    const float v4[4] = {vq[m].x, vq[m].y, vq[m].z, vq[m].w};
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        float g = lds[(k * 64 + c) * pitch + t];
                        if (sn) g = (g - su * v4[x]) * inv_sigma;
                        d4[x] += g;
                        if (++t == T) { t = 0; ++c; }
                    }
                    *reinterpret_cast<float4*>(dst + ((size_t)(tl.co0 + k) * s.cin + tl.ci0) * T + e) = make_float4(d4[0], d4[1], d4[2], d4[3]);
                }
            }
            return;
        }
        const int c0 = (int)threadIdx.x / T, t0 = (int)threadIdx.x - c0 * T, dc = 256 / T, dt = 256 - dc * T;
        for (int k = 0; k < nk; ++k) {
            float* d = dst + ((size_t)(tl.co0 + k) * s.cin + tl.ci0) * T;
            const float su = sn ? sv * s.u[tl.co0 + k] : 0.f;
            const float* l = lds + k * 64 * pitch;
            for (int e = threadIdx.x, c = c0, t = t0; e < run; e += 256) {
                float g = l[c * pitch + t];
                if (sn) g = (g - su * vv[e]) * inv_sigma;
                d[e] += g;
                c += dc; t += dt;
                if (t >= T) { t -= T; ++c; }
            }
        }
        return;
    }
    const int c0 = (int)threadIdx.x / T, t0 = (int)threadIdx.x - c0 * T, dc = 256 / T, dt = 256 - dc * T;
    for (int k = 0; k < CO_PER && tl.co0 + k < s.cout; ++k) {
        const int co = tl.co0 + k;
        __syncthreads();
        load_tile<true>(s, tl.which, co, tl.ci0, lds, pitch);
        __syncthreads();
        float* d = dst + ((size_t)co * s.cin + tl.ci0) * T;
        const float su = sn ? sv * s.u[co] : 0.f;
        for (int e = threadIdx.x, c = c0, t = t0; e < run; e += 256) {
            float g = lds[c * pitch + t];
            if (sn) g = (g - su * vv[e]) * inv_sigma;
            d[e] += g;
            c += dc; t += dt;
            if (t >= T) { t -= T; ++c; }
        }
    }
}

}  // namespace

extern "C" int mg_grad_drain(const mg_grad_slot* table_dev, int32_t nslots, const int32_t* block_slot_dev, int32_t nblocks,
                             double* partial, void* stream)
{
    MG_CHECK_ARG(table_dev && block_slot_dev && nslots > 0 && nblocks > 0, "mg_grad_drain: bad arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (partial) {                                   // spectral-normed slots present: their dot products first
        hipLaunchKernelGGL(grad_sn_dot_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, table_dev, block_slot_dev, partial);
        MG_CHECK_LAUNCH("mg_grad_drain(sn dot)");
        hipLaunchKernelGGL(grad_sn_finish_kernel, dim3((unsigned)nslots), dim3(256), 0, st, table_dev, (const double*)partial, nblocks, block_slot_dev);
        MG_CHECK_LAUNCH("mg_grad_drain(sn finish)");
    }
    hipLaunchKernelGGL(grad_drain_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, table_dev, block_slot_dev);
    MG_CHECK_LAUNCH("mg_grad_drain");
    return MG_OK;
}

extern "C" int64_t mg_grad_slot_blocks(int32_t cout, int32_t cin, int32_t ntens)
{
    if (cout <= 0 || cin <= 0 || ntens < 1 || ntens > 2) return -1;
    return (int64_t)ntens * ((cin + 63) / 64) * ((cout + CO_PER - 1) / CO_PER) + 1;      // + the bias block
}
