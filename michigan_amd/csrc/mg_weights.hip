// mg_weights.hip -- batched weight preparation: every per-layer launch of the weight path folded into a few
// network-wide ones.
//
//   mg_pack_weights         ONE launch that writes any number of GEMM images (mg_pack_weight's gather: permute + zero-pad
//                           + cast + gamma|beta row interleave, optionally divided by a spectral-norm sigma) and plain
//                           W / sigma copies; a job table in device memory says what goes where.  A training step issued
//                           ~166 single-image pack launches of ~10 us (1.65 ms, profiles/r02a_kernel_stats.csv).
//   mg_sn_power_iteration   torch.nn.utils.spectral_norm's power iteration (dim 0, one iteration) for ALL spectral-normed
//                           layers of a network at once: v <- normalize(W^T u), u <- normalize(W v), sigma = u . (W v)
//                           in four launches (two streaming passes over the weights + two tiny per-layer finishes)
//                           instead of 2 rocBLAS gemv + 2 normalize launches per layer (architecture.py:39-42,
//                           normalization.py:28-29: 18 layers in G, 6 in D, twice per training step each).
// HBM-bound (weights only): K1 and K3 read every spectral-normed weight once each; no MFMA.
#include "mg_common.h"
#include "mg_reduce.h"

namespace {

constexpr int PACK_PER_BLOCK = 4096;      // mode 2: elements per workgroup (16 per thread, all loads in flight before the first store)
constexpr int K1_ROWS = 128;              // rows of W per W^T u partial block (32: the per-layer finish walked 32 partials per column, 53 us)
constexpr int K1_COLS = 1024;             // columns per block: four per thread, 16-byte loads
constexpr int K3_ROWS = 4;                // rows of W per W v block (one wave each)

__device__ __forceinline__ int row_to_co2(int r, int cout, bool two, int& which)
{
    if (!two) { which = 0; return r < cout ? r : -1; }
    const int b = r >> 6, rem = r & 63;
    which = rem >> 5;
    const int co = b * 32 + (rem & 31);
    return co < cout ? co : -1;
}

// Destination element (t, r, c) of a GEMM image comes from
//   mode 0: W[co(r)][ci = c][t]      mode 1: W[co(c)][ci = r][t]       (co() = identity, or the gamma|beta row interleave)
// The reference layout has t fastest, so a gather by destination index (what the per-image pack_kernel does) touches every
// 64-byte line of W once per tap, T blocks apart: with 438 MB of generator weights that is T re-reads from HBM (the first batched
// version measured 1.5 TB/s of useful bytes).  Here a workgroup reads its sources as contiguous runs (mode 0: one run of CW*T
// floats per row, mode 1: one run of R*T floats per column), transposes through LDS and writes whole destination rows: every
// byte of W is read once.
//
// Tile = R destination rows x CW destination columns x all T taps:
//   CW = 128 where the image is wider than 64 columns (a wave's 16-byte stores then cover whole 256-byte bf16 runs), else 64;
//   R * CW = 512 (2048 for T = 1, where a 512-element tile is two elements per thread), so a T <= 16 tile is 18-32 KB of W.
// A thread issues all its loads (up to eight 16-byte ones) before the first LDS write.  The first version moved 9 KB per
// workgroup with 4-byte loads and stores and a barrier pair per sub-tile, and sat at 2.9 TB/s (latency-bound).
// 16-byte loads need every run to start on a 16-byte boundary: cin * T % 4 == 0 and aligned tensors (a 3-channel layer has rows
// of 27 floats: 4-byte loads, eight in flight); 16-byte stores need cols_p % 8 == 0 and an aligned image, else column pairs.
// LDS holds the tile in destination order, [t][r][c] with a plane pitch of R*SC + 4 floats, so that a store item (eight
// consecutive columns of one (tap, row)) is two ds_read_b128.  T > 16 (5x5, 7x7) goes through in sub-tiles of SC = 32 columns
// x 4 rows, which keeps the buffer at 33 KB for every window: four workgroups per CU (a 50 KiB 7x7 tile capped EVERY workgroup
// of the launch at 3 per CU, profiles/r02_pack_ab.txt).
constexpr int PK_MAXT = 49;
constexpr int PK_LDS_FLOATS = 16 * (512 + 4);                    // T <= 16: 16 planes; T = 1: 2052; T = 49: 49 x 132 = 6468
__host__ __device__ constexpr int pk_cw(int cols_p) { return cols_p > 64 ? 128 : 64; }
__host__ __device__ constexpr int pk_rows(int taps, int cw) { return taps == 1 ? 2048 / cw : taps <= 16 ? 512 / cw : 4; }
__host__ __device__ constexpr int pk_sub(int taps, int cw) { return taps <= 16 ? cw : 32; }

// TT = 0: any window (run-time divisions); the windows the networks use are instantiated with constant divisors
template <int TT, int CW>
__device__ __forceinline__ void pack_tile(const mg_pack_job& j, const int rel, float* __restrict__ tile)
{
    const int T = TT ? TT : j.taps;
    const int R = pk_rows(T, CW), SC = pk_sub(T, CW), plane = R * SC + 4;
    const int tid = threadIdx.x;
    const bool two = j.w1 != nullptr, m0 = j.mode == 0;
    const int cblocks = (j.cols_p + CW - 1) / CW;
    const int r0 = (rel / cblocks) * R, cb0 = (rel % cblocks) * CW;
    const float sg = j.sigma ? j.sigma[0] : 1.f;
    // a sub-tile is `nrun` contiguous source runs with room for L floats each: mode 0 one per row (SC columns x T),
    // mode 1 one per column (R rows x T).  Element e of run u is (x = e / T, t = e % T) -> (r, c) = mode 0 ? (u, x) : (x, u)
    const int nrun = m0 ? R : SC, L = (m0 ? SC : R) * T;
    const bool vec_ld = ((j.cin * T) & 3) == 0 && (((uintptr_t)j.w0 | (uintptr_t)j.w1) & 15) == 0;
    const bool vec_st = (j.cols_p & 7) == 0 && ((uintptr_t)j.dst & 15) == 0;
    for (int sc = 0; sc < CW; sc += SC) {
        const int c0 = cb0 + sc;
        if (c0 >= j.cols_p) break;                               // uniform
        if (sc) __syncthreads();                                 // the previous sub-tile has been stored
        // source run u: its first element and how many of its L floats exist (the rest of the tile is zero padding)
        auto run = [&](int u, int& valid) -> const float* {
            int which = 0;
            const int g = m0 ? r0 + u : c0 + u;                  // GEMM output-channel index
            const int co = g < (m0 ? j.rows_p : j.cols_p) ? row_to_co2(g, j.cout, two, which) : -1;
            const int ci0 = m0 ? c0 : r0;
            valid = co >= 0 ? max(0, min(m0 ? SC : R, j.cin - ci0)) * T : 0;
            return (which ? j.w1 : j.w0) + ((size_t)max(co, 0) * j.cin + ci0) * T;
        };
        if (vec_ld) {
            const int L4 = L >> 2, items = nrun * L4;            // <= 2048 16-byte pieces
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = tid + k * 256;
                v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q < items) {
                    const int u = q / L4, e = (q - u * L4) * 4;
                    int valid;
                    const float* src = run(u, valid);
                    if (e < valid) v[k] = *reinterpret_cast<const float4*>(src + e);       // valid % 4 == 0
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q = tid + k * 256;
                if (q < items) {
                    const int u = q / L4, e = (q - u * L4) * 4;
                    int x = e / T, t = e - x * T;
                    const float vv[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        tile[t * plane + (m0 ? u * SC + x : x * SC + u)] = vv[i];
                        if (++t == T) { t = 0; ++x; }
                    }
                }
            }
        } else {
            const int items = nrun * L;                          // <= 8192 floats: four rounds of eight loads in flight
            for (int kb = 0; kb < 32 && kb * 256 < items; kb += 8) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int q = tid + (kb + k) * 256;
                    v[k] = 0.f;
                    if (q < items) {
                        const int u = q / L, e = q - u * L;
                        int valid;
                        const float* src = run(u, valid);
                        if (e < valid) v[k] = src[e];
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int q = tid + (kb + k) * 256;
                    if (q < items) {
                        const int u = q / L, e = q - u * L;
                        const int x = e / T, t = e - x * T;
                        tile[t * plane + (m0 ? u * SC + x : x * SC + u)] = v[k];
                    }
                }
            }
        }
        __syncthreads();
        // ---- store: eight consecutive destination columns of one (tap, row) per item -----------------------------------------------
        const int g8 = SC >> 3, per_t = R * g8;                  // powers of two
        for (int q = tid; q < T * per_t; q += 256) {
            const int t = q / per_t, rem = q - t * per_t;
            const int rr = rem / g8, cg = rem - rr * g8;
            const int r = r0 + rr, c = c0 + cg * 8;
            if (r >= j.rows_p || c >= j.cols_p) continue;
            const float* p = tile + t * plane + rr * SC + cg * 8;
            const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
            float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            if (j.sigma) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = v[i] / sg;    // a true division, like torch
            }
            const size_t o = ((size_t)t * j.rows_p + r) * j.cols_p + c;
            if (j.dtype == MG_BF16) {
                uint16_t* d = reinterpret_cast<uint16_t*>(j.dst) + o;
                if (vec_st) *reinterpret_cast<uint4*>(d) = make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7]));
                else {
#pragma unroll
                    for (int i = 0; i < 8; i += 2) if (c + i < j.cols_p) *reinterpret_cast<uint32_t*>(d + i) = f2bf2(v[i], v[i + 1]);     // cols_p is even
                }
            } else {
                float* d = reinterpret_cast<float*>(j.dst) + o;
                if (vec_st) {
                    *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i += 2) if (c + i < j.cols_p) { float2 pv; pv.x = v[i]; pv.y = v[i + 1]; *reinterpret_cast<float2*>(d + i) = pv; }
                }
            }
        }
    }
}

template <int TT>
__device__ __forceinline__ void pack_tile_w(const mg_pack_job& j, const int rel, float* __restrict__ tile)
{
    if (pk_cw(j.cols_p) == 128) pack_tile<TT, 128>(j, rel, tile);
    else pack_tile<TT, 64>(j, rel, tile);
}

// four waves per SIMD = four workgroups per CU (what the LDS tile allows): 128 registers; 143 and three workgroups measured 14 % slower
__global__ __launch_bounds__(256, 4) void pack_weights_kernel(const mg_pack_job* __restrict__ jobs, const int32_t* __restrict__ block_job)
{
    __shared__ __attribute__((aligned(16))) float tile[PK_LDS_FLOATS];
    const mg_pack_job& j = jobs[block_job[blockIdx.x]];
    const int rel = (int)((int64_t)blockIdx.x - j.first_block);
    const int tid = threadIdx.x;
    if (j.mode == 2) {                                           // fp32 copy of w0 / sigma, reference layout
        const int64_t total = (int64_t)j.cout * j.cin * j.taps, base = (int64_t)rel * PACK_PER_BLOCK;
        const float sg = j.sigma ? j.sigma[0] : 1.f;
        float* const dst = reinterpret_cast<float*>(j.dst);
        if ((((uintptr_t)j.w0 | (uintptr_t)j.dst) & 15) == 0) {  // (inside SpectralPlan's buffer the destination is only 4-byte aligned)
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + (k * 256 + tid) * 4;
                if (i + 4 <= total) v[k] = *reinterpret_cast<const float4*>(j.w0 + i);
                else { v[k].x = i < total ? j.w0[i] : 0.f; v[k].y = i + 1 < total ? j.w0[i + 1] : 0.f; v[k].z = i + 2 < total ? j.w0[i + 2] : 0.f; v[k].w = 0.f; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + (k * 256 + tid) * 4;
                float4 o = v[k];
                if (j.sigma) { o.x = o.x / sg; o.y = o.y / sg; o.z = o.z / sg; o.w = o.w / sg; }      // a true division, like torch
                if (i + 4 <= total) *reinterpret_cast<float4*>(dst + i) = o;
                else { if (i < total) dst[i] = o.x; if (i + 1 < total) dst[i + 1] = o.y; if (i + 2 < total) dst[i + 2] = o.z; }
            }
            return;
        }
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * 256 + tid;
            v[k] = i < total ? j.w0[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * 256 + tid;
            if (i < total) dst[i] = j.sigma ? v[k] / sg : v[k];
        }
        return;
    }
    switch (j.taps) {
        case 1:  pack_tile_w<1>(j, rel, tile); break;
        case 9:  pack_tile_w<9>(j, rel, tile); break;
        case 16: pack_tile_w<16>(j, rel, tile); break;
        case 49: pack_tile_w<49>(j, rel, tile); break;
        default: pack_tile_w<0>(j, rel, tile); break;
    }
}

// ---- spectral-norm power iteration ---------------------------------------------------------------------------------------
// K1: partial[chunk][c] = sum over the chunk's K1_ROWS rows of W[r][c] * u[r]   (block = 256 columns x one row chunk)
__global__ __launch_bounds__(256) void sn_wtu_kernel(const mg_sn_layer* __restrict__ layers, const int32_t* __restrict__ block_layer)
{
    const mg_sn_layer& L = layers[block_layer[blockIdx.x]];
    const int rel = blockIdx.x - L.first_block_k1;
    const int cblocks = (L.cols + K1_COLS - 1) / K1_COLS;
    const int chunk = rel / cblocks, c = ((rel % cblocks) * 256 + threadIdx.x) * 4;
    if (c >= L.cols) return;
    const int r0 = chunk * K1_ROWS, r1 = min(r0 + K1_ROWS, L.rows);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if ((L.cols & 3) == 0 && (((uintptr_t)L.w | (uintptr_t)L.partial) & 15) == 0) {   // rows stay 16-byte aligned: one dwordx4 load per row (4x the bytes in flight)
        const float* __restrict__ w = L.w + (size_t)r0 * L.cols + c;
#pragma unroll 8
        for (int r = r0; r < r1; ++r, w += L.cols) {
            const float4 w4 = *reinterpret_cast<const float4*>(w);
            const float u = L.u[r];
            acc[0] += w4.x * u; acc[1] += w4.y * u; acc[2] += w4.z * u; acc[3] += w4.w * u;
        }
        float4 o; o.x = acc[0]; o.y = acc[1]; o.z = acc[2]; o.w = acc[3];
        *reinterpret_cast<float4*>(L.partial + (size_t)chunk * L.cols + c) = o;
        return;
    }
    for (int r = r0; r < r1; ++r) {
        const float u = L.u[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c + j < L.cols) acc[j] += L.w[(size_t)r * L.cols + c + j] * u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) if (c + j < L.cols) L.partial[(size_t)chunk * L.cols + c + j] = acc[j];
}

// K2: t1 = sum of the partials (fixed order), v = t1 / max(||t1||, eps)  (one 1024-thread block per layer)
__global__ __launch_bounds__(1024) void sn_finish_v_kernel(const mg_sn_layer* __restrict__ layers, float eps)
{
    __shared__ float red[16];
    const mg_sn_layer& L = layers[blockIdx.x];
    const int chunks = (L.rows + K1_ROWS - 1) / K1_ROWS;
    float ss = 0.f;
    for (int c = threadIdx.x; c < L.cols; c += 1024) {
        float t = 0.f;
        for (int k = 0; k < chunks; ++k) t += L.partial[(size_t)k * L.cols + c];
        L.t1[c] = t;
        ss += t * t;
    }
    ss = mg_block_sum_all<MgJoin::LeftToRight>(ss, red);
    const float denom = fmaxf(sqrtf(ss), eps);
    for (int c = threadIdx.x; c < L.cols; c += 1024) {
        const float q = L.t1[c] / denom;
        L.v[c] = q;
        if (L.v_copy) L.v_copy[c] = q;
    }
}

// K3: t2[r] = W[r] . v   (one wave per row)
__global__ __launch_bounds__(256) void sn_wv_kernel(const mg_sn_layer* __restrict__ layers, const int32_t* __restrict__ block_layer)
{
    const mg_sn_layer& L = layers[block_layer[blockIdx.x]];
    const int r = (blockIdx.x - L.first_block_k3) * K3_ROWS + (threadIdx.x >> 6);
    if (r >= L.rows) return;
    const float* __restrict__ w = L.w + (size_t)r * L.cols;
    float acc = 0.f;
    if ((L.cols & 3) == 0 && (((uintptr_t)L.w | (uintptr_t)L.v) & 15) == 0) {
        float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int c = (threadIdx.x & 63) * 4; c < L.cols; c += 256) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + c), v4 = *reinterpret_cast<const float4*>(L.v + c);
            a4[0] += w4.x * v4.x; a4[1] += w4.y * v4.y; a4[2] += w4.z * v4.z; a4[3] += w4.w * v4.w;
        }
        acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    } else {
        for (int c = threadIdx.x & 63; c < L.cols; c += 64) acc += w[c] * L.v[c];
    }
    acc = mg_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) L.t2[r] = acc;
}

// K4: power iteration: u = t2 / max(||t2||, eps), sigma = u . t2; without it: sigma = u . t2 with the stored u
__global__ __launch_bounds__(1024) void sn_finish_u_kernel(const mg_sn_layer* __restrict__ layers, float eps, int power_iteration)
{
    __shared__ float red[16];
    const mg_sn_layer& L = layers[blockIdx.x];
    float dot = 0.f;
    if (power_iteration) {
        float ss = 0.f;
        for (int r = threadIdx.x; r < L.rows; r += 1024) ss += L.t2[r] * L.t2[r];
        ss = mg_block_sum_all<MgJoin::LeftToRight>(ss, red);
        const float denom = fmaxf(sqrtf(ss), eps);
        for (int r = threadIdx.x; r < L.rows; r += 1024) {
            const float q = L.t2[r] / denom;
            L.u[r] = q;
            if (L.u_copy) L.u_copy[r] = q;
            dot += q * L.t2[r];
        }
    } else {
        for (int r = threadIdx.x; r < L.rows; r += 1024) dot += L.u[r] * L.t2[r];
    }
    dot = mg_block_sum_all<MgJoin::LeftToRight>(dot, red);
    if (threadIdx.x == 0) L.sigma[0] = dot;
}

}  // namespace

extern "C" int64_t mg_pack_job_blocks(int32_t mode, int32_t cout, int32_t cin, int32_t taps, int32_t rows_p, int32_t cols_p)
{
    if (mode == 2) return cout > 0 && cin > 0 && taps > 0 ? ((int64_t)cout * cin * taps + PACK_PER_BLOCK - 1) / PACK_PER_BLOCK : -1;
    if ((mode != 0 && mode != 1) || rows_p <= 0 || cols_p <= 0 || (cols_p & 1) || taps <= 0 || taps > PK_MAXT) return -1;
    const int cw = pk_cw(cols_p), r = pk_rows(taps, cw);
    return (int64_t)((rows_p + r - 1) / r) * ((cols_p + cw - 1) / cw);
}

extern "C" int mg_pack_weights(const mg_pack_job* jobs_dev, int32_t njobs, const int32_t* block_job_dev, int32_t nblocks, void* stream)
{
    MG_CHECK_ARG(jobs_dev && block_job_dev && njobs > 0 && nblocks > 0, "mg_pack_weights: bad arguments");
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)nblocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), jobs_dev, block_job_dev);
    MG_CHECK_LAUNCH("mg_pack_weights");
    return MG_OK;
}

extern "C" int64_t mg_sn_layer_blocks(int32_t rows, int32_t cols, int32_t which)
{
    if (rows <= 0 || cols <= 0) return -1;
    if (which == 0) return (int64_t)((cols + K1_COLS - 1) / K1_COLS) * ((rows + K1_ROWS - 1) / K1_ROWS);      // K1 workgroups
    if (which == 1) return (rows + K3_ROWS - 1) / K3_ROWS;                                         // K3 workgroups
    if (which == 2) return (rows + K1_ROWS - 1) / K1_ROWS;                                         // row chunks = rows of `partial`
    return -1;
}

extern "C" int mg_sn_power_iteration(const mg_sn_layer* layers_dev, int32_t nlayers, const int32_t* block_layer_k1, int32_t nblocks_k1,
                                     const int32_t* block_layer_k3, int32_t nblocks_k3, int32_t do_power_iteration, float eps, void* stream)
{
    MG_CHECK_ARG(layers_dev && nlayers > 0 && block_layer_k3 && nblocks_k3 > 0, "mg_sn_power_iteration: bad arguments");
    MG_CHECK_ARG(!do_power_iteration || (block_layer_k1 && nblocks_k1 > 0), "mg_sn_power_iteration: missing K1 table");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (do_power_iteration) {
        hipLaunchKernelGGL(sn_wtu_kernel, dim3((unsigned)nblocks_k1), dim3(256), 0, st, layers_dev, block_layer_k1);
        MG_CHECK_LAUNCH("mg_sn_power_iteration(W^T u)");
        hipLaunchKernelGGL(sn_finish_v_kernel, dim3((unsigned)nlayers), dim3(1024), 0, st, layers_dev, eps);
        MG_CHECK_LAUNCH("mg_sn_power_iteration(v)");
    }
    hipLaunchKernelGGL(sn_wv_kernel, dim3((unsigned)nblocks_k3), dim3(256), 0, st, layers_dev, block_layer_k3);
    MG_CHECK_LAUNCH("mg_sn_power_iteration(W v)");
    hipLaunchKernelGGL(sn_finish_u_kernel, dim3((unsigned)nlayers), dim3(1024), 0, st, layers_dev, eps, do_power_iteration);
    MG_CHECK_LAUNCH("mg_sn_power_iteration(u, sigma)");
    return MG_OK;
}
