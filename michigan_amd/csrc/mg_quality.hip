// mg_quality.hip -- the quality extension group (include/michigan_hip/evaluation/quality.h): what an evaluation pass measures.
//
// mgq_image_quality_u8    PSNR and SSIM ingredients of two u8 NHWC batches in one pass over the bytes.  A workgroup owns a 16 x 16
//                         tile of one sample.  It stages the tile with a halo of k / 2 of BOTH images, every channel, in LDS once
//                         (bytes, as they lie in memory: a patch row is (16 + k - 1) c consecutive bytes, so consecutive lanes
//                         read consecutive bytes), then per channel: the x pass leaves the five row moments W * a, W * b, W * aa,
//                         W * bb, W * ab of the (16 + k - 1) x 16 strip in LDS as doubles, the y pass gives each thread the five
//                         moments of its own pixel, and the thread forms its ssim value, its squared difference and its counts.
//                         The workgroup's sums (mg_reduce.h: wave tree, waves left to right) go to the workspace; a second
//                         launch adds the partials of a (sample, channel) in a fixed order.  k is a template parameter, so the
//                         window's taps are read from the kernel arguments as scalars and both passes are fully unrolled.
//                         Everything is double: E[x^2] - mu^2 cancels up to 5e-4 of the map away in fp32 on bright flat patches.
// mgq_orient_distance_u8  min(|a - b|, 255 - |a - b|) summed under a mask: 16 bytes a lane when the three planes allow it, bytes
//                         otherwise; 32-bit sums per thread, the workgroup's sum, one 64-bit integer atomic add per workgroup
//                         and term (integers: exact in any order).
#include "mg_common.h"
#include "mg_reduce.h"
#include "michigan_hip/evaluation/quality.h"

namespace {

typedef unsigned long long u64;
constexpr int NTHREADS = 256, NWAVES = NTHREADS / 64;
constexpr int QT = MGQ_TILE, MAXC = MGQ_MAX_C, SLOTS = MGQ_WS_SLOTS, NI = MGQ_INT_TERMS, ND = MGQ_SSIM_TERMS;
static_assert(QT * QT == NTHREADS && NI + ND == SLOTS, "one thread per pixel of the tile; a slot per term");

struct Window { double w[MGQ_MAX_K]; };

// the map value from the five moments, evaluated as the header spells it: one rounding per operation, nothing contracted (for
// a == b the numerator and the denominator must be the same bits)
__device__ __forceinline__ double ssim_value(double mu_a, double mu_b, double e_aa, double e_bb, double e_ab)
{
#pragma clang fp contract(off)
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    const double var_a = e_aa - mu_a * mu_a, var_b = e_bb - mu_b * mu_b, cov = e_ab - mu_a * mu_b;
    const double num = ((2.0 * mu_a) * mu_b + C1) * (2.0 * cov + C2);
    const double den = ((mu_a * mu_a + mu_b * mu_b) + C1) * ((var_a + var_b) + C2);
    return num / den;
}

template <int K>
__global__ __launch_bounds__(NTHREADS) void quality_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                const uint8_t* __restrict__ mask, const Window win, u64* __restrict__ ws,
                                                                int H, int W, int C, int tiles_x, int tiles_y)
{
    constexpr int R = K / 2, PH = QT + K - 1, PW = QT + K - 1;
    constexpr int PS = PW * MAXC;                                      // patch row stride in bytes (a row holds PW * C <= PS of them)
    __shared__ uint8_t pa[PH * PS], pb[PH * PS];                       // 2 x 3.5 KiB at k = 15
    __shared__ double hm[5][PH][QT];                                   // the row moments of one channel: 18.75 KiB at k = 15
    __shared__ double redd[ND][NWAVES];
    __shared__ u64 redu[NI][NWAVES];
    const int tid = threadIdx.x;
    int t_ = blockIdx.x;
    const int tx = t_ % tiles_x; t_ /= tiles_x;
    const int ty = t_ % tiles_y;
    const int n = t_ / tiles_y;
    const int x0 = tx * QT, y0 = ty * QT;

    // the patch: rows y0 - R .. y0 + QT + R - 1, columns x0 - R .. x0 + QT + R - 1, every channel; outside the image 0 (such a byte
    // reaches only pixels outside the valid region, which are not summed)
    const int nb = PW * C;
    for (int i = tid; i < PH * nb; i += NTHREADS) {
        const int r = i / nb, cb = i - r * nb;
        const int y = y0 - R + r, x = x0 - R + cb / C;
        uint8_t va = 0, vb = 0;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            const size_t g = ((size_t)n * H + y) * ((size_t)W * C) + (size_t)((x0 - R) * C + cb);   // x >= 0: the offset in the row is >= 0
            va = a[g];
            vb = b[g];
        }
        pa[r * PS + cb] = va;
        pb[r * PS + cb] = vb;
    }
    const int px = tid % QT, py = tid / QT;
    const int x = x0 + px, y = y0 + py;
    const bool inside = x < W && y < H;
    const bool valid = inside && y >= R && y < H - R && x >= R && x < W - R;
    const bool in_mask = inside && (mask == nullptr || mask[((size_t)n * H + y) * W + x] != 0);
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        // x pass: hm[q][r][col] = sum_j w[j] f_q(patch[r][col + j]), ascending j from +0, one fma a tap
        for (int i = tid; i < PH * QT; i += NTHREADS) {
            const int r = i / QT, col = i - r * QT;
            const uint8_t* ra = pa + r * PS + col * C + c;
            const uint8_t* rb = pb + r * PS + col * C + c;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int ia = ra[j * C], ib = rb[j * C];
                const double w = win.w[j];
                s0 = __builtin_fma(w, (double)ia, s0);
                s1 = __builtin_fma(w, (double)ib, s1);
                s2 = __builtin_fma(w, (double)(ia * ia), s2);
                s3 = __builtin_fma(w, (double)(ib * ib), s3);
                s4 = __builtin_fma(w, (double)(ia * ib), s4);
            }
            hm[0][r][col] = s0; hm[1][r][col] = s1; hm[2][r][col] = s2; hm[3][r][col] = s3; hm[4][r][col] = s4;
        }
        __syncthreads();
        // y pass: this thread's pixel is patch row py + R, so its window is strip rows py .. py + K - 1
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double w = win.w[i];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = __builtin_fma(w, hm[q][py + i][px], m[q]);
        }
        const double s = ssim_value(m[0], m[1], m[2], m[3], m[4]);
        const int d = (int)pa[(py + R) * PS + (px + R) * C + c] - (int)pb[(py + R) * PS + (px + R) * C + c];
        const u64 e = inside ? (u64)(d * d) : 0ull;
        const double vd[ND] = {valid ? s : 0.0, valid && in_mask ? s : 0.0};
        const u64 vu[NI] = {e, in_mask ? e : 0ull, in_mask ? 1ull : 0ull, valid && in_mask ? 1ull : 0ull};
        mg_put_wave_sums(vd, redd);
        mg_put_wave_sums(vu, redu);
        __syncthreads();                                               // behind the wave sums, and behind every read of hm: the next channel overwrites it
        u64* slot = ws + ((size_t)blockIdx.x * C + c) * SLOTS;
        if (tid < NI) slot[tid] = mg_join<MgJoin::LeftToRight>(redu[tid]);
        else if (tid < NI + ND) reinterpret_cast<double*>(slot)[tid] = mg_join<MgJoin::LeftToRight>(redd[tid - NI]);
        // redd / redu are next written after the barrier that follows the next x pass
    }
}

// one workgroup per (sample, channel): thread t adds tiles t, t + 256, ... ascending, then the workgroup's join
__global__ __launch_bounds__(NTHREADS) void quality_join_kernel(const u64* __restrict__ ws, u64* __restrict__ out_int, double* __restrict__ out_ssim,
                                                                int C, int tiles)
{
    __shared__ double redd[ND][NWAVES];
    __shared__ u64 redu[NI][NWAVES];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / C, c = blockIdx.x - n * C;
    double vd[ND] = {0.0, 0.0};
    u64 vu[NI] = {0ull, 0ull, 0ull, 0ull};
    for (int i = tid; i < tiles; i += NTHREADS) {
        const u64* slot = ws + (((size_t)n * tiles + i) * C + c) * SLOTS;
#pragma unroll
        for (int q = 0; q < NI; ++q) vu[q] += slot[q];
#pragma unroll
        for (int q = 0; q < ND; ++q) vd[q] += reinterpret_cast<const double*>(slot)[NI + q];
    }
    mg_put_wave_sums(vd, redd);
    mg_put_wave_sums(vu, redu);
    __syncthreads();
    if (tid < NI) out_int[(size_t)blockIdx.x * NI + tid] = mg_join<MgJoin::LeftToRight>(redu[tid]);
    else if (tid < NI + ND) out_ssim[(size_t)blockIdx.x * ND + (tid - NI)] = mg_join<MgJoin::LeftToRight>(redd[tid - NI]);
}

constexpr int OCHUNK = NTHREADS * 16 * 4;                              // pixels a workgroup of the orientation pass owns: four 16-byte rounds

__device__ __forceinline__ void orient_term(uint32_t av, uint32_t bv, uint32_t mv, uint32_t& sum, uint32_t& cnt)
{
    const int d0 = abs((int)av - (int)bv);
    const int d = min(d0, MGQ_ORIENT_PERIOD - d0);
    sum += mv ? (uint32_t)d : 0u;
    cnt += mv ? 1u : 0u;
}

template <bool VEC>
__global__ __launch_bounds__(NTHREADS) void orient_distance_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                   const uint8_t* __restrict__ mask, u64* __restrict__ out, int P, int chunks)
{
    __shared__ u64 redu[2][NWAVES];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    const size_t base = (size_t)n * P + (size_t)chunk * OCHUNK;        // the chunk's first pixel
    const int len = (int)min((long long)OCHUNK, (long long)P - (long long)chunk * OCHUNK);   // 1 .. OCHUNK: every index below is a small offset from base
    uint32_t sum = 0, cnt = 0;                                         // at most 64 pixels a thread: 64 * 127 fits easily
    if (VEC) {                                                         // P % 16 == 0 and the three planes are 16-byte aligned, so is every chunk and len % 16 == 0
        for (int i = tid * 16; i < len; i += NTHREADS * 16) {
            const uint4 ua = *reinterpret_cast<const uint4*>(a + base + i);
            const uint4 ub = *reinterpret_cast<const uint4*>(b + base + i);
            const uint4 um = *reinterpret_cast<const uint4*>(mask + base + i);
            const uint32_t wa[4] = {ua.x, ua.y, ua.z, ua.w}, wb[4] = {ub.x, ub.y, ub.z, ub.w}, wm[4] = {um.x, um.y, um.z, um.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int s = 0; s < 32; s += 8) orient_term((wa[j] >> s) & 255u, (wb[j] >> s) & 255u, (wm[j] >> s) & 255u, sum, cnt);
        }
    } else {
        for (int i = tid; i < len; i += NTHREADS) orient_term(a[base + i], b[base + i], mask[base + i], sum, cnt);
    }
    const u64 v[2] = {sum, cnt};
    mg_put_wave_sums(v, redu);
    __syncthreads();
    if (tid < 2) atomicAdd(out + (size_t)n * 2 + tid, mg_join<MgJoin::LeftToRight>(redu[tid]));
}

bool quality_geometry_ok(int64_t n, int64_t h, int64_t w, int64_t c)
{
    return n > 0 && h >= 1 && w >= 1 && c >= 1 && c <= MAXC && n * h * w * c < (1ll << 31);
}

}  // namespace

extern "C" int64_t mgq_quality_workspace(int32_t n, int32_t h, int32_t w, int32_t c)
{
    if (!quality_geometry_ok(n, h, w, c)) return 0;
    const int64_t tx = (w + QT - 1) / QT, ty = (h + QT - 1) / QT;
    return (int64_t)n * tx * ty * c * SLOTS * 8;
}

extern "C" int mgq_image_quality_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, const double* window, int32_t k, void* ws,
                                    uint64_t* out_int, double* out_ssim, int32_t n, int32_t h, int32_t w, int32_t c, void* stream)
{
    MG_CHECK_ARG(a && b && window && ws && out_int && out_ssim, "mgq_image_quality_u8: null pointer");
    MG_CHECK_ARG(k >= MGQ_MIN_K && k <= MGQ_MAX_K && (k & 1), "mgq_image_quality_u8: bad window length k=%d (odd, %d .. %d)", k, MGQ_MIN_K, MGQ_MAX_K);
    MG_CHECK_ARG(c >= 1 && c <= MAXC, "mgq_image_quality_u8: bad channel count c=%d (1 .. %d)", c, MAXC);
    MG_CHECK_ARG(quality_geometry_ok(n, h, w, c), "mgq_image_quality_u8: bad geometry n=%d h=%d w=%d c=%d (n h w c must be in [1, 2^31))", n, h, w, c);
    MG_CHECK_ARG(h >= k && w >= k, "mgq_image_quality_u8: the image %d x %d is smaller than the window k=%d", h, w, k);
    MG_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)out_int & 7) == 0 && ((uintptr_t)out_ssim & 7) == 0,
                 "mgq_image_quality_u8: ws, out_int and out_ssim must be 8-byte aligned");
    Window win;
    for (int i = 0; i < MGQ_MAX_K; ++i) win.w[i] = i < k ? window[i] : 0.0;
    const int tx = (w + QT - 1) / QT, ty = (h + QT - 1) / QT;
    const unsigned blocks = (unsigned)((int64_t)n * tx * ty);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    u64* wsp = reinterpret_cast<u64*>(ws);
#define MGQ_LAUNCH(KK) case KK: hipLaunchKernelGGL(quality_tile_kernel<KK>, dim3(blocks), dim3(NTHREADS), 0, st, a, b, mask, win, wsp, h, w, c, tx, ty); break
    switch (k) {
        MGQ_LAUNCH(3); MGQ_LAUNCH(5); MGQ_LAUNCH(7); MGQ_LAUNCH(9); MGQ_LAUNCH(11); MGQ_LAUNCH(13); MGQ_LAUNCH(15);
    }
#undef MGQ_LAUNCH
    MG_CHECK_LAUNCH("mgq_image_quality_u8");
    hipLaunchKernelGGL(quality_join_kernel, dim3((unsigned)(n * c)), dim3(NTHREADS), 0, st, wsp, reinterpret_cast<u64*>(out_int), out_ssim, c, tx * ty);
    MG_CHECK_LAUNCH("mgq_image_quality_u8 (join)");
    return MG_OK;
}

extern "C" int mgq_orient_distance_u8(const uint8_t* a, const uint8_t* b, const uint8_t* mask, uint64_t* out, int32_t n, int32_t h, int32_t w,
                                      void* stream)
{
    MG_CHECK_ARG(a && b && mask && out, "mgq_orient_distance_u8: null pointer");
    MG_CHECK_ARG(n > 0 && h >= 1 && w >= 1 && (int64_t)n * h * w < (1ll << 31), "mgq_orient_distance_u8: bad geometry n=%d h=%d w=%d (n h w must be in [1, 2^31))", n, h, w);
    MG_CHECK_ARG(((uintptr_t)out & 7) == 0, "mgq_orient_distance_u8: out must be 8-byte aligned");
    const int P = h * w;
    const int chunks = (int)(((int64_t)P + OCHUNK - 1) / OCHUNK);
    const bool vec = P % 16 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)mask) & 15) == 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 2 * sizeof(uint64_t), st);
    if (e != hipSuccess) return mg_fail(MG_ERR_LAUNCH, "mgq_orient_distance_u8: clearing out: %s", hipGetErrorString(e));
    u64* o = reinterpret_cast<u64*>(out);
    if (vec) hipLaunchKernelGGL(orient_distance_kernel<true>, dim3((unsigned)(n * chunks)), dim3(NTHREADS), 0, st, a, b, mask, o, P, chunks);
    else hipLaunchKernelGGL(orient_distance_kernel<false>, dim3((unsigned)(n * chunks)), dim3(NTHREADS), 0, st, a, b, mask, o, P, chunks);
    MG_CHECK_LAUNCH("mgq_orient_distance_u8");
    return MG_OK;
}
