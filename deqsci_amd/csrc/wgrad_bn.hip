// The weight gradients of the denoisers with a frozen (eval-mode) BatchNorm: FFDNet and the conv + BN + ReLU DnCNN.  Same contract as
// csrc/wgrad.hip: fixed runs of tiles per workgroup, fp32 accumulators added to a float64 partial at the latest every DEQSCI_WGRAD_CHAIN
// pixels, a second launch that sums the partials per entry in ascending workgroup order and rounds once; no atomics, no waiting.
//
//   W0-BN wgrad_c64_kernel<true>   W0's kernel (wgrad.hpp: one body, the nine-tap arithmetic of R = wgrad(x, g) is W0's bit for bit) plus the
//                                  per-channel sums of g from the tile that is in LDS anyway.
//         wgrad_bn_sum_kernel      one workgroup per output channel co, one thread per (tap, ci): the float64 entry sums R in W0's order, then
//                                  dw = (float)(scale[co] R), ddot[co] = (float) sum_{ci,tap} w R in float64 (a fixed order: nine terms per
//                                  lane, then the wave's tree), dsum[co] = (float) sum over the workgroups' sums of g.
//                                  With y = relu(s conv(x, W) + t), s = gamma / sqrt(var + eps): dW = s R, dbeta = dsum,
//                                  dgamma = (ddot - mean dsum) / sqrt(var + eps), since sum_p g c = sum_{ci,tap} W R - no stored
//                                  pre-activation, no division by gamma.
//   W2    wgrad_shuffle_kernel     FFDNet's edge layers, read through the 2x2 pixel-unshuffle from the full-resolution planar image: lane =
//                                  channel as in W1, a wave walks 8 half-resolution pixels of a tile, the six full-resolution rows of the
//                                  tile's halo are in LDS.  acc[k][tap] = sum_p t[p,c] u[p + d, k], u the unshuffled image (phase 2i + j =
//                                  pixel (2h + i, 2w + j)); which = 0 has one more channel in front, sigma's: sum_p sigma[img] t[p,c] over
//                                  the taps inside the half-resolution image.  which = 1 is the same sum with the taps reversed, as in W1.
//         wgrad_shuffle_sum_kernel the second launch: which = 0 -> dw (64,5,3,3), which = 1 -> dw (4,64,3,3).
#include "wgrad.hpp"

namespace deqsci {
namespace wgrad {

constexpr int W2_MAX_WG = 512;
constexpr int W0BN_STRIDE = W0_ENTRIES + W0_SUMS;
constexpr int W2_MAX_ENTRIES = 5 * 9 * 64;
constexpr int SW = 2 * XW;                                                   // a full-resolution row of a tile with its halo
constexpr int BN_SUM_TB = 9 * 64;                                            // one thread per entry of an output channel, as in wgrad_sum_kernel

__global__ __launch_bounds__(BN_SUM_TB) void wgrad_bn_sum_kernel(const double* __restrict__ part, const float* __restrict__ w,
                                                                 const float* __restrict__ scale, float* __restrict__ dw,
                                                                 float* __restrict__ dsum, float* __restrict__ ddot, int wgs) {
    __shared__ double prod[BN_SUM_TB];
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE, co = (int)blockIdx.x;
    {
        const int tap = wave, ci = lane;
        const double* p = part + ((tap * 64 + co) * 64 + ci);
        double sum = 0.0;
#pragma unroll 16
        for (int b = 0; b < wgs; ++b) sum += p[(int64_t)b * W0BN_STRIDE];
        const int o = (co * 64 + ci) * 9 + tap;
        dw[o] = (float)((double)scale[co] * sum);
        prod[tid] = (double)w[o] * sum;
    }
    __syncthreads();
    if (wave == 0) {
        double d = 0.0;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) d += prod[tap * 64 + lane];
        d = wave_sum(d);
        if (lane == 0) ddot[co] = (float)d;
    } else if (tid == WAVE) {
        double sum = 0.0;
#pragma unroll 16
        for (int b = 0; b < wgs; ++b) sum += part[(int64_t)b * W0BN_STRIDE + W0_ENTRIES + co];
        dsum[co] = (float)sum;
    }
}

template <bool SIGMA>
__global__ __launch_bounds__(TB) void wgrad_shuffle_kernel(const float* __restrict__ img, const float* __restrict__ sigma, int64_t sigma_stride,
                                                           const float* __restrict__ t, double* __restrict__ part, int H, int W, int tilesW,
                                                           int64_t tiles, int64_t per_wg) {
    constexpr int K = SIGMA ? 5 : 4, K0 = SIGMA ? 1 : 0, ENTRIES = K * 9 * 64;   // H, W: the half-resolution sides
    __shared__ float sL[6 * SW];
    __shared__ float red[(TB / WAVE) * ENTRIES];
    constexpr int PX = TW / (TB / WAVE);                                    // pixels of a tile per wave
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t t0 = (int64_t)blockIdx.x * per_wg, t1 = t0 + per_wg < tiles ? t0 + per_wg : tiles;
    double* const mine = part + (int64_t)blockIdx.x * ENTRIES;
    float acc[K * 9];
#pragma unroll
    for (int i = 0; i < K * 9; ++i) acc[i] = 0.0f;

    auto flush = [&](bool first) {
#pragma unroll
        for (int i = 0; i < K * 9; ++i) {
            red[(wave * K * 9 + i) * 64 + lane] = acc[i];
            acc[i] = 0.0f;
        }
        __syncthreads();
        for (int e = tid; e < ENTRIES; e += TB) {
            double d = 0.0;
            for (int wv = 0; wv < TB / WAVE; ++wv) d += (double)red[wv * ENTRIES + e];
            mine[e] = first ? d : mine[e] + d;
        }
        __syncthreads();
    };

    int since = 0;
    bool first = true;
    for (int64_t tt = t0; tt < t1; ++tt) {
        const Tile tl = tile_at(tt, H, tilesW);
        __syncthreads();
        for (int i = tid; i < 6 * SW; i += TB) {
            const int fr = i / SW, fc = i - fr * SW, hh = tl.h + (fr >> 1) - 1, ww = tl.w0 + (fc >> 1) - 1;
            sL[i] = (hh >= 0 && hh < H && ww >= 0 && ww < W)
                        ? img[((tl.row + (fr >> 1) - 1) * 2 + (fr & 1)) * (2 * (int64_t)W) + 2 * ww + (fc & 1)]
                        : 0.0f;
        }
        float sg = 0.0f;
        if constexpr (SIGMA) sg = sigma[(tl.row / H) * sigma_stride];
        float tv[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int w = tl.w0 + wave * PX + j;
            tv[j] = w < W ? t[(tl.row * W + w) * 64 + lane] : 0.0f;
        }
        __syncthreads();
        const bool rowok[3] = {tl.h > 0, true, tl.h < H - 1};
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int px = wave * PX + j, w = tl.w0 + px;
            if (w >= W) continue;                                           // (uniform in the wave)
            const bool colok[3] = {w > 0, true, w < W - 1};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    if (rowok[ky] && colok[kx]) {                           // a tap outside the half-resolution image is never multiplied
                        const int tap = ky * 3 + kx;
                        if constexpr (SIGMA) acc[tap] = fmaf(tv[j], sg, acc[tap]);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[(K0 + q) * 9 + tap] = fmaf(tv[j], sL[(2 * ky + (q >> 1)) * SW + 2 * (px + kx) + (q & 1)], acc[(K0 + q) * 9 + tap]);
                    }
        }
        if (++since == FLUSH_TILES) {
            flush(first);
            first = false;
            since = 0;
        }
    }
    if (since > 0) flush(first);
}

// entry e = (k * 9 + tap) * 64 + c  ->  which = 0: dw[c][k][tap] of (64,5,3,3);  which = 1: dw[k][c][8 - tap] of (4,64,3,3)
__global__ __launch_bounds__(TB) void wgrad_shuffle_sum_kernel(const double* __restrict__ part, float* __restrict__ dw, int entries, int wgs,
                                                               int which) {
    const int e = (int)(blockIdx.x * TB + threadIdx.x);
    if (e >= entries) return;
    double sum = 0.0;
#pragma unroll 16
    for (int b = 0; b < wgs; ++b) sum += part[(int64_t)b * entries + e];
    const int c = e & 63, kt = e >> 6, k = kt / 9, tap = kt - k * 9;
    dw[which ? (k * 64 + c) * 9 + (8 - tap) : (c * 5 + k) * 9 + tap] = (float)sum;
}

inline size_t bn_workspace_bytes(int64_t n, int64_t H, int64_t W) {
    const int64_t a = split(n, H, W, W0_MAX_WG).wgs * W0BN_STRIDE, b = split(n, H, W, W2_MAX_WG).wgs * W2_MAX_ENTRIES;
    return (size_t)(a > b ? a : b) * sizeof(double);
}

}  // namespace wgrad
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_wgrad_bn_workspace_bytes(int64_t n, int64_t H, int64_t W) {
    if (!wgrad::sizes_ok(n, H, W) || !wgrad::supported(n, H, W)) return 0;
    return wgrad::bn_workspace_bytes(n, H, W);
}

int deqsci_wgrad3x3_c64_c64_bn_f32(const float* x, const float* g, const float* w, const float* scale, float* dw, float* dsum, float* ddot,
                                   int64_t n, int64_t H, int64_t W, void* workspace, deqsci_stream_t stream) {
    if (!x || !g || !w || !scale || !dw || !dsum || !ddot || !workspace) return DEQSCI_ERR_NULL;
    if (!wgrad::sizes_ok(n, H, W)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(x) || !aligned16(g) || misaligned(w, 4) || misaligned(scale, 4) || misaligned(dw, 4) || misaligned(dsum, 4) ||
        misaligned(ddot, 4) || misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    if (!wgrad::supported(n, H, W)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t act = n * H * W * 64 * (int64_t)sizeof(float), wb = wgrad::W0_ENTRIES * (int64_t)sizeof(float), cb = 64 * (int64_t)sizeof(float);
    const int64_t ws = (int64_t)wgrad::bn_workspace_bytes(n, H, W);
    const void* in[4] = {x, g, w, scale};
    const int64_t in_bytes[4] = {act, act, wb, cb};
    const void* out[4] = {dw, dsum, ddot, workspace};
    const int64_t out_bytes[4] = {wb, cb, cb, ws};
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 4; ++i)
            if (overlaps(out[o], out_bytes[o], in[i], in_bytes[i])) return DEQSCI_ERR_UNSUPPORTED;
        for (int p = o + 1; p < 4; ++p)
            if (overlaps(out[o], out_bytes[o], out[p], out_bytes[p])) return DEQSCI_ERR_UNSUPPORTED;
    }
    const wgrad::Split sp = wgrad::split(n, H, W, wgrad::W0_MAX_WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(wgrad::wgrad_c64_kernel<true>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, x, g, part, (int)H, (int)W,
                       (int)ceil_div(W, wgrad::TW), sp.tiles, sp.per_wg);
    int rc = launch_status();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(wgrad::wgrad_bn_sum_kernel, dim3(64), dim3(wgrad::BN_SUM_TB), 0, st, part, w, scale, dw, dsum, ddot, (int)sp.wgs);
    return launch_status();
}

int deqsci_wgrad3x3_shuffle_f32(const float* img, const float* sigma, int64_t sigma_stride, const float* t, float* dw, int which, int64_t n,
                                int64_t H, int64_t W, void* workspace, deqsci_stream_t stream) {
    if (!img || !t || !dw || !workspace || (which == 0 && !sigma)) return DEQSCI_ERR_NULL;
    if (!wgrad::sizes_ok(n, H, W) || (H & 1) || (W & 1)) return DEQSCI_ERR_SHAPE;
    if (misaligned(img, 4) || misaligned(sigma, 4) || misaligned(t, 4) || misaligned(dw, 4) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    const int64_t Hh = H / 2, Wh = W / 2;
    if ((which != 0 && which != 1) || (which == 0 && sigma_stride != 0 && sigma_stride != 1) || !wgrad::supported(n, Hh, Wh))
        return DEQSCI_ERR_UNSUPPORTED;
    const int entries = (which ? 4 : 5) * 9 * 64;
    const int64_t ib = n * H * W * (int64_t)sizeof(float), act = n * Hh * Wh * 64 * (int64_t)sizeof(float), out = entries * (int64_t)sizeof(float);
    const int64_t sb = (which ? 0 : (sigma_stride ? n : 1)) * (int64_t)sizeof(float), ws = (int64_t)wgrad::bn_workspace_bytes(n, Hh, Wh);
    if (overlaps(dw, out, img, ib) || overlaps(dw, out, t, act) || overlaps(workspace, ws, img, ib) || overlaps(workspace, ws, t, act) ||
        overlaps(workspace, ws, dw, out) || (sb && (overlaps(dw, out, sigma, sb) || overlaps(workspace, ws, sigma, sb))))
        return DEQSCI_ERR_UNSUPPORTED;
    const wgrad::Split sp = wgrad::split(n, Hh, Wh, wgrad::W2_MAX_WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    if (which == 0)
        hipLaunchKernelGGL(wgrad::wgrad_shuffle_kernel<true>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, img, sigma, sigma_stride, t, part,
                           (int)Hh, (int)Wh, (int)ceil_div(Wh, wgrad::TW), sp.tiles, sp.per_wg);
    else
        hipLaunchKernelGGL(wgrad::wgrad_shuffle_kernel<false>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, img, sigma, sigma_stride, t, part,
                           (int)Hh, (int)Wh, (int)ceil_div(Wh, wgrad::TW), sp.tiles, sp.per_wg);
    int rc = launch_status();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(wgrad::wgrad_shuffle_sum_kernel, dim3((unsigned)ceil_div(entries, TB)), dim3(TB), 0, st, part, dw, entries, (int)sp.wgs,
                       which);
    return launch_status();
}

}  // extern "C"
