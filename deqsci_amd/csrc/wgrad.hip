// The denoiser's weight gradients (the taped call z = f(z*) of the training forward: autograd forms (df/dtheta)^T g from it, and for a
// bias-free conv + ReLU stack that is one weight gradient per 3x3 convolution, from the layer's input and the masked gradient behind it).
//
//   W0 wgrad_c64_kernel   dw[co][ci][ky][kx] = sum_p g[p,co] x[p + (ky-1, kx-1), ci] for a 64 -> 64 layer, x and g fp32 channels_last.
//                         A GEMM with the pixels as K on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32: A = g^T (co x pixel),
//                         B = x shifted by the tap (pixel x ci), two pixels per instruction.  Four waves, wave w owns the 32 x 32 quadrant
//                         (co half w >> 1, ci half w & 1) of all nine taps: 9 x 16 accumulator registers.  A tile is a run of TW = 32
//                         pixels of one image row: its g and the three haloed x rows (zero outside the image) are staged in LDS, the next
//                         tile's are in flight in registers meanwhile.  A tap outside the image is never multiplied (a 0 x NaN would be a
//                         NaN the sum does not contain): a tap row or column outside the image and a pixel beyond the row's end get a
//                         zero on BOTH operands.
//   W1 wgrad_c1_kernel    the two edge layers: dw[c][ky][kx] = sum_p t[p,c] s[p + (ky-1, kx-1)], s a planar scalar image, t channels_last.
//                         Lane = channel, a wave walks 8 pixels of a tile, the nine s taps come from LDS; nine accumulators per lane.
//                         The last layer's form sum_p s[p] t[p + d, c] is the same sum with the taps reversed (q = p + d), so the
//                         second launch writes tap 8 - tap for flip = 1.
//   wgrad_sum_kernel      the second launch of both: per entry, the workgroups' float64 partials in ascending workgroup order, rounded once.
//
// Every workgroup owns a fixed run of consecutive tiles, accumulates in fp32 and adds its accumulators to its float64 partial in the
// workspace (first flush: a store, so the workspace needs no initialisation) at the latest every DEQSCI_WGRAD_CHAIN pixels and at the end
// of its run.  No atomics, no workgroup waits for another: bit-for-bit deterministic.  (The tiling and W0's kernel live in wgrad.hpp: the
// frozen-BatchNorm form of csrc/wgrad_bn.hip is the same body with two more outputs.)
#include "wgrad.hpp"

namespace deqsci {
namespace wgrad {

__global__ __launch_bounds__(TB) void wgrad_c1_kernel(const float* __restrict__ s, const float* __restrict__ t, double* __restrict__ part,
                                                      int H, int W, int tilesW, int64_t tiles, int64_t per_wg) {
    __shared__ float sL[3 * XW];
    __shared__ float red[(TB / WAVE) * 9 * 64];
    constexpr int PX = TW / (TB / WAVE);                                    // pixels of a tile per wave
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t t0 = (int64_t)blockIdx.x * per_wg, t1 = t0 + per_wg < tiles ? t0 + per_wg : tiles;
    double* const mine = part + (int64_t)blockIdx.x * W1_ENTRIES;
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0f;

    auto flush = [&](bool first) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            red[(wave * 9 + tap) * 64 + lane] = acc[tap];
            acc[tap] = 0.0f;
        }
        __syncthreads();
        for (int e = tid; e < W1_ENTRIES; e += TB) {
            double d = 0.0;
            for (int wv = 0; wv < TB / WAVE; ++wv) d += (double)red[wv * W1_ENTRIES + e];
            mine[e] = first ? d : mine[e] + d;
        }
        __syncthreads();
    };

    int since = 0;
    bool first = true;
    for (int64_t tt = t0; tt < t1; ++tt) {
        const Tile tl = tile_at(tt, H, tilesW);
        __syncthreads();
        if (tid < 3 * XW) {
            const int row = tid / XW, c = tid - row * XW, hh = tl.h + row - 1, ww = tl.w0 + c - 1;
            sL[tid] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? s[(tl.row + row - 1) * W + ww] : 0.0f;
        }
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
                    if (rowok[ky] && colok[kx]) acc[ky * 3 + kx] = fmaf(tv[j], sL[ky * XW + px + kx], acc[ky * 3 + kx]);
        }
        if (++since == FLUSH_TILES) {
            flush(first);
            first = false;
            since = 0;
        }
    }
    if (since > 0) flush(first);
}

// entry e = tap * per_tap + r  ->  dw[r * 9 + (flip ? 8 - tap : tap)]
__global__ __launch_bounds__(TB) void wgrad_sum_kernel(const double* __restrict__ part, float* __restrict__ dw, int entries, int per_tap,
                                                       int wgs, int flip) {
    const int e = (int)(blockIdx.x * TB + threadIdx.x);
    if (e >= entries) return;
    double sum = 0.0;
#pragma unroll 16
    for (int b = 0; b < wgs; ++b) sum += part[(int64_t)b * entries + e];
    const int tap = e / per_tap, r = e - tap * per_tap;
    dw[r * 9 + (flip ? 8 - tap : tap)] = (float)sum;
}

inline size_t workspace_bytes(int64_t n, int64_t H, int64_t W) {
    const int64_t a = split(n, H, W, W0_MAX_WG).wgs * W0_ENTRIES, b = split(n, H, W, W1_MAX_WG).wgs * W1_ENTRIES;
    return (size_t)(a > b ? a : b) * sizeof(double);
}

}  // namespace wgrad
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_wgrad_workspace_bytes(int64_t n, int64_t H, int64_t W) {
    if (!wgrad::sizes_ok(n, H, W) || !wgrad::supported(n, H, W)) return 0;
    return wgrad::workspace_bytes(n, H, W);
}

int deqsci_wgrad3x3_c64_c64_f32(const float* x, const float* g, float* dw, int64_t n, int64_t H, int64_t W, void* workspace,
                                deqsci_stream_t stream) {
    if (!x || !g || !dw || !workspace) return DEQSCI_ERR_NULL;
    if (!wgrad::sizes_ok(n, H, W)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(x) || !aligned16(g) || misaligned(dw, 4) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    if (!wgrad::supported(n, H, W)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t act = n * H * W * 64 * (int64_t)sizeof(float), out = wgrad::W0_ENTRIES * (int64_t)sizeof(float);
    const int64_t ws = (int64_t)wgrad::workspace_bytes(n, H, W);
    if (overlaps(dw, out, x, act) || overlaps(dw, out, g, act) || overlaps(workspace, ws, x, act) || overlaps(workspace, ws, g, act) ||
        overlaps(workspace, ws, dw, out))
        return DEQSCI_ERR_UNSUPPORTED;
    const wgrad::Split sp = wgrad::split(n, H, W, wgrad::W0_MAX_WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(wgrad::wgrad_c64_kernel<false>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, x, g, part, (int)H, (int)W,
                       (int)ceil_div(W, wgrad::TW), sp.tiles, sp.per_wg);
    int rc = launch_status();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(wgrad::wgrad_sum_kernel, dim3((unsigned)ceil_div(wgrad::W0_ENTRIES, TB)), dim3(TB), 0, st, part, dw,
                       wgrad::W0_ENTRIES, 64 * 64, (int)sp.wgs, 0);
    return launch_status();
}

int deqsci_wgrad3x3_c1_c64_f32(const float* s, const float* t, float* dw, int flip, int64_t n, int64_t H, int64_t W, void* workspace,
                               deqsci_stream_t stream) {
    if (!s || !t || !dw || !workspace) return DEQSCI_ERR_NULL;
    if (!wgrad::sizes_ok(n, H, W)) return DEQSCI_ERR_SHAPE;
    if (misaligned(s, 4) || misaligned(t, 4) || misaligned(dw, 4) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    if ((flip != 0 && flip != 1) || !wgrad::supported(n, H, W)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t img = n * H * W * (int64_t)sizeof(float), act = img * 64, out = wgrad::W1_ENTRIES * (int64_t)sizeof(float);
    const int64_t ws = (int64_t)wgrad::workspace_bytes(n, H, W);
    if (overlaps(dw, out, s, img) || overlaps(dw, out, t, act) || overlaps(workspace, ws, s, img) || overlaps(workspace, ws, t, act) ||
        overlaps(workspace, ws, dw, out))
        return DEQSCI_ERR_UNSUPPORTED;
    const wgrad::Split sp = wgrad::split(n, H, W, wgrad::W1_MAX_WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(wgrad::wgrad_c1_kernel, dim3((unsigned)sp.wgs), dim3(TB), 0, st, s, t, part, (int)H, (int)W,
                       (int)ceil_div(W, wgrad::TW), sp.tiles, sp.per_wg);
    int rc = launch_status();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(wgrad::wgrad_sum_kernel, dim3((unsigned)ceil_div(wgrad::W1_ENTRIES, TB)), dim3(TB), 0, st, part, dw,
                       wgrad::W1_ENTRIES, 64, (int)sp.wgs, flip);
    return launch_status();
}

}  // extern "C"
