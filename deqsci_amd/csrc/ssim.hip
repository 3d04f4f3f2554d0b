// Per-frame mean SSIM for MI355X (gfx950): an evaluation metric, run once per batch, never inside the loop.
//
//   S1 ssim_tile_kernel    one workgroup = one (measurement, frame, 32 x 16 output tile): x and y of the tile plus its
//                          window//2 halo are staged in LDS (zero outside the image, x optionally clamped to [0,1]),
//                          a horizontal pass writes the five moment planes (x, y, x^2, y^2, xy) for every staged row,
//                          a vertical pass forms the SSIM map, and the tile's sum of map values is written in fp64
//   S2 ssim_reduce_kernel  per (measurement, frame): the tile sums in a fixed order (one wave), divided by the number of map values
//
// Definition: pytorch_ssim._ssim (the reference's, Wang et al. 2004 with a Gaussian window of sigma 1.5, zero padding of
// window//2, C1 = 0.01^2, C2 = 0.03^2), i.e. the map is
//     ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),   s11 = E[x^2] - mu1^2 ...
// "same" averages all H*W map values; "valid" only those whose window lies inside the image.
//
// Arithmetic: the taps are the reference's (fp32 exp values normalised by their fp32 sum), the 2-D window their outer
// product (separable).  Everything after the load is fp64: s11 = E[x^2] - mu1^2 cancels in flat regions, and in fp32 the
// reference's own values are up to 1.2e-5 away from exact on the shipped clips.  A NaN anywhere in a frame reaches the
// frame's sum (the clamp is written with comparisons, which keep NaN, as torch.clamp does).
// Determinism: no atomics; the per-thread, per-wave and per-workgroup summation orders are fixed, so are S2's.
#include <math.h>

#include "rows.hpp"

namespace deqsci {
namespace ssim {

constexpr int TW = 32;            // output columns per tile (= one double per lane across half a wave)
constexpr int TH = 16;            // output rows per tile
constexpr int MAXWIN = 15;

struct Taps {
    float g[MAXWIN];
};

// LDS: the five moment planes (fp64, (TH + 2R) x TW each), then x and y of the haloed tile (fp32, (TH + 2R) x (TW + 2R)).
inline size_t lds_bytes(int R) {
    const size_t rh = TH + 2 * R, rw = TW + 2 * R;
    return 5 * rh * TW * sizeof(double) + 2 * rh * rw * sizeof(float);
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN stays NaN

template <int WIN>
__global__ __launch_bounds__(TB) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       double* __restrict__ part, Taps taps, int64_t M, int64_t H, int64_t W,
                                                       int64_t B, int layout, int valid, int clamp_x, int64_t tiles_x,
                                                       int64_t n_tiles) {
    constexpr int R = WIN / 2;
    constexpr int RH = TH + 2 * R, RW = TW + 2 * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* hm = reinterpret_cast<double*>(lds_raw);                  // [5][RH][TW]
    float* xs = reinterpret_cast<float*>(hm + 5 * RH * TW);            // [RH][RW]
    float* ys = xs + RH * RW;
    __shared__ double wsum[TB / WAVE];

    const int tid = threadIdx.x;
    const int64_t total = M * n_tiles * B;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        // item = (m * B + f) * n_tiles + t: consecutive workgroups walk the tiles of one frame
        const int64_t t = item % n_tiles;
        const int64_t mf = item / n_tiles;
        const int64_t f = mf % B, m = mf / B;
        const int64_t r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
        int64_t base, sp, sr;                                          // element (m, h, w, f) = base + h * sr + w * sp
        if (layout == DEQSCI_LAYOUT_HWB) { base = m * H * W * B + f; sp = B; sr = W * B; }
        else { base = (m * B + f) * H * W; sp = 1; sr = W; }

        __syncthreads();                                               // the previous item's LDS readers are done
        for (int i = tid; i < RH * RW; i += TB) {
            const int rr = i / RW, cc = i % RW;
            const int64_t h = r0 - R + rr, w = c0 - R + cc;
            float xv = 0.0f, yv = 0.0f;
            if (h >= 0 && h < H && w >= 0 && w < W) {
                const int64_t e = base + h * sr + w * sp;
                xv = x[e];
                yv = y[e];
                if (clamp_x) xv = clamp01(xv);
            }
            xs[i] = xv;
            ys[i] = yv;
        }
        __syncthreads();
        // horizontal pass: every staged row, the TW output columns
        for (int i = tid; i < RH * TW; i += TB) {
            const int rr = i / TW, cc = i % TW;
            const float* xr = xs + rr * RW + cc;
            const float* yr = ys + rr * RW + cc;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double g = (double)taps.g[k];
                const double a = (double)xr[k], b = (double)yr[k];
                s0 = fma(g, a, s0);
                s1 = fma(g, b, s1);
                s2 = fma(g, a * a, s2);
                s3 = fma(g, b * b, s3);
                s4 = fma(g, a * b, s4);
            }
            hm[0 * RH * TW + i] = s0;
            hm[1 * RH * TW + i] = s1;
            hm[2 * RH * TW + i] = s2;
            hm[3 * RH * TW + i] = s3;
            hm[4 * RH * TW + i] = s4;
        }
        __syncthreads();
        // vertical pass and the map, summed per thread
        const int64_t rlo = valid ? R : 0, rhi = valid ? H - R : H;        // counted rows [rlo, rhi), columns likewise
        const int64_t clo = valid ? R : 0, chi = valid ? W - R : W;
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        double acc = 0.0;
        for (int i = tid; i < TH * TW; i += TB) {
            const int rr = i / TW, cc = i % TW;
            const int64_t h = r0 + rr, w = c0 + cc;
            if (h < rlo || h >= rhi || w < clo || w >= chi) continue;
            double v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const double* col = hm + q * RH * TW + rr * TW + cc;
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < WIN; ++k) s = fma((double)taps.g[k], col[k * TW], s);
                v[q] = s;
            }
            const double mu1 = v[0], mu2 = v[1];
            const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const double s11 = v[2] - mu1_sq, s22 = v[3] - mu2_sq, s12 = v[4] - mu12;
            acc += ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2));
        }
        // workgroup sum in a fixed order: wave butterfly, then the four wave sums in wave order
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
        if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = acc;
        __syncthreads();
        if (tid == 0) part[item] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// one wave per (measurement, frame): its tile sums by rows::wave_fold, divided by the number of map values
__global__ __launch_bounds__(TB) void ssim_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int64_t MB,
                                                         int64_t n_tiles, double count) {
    for (int64_t i = (int64_t)blockIdx.x * (TB / WAVE) + threadIdx.x / WAVE; i < MB; i += (int64_t)gridDim.x * (TB / WAVE)) {
        const double s = rows::wave_fold(part + i * n_tiles, n_tiles);
        if ((threadIdx.x & (WAVE - 1)) == 0) out[i] = s / count;
    }
}

// the reference's gaussian(window, 1.5): exp in double, rounded to fp32, divided by the fp32 sum
inline Taps make_taps(int win) {
    Taps tp = {};
    float sum = 0.0f;
    for (int k = 0; k < win; ++k) {
        const double d = (double)(k - win / 2);
        tp.g[k] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += tp.g[k];
    }
    for (int k = 0; k < win; ++k) tp.g[k] = tp.g[k] / sum;
    return tp;
}

inline int64_t tiles_of(int64_t H, int64_t W) { return ceil_div(H, TH) * ceil_div(W, TW); }

inline int check(int64_t M, int64_t H, int64_t W, int64_t B, int layout) {
    if (M < 0 || B < 0 || H < 1 || W < 1) return DEQSCI_ERR_SHAPE;
    if (layout != DEQSCI_LAYOUT_HWB && layout != DEQSCI_LAYOUT_BHW) return DEQSCI_ERR_UNSUPPORTED;
    // (the element offsets below are int64: refuse sizes whose byte counts would overflow it)
    if (H > (int64_t)1 << 30 || W > (int64_t)1 << 30 || (M > 0 && B > 0 && M * B > ((int64_t)1 << 60) / (H * W))) return DEQSCI_ERR_SHAPE;
    return 0;
}

}  // namespace ssim
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int64_t deqsci_ssim_workspace_bytes(int64_t M, int64_t H, int64_t W, int64_t B, int layout) {
    if (int e = ssim::check(M, H, W, B, layout)) return e;
    return M * B * ssim::tiles_of(H, W) * (int64_t)sizeof(double);
}

int deqsci_ssim_f32(const float* x, const float* y, double* out, int64_t M, int64_t H, int64_t W, int64_t B, int layout, int window,
                    int valid, int clamp_x, void* workspace, deqsci_stream_t stream) {
    if (!x || !y || !out || !workspace) return DEQSCI_ERR_NULL;
    if (int e = ssim::check(M, H, W, B, layout)) return e;
    if (window < 3 || window > ssim::MAXWIN || window % 2 == 0) return DEQSCI_ERR_SHAPE;
    if (valid && (H < window || W < window)) return DEQSCI_ERR_SHAPE;          // empty interior
    if (M == 0 || B == 0) return 0;
    if (misaligned(x, 4) || misaligned(y, 4) || misaligned(out, 8) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    const int64_t n_in = M * H * W * B * (int64_t)sizeof(float);
    const int64_t n_out = M * B * (int64_t)sizeof(double);
    const int64_t n_ws = deqsci_ssim_workspace_bytes(M, H, W, B, layout);
    if (overlaps(out, n_out, x, n_in) || overlaps(out, n_out, y, n_in) || overlaps(workspace, n_ws, x, n_in) ||
        overlaps(workspace, n_ws, y, n_in) || overlaps(workspace, n_ws, out, n_out))
        return DEQSCI_ERR_UNSUPPORTED;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const ssim::Taps taps = ssim::make_taps(window);
    const int64_t tiles_x = ceil_div(W, ssim::TW);
    const int64_t n_tiles = ssim::tiles_of(H, W);
    const int64_t total = M * B * n_tiles;
    const dim3 grid((unsigned)(total < ((int64_t)1 << 30) ? total : ((int64_t)1 << 30)));
    const size_t lds = ssim::lds_bytes(window / 2);                  // <= 49.4 KB (window 15): three workgroups per CU
    double* part = static_cast<double*>(workspace);
#define SSIM_LAUNCH(WIN)                                                                                                         \
    case WIN:                                                                                                                    \
        hipLaunchKernelGGL(ssim::ssim_tile_kernel<WIN>, grid, dim3(TB), lds, st, x, y, part, taps, M, H, W, B, layout, valid,  \
                           clamp_x, tiles_x, n_tiles);                                                                          \
        break;
    switch (window) {
        SSIM_LAUNCH(3) SSIM_LAUNCH(5) SSIM_LAUNCH(7) SSIM_LAUNCH(9) SSIM_LAUNCH(11) SSIM_LAUNCH(13) SSIM_LAUNCH(15)
    }
#undef SSIM_LAUNCH
    if (int e = launch_status()) return e;
    const int64_t count = valid ? (H - window + 1) * (W - window + 1) : H * W;
    const int64_t MB = M * B;
    const int64_t nb = ceil_div(MB, TB / WAVE);
    hipLaunchKernelGGL(ssim::ssim_reduce_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(TB), 0, st, part, out, MB, n_tiles,
                       (double)count);
    return launch_status();
}

}  // extern "C"
