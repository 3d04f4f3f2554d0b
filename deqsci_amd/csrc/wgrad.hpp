// What the weight-gradient files share (csrc/wgrad.hip: W0, W1; csrc/wgrad_bn.hip: W0-BN, W2): the tiling, the split of the tiles over the
// workgroups, and the 64 -> 64 matrix-instruction kernel itself - ONE body, so that the nine-tap arithmetic of W0-BN is W0's bit for bit.
#pragma once
#include "common.hpp"

namespace deqsci {
namespace wgrad {

constexpr int TW = 32;                                   // pixels of a tile
constexpr int XW = TW + 2;                               // with the halo columns
constexpr int CHAIN = DEQSCI_WGRAD_CHAIN;
constexpr int FLUSH_TILES = CHAIN / TW;                  // a partial is flushed after this many tiles
constexpr int W0_MAX_WG = 256, W1_MAX_WG = 512;          // fixed, not the device's: the workspace query has no device
constexpr int W0_ENTRIES = 9 * 64 * 64, W1_ENTRIES = 9 * 64;
constexpr int W0_SUMS = 64;                              // W0-BN: the per-channel sums of g behind a workgroup's W0_ENTRIES
constexpr int64_t MAX_SIDE = 1 << 20;
static_assert(CHAIN % TW == 0 && FLUSH_TILES >= 1, "a flush falls on a tile boundary");

typedef float v16f __attribute__((ext_vector_type(16)));

struct Split {
    int64_t tiles, per_wg, wgs;
};
inline bool sizes_ok(int64_t n, int64_t H, int64_t W) { return n >= 1 && H >= 1 && W >= 1; }
inline bool supported(int64_t n, int64_t H, int64_t W) {
    return n <= MAX_SIDE && H <= MAX_SIDE && W <= MAX_SIDE && (double)n * (double)H * (double)ceil_div(W, TW) <= (double)INT32_MAX;
}
inline Split split(int64_t n, int64_t H, int64_t W, int max_wg) {
    Split s;
    s.tiles = n * H * ceil_div(W, TW);
    s.per_wg = ceil_div(s.tiles, max_wg);
    s.wgs = ceil_div(s.tiles, s.per_wg);                 // (no idle workgroup: every one has at least one tile)
    return s;
}

struct Tile {
    int64_t row;                                         // img * H + h
    int h, w0;
};
__device__ __forceinline__ Tile tile_at(int64_t t, int H, int tilesW) {
    Tile r;
    r.row = t / tilesW;
    r.w0 = (int)(t - r.row * tilesW) * TW;
    r.h = (int)(r.row % H);
    return r;
}

// SUMS: W0-BN's second output from the same pass - the tile of g is in LDS anyway, wave w adds its 8 pixels of channel `lane` in fp32
// (at most FLUSH_TILES * 8 terms between two flushes), and a flush adds the four waves' sums, in wave order, to the 64 float64 words behind
// the workgroup's W0_ENTRIES.  A pixel beyond the row's end is staged as zero and adds nothing.
template <bool SUMS>
__global__ __launch_bounds__(TB) void wgrad_c64_kernel(const float* __restrict__ x, const float* __restrict__ g, double* __restrict__ part,
                                                       int H, int W, int tilesW, int64_t tiles, int64_t per_wg) {
    __shared__ float gL[TW * 64];
    __shared__ float xL[3 * XW * 64];
    __shared__ float sumL[SUMS ? TB : 1];
    const int tid = (int)threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int cob = (wave >> 1) * 32, cib = (wave & 1) * 32, col = lane & 31, half = lane >> 5;
    const int64_t t0 = (int64_t)blockIdx.x * per_wg, t1 = t0 + per_wg < tiles ? t0 + per_wg : tiles;

    v16f acc[9];
    float gsum = 0.0f;
    float4 rg[2], rx[7];
    auto fetch = [&](const Tile& tl) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * TB, px = idx >> 4, c4 = idx & 15, w = tl.w0 + px;
            rg[i] = w < W ? ld4(g + ((tl.row * W + w) * 64 + c4 * 4)) : f4(0.0f);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int idx = tid + i * TB;
            rx[i] = f4(0.0f);
            if (idx < 3 * XW * 16) {
                const int row = idx / (XW * 16), rem = idx - row * (XW * 16), c = rem >> 4, c4 = rem & 15;
                const int hh = tl.h + row - 1, ww = tl.w0 + c - 1;
                if (hh >= 0 && hh < H && ww >= 0 && ww < W) rx[i] = ld4(x + (((tl.row + row - 1) * W + ww) * 64 + c4 * 4));
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) st4(gL + (tid + i * TB) * 4, rg[i]);
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (tid + i * TB < 3 * XW * 16) st4(xL + (tid + i * TB) * 4, rx[i]);
    };
    double* const mine = part + (int64_t)blockIdx.x * (W0_ENTRIES + (SUMS ? W0_SUMS : 0));
    auto flush = [&](bool first) {
        double* base = mine + ((cob + 4 * half) * 64 + cib + col);
        asm volatile("" : "+v"(base));                                      // (the 144 addresses are formed here, not kept across the tile loop)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double* p = base + ((tap * 64 + (r & 3) + 8 * (r >> 2)) * 64);
                *p = first ? (double)acc[tap][r] : *p + (double)acc[tap][r];
            }
            asm volatile("" ::: "memory");                                  // one tap's 16 doubles in flight, not all 144
        }
        if constexpr (SUMS) {
            sumL[tid] = gsum;                                               // (the tile loop's closing barrier lies between the last read and this)
            gsum = 0.0f;
            __syncthreads();
            if (tid < W0_SUMS) {
                double d = 0.0;
#pragma unroll
                for (int wv = 0; wv < TB / WAVE; ++wv) d += (double)sumL[wv * WAVE + tid];
                mine[W0_ENTRIES + tid] = first ? d : mine[W0_ENTRIES + tid] + d;
            }
        }
    };

    Tile cur = tile_at(t0, H, tilesW);
    fetch(cur);
    const float* const gb = gL + cob + col;
    const float* const xb = xL + cib + col;
    for (int64_t c0 = t0; c0 < t1; c0 += FLUSH_TILES) {                     // one partial per FLUSH_TILES tiles: the accumulators live in this loop only
        const int64_t c1 = c0 + FLUSH_TILES < t1 ? c0 + FLUSH_TILES : t1;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        for (int64_t t = c0; t < c1; ++t) {
            stage();
            __syncthreads();
            const Tile now = cur;
            if (t + 1 < t1) {
                cur = tile_at(t + 1, H, tilesW);
                fetch(cur);
            }
            if constexpr (SUMS) {
                constexpr int PX = TW / (TB / WAVE);
#pragma unroll
                for (int j = 0; j < PX; ++j) gsum += gL[(wave * PX + j) * 64 + lane];
            }
            const bool rowok[3] = {now.h > 0, true, now.h < H - 1};
#pragma unroll 4
            for (int pp = 0; pp < TW / 2; ++pp) {
                const int px = 2 * pp + half, w = now.w0 + px;
                // every operand is read unconditionally; what must not be multiplied is zero on both sides by construction: g is staged as
                // zero beyond the row's end and x as zero outside the image, a tap row / column outside the image zeroes a, and the one real
                // x value a pixel beyond the row's end could meet (w == W, kx == 0: x[W-1]) is read one column further, where x is zero
                const float a = gb[px * 64];
                const float ax[3] = {w == 0 ? 0.0f : a, a, w == W - 1 ? 0.0f : a};
                const int xc[3] = {px + (w == W ? 1 : 0), px + 1, px + 2};
                float b[9];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) b[ky * 3 + kx] = xb[(ky * XW + xc[kx]) * 64];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
                        acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(rowok[ky] ? ax[kx] : 0.0f, b[ky * 3 + kx], acc[ky * 3 + kx], 0, 0, 0);
            }
            __syncthreads();
        }
        flush(c0 == t0);
    }
}

}  // namespace wgrad
}  // namespace deqsci
