// Real spectral normalisation in train mode for MI355X (gfx950): the power-iteration step of a spectrally normalised 3x3 convolution
// (networks/provable/model/conv_sn_chen.py:29-50 in the reference) and the gradient of the normalised weight, without host traffic.
//
//   R1 deqsci_realsn_power_f32, n_iters times S1-S3, then S4:
//      S1 conv_kernel<.., true>   t1 = W^T u (the adjoint of the pad-1 convolution), and the float64 sum of t1^2 per workgroup
//      S2 conv_kernel<.., false>  v = t1 / max(|t1|, eps) formed while the tile is staged (and written once, by the first channel
//                                 group), t2 = W v, and the float64 sum of t2^2 per workgroup
//      S3 normalise_kernel        u = t2 / max(|t2|, eps), and the float64 chunk sums of u * t2 (= u * (W v): cur_sigma)
//      S4 weight_kernel           weight = W / cur_sigma * sigma_t, the record (|W^T u|, |W v|, cur_sigma)
//   R2 deqsci_realsn_grad_f32:
//      T1 cgrad_kernel            C[o,i,ky,kx] = sum_p u[o,p] v[i, p + (ky-1, kx-1)], one wave per (o, i); its first workgroups form the
//                                 float64 chunk sums of G * W instead
//      T2 grad_final_kernel       dW = (sigma_t / cur_sigma) * (G - (sum(G W) / cur_sigma) * C)
//   R3 deqsci_realsn_pack_f32, one launch: the weight R1 wrote -> the packs the convolution kernels read, so that a weight that changes at
//      every f-call never goes through the host packers (a dozen torch operations and a host -> device copy of G each)
//      pack64_kernel              (64,64): U = G g G^T of F(2x2,3x3) and of F(4x4,3x3) in the MFMA-lane order of csrc/winograd.hip /
//                                 csrc/winograd44.hip, and the F(2x2,3x3) pack of the transposed weight; float64, one rounding to fp32
//      pack_edge_kernel           (1,64) / (64,1): the two stencil packs (csrc/ffdnet_edges.hip) of the layer and of its transpose, permutations
//
// A norm gates the stage behind it, so a stage boundary is a launch boundary: every workgroup of the next launch folds the partial sums
// itself, in the same order (rows::wave_fold), and gets the same bits.  No atomics, no counters: bit-equal run to run.
// Arithmetic: the convolutions accumulate in fp32 by fmaf over (input channel, ky, kx) ascending, a tap outside the map is a zero of
// the staged tile; C accumulates p = lane, lane + 64, ... by fmaf and then the wave's xor butterfly in fp32.  The sums of squares, cur_sigma
// and sum(G W) are float64: fma of converted floats (exact products) per thread, then rows::block_sum / rows::wave_fold; S3 and the G W sum
// walk their rows in the chunk order of csrc/rows.hpp.  sqrt in float64; then, in fp32: the rounding of the norm, max(., eps) as Python's
// max(norm, eps) (a NaN norm stays NaN), the elementwise division, and W / cur_sigma * sigma_t in that order (cur_sigma = 0: +-Inf where
// W != 0, NaN where W = 0, as the reference's expression gives).
#include "rows.hpp"

namespace deqsci {
namespace realsn {

using namespace rows;

constexpr int TILE = 16;                                  // a workgroup's output tile: TILE x TILE pixels = TB threads
constexpr int HALO = TILE + 2;
constexpr int CI_CHUNK = 16;                              // input channels staged at a time
constexpr int STAGE = (CI_CHUNK * HALO * HALO + TB - 1) / TB;   // halo-tile elements a thread stages per chunk
constexpr int CMAX = 64;                                  // the widest layer
constexpr int CG_UNROLL = 4;                              // pixels per lane whose loads the C kernel keeps in flight
constexpr int PER_THREAD = 4;
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                       // 4096 elements per workgroup of the row sums
constexpr int64_t MAX_PIXELS = (int64_t)1 << 20;          // h * w: every element offset stays far below 2^31

static_assert(TILE * TILE == TB, "one thread per pixel of the tile");

// max(norm, eps) as the reference's Python expression evaluates it: eps only where eps > norm, so a NaN norm stays NaN
__device__ __forceinline__ float denominator(double sumsq, float eps) {
    const float n = (float)sqrt(sumsq);
    return eps > n ? eps : n;
}

// out[co, p] = sum_{ci, ky, kx} Wsel[co, ci, ky, kx] * in[ci, p + (ky-1, kx-1)], in = `in` / max(sqrt(sum in_part), eps) where in_part is given.
// TRANSPOSE = false: Wsel[co, ci, k] = W[co, ci, k] (W is (CO, CI, 3, 3)); true: Wsel[co, ci, k] = W[ci, co, 8 - k] (W is (CI, CO, 3, 3)).
// grid (tiles, CO / COT); part[blockIdx.y * tiles + blockIdx.x] = the workgroup's float64 sum of out^2.
template <int COT, bool TRANSPOSE>
__global__ __launch_bounds__(TB) void conv_kernel(const float* __restrict__ W, const float* __restrict__ in, const double* __restrict__ in_part,
                                                  int n_in_part, float eps, float* __restrict__ in_norm_out, double* __restrict__ in_norm_rec,
                                                  float* __restrict__ out, double* __restrict__ part, int CI, int CO, int h, int w) {
    __shared__ float sW[CMAX * 9 * COT];
    __shared__ float sIn[CI_CHUNK][HALO * HALO];
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int tiles_x = (w + TILE - 1) / TILE;
    const int ty0 = ((int)blockIdx.x / tiles_x) * TILE, tx0 = ((int)blockIdx.x % tiles_x) * TILE;
    const int co0 = (int)blockIdx.y * COT;
    const int P = h * w;
    float d = 1.0f;
    if (in_part) {
        const double s = wave_fold(in_part, n_in_part);
        d = denominator(s, eps);
        if (in_norm_rec && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *in_norm_rec = sqrt(s);
    }
    for (int idx = tid; idx < CI * 9 * COT; idx += TB) {
        const int c = idx % COT, k = (idx / COT) % 9, ci = idx / (COT * 9), co = co0 + c;
        float v = 0.0f;
        if (co < CO) v = TRANSPOSE ? W[(ci * CO + co) * 9 + (8 - k)] : W[(co * CI + ci) * 9 + k];
        sW[idx] = v;
    }
    const int ly = tid / TILE, lx = tid % TILE;
    float acc[COT];
#pragma unroll
    for (int c = 0; c < COT; ++c) acc[c] = 0.0f;
    // a chunk's halo tiles travel global -> registers -> LDS; the next chunk's loads are issued before this chunk's products, all at once
    float r[STAGE];
    int re[STAGE];                                         // the element each register holds, -1 outside the map
    auto fetch = [&](int c0) {
        const int nci = CI - c0 < CI_CHUNK ? CI - c0 : CI_CHUNK;
#pragma unroll
        for (int q = 0; q < STAGE; ++q) {
            const int idx = tid + q * TB, cc = idx / (HALO * HALO), rr = idx % (HALO * HALO);
            const int y = ty0 + rr / HALO - 1, x = tx0 + rr % HALO - 1;
            const bool inside = idx < nci * HALO * HALO && y >= 0 && y < h && x >= 0 && x < w;
            re[q] = inside ? (c0 + cc) * P + y * w + x : -1;
            r[q] = inside ? in[re[q]] : 0.0f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < CI; c0 += CI_CHUNK) {
        const int nci = CI - c0 < CI_CHUNK ? CI - c0 : CI_CHUNK;
        __syncthreads();                                   // the previous chunk's readers are done (and sW is written)
#pragma unroll
        for (int q = 0; q < STAGE; ++q) {
            const int idx = tid + q * TB, rr = idx % (HALO * HALO), hy = rr / HALO, hx = rr % HALO;
            if (idx < nci * HALO * HALO) {
                float v = r[q];
                if (re[q] >= 0) {
                    if (in_part) v = v / d;
                    if (in_norm_out && blockIdx.y == 0 && hy >= 1 && hy <= TILE && hx >= 1 && hx <= TILE) in_norm_out[re[q]] = v;
                }
                sIn[idx / (HALO * HALO)][rr] = v;
            }
        }
        __syncthreads();
        if (c0 + CI_CHUNK < CI) fetch(c0 + CI_CHUNK);
        for (int cc = 0; cc < nci; ++cc) {
            const float* wr = sW + (c0 + cc) * 9 * COT;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float a = sIn[cc][(ly + k / 3) * HALO + lx + k % 3];
#pragma unroll
                for (int c = 0; c < COT; ++c) acc[c] = fmaf(wr[k * COT + c], a, acc[c]);
            }
        }
    }
    const int y = ty0 + ly, x = tx0 + lx;
    double s = 0.0;
    if (y < h && x < w) {
#pragma unroll
        for (int c = 0; c < COT; ++c) {
            if (co0 + c < CO) {
                out[(co0 + c) * P + y * w + x] = acc[c];
                s = fma((double)acc[c], (double)acc[c], s);
            }
        }
    }
    s = block_sum(s, wsum);
    if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// u = t / max(sqrt(sum t_part), eps) and the chunk sums of u * t, in the order of csrc/rows.hpp (t, u 16-byte aligned)
__global__ __launch_bounds__(TB) void normalise_kernel(const float* __restrict__ t, const double* __restrict__ t_part, int n_t_part, float eps,
                                                       float* __restrict__ u, double* __restrict__ part, double* __restrict__ norm_rec,
                                                       int64_t N, int64_t n_chunks) {
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const double sq = wave_fold(t_part, n_t_part);
    const float d = denominator(sq, eps);
    if (blockIdx.x == 0 && tid == 0) *norm_rec = sqrt(sq);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            const float4 tv = load4(t, e, N, true);
            const float4 uv = inside4(tv / f4(d), e, N);
            store4(u, e, N, true, uv);
            acc = dot4(uv, tv, acc);
        }
        acc = block_sum(acc, wsum);
        if (tid == 0) part[c] = acc;
    }
}

// weight = W / cur_sigma * sigma_t (two fp32 roundings, in this order), cur_sigma = the fold of the chunk sums, rounded to fp32
__global__ __launch_bounds__(TB) void weight_kernel(const float* __restrict__ W, const double* __restrict__ part, int n_part, float sigma_t,
                                                    float* __restrict__ weight, double* __restrict__ sigma_rec, int64_t N) {
    const double cs = wave_fold(part, n_part);
    const float csf = (float)cs;
    if (blockIdx.x == 0 && threadIdx.x == 0) *sigma_rec = cs;
    const int64_t e = ((int64_t)blockIdx.x * TB + threadIdx.x) * 4;
    if (e >= N) return;
    const float4 q = load4(W, e, N, true) / f4(csf);
    store4(weight, e, N, true, q * f4(sigma_t));
}

// workgroups [0, n_gw): the float64 chunk sums of G * W (rows.hpp's order); the others: one wave per (o, i), C[o, i, :] over the map
__global__ __launch_bounds__(TB) void cgrad_kernel(const float* __restrict__ G, const float* __restrict__ W, const float* __restrict__ u,
                                                   const float* __restrict__ v, float* __restrict__ C, double* __restrict__ gw_part, int CI,
                                                   int CO, int h, int w, int64_t N, int n_gw) {
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < n_gw) {
        const int64_t base = (int64_t)blockIdx.x * CHUNK;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            acc = dot4(load4(G, e, N, true), load4(W, e, N, true), acc);
        }
        acc = block_sum(acc, wsum);
        if (tid == 0) gw_part[blockIdx.x] = acc;
        return;
    }
    const int pair = ((int)blockIdx.x - n_gw) * NW + tid / WAVE, lane = tid & (WAVE - 1);
    if (pair >= CO * CI) return;
    const int o = pair / CI, i = pair % CI, P = h * w;
    const float* ur = u + o * P;
    const float* vr = v + i * P;
    float acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
    // CG_UNROLL pixels per lane and round: their loads are issued together, their products added in the order p = lane, lane + 64, ...
    for (int p0 = lane; p0 < P; p0 += WAVE * CG_UNROLL) {
        float a[CG_UNROLL], b[CG_UNROLL][9];
#pragma unroll
        for (int j = 0; j < CG_UNROLL; ++j) {
            const int p = p0 + j * WAVE, y = p / w, x = p % w;
            a[j] = p < P ? ur[p] : 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                b[j][k] = (p < P && yy >= 0 && yy < h && xx >= 0 && xx < w) ? vr[yy * w + xx] : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < CG_UNROLL; ++j) {
            const int p = p0 + j * WAVE, y = p / w, x = p % w;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                if (p < P && yy >= 0 && yy < h && xx >= 0 && xx < w) acc[k] = fmaf(a[j], b[j][k], acc[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int s = WAVE / 2; s > 0; s >>= 1) acc[k] += __shfl_xor(acc[k], s, WAVE);
    }
    if (lane < 9) {
        float r = acc[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) r = lane == k ? acc[k] : r;
        C[pair * 9 + lane] = r;
    }
}

// dW = a * (G - s * C), s = (float)(sum(G W) / cur_sigma) in float64, a = sigma_t / (float)cur_sigma; every fp32 step rounded separately
__global__ __launch_bounds__(TB) void grad_final_kernel(const float* __restrict__ G, const float* __restrict__ C, const double* __restrict__ gw_part,
                                                        int n_gw, const double* __restrict__ record, float sigma_t, float* __restrict__ dW,
                                                        int64_t N) {
    const double gw = wave_fold(gw_part, n_gw);
    const double cs = record[2];
    const float s = (float)(gw / cs), a = sigma_t / (float)cs;
    const int64_t e = ((int64_t)blockIdx.x * TB + threadIdx.x) * 4;
    if (e >= N) return;
    const float4 sc = f4(s) * load4(C, e, N, true);
    store4(dW, e, N, true, f4(a) * (load4(G, e, N, true) - sc));
}

// ---- R3: the weight R1 wrote -> the packs the convolution kernels read
// The Winograd weight transforms, the constants of _hip.pack_winograd_weights / pack_winograd44_weights as doubles
__constant__ double G22[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
__constant__ double G44[6][3] = {{1.0 / 4.0, 0.0, 0.0},
                                 {-1.0 / 6.0, -1.0 / 6.0, -1.0 / 6.0},
                                 {-1.0 / 6.0, 1.0 / 6.0, -1.0 / 6.0},
                                 {1.0 / 24.0, 1.0 / 12.0, 1.0 / 6.0},
                                 {1.0 / 24.0, -1.0 / 12.0, 1.0 / 6.0},
                                 {0.0, 0.0, 1.0}};
constexpr int PACK_LANES = 256;                           // the (q, i, j, s) positions of one (cin chunk, cout half): contiguous in both packs
constexpr int64_t PACK22 = 64 * 64 * 16, PACK44 = 64 * 64 * 36, PACK_EDGE = 64 * 9;
static_assert(PACK_LANES == TB, "one thread per (q, i, j, s) position");

// U[a][b] = sum_k (sum_j G[a][j] g[j][k]) G[b][k] in float64: T = G g first, then T G^T; every sum left to right from its first product (the
// zero entries of G are multiplied and added like the others), every product and sum rounded by itself; one rounding to fp32 at the store
template <int R>
__device__ __forceinline__ void transform(const double (&G)[R][3], const double (&g)[3][3], double (&T)[R][3]) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            T[a][k] = __dadd_rn(__dadd_rn(__dmul_rn(G[a][0], g[0][k]), __dmul_rn(G[a][1], g[1][k])), __dmul_rn(G[a][2], g[2][k]));
    }
}
template <int R>
__device__ __forceinline__ float transformed(const double (&G)[R][3], const double (&T)[R][3], int a, int b) {
    return (float)__dadd_rn(__dadd_rn(__dmul_rn(T[a][0], G[b][0]), __dmul_rn(T[a][1], G[b][1])), __dmul_rn(T[a][2], G[b][2]));
}

// (64,64,3,3) weight -> blockIdx.y = 0: the F(2x2,3x3) pack, 1: the F(4x4,3x3) pack, 2: the F(2x2,3x3) pack of the transposed weight
// (wt[co, ci, ky, kx] = w[ci, co, 2 - ky, 2 - kx]).  blockIdx.x = 2 c + wn; thread = (q, i, j, s): cout = 32 wn + 16 j + i, cin = 8 c + 2 q + s,
// so that every store of a workgroup is 256 consecutive floats.  A NULL pack's workgroups return at once.
__global__ __launch_bounds__(TB) void pack64_kernel(const float* __restrict__ w, float* __restrict__ u22, float* __restrict__ u44,
                                                    float* __restrict__ t22) {
    const int kind = (int)blockIdx.y;
    float* out = kind == 0 ? u22 : kind == 1 ? u44 : t22;
    if (!out) return;
    const int t = (int)threadIdx.x, c = (int)blockIdx.x >> 1, wn = (int)blockIdx.x & 1;
    const int s = t & 1, j = (t >> 1) & 1, i = (t >> 2) & 15, q = t >> 6;
    const int cout = 32 * wn + 16 * j + i, cin = 8 * c + 2 * q + s;
    double g[3][3];
    const float* src = kind == 2 ? w + (cin * 64 + cout) * 9 : w + (cout * 64 + cin) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = (double)src[kind == 2 ? 8 - k : k];
    if (kind == 1) {
        double T[6][3];
        transform<6>(G44, g, T);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = 0; b < 6; ++b)       // [c][s = 6 (a % 3) + b][rg = a / 3][cgp = wn][q][i][j][ks]
                out[(((c * 18 + (a % 3) * 6 + b) * 2 + a / 3) * 2 + wn) * PACK_LANES + t] = transformed<6>(G44, T, a, b);
        }
    } else {
        double T[4][3];
        transform<4>(G22, g, T);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b)       // [c][xi = 4 a + b][wn][q][i][j][s]
                out[((c * 16 + a * 4 + b) * 2 + wn) * PACK_LANES + t] = transformed<4>(G22, T, a, b);
        }
    }
}

// An edge layer's 64 x 9 weight w[ch * 9 + k] (ch the layer's 64-channel side) -> the two stencil packs, pure permutations:
//   wide[k * 64 + ch]                        = w[ch * 9 + k']     (_hip.pack_c1_to_64_weights: [tap][cout / 4][cout % 4])
//   narrow[((ch / 32) * 9 + k) * 32 + ch % 32] = w[ch * 9 + k']   (_hip.pack_c64_to_1_weights: [half][tap][cin % 32])
// k' = k for the layer's own pack, 8 - k for the pack of its transpose (vjp._transposed: the other layout).  C_in = 1: wide is the layer's
// own, narrow the transposed; C_in = 64: the other way round.
__global__ __launch_bounds__(TB) void pack_edge_kernel(const float* __restrict__ w, float* __restrict__ wide, float* __restrict__ narrow,
                                                       int flip_wide) {
    const int e = (int)(blockIdx.x * TB + threadIdx.x);
    if (e >= (int)PACK_EDGE) return;
    if (wide) {
        const int k = e / 64, ch = e % 64;
        wide[e] = w[ch * 9 + (flip_wide ? 8 - k : k)];
    }
    if (narrow) {
        const int half = e / 288, k = (e / 32) % 9, ch = half * 32 + e % 32;
        narrow[e] = w[ch * 9 + (flip_wide ? k : 8 - k)];
    }
}

// the sizes of a layer and the layout of its workspace: float64 partials first, then t1, t2 and C (every piece 16-byte aligned)
struct Plan {
    int CI, CO, h, w, tiles, cot_fwd, cot_adj;
    int64_t P, NWT, n_p1, n_p2, n_p3, n_gw;
    int64_t off_p1, off_p2, off_p3, off_gw, off_t1, off_t2, off_C, bytes;
};
inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }
// 0, or the DEQSCI_ERR_* of the sizes
inline int make_plan(int64_t C_in, int64_t C_out, int64_t h, int64_t w, Plan* pl) {
    if (C_in <= 0 || C_out <= 0 || h <= 0 || w <= 0) return DEQSCI_ERR_SHAPE;
    if (!((C_in == 1 && C_out == CMAX) || (C_in == CMAX && C_out == CMAX) || (C_in == CMAX && C_out == 1))) return DEQSCI_ERR_UNSUPPORTED;
    if (h > MAX_PIXELS || w > MAX_PIXELS || h * w > MAX_PIXELS) return DEQSCI_ERR_UNSUPPORTED;
    Plan p;
    p.CI = (int)C_in, p.CO = (int)C_out, p.h = (int)h, p.w = (int)w;
    p.P = h * w;
    p.NWT = C_in * C_out * 9;
    p.tiles = (int)(ceil_div(h, TILE) * ceil_div(w, TILE));
    p.cot_fwd = C_out == 1 ? 1 : 4;                        // output channels per thread of W v ...
    p.cot_adj = C_in == 1 ? 1 : 4;                         // ... and of W^T u
    p.n_p1 = (int64_t)p.tiles * (C_in / p.cot_adj);
    p.n_p2 = (int64_t)p.tiles * (C_out / p.cot_fwd);
    p.n_p3 = ceil_div(C_out * p.P, CHUNK);
    p.n_gw = ceil_div(p.NWT, CHUNK);
    int64_t o = 0;
    p.off_p1 = o, o = pad16(o + p.n_p1 * 8);
    p.off_p2 = o, o = pad16(o + p.n_p2 * 8);
    p.off_p3 = o, o = pad16(o + p.n_p3 * 8);
    p.off_gw = o, o = pad16(o + p.n_gw * 8);
    p.off_t1 = o, o = pad16(o + C_in * p.P * 4);
    p.off_t2 = o, o = pad16(o + C_out * p.P * 4);
    p.off_C = o, o = pad16(o + p.NWT * 4);
    p.bytes = o;
    *pl = p;
    return 0;
}

template <bool TRANSPOSE>
inline void launch_conv(int cot, dim3 grid, hipStream_t st, const float* W, const float* in, const double* in_part, int n_in_part, float eps,
                        float* in_norm_out, double* in_norm_rec, float* out, double* part, int CI, int CO, int h, int w) {
    if (cot == 1)
        hipLaunchKernelGGL((conv_kernel<1, TRANSPOSE>), grid, dim3(TB), 0, st, W, in, in_part, n_in_part, eps, in_norm_out, in_norm_rec, out, part, CI, CO, h, w);
    else
        hipLaunchKernelGGL((conv_kernel<4, TRANSPOSE>), grid, dim3(TB), 0, st, W, in, in_part, n_in_part, eps, in_norm_out, in_norm_rec, out, part, CI, CO, h, w);
}

}  // namespace realsn
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_realsn_workspace_bytes(int64_t C_in, int64_t C_out, int64_t h, int64_t w) {
    realsn::Plan p;
    if (realsn::make_plan(C_in, C_out, h, w, &p)) return 0;
    return (size_t)p.bytes;
}

int deqsci_realsn_power_f32(const float* W, float* u, float* v, float* weight, double* record, int n_iters, float sigma_t, float eps,
                            int64_t C_in, int64_t C_out, int64_t h, int64_t w, void* workspace, deqsci_stream_t stream) {
    if (!W || !u || !v || !weight || !record || !workspace) return DEQSCI_ERR_NULL;
    if (n_iters < 1) return DEQSCI_ERR_SHAPE;
    realsn::Plan p;
    if (int e = realsn::make_plan(C_in, C_out, h, w, &p)) return e;
    if (!aligned16(W) || !aligned16(u) || !aligned16(v) || !aligned16(weight) || !aligned16(workspace) || misaligned(record, 8))
        return DEQSCI_ERR_ALIGN;
    const void* ptr[6] = {W, u, v, weight, record, workspace};
    const int64_t len[6] = {p.NWT * 4, C_out * p.P * 4, C_in * p.P * 4, p.NWT * 4, 3 * 8, p.bytes};
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (overlaps(ptr[a], len[a], ptr[b], len[b])) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* p1 = reinterpret_cast<double*>(ws + p.off_p1);
    double* p2 = reinterpret_cast<double*>(ws + p.off_p2);
    double* p3 = reinterpret_cast<double*>(ws + p.off_p3);
    float* t1 = reinterpret_cast<float*>(ws + p.off_t1);
    float* t2 = reinterpret_cast<float*>(ws + p.off_t2);
    const int64_t NU = C_out * p.P;
    for (int it = 0; it < n_iters; ++it) {
        // S1: t1 = W^T u - the convolution's inputs are u's C_out channels, its outputs t1's C_in
        realsn::launch_conv<true>(p.cot_adj, dim3(p.tiles, p.CI / p.cot_adj), st, W, u, nullptr, 0, eps, nullptr, nullptr, t1, p1, p.CO, p.CI, p.h, p.w);
        if (int e = launch_status()) return e;
        // S2: v = t1 / max(|t1|, eps), t2 = W v
        realsn::launch_conv<false>(p.cot_fwd, dim3(p.tiles, p.CO / p.cot_fwd), st, W, t1, p1, (int)p.n_p1, eps, v, record, t2, p2, p.CI, p.CO, p.h, p.w);
        if (int e = launch_status()) return e;
        // S3: u = t2 / max(|t2|, eps), the chunk sums of u * t2
        hipLaunchKernelGGL(realsn::normalise_kernel, dim3((unsigned)p.n_p3), dim3(TB), 0, st, t2, p2, (int)p.n_p2, eps, u, p3, record + 1, NU, p.n_p3);
        if (int e = launch_status()) return e;
    }
    hipLaunchKernelGGL(realsn::weight_kernel, dim3((unsigned)ceil_div(p.NWT, TB * 4)), dim3(TB), 0, st, W, p3, (int)p.n_p3, sigma_t, weight, record + 2, p.NWT);
    return launch_status();
}

int deqsci_realsn_grad_f32(const float* G, const float* W, const float* u, const float* v, const double* record, float* dW, float sigma_t,
                           int64_t C_in, int64_t C_out, int64_t h, int64_t w, void* workspace, deqsci_stream_t stream) {
    if (!G || !W || !u || !v || !record || !dW || !workspace) return DEQSCI_ERR_NULL;
    realsn::Plan p;
    if (int e = realsn::make_plan(C_in, C_out, h, w, &p)) return e;
    if (!aligned16(G) || !aligned16(W) || !aligned16(u) || !aligned16(v) || !aligned16(dW) || !aligned16(workspace) || misaligned(record, 8))
        return DEQSCI_ERR_ALIGN;
    const void* in[5] = {G, W, u, v, record};
    const int64_t len[5] = {p.NWT * 4, p.NWT * 4, C_out * p.P * 4, C_in * p.P * 4, 3 * 8};
    for (int a = 0; a < 5; ++a)
        if (overlaps(in[a], len[a], dW, p.NWT * 4) || overlaps(in[a], len[a], workspace, p.bytes)) return DEQSCI_ERR_UNSUPPORTED;
    if (overlaps(dW, p.NWT * 4, workspace, p.bytes)) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* gw = reinterpret_cast<double*>(ws + p.off_gw);
    float* C = reinterpret_cast<float*>(ws + p.off_C);
    const int64_t pairs = C_in * C_out;
    hipLaunchKernelGGL(realsn::cgrad_kernel, dim3((unsigned)(p.n_gw + ceil_div(pairs, rows::NW))), dim3(TB), 0, st, G, W, u, v, C, gw, p.CI, p.CO, p.h,
                       p.w, p.NWT, (int)p.n_gw);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(realsn::grad_final_kernel, dim3((unsigned)ceil_div(p.NWT, TB * 4)), dim3(TB), 0, st, G, C, gw, (int)p.n_gw, record, sigma_t, dW, p.NWT);
    return launch_status();
}

int deqsci_realsn_pack_f32(const float* weight, float* pack, float* pack44, float* pack_t, int64_t C_in, int64_t C_out, deqsci_stream_t stream) {
    if (!weight || (!pack && !pack44 && !pack_t)) return DEQSCI_ERR_NULL;
    const bool mid = C_in == realsn::CMAX && C_out == realsn::CMAX;
    const bool edge = (C_in == 1 && C_out == realsn::CMAX) || (C_in == realsn::CMAX && C_out == 1);
    if (!mid && !edge) return DEQSCI_ERR_UNSUPPORTED;
    if (edge && pack44) return DEQSCI_ERR_UNSUPPORTED;      // an edge layer has no F(4x4,3x3) pack
    if (!aligned16(weight) || !aligned16(pack) || !aligned16(pack44) || !aligned16(pack_t)) return DEQSCI_ERR_ALIGN;
    const void* ptr[4] = {weight, pack, pack44, pack_t};
    const int64_t len[4] = {C_in * C_out * 9 * 4, (mid ? realsn::PACK22 : realsn::PACK_EDGE) * 4, realsn::PACK44 * 4,
                            (mid ? realsn::PACK22 : realsn::PACK_EDGE) * 4};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (overlaps(ptr[a], len[a], ptr[b], len[b])) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mid) {
        hipLaunchKernelGGL(realsn::pack64_kernel, dim3(16, 3), dim3(TB), 0, st, weight, pack, pack44, pack_t);
    } else {
        const bool first = C_in == 1;                      // 1 -> 64: the layer's own pack is the wide one, its transpose's the narrow one
        hipLaunchKernelGGL(realsn::pack_edge_kernel, dim3((unsigned)ceil_div(realsn::PACK_EDGE, TB)), dim3(TB), 0, st, weight,
                           first ? pack : pack_t, first ? pack_t : pack, first ? 0 : 1);
    }
    return launch_status();
}

}  // extern "C"
