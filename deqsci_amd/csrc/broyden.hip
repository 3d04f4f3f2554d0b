// Broyden's method for g(x) = f(x) - x = 0 on MI355X (gfx950): the low-rank arithmetic of one step of the reference's
// solvers/broyd_equilibrium_utils.py:170-177 on a planar history U, V : (bsz, L, N) fp32 with contiguous rows (the reference's Us, VTs,
// whose history index is innermost).  dx = the update just taken, dg = gx_new - gx_old (fp32, formed on the fly, never stored):
//
//   B1 dots_partial_kernel    one workgroup = one (sample, chunk of CHUNK elements): a_j = <dx, U_j>, b_j = <V_j, dg>, c_j = <V_j, gx_new>
//                             for j < t and |gx_new|^2, float64 products and sums (per thread, per wave, per workgroup)
//                             -> part[sample][chunk][table slot]
//   B2 dots_final_kernel      one workgroup = one (table slot, sample): the chunk sums in ONE fixed order -> table[sample][slot]
//   B3 rank_one_kernel        vT = -dx + sum_j a_j V_j -> V[slot] (NaN -> 0), w = dx - (sum_j b_j U_j - dg) -> U[slot] (unscaled);
//                             d = <vT, dg> and c_new = <vT, gx_new> from vT before its NaNs are zeroed, float64 -> part
//   B4 apply_kernel           every workgroup sums its sample's (d, c_new) in one fixed order; U[slot] = w / d (a true fp32 division,
//                             NaN -> 0, infinities stay), update = gx_new - sum_j c_j U_j over the rows j < min(nstep, L) in ascending j,
//                             the new row in its place with c_new - a row it replaces (wrap) does not contribute -, x_next = x + update
//
// The coefficients are rounded to fp32 once; the combinations are summed in fp32 in ascending j (products and sums rounded separately:
// the library is built with -ffp-contract=off).  A float64 fma of two converted floats is exact in its product, so it IS product + sum.
// Determinism: the two-stage order of csrc/rows.hpp (rows are read as float4 where N is a multiple of 4 and the pointers are 16-byte
// aligned, else element by element: the same sums); nothing depends on the other samples of the batch.  HBM-streaming: per step and sample 4 N (5 t + 13) bytes.
#include "rows.hpp"

namespace deqsci {
namespace broyden {

using namespace rows;

constexpr int MAXL = DEQSCI_BROYDEN_MAX_L;
constexpr int TS = DEQSCI_BROYDEN_TABLE_STRIDE;          // doubles per sample of the table, and per (sample, chunk) of the partials
constexpr int SLOT_A = 0, SLOT_B = MAXL, SLOT_C = 2 * MAXL, SLOT_GG = 3 * MAXL, SLOT_D = 3 * MAXL + 1, SLOT_CN = 3 * MAXL + 2;
static_assert(SLOT_CN + 1 == TS, "table layout");
constexpr int PER_THREAD = 2;                            // float4 per thread and row
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                      // 2048 elements per workgroup

// every row of a (bsz, L, N) history starts 16-byte aligned iff the base does and N is a multiple of 4
template <typename... P>
__device__ __forceinline__ bool all_vec(int64_t N, const P*... p) { return aligned16_all(p...) && (N & 3) == 0; }

// ---- B1
__global__ __launch_bounds__(TB) void dots_partial_kernel(const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ dx,
                                                          const float* __restrict__ g0, const float* __restrict__ g1, double* __restrict__ part,
                                                          int64_t N, int64_t n_chunks, int L, int t) {
    __shared__ double wsum[NW][TS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t s = blockIdx.y;
    const float* Us = U + s * L * N;
    const float* Vs = V + s * L * N;
    const float* dxr = dx + s * N;
    const float* g0r = g0 + s * N;
    const float* g1r = g1 + s * N;
    const bool vec = all_vec(N, U, V, dx, g0, g1);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        float4 xv[PER_THREAD], dg[PER_THREAD], gn[PER_THREAD];
        double gg = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            xv[q] = load4(dxr, e, N, vec);
            gn[q] = load4(g1r, e, N, vec);
            dg[q] = gn[q] - load4(g0r, e, N, vec);
            gg = dot4(gn[q], gn[q], gg);
        }
        for (int j = 0; j < t; ++j) {
            const float* Uj = Us + (int64_t)j * N;
            const float* Vj = Vs + (int64_t)j * N;
            float4 u[PER_THREAD], v[PER_THREAD];
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                const int64_t e = Ch::elem(base, q, tid);
                u[q] = load4(Uj, e, N, vec);
                v[q] = load4(Vj, e, N, vec);
            }
            double a = 0.0, b = 0.0, cc = 0.0;
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                a = dot4(xv[q], u[q], a);
                b = dot4(v[q], dg[q], b);
                cc = dot4(v[q], gn[q], cc);
            }
            a = wave_all_sum(a);
            b = wave_all_sum(b);
            cc = wave_all_sum(cc);
            if (lane == 0) {
                wsum[wave][SLOT_A + j] = a;
                wsum[wave][SLOT_B + j] = b;
                wsum[wave][SLOT_C + j] = cc;
            }
        }
        gg = wave_all_sum(gg);
        if (lane == 0) wsum[wave][SLOT_GG] = gg;
        __syncthreads();
        if (tid <= SLOT_GG && (tid == SLOT_GG || tid % MAXL < t))
            part[(s * n_chunks + c) * TS + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
        __syncthreads();                                  // wsum is rewritten by the next chunk
    }
}

// ---- B2: blockIdx.x < 3 t: kind blockIdx.x / t (a, b, c) of row blockIdx.x % t; blockIdx.x == 3 t: |gx_new|^2
__global__ __launch_bounds__(TB) void dots_final_kernel(const double* __restrict__ part, double* __restrict__ table, int64_t n_chunks, int t) {
    __shared__ double wsum[NW];
    const int k = blockIdx.x;
    const int slot = k < 3 * t ? (k / t) * MAXL + k % t : SLOT_GG;
    const int64_t s = blockIdx.y;
    double v = 0.0;
    for (int64_t c = threadIdx.x; c < n_chunks; c += TB) v += part[(s * n_chunks + c) * TS + slot];
    v = block_sum(v, wsum);
    if (threadIdx.x == 0) table[s * TS + slot] = v;
}

// ---- B3 (U and V are read and written: row `slot` may be one of the t rows read, every element by the thread that rewrites it)
__global__ __launch_bounds__(TB) void rank_one_kernel(float* U, float* V, const float* __restrict__ dx, const float* __restrict__ g0,
                                                      const float* __restrict__ g1, const double* __restrict__ table, double* __restrict__ part,
                                                      int64_t N, int64_t n_chunks, int L, int t, int slot) {
    __shared__ float af[MAXL], bf[MAXL];
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    if (tid < t) {
        af[tid] = (float)table[s * TS + SLOT_A + tid];
        bf[tid] = (float)table[s * TS + SLOT_B + tid];
    }
    __syncthreads();
    float* Us = U + s * L * N;
    float* Vs = V + s * L * N;
    const float* dxr = dx + s * N;
    const float* g0r = g0 + s * N;
    const float* g1r = g1 + s * N;
    const bool vec = all_vec(N, U, V, dx, g0, g1);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        float4 accv[PER_THREAD], accu[PER_THREAD];
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) accv[q] = accu[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int j = 0; j < t; ++j) {
            const float a = af[j], b = bf[j];
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                const int64_t e = Ch::elem(base, q, tid);
                accv[q] = accv[q] + a * load4(Vs + (int64_t)j * N, e, N, vec);
                accu[q] = accu[q] + b * load4(Us + (int64_t)j * N, e, N, vec);
            }
        }
        double d = 0.0, cn = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            const float4 xv = load4(dxr, e, N, vec);
            const float4 gn = load4(g1r, e, N, vec);
            const float4 dg = gn - load4(g0r, e, N, vec);
            const float4 vT = accv[q] - xv;               // -dx + sum_j a_j V_j
            const float4 w = xv - (accu[q] - dg);         // dx - (-dg + sum_j b_j U_j)
            d = dot4(vT, dg, d);
            cn = dot4(vT, gn, cn);
            store4(Vs + (int64_t)slot * N, e, N, vec, nan_to_zero(vT));
            store4(Us + (int64_t)slot * N, e, N, vec, w);
        }
        d = block_sum(d, wsum);
        cn = block_sum(cn, wsum);
        if (tid == 0) {
            part[(s * n_chunks + c) * TS + SLOT_D] = d;
            part[(s * n_chunks + c) * TS + SLOT_CN] = cn;
        }
    }
}

// ---- B4 (x_next may be x, update may be gx_new: every element is read and written by the same thread)
__global__ __launch_bounds__(TB) void apply_kernel(float* U, const float* g1, const float* x, float* x_next, float* update,
                                                   double* __restrict__ table, const double* __restrict__ part, int64_t N, int64_t n_chunks,
                                                   int L, int t, int slot) {
    __shared__ float cf[MAXL];
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    // the sample's (d, c_new), thread i summing chunks i, i + TB, ... in order: the same order in every workgroup of the sample
    double d = 0.0, cn = 0.0;
    for (int64_t c = tid; c < n_chunks; c += TB) {
        d += part[(s * n_chunks + c) * TS + SLOT_D];
        cn += part[(s * n_chunks + c) * TS + SLOT_CN];
    }
    d = block_sum(d, wsum);
    cn = block_sum(cn, wsum);
    if (blockIdx.x == 0 && tid == 0) {
        table[s * TS + SLOT_D] = d;
        table[s * TS + SLOT_CN] = cn;
    }
    const float d32 = (float)d;
    const int rows = t > slot + 1 ? t : slot + 1;         // min(nstep, L): the t old rows and the new one
    if (tid < rows) cf[tid] = tid == slot ? (float)cn : (float)table[s * TS + SLOT_C + tid];
    __syncthreads();
    float* Us = U + s * L * N;
    const float* g1r = g1 + s * N;
    const float* xr = x ? x + s * N : nullptr;
    float* xn = x_next ? x_next + s * N : nullptr;
    float* up = update + s * N;
    const bool vec = all_vec(N, U, g1, x, x_next, update);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        float4 u[PER_THREAD], acc[PER_THREAD];
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = base + ((int64_t)q * TB + tid) * 4;   // Ch::elem, spelled out
            u[q] = nan_to_zero(load4(Us + (int64_t)slot * N, e, N, vec) / f4(d32));
            store4(Us + (int64_t)slot * N, e, N, vec, u[q]);
            acc[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        for (int j = 0; j < rows; ++j) {
            const float cj = cf[j];
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                const int64_t e = base + ((int64_t)q * TB + tid) * 4;   // Ch::elem, spelled out
                acc[q] = acc[q] + cj * (j == slot ? u[q] : load4(Us + (int64_t)j * N, e, N, vec));
            }
        }
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = base + ((int64_t)q * TB + tid) * 4;   // Ch::elem, spelled out
            const float4 upd = load4(g1r, e, N, vec) - acc[q];
            if (xn) store4(xn, e, N, vec, load4(xr, e, N, vec) + upd);
            store4(up, e, N, vec, upd);
        }
    }
}

inline bool sizes_ok(int64_t bsz, int64_t N, int L) { return bsz > 0 && N > 0 && L >= 1 && L <= MAXL; }
// (every workgroup of apply_kernel sums its sample's N / CHUNK partial pairs again: 2^28 elements are 2^17 of them, 512 per thread)
inline bool supported(int64_t bsz, int64_t N) { return bsz <= 65535 && N <= ((int64_t)1 << 28); }

}  // namespace broyden
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int64_t deqsci_broyden_chunk(void) { return broyden::CHUNK; }

size_t deqsci_broyden_workspace_bytes(int64_t bsz, int64_t N, int L) {
    if (!broyden::sizes_ok(bsz, N, L) || !broyden::supported(bsz, N)) return 0;
    return (size_t)(bsz * ceil_div(N, broyden::CHUNK)) * broyden::TS * sizeof(double);
}

int deqsci_broyden_dots_f32(const float* U, const float* V, const float* dx, const float* gx_old, const float* gx_new, double* table,
                            void* workspace, int64_t bsz, int64_t N, int L, int t, deqsci_stream_t stream) {
    if (!U || !V || !dx || !gx_old || !gx_new || !table || !workspace) return DEQSCI_ERR_NULL;
    if (!broyden::sizes_ok(bsz, N, L) || t < 0 || t > L) return DEQSCI_ERR_SHAPE;
    if (misaligned(U, 4) || misaligned(V, 4) || misaligned(dx, 4) || misaligned(gx_old, 4) ||
        misaligned(gx_new, 4) || misaligned(table, 8) || misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    if (!broyden::supported(bsz, N)) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, broyden::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(broyden::dots_partial_kernel, rows::chunk_grid(n_chunks, bsz), dim3(TB), 0, st, U, V, dx, gx_old, gx_new, part, N,
                       n_chunks, L, t);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(broyden::dots_final_kernel, dim3((unsigned)(3 * t + 1), (unsigned)bsz), dim3(TB), 0, st, (const double*)part, table,
                       n_chunks, t);
    return launch_status();
}

int deqsci_broyden_update_f32(float* U, float* V, const float* dx, const float* gx_old, const float* gx_new, const float* x, float* x_next,
                              float* update, double* table, void* workspace, int64_t bsz, int64_t N, int L, int t, int slot,
                              deqsci_stream_t stream) {
    if (!U || !V || !dx || !gx_old || !gx_new || !update || !table || !workspace || (x_next && !x)) return DEQSCI_ERR_NULL;
    if (!broyden::sizes_ok(bsz, N, L) || t < 0 || t > L || slot < 0 || slot >= L || slot > t || (slot < t && t < L))
        return DEQSCI_ERR_SHAPE;                               // slot == t (the history fills) or slot < t == L (it wraps)
    if (misaligned(U, 4) || misaligned(V, 4) || misaligned(dx, 4) || misaligned(gx_old, 4) ||
        misaligned(gx_new, 4) || misaligned(x, 4) || misaligned(x_next, 4) || misaligned(update, 4) ||
        misaligned(table, 8) || misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    if (!broyden::supported(bsz, N)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t hist = bsz * L * N * 4, row = bsz * N * 4;    // bytes
    const float* rows[] = {update, x_next, dx, gx_old, gx_new, x};      // none of them may be (part of) a history row
    for (const float* r : rows)
        if (overlaps(r, row, U, hist) || overlaps(r, row, V, hist)) return DEQSCI_ERR_UNSUPPORTED;
    if (overlaps(U, hist, V, hist) || overlaps(update, row, x_next, row)) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, broyden::CHUNK);
    double* part = static_cast<double*>(workspace);
    const dim3 grid = rows::chunk_grid(n_chunks, bsz);
    hipLaunchKernelGGL(broyden::rank_one_kernel, grid, dim3(TB), 0, st, U, V, dx, gx_old, gx_new, (const double*)table, part, N, n_chunks, L, t,
                       slot);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(broyden::apply_kernel, grid, dim3(TB), 0, st, U, gx_new, x, x_next, update, table, (const double*)part, N, n_chunks, L, t,
                       slot);
    return launch_status();
}

}  // extern "C"
