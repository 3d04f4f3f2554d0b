// The vector epsilon-algorithm (Aitken's delta-squared extrapolation of x, f(x), f(f(x))) on MI355X (gfx950): the arithmetic of one iteration
// of the reference's solvers/new_equilibrium_utils_yaping.py:194-211 (epsilon2) on planar rows x, f_x, f_fx : (bsz, N) fp32.
// dx = f_x - x, df = f_fx - f_x, d2 = df - dx (fp32, formed on the fly, never stored):
//
//   E1 norms_partial_kernel   one workgroup = one (sample, chunk of CHUNK elements): the squares of dx, df, d2 summed in float64 (per thread,
//                             per wave, per workgroup) -> part[sample][chunk][0..2]
//   E2 fold_kernel            one workgroup = one (column, sample): the chunk sums in ONE fixed order -> table[sample][0..2]
//   E3 update_kernel          a = fp32(sum dx^2), b = fp32(sum df^2), c = fp32(sum d2^2) + lam (an fp32 sum), then elementwise in fp32
//                             x_new = f_x + (df * a - dx * b) / c  (products, difference, a true division and the sum rounded one by one:
//                             the library is built with -ffp-contract=off); the squares of x_new - x (an fp32 difference) and of x_new
//                             summed in float64 as in E1 -> part[sample][chunk][0..1]
//   E2 again                  -> table[sample][3..4]
//
// A float64 fma of two converted floats is exact in its product, so it IS product + sum.  Determinism: no atomics, no counters; element e of
// a row always belongs to thread ((e / 4) % TB) of chunk e / CHUNK, whether the row is read as float4 (N a multiple of 4 and 16-byte aligned
// pointers) or element by element, so the sums do not depend on alignment, and nothing depends on the other samples of the batch.
// HBM-streaming: per iteration and sample 28 N bytes (three rows read, then three read and one written).
#include "common.hpp"

namespace deqsci {
namespace epsilon2 {

constexpr int TS = DEQSCI_EPSILON2_TABLE_STRIDE;         // doubles per sample of the table
constexpr int COL_A = 0, COL_B = 1, COL_C = 2, COL_STEP = 3, COL_NEW = 4;
static_assert(COL_NEW + 1 == TS, "table layout");
constexpr int PS = 3;                                    // doubles per (sample, chunk) of the partials: E1 fills three, E3 two
constexpr int PER_THREAD = 2;                            // float4 per thread and row
constexpr int64_t CHUNK = (int64_t)TB * 4 * PER_THREAD;  // 2048 elements per workgroup
constexpr int NW = TB / WAVE;

// elements e .. e + 3 of a row, zeros beyond N (exact in every square summed below)
__device__ __forceinline__ float4 load4(const float* r, int64_t e, int64_t N, bool vec) {
    if (vec && e + 4 <= N) return ld4(r + e);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e < N) v.x = r[e];
    if (e + 1 < N) v.y = r[e + 1];
    if (e + 2 < N) v.z = r[e + 2];
    if (e + 3 < N) v.w = r[e + 3];
    return v;
}
__device__ __forceinline__ void store4(float* r, int64_t e, int64_t N, bool vec, float4 v) {
    if (vec && e + 4 <= N) { st4(r + e, v); return; }
    if (e < N) r[e] = v.x;
    if (e + 1 < N) r[e + 1] = v.y;
    if (e + 2 < N) r[e + 2] = v.z;
    if (e + 3 < N) r[e + 3] = v.w;
}
// zeros in the components beyond N (0 / c is not 0 for every c: what lies past the row must not reach a sum)
__device__ __forceinline__ float4 inside4(float4 v, int64_t e, int64_t N) {
    return make_float4(e < N ? v.x : 0.0f, e + 1 < N ? v.y : 0.0f, e + 2 < N ? v.z : 0.0f, e + 3 < N ? v.w : 0.0f);
}
__device__ __forceinline__ double sq4(float4 a, double acc) {
    acc = fma((double)a.x, (double)a.x, acc);
    acc = fma((double)a.y, (double)a.y, acc);
    acc = fma((double)a.z, (double)a.z, acc);
    return fma((double)a.w, (double)a.w, acc);
}
__device__ __forceinline__ double wave_all_sum(double v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
// K <= PS sums of the workgroup in a fixed order: wave butterflies, then the four wave sums in wave order -> out[0..K-1] (threads 0..K-1)
template <int K>
__device__ __forceinline__ void block_sums_to(const double (&v)[K], double (*wsum)[PS], double* out) {
    static_assert(NW == 4 && K <= PS, "block_sums_to adds exactly four wave sums");
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = wave_all_sum(v[k]);
    __syncthreads();                                      // the previous reader of wsum is done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) wsum[wave][k] = w[k];
    }
    __syncthreads();
    if (tid < K) out[tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
}
__device__ __forceinline__ bool all_vec(int64_t N, const void* a, const void* b, const void* c, const void* d) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(d);
    return (bits & 15u) == 0 && (N & 3) == 0;
}

// ---- E1
__global__ __launch_bounds__(TB) void norms_partial_kernel(const float* __restrict__ x, const float* __restrict__ fx, const float* __restrict__ ffx,
                                                           double* __restrict__ part, int64_t N, int64_t n_chunks) {
    __shared__ double wsum[NW][PS];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float* xr = x + s * N;
    const float* fr = fx + s * N;
    const float* gr = ffx + s * N;
    const bool vec = all_vec(N, x, fx, ffx, nullptr);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = base + ((int64_t)q * TB + tid) * 4;
            const float4 xv = load4(xr, e, N, vec);
            const float4 fv = load4(fr, e, N, vec);
            const float4 dx = fv - xv;
            const float4 df = load4(gr, e, N, vec) - fv;
            v[0] = sq4(dx, v[0]);
            v[1] = sq4(df, v[1]);
            v[2] = sq4(df - dx, v[2]);
        }
        block_sums_to<3>(v, wsum, part + (s * n_chunks + c) * PS);
    }
}

// ---- E2: column blockIdx.x of the partials of sample blockIdx.y -> table[sample][col0 + blockIdx.x]; thread i sums chunks i, i + TB, ...
__global__ __launch_bounds__(TB) void fold_kernel(const double* __restrict__ part, double* __restrict__ table, int64_t n_chunks, int col0) {
    __shared__ double wsum[NW][PS];
    const int k = blockIdx.x;
    const int64_t s = blockIdx.y;
    double v[1] = {0.0};
    for (int64_t c = threadIdx.x; c < n_chunks; c += TB) v[0] += part[(s * n_chunks + c) * PS + k];
    block_sums_to<1>(v, wsum, table + s * TS + col0 + k);
}

// ---- E3
__global__ __launch_bounds__(TB) void update_kernel(const float* __restrict__ x, const float* __restrict__ fx, const float* __restrict__ ffx,
                                                    float* __restrict__ xnew, const double* __restrict__ table, double* __restrict__ part,
                                                    int64_t N, int64_t n_chunks, float lam) {
    __shared__ double wsum[NW][PS];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float a = (float)table[s * TS + COL_A], b = (float)table[s * TS + COL_B];
    const float4 c4 = f4((float)table[s * TS + COL_C] + lam);
    const float* xr = x + s * N;
    const float* fr = fx + s * N;
    const float* gr = ffx + s * N;
    float* nr = xnew + s * N;
    const bool vec = all_vec(N, x, fx, ffx, xnew);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double v[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = base + ((int64_t)q * TB + tid) * 4;
            const float4 xv = load4(xr, e, N, vec);
            const float4 fv = load4(fr, e, N, vec);
            const float4 dx = fv - xv;
            const float4 df = load4(gr, e, N, vec) - fv;
            const float4 xn = inside4(fv + (a * df - b * dx) / c4, e, N);
            store4(nr, e, N, vec, xn);
            v[0] = sq4(xn - xv, v[0]);
            v[1] = sq4(xn, v[1]);
        }
        block_sums_to<2>(v, wsum, part + (s * n_chunks + c) * PS);
    }
}

inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }
// (fold_kernel's threads walk N / CHUNK partials: 2^28 elements are 2^17 of them, 512 per thread)
inline bool sizes_ok(int64_t bsz, int64_t N) { return bsz > 0 && N > 0 && N <= ((int64_t)1 << 28); }
inline bool supported(int64_t bsz) { return bsz <= 65535; }
// [p, p + n) and [q, q + n) floats share an element
inline bool overlaps(const float* p, const float* q, int64_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)n * 4 && b < a + (uintptr_t)n * 4;
}
inline dim3 grid_for(int64_t n_chunks, int64_t bsz) { return dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536), (unsigned)bsz); }

}  // namespace epsilon2
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int64_t deqsci_epsilon2_chunk(void) { return epsilon2::CHUNK; }

size_t deqsci_epsilon2_workspace_bytes(int64_t bsz, int64_t N) {
    if (!epsilon2::sizes_ok(bsz, N) || !epsilon2::supported(bsz)) return 0;
    return (size_t)(bsz * ceil_div(N, epsilon2::CHUNK)) * epsilon2::PS * sizeof(double);
}

int deqsci_epsilon2_norms_f32(const float* x, const float* f_x, const float* f_fx, double* table, void* workspace, int64_t bsz, int64_t N,
                              deqsci_stream_t stream) {
    if (!x || !f_x || !f_fx || !table || !workspace) return DEQSCI_ERR_NULL;
    if (!epsilon2::sizes_ok(bsz, N)) return DEQSCI_ERR_SHAPE;
    if (epsilon2::misaligned4(x) || epsilon2::misaligned4(f_x) || epsilon2::misaligned4(f_fx) || epsilon2::misaligned8(table) ||
        epsilon2::misaligned8(workspace))
        return DEQSCI_ERR_ALIGN;
    if (!epsilon2::supported(bsz)) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, epsilon2::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(epsilon2::norms_partial_kernel, epsilon2::grid_for(n_chunks, bsz), dim3(TB), 0, st, x, f_x, f_fx, part, N, n_chunks);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(epsilon2::fold_kernel, dim3(3, (unsigned)bsz), dim3(TB), 0, st, (const double*)part, table, n_chunks, epsilon2::COL_A);
    return launch_status();
}

int deqsci_epsilon2_update_f32(const float* x, const float* f_x, const float* f_fx, float* x_new, double* table, void* workspace, int64_t bsz,
                               int64_t N, float lam, deqsci_stream_t stream) {
    if (!x || !f_x || !f_fx || !x_new || !table || !workspace) return DEQSCI_ERR_NULL;
    if (!epsilon2::sizes_ok(bsz, N)) return DEQSCI_ERR_SHAPE;
    if (epsilon2::misaligned4(x) || epsilon2::misaligned4(f_x) || epsilon2::misaligned4(f_fx) || epsilon2::misaligned4(x_new) ||
        epsilon2::misaligned8(table) || epsilon2::misaligned8(workspace))
        return DEQSCI_ERR_ALIGN;
    if (!epsilon2::supported(bsz)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t row = bsz * N;
    if (epsilon2::overlaps(x_new, x, row) || epsilon2::overlaps(x_new, f_x, row) || epsilon2::overlaps(x_new, f_fx, row))
        return DEQSCI_ERR_UNSUPPORTED;                         // every workgroup reads its inputs through __restrict__ pointers
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, epsilon2::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(epsilon2::update_kernel, epsilon2::grid_for(n_chunks, bsz), dim3(TB), 0, st, x, f_x, f_fx, x_new, (const double*)table, part,
                       N, n_chunks, lam);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(epsilon2::fold_kernel, dim3(2, (unsigned)bsz), dim3(TB), 0, st, (const double*)part, table, n_chunks, epsilon2::COL_STEP);
    return launch_status();
}

}  // extern "C"
