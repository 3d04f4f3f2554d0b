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
// Determinism: the two-stage order of csrc/rows.hpp (rows are read as float4 where N is a multiple of 4 and the pointers are 16-byte aligned,
// else element by element: the same sums); nothing depends on the other samples of the batch.
// HBM-streaming: per iteration and sample 28 N bytes (three rows read, then three read and one written).
#include "rows.hpp"

namespace deqsci {
namespace epsilon2 {

using namespace rows;

constexpr int TS = DEQSCI_EPSILON2_TABLE_STRIDE;         // doubles per sample of the table
constexpr int COL_A = 0, COL_B = 1, COL_C = 2, COL_STEP = 3, COL_NEW = 4;
static_assert(COL_NEW + 1 == TS, "table layout");
constexpr int PS = 3;                                    // doubles per (sample, chunk) of the partials: E1 fills three, E3 two
constexpr int PER_THREAD = 2;                            // float4 per thread and row
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                      // 2048 elements per workgroup

// every row of a (bsz, N) array starts 16-byte aligned iff the base does and N is a multiple of 4
template <typename... P>
__device__ __forceinline__ bool all_vec(int64_t N, const P*... p) { return aligned16_all(p...) && (N & 3) == 0; }

// ---- E1
__global__ __launch_bounds__(TB) void norms_partial_kernel(const float* __restrict__ x, const float* __restrict__ fx, const float* __restrict__ ffx,
                                                           double* __restrict__ part, int64_t N, int64_t n_chunks) {
    __shared__ double wsum[NW][PS];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float* xr = x + s * N;
    const float* fr = fx + s * N;
    const float* gr = ffx + s * N;
    const bool vec = all_vec(N, x, fx, ffx);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
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
            const int64_t e = Ch::elem(base, q, tid);
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

// (fold_kernel's threads walk N / CHUNK partials: 2^28 elements are 2^17 of them, 512 per thread)
inline bool sizes_ok(int64_t bsz, int64_t N) { return bsz > 0 && N > 0 && N <= ((int64_t)1 << 28); }
inline bool supported(int64_t bsz) { return bsz <= 65535; }

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
    if (misaligned(x, 4) || misaligned(f_x, 4) || misaligned(f_fx, 4) || misaligned(table, 8) ||
        misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    if (!epsilon2::supported(bsz)) return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, epsilon2::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(epsilon2::norms_partial_kernel, rows::chunk_grid(n_chunks, bsz), dim3(TB), 0, st, x, f_x, f_fx, part, N, n_chunks);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(epsilon2::fold_kernel, dim3(3, (unsigned)bsz), dim3(TB), 0, st, (const double*)part, table, n_chunks, epsilon2::COL_A);
    return launch_status();
}

int deqsci_epsilon2_update_f32(const float* x, const float* f_x, const float* f_fx, float* x_new, double* table, void* workspace, int64_t bsz,
                               int64_t N, float lam, deqsci_stream_t stream) {
    if (!x || !f_x || !f_fx || !x_new || !table || !workspace) return DEQSCI_ERR_NULL;
    if (!epsilon2::sizes_ok(bsz, N)) return DEQSCI_ERR_SHAPE;
    if (misaligned(x, 4) || misaligned(f_x, 4) || misaligned(f_fx, 4) || misaligned(x_new, 4) ||
        misaligned(table, 8) || misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    if (!epsilon2::supported(bsz)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t row = bsz * N * 4;                          // bytes
    if (overlaps(x_new, row, x, row) || overlaps(x_new, row, f_x, row) || overlaps(x_new, row, f_fx, row))
        return DEQSCI_ERR_UNSUPPORTED;                         // every workgroup reads its inputs through __restrict__ pointers
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, epsilon2::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(epsilon2::update_kernel, rows::chunk_grid(n_chunks, bsz), dim3(TB), 0, st, x, f_x, f_fx, x_new, (const double*)table, part,
                       N, n_chunks, lam);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(epsilon2::fold_kernel, dim3(2, (unsigned)bsz), dim3(TB), 0, st, (const double*)part, table, n_chunks, epsilon2::COL_STEP);
    return launch_status();
}

}  // extern "C"
