// Per-sample squared error of an iterate against the ground truth for MI355X (gfx950): the numerator of the per-iteration PSNR trace
// (DEQSCIEngine.reconstruct(trace=True, gt=...)), one launch pair behind every f-call, no host traffic.
//
//   Q1 sqerr_chunk_kernel   one workgroup = one (sample, chunk of CHUNK elements): d = clamp(x) - gt and d * d in fp32 (harness.psnr's
//                           arithmetic), summed in fp64 per thread, per wave, per workgroup -> part[sample][chunk]
//   Q2 sqerr_reduce_kernel  one wave per sample: its chunk sums in a fixed order -> out[sample]
//
// x is a row of the Anderson history, F_hist[:, slot]: rows x_stride elements apart (m * N there); gt rows are dense (N apart).
// Determinism: the two-stage order of csrc/rows.hpp (a row is read as float4 where both row starts are 16-byte aligned, else element by
// element: the same sums).  A NaN reaches the sum of its own sample only (the clamp is written with comparisons, which keep NaN).
// HBM-streaming: 8 bytes per element, read once.
#include "rows.hpp"

namespace deqsci {
namespace sqerr {

using namespace rows;

constexpr int PER_THREAD = 4;                            // float4 per thread and row
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                      // 4096 elements per workgroup

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN stays NaN
__device__ __forceinline__ float4 clamp01(float4 v) { return make_float4(clamp01(v.x), clamp01(v.y), clamp01(v.z), clamp01(v.w)); }

__global__ __launch_bounds__(TB) void sqerr_chunk_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                         double* __restrict__ part, int64_t N, int64_t x_stride, int clamp_x,
                                                         int64_t n_chunks) {
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float* xr = x + s * x_stride;
    const float* gr = gt + s * N;
    const bool vec = aligned16_all(xr, gr);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            const float4 xv = load4(xr, e, N, vec);
            const float4 d = (clamp_x ? clamp01(xv) : xv) - load4(gr, e, N, vec);
            const float4 sq = d * d;                       // fp32, as harness.psnr's (beyond N: +0.0)
            acc = (((acc + (double)sq.x) + (double)sq.y) + (double)sq.z) + (double)sq.w;
        }
        acc = block_sum(acc, wsum);
        if (tid == 0) part[s * n_chunks + c] = acc;
    }
}

// one wave per sample: its chunk sums by wave_fold -> out[sample]
__global__ __launch_bounds__(TB) void sqerr_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int64_t bsz,
                                                          int64_t n_chunks) {
    for (int64_t i = (int64_t)blockIdx.x * NW + threadIdx.x / WAVE; i < bsz; i += (int64_t)gridDim.x * NW) {
        const double s = wave_fold(part + i * n_chunks, n_chunks);
        if ((threadIdx.x & (WAVE - 1)) == 0) out[i] = s;
    }
}

inline bool sizes_ok(int64_t bsz, int64_t N) {
    // (bsz is the grid's y extent; the element offsets are int64)
    return bsz >= 0 && N >= 0 && bsz <= 65535 && N <= ((int64_t)1 << 40);
}

}  // namespace sqerr
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_sqerr_workspace_bytes(int64_t bsz, int64_t N) {
    if (!sqerr::sizes_ok(bsz, N)) return 0;
    return (size_t)(bsz * ceil_div(N, sqerr::CHUNK)) * sizeof(double);
}

int deqsci_sqerr_rows_f32(const float* x, const float* gt, double* out, int64_t bsz, int64_t N, int64_t x_stride, int clamp_x,
                          void* workspace, deqsci_stream_t stream) {
    if (!sqerr::sizes_ok(bsz, N) || x_stride < N) return DEQSCI_ERR_SHAPE;
    if (bsz == 0 || N == 0) return 0;
    if (!x || !gt || !out || !workspace) return DEQSCI_ERR_NULL;
    if (misaligned(x, 4) || misaligned(gt, 4) || misaligned(out, 8) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, sqerr::CHUNK);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(sqerr::sqerr_chunk_kernel, rows::chunk_grid(n_chunks, bsz), dim3(TB), 0, st, x, gt, part, N, x_stride, clamp_x, n_chunks);
    if (int e = launch_status()) return e;
    const int64_t nb = ceil_div(bsz, TB / WAVE);
    hipLaunchKernelGGL(sqerr::sqerr_reduce_kernel, dim3((unsigned)nb), dim3(TB), 0, st, part, out, bsz, n_chunks);
    return launch_status();
}

}  // extern "C"
