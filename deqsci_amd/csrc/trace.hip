// Per-sample squared error of an iterate against the ground truth for MI355X (gfx950): the numerator of the per-iteration PSNR trace
// (DEQSCIEngine.reconstruct(trace=True, gt=...)), one launch pair behind every f-call, no host traffic.
//
//   Q1 sqerr_chunk_kernel   one workgroup = one (sample, chunk of CHUNK elements): d = clamp(x) - gt and d * d in fp32 (harness.psnr's
//                           arithmetic), summed in fp64 per thread, per wave, per workgroup -> part[sample][chunk]
//   Q2 sqerr_reduce_kernel  one wave per sample: its chunk sums in a fixed order -> out[sample]
//
// x is a row of the Anderson history, F_hist[:, slot]: rows x_stride elements apart (m * N there); gt rows are dense (N apart).
// Determinism: no atomics; element e of a row always belongs to thread ((e / 4) % TB) of chunk e / CHUNK, whether the row is read as
// float4 (both row bases 16-byte aligned) or element by element (any other row; the tail of N % 4 != 0), so the summation order does
// not depend on the alignment.  A NaN reaches the sum of its own sample only (the clamp is written with comparisons, which keep NaN).
// HBM-streaming: 8 bytes per element, read once.
#include "common.hpp"

namespace deqsci {
namespace sqerr {

constexpr int PER_THREAD = 4;                          // float4 loads per thread
constexpr int64_t CHUNK = (int64_t)TB * 4 * PER_THREAD;  // 4096 elements per workgroup

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN stays NaN

__device__ __forceinline__ double term(float xv, float gv, int clamp_x) {
    if (clamp_x) xv = clamp01(xv);
    const float d = xv - gv;
    return (double)(d * d);
}

__global__ __launch_bounds__(TB) void sqerr_chunk_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                         double* __restrict__ part, int64_t N, int64_t x_stride, int clamp_x,
                                                         int64_t n_chunks) {
    __shared__ double wsum[TB / WAVE];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float* xr = x + s * x_stride;
    const float* gr = gt + s * N;
    const bool vec = ((reinterpret_cast<uintptr_t>(xr) | reinterpret_cast<uintptr_t>(gr)) & 15u) == 0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) {
            const int64_t e = base + ((int64_t)j * TB + tid) * 4;
            if (vec && e + 4 <= N) {
                const float4 a = ld4(xr + e), b = ld4(gr + e);
                acc += term(a.x, b.x, clamp_x);
                acc += term(a.y, b.y, clamp_x);
                acc += term(a.z, b.z, clamp_x);
                acc += term(a.w, b.w, clamp_x);
            } else {
                for (int q = 0; q < 4; ++q)
                    if (e + q < N) acc += term(xr[e + q], gr[e + q], clamp_x);
            }
        }
        // workgroup sum in a fixed order: wave butterfly, then the four wave sums in wave order
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
        __syncthreads();                                   // the previous chunk's reader of wsum is done
        if ((tid & (WAVE - 1)) == 0) wsum[tid / WAVE] = acc;
        __syncthreads();
        if (tid == 0) part[s * n_chunks + c] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// one wave per sample: lane l sums chunks l, l + 64, ... in order, then a fixed xor butterfly
__global__ __launch_bounds__(TB) void sqerr_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int64_t bsz,
                                                          int64_t n_chunks) {
    const int lane = threadIdx.x & (WAVE - 1);
    for (int64_t i = (int64_t)blockIdx.x * (TB / WAVE) + threadIdx.x / WAVE; i < bsz; i += (int64_t)gridDim.x * (TB / WAVE)) {
        const double* p = part + i * n_chunks;
        double s = 0.0;
        for (int64_t t = lane; t < n_chunks; t += WAVE) s += p[t];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
        if (lane == 0) out[i] = s;
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
    if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(gt) & 3u) || (reinterpret_cast<uintptr_t>(out) & 7u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, sqerr::CHUNK);
    double* part = static_cast<double*>(workspace);
    const dim3 grid((unsigned)(n_chunks < 65536 ? n_chunks : 65536), (unsigned)bsz);
    hipLaunchKernelGGL(sqerr::sqerr_chunk_kernel, grid, dim3(TB), 0, st, x, gt, part, N, x_stride, clamp_x, n_chunks);
    if (int e = launch_status()) return e;
    const int64_t nb = ceil_div(bsz, TB / WAVE);
    hipLaunchKernelGGL(sqerr::sqerr_reduce_kernel, dim3((unsigned)nb), dim3(TB), 0, st, part, out, bsz, n_chunks);
    return launch_status();
}

}  // extern "C"
