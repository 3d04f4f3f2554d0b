// Float64 sums over planar fp32 rows (bsz, N) in ONE fixed two-stage order, shared by csrc/trace.hip, csrc/jacobian.hip (J2),
// csrc/broyden.hip and csrc/epsilon2.hip (csrc/ssim.hip and csrc/tv.hip take the wave sums).  tests/rows_order.py restates the order in
// numpy and tests/test_rows_order_gpu.py holds the device to it bit for bit.
//
// Stage 1: one workgroup = one (sample, chunk of Chunk<P>::SIZE = TB * 4 * P elements).  Thread tid owns the float4 groups q = 0 .. P-1 at
//          element Chunk<P>::elem(base, q, tid) = base + (q * TB + tid) * 4 and adds its terms to a float64 accumulator in that order,
//          component x, y, z, w (dot4); then the wave's xor butterfly (wave_all_sum) and the four wave sums in wave order (block_sum,
//          block_sums_to) -> one partial per chunk.
// Stage 2: the chunk partials of a sample, either by a workgroup (thread i adds chunks i, i + TB, ... in order, then block_sum) or by one
//          wave (wave_fold: lane l adds chunks l, l + 64, ..., then the butterfly).
//
// Determinism: no atomics, no counters.  Element e of a row always belongs to thread (e / 4) % TB of chunk e / SIZE, whether its group is
// read as a float4 (load4 with vec: the caller's promise that every row start is 16-byte aligned) or element by element, and what lies
// beyond N is read as +0.0, which changes no sum; so a sum depends neither on the alignment nor on the other samples of the batch.
// A float64 fma of two converted floats is exact in its product, so it IS product + sum.
#pragma once
#include "common.hpp"

namespace deqsci {
namespace rows {

constexpr int NW = TB / WAVE;

template <int PER_THREAD>                                 // float4 per thread and row
struct Chunk {
    static constexpr int64_t SIZE = (int64_t)TB * 4 * PER_THREAD;
    static __device__ __forceinline__ int64_t elem(int64_t base, int q, int tid) { return base + ((int64_t)q * TB + tid) * 4; }
};

// elements e .. e + 3 of a row, zeros beyond N (exact in every product and sum built on them)
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
__device__ __forceinline__ double dot4(float4 a, float4 b, double acc) {
    acc = fma((double)a.x, (double)b.x, acc);
    acc = fma((double)a.y, (double)b.y, acc);
    acc = fma((double)a.z, (double)b.z, acc);
    return fma((double)a.w, (double)b.w, acc);
}
__device__ __forceinline__ double sq4(float4 a, double acc) { return dot4(a, a, acc); }
__device__ __forceinline__ float nan_to_zero(float v) { return v != v ? 0.0f : v; }
__device__ __forceinline__ float4 nan_to_zero(float4 v) {
    return make_float4(nan_to_zero(v.x), nan_to_zero(v.y), nan_to_zero(v.z), nan_to_zero(v.w));
}
// every pointer 16-byte aligned (a null pointer is).  Row pointers: those rows may be read as float4.  The bases of (bsz, [L,] N) arrays
// together with N % 4 == 0: every row of them starts 16-byte aligned.
template <typename... P>
__device__ __forceinline__ bool aligned16_all(const P*... p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15u) == 0;
}

__device__ __forceinline__ double wave_all_sum(double v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
// the workgroup's sum in a fixed order: wave butterfly, then the four wave sums in wave order (valid in every thread)
__device__ __forceinline__ double block_sum(double v, double* wsum) {
    static_assert(NW == 4, "block_sum adds exactly four wave sums");
    v = wave_all_sum(v);
    __syncthreads();                                      // the previous reader of wsum is done
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// K <= STRIDE sums of the workgroup in the same order -> out[0..K-1] (written by threads 0..K-1)
template <int K, int STRIDE>
__device__ __forceinline__ void block_sums_to(const double (&v)[K], double (*wsum)[STRIDE], double* out) {
    static_assert(NW == 4 && K <= STRIDE, "block_sums_to adds exactly four wave sums");
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
// one wave's sum of p[0..n): lane l adds p[l], p[l + 64], ... in order, then the butterfly (valid in every lane)
__device__ __forceinline__ double wave_fold(const double* p, int64_t n) {
    double s = 0.0;
    for (int64_t t = threadIdx.x & (WAVE - 1); t < n; t += WAVE) s += p[t];
    return wave_all_sum(s);
}

// stage 1's grid: the chunks of a row along x (a workgroup strides over them beyond 65536), the samples along y
inline dim3 chunk_grid(int64_t n_chunks, int64_t bsz) { return dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536), (unsigned)bsz); }

}  // namespace rows
}  // namespace deqsci
