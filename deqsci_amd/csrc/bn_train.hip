// BatchNorm2d in train mode behind a 64 -> 64 convolution: the batch statistics, the normalisation and their backward, on the fp32
// channels_last activation (P, 64), P = n H W pixels - the layout the Winograd, masked and wgrad kernels read and write.  The reference
// trains FFDNet with its 13 BatchNorm2d layers in train mode (it only calls .eval() under --inference), so every f-call of a training
// step normalises by the batch, differentiates through the statistics and moves the running buffers.
//
// One layout for every kernel: a workgroup owns a fixed run of `chunk` pixels (bn_train::split), a quarter-wave (16 lanes x float4) reads
// one pixel's 64 channels as 256 contiguous bytes, a thread keeps float64 accumulators for its 4 channels over the pixels
// base + q + 16 k (q its quarter-wave of the workgroup's 16), the 16 quarter-waves are folded through LDS in ascending q, and the
// workgroup writes one double[64] (T3: [128]) partial.  A closing launch (one wave per channel) sums the partials: lane j its contiguous
// run of workgroups in ascending order, then the wave's tree.  No atomics, nothing waits: bit-equal run to run.
//
//   T1 stats       sum c -> mean;  sum (c - mean)^2 -> the BIASED variance (a second, centred pass: the variance keeps its digits under any
//                  offset of the data, which E[c^2] - mean^2 does not);  record = mean[64], var[64] in float64.  The closing launch applies
//                  torch's update in float64, rounded once: running_mean <- (1 - m) running_mean + m mean,
//                  running_var <- (1 - m) running_var + m var P / (P - 1), num_batches_tracked += 1.  4 launches.
//   T2 apply       inv = 1 / sqrt(var + eps), a = gamma inv (float64);  y = (float) fma(a, (double)c - mean, (double)beta), then the ReLU
//                  (relu_nan: a NaN stays one); optionally V0's mask word per pixel, bit ch = (y > 0), in the same pass.  1 launch.
//   T3 grad stats  dbeta = sum gy,  dgamma = inv sum gy ((double)c - mean): float64 products and sums;  grad_record = dbeta[64], dgamma[64]
//                  in float64, also rounded to the fp32 outputs.  2 launches.
//   T4 grad apply  k1 = dbeta / P, k2 = dgamma inv / P, a = gamma inv (float64);
//                  dc = (float)(a (((double)gy - k1) - ((double)c - mean) k2)).  1 launch.
#include "common.hpp"

namespace deqsci {
namespace bn_train {

constexpr int QW = 16;                                   // lanes of a quarter-wave: one pixel's 64 channels as 16 float4
constexpr int PIX = TB / QW;                             // pixels a workgroup reads per step
constexpr int64_t MIN_CHUNK = DEQSCI_BN_TRAIN_CHUNK;     // pixels per workgroup, at least
constexpr int64_t MAX_WG = DEQSCI_BN_TRAIN_MAX_WG;
constexpr int STRIDE = 128;                              // doubles per workgroup partial
constexpr int64_t MAX_P = (int64_t)1 << 31;

struct Split {
    int64_t chunk, wgs;
};
// chunk: a multiple of 16 pixels, MIN_CHUNK until that would take more than MAX_WG workgroups
inline Split split(int64_t P) {
    Split s;
    s.chunk = MIN_CHUNK;
    if (ceil_div(P, s.chunk) > MAX_WG) s.chunk = ceil_div(ceil_div(P, MAX_WG), PIX) * PIX;
    s.wgs = ceil_div(P, s.chunk);
    return s;
}
inline bool size_ok(int64_t P) { return P >= 2 && P < MAX_P; }

struct Thread {
    int q, l;
    int64_t p0, p1;                                      // this thread's pixels: p0, p0 + 16, ... < p1
};
__device__ __forceinline__ Thread whoami(int64_t P, int64_t chunk) {
    Thread t;
    t.q = (int)threadIdx.x / QW;
    t.l = (int)threadIdx.x & (QW - 1);
    const int64_t base = (int64_t)blockIdx.x * chunk;
    t.p1 = base + chunk < P ? base + chunk : P;
    t.p0 = base + t.q;
    return t;
}

// the 16 quarter-waves' accumulators -> entry [ch] of the workgroup's partial, summed in ascending q
__device__ __forceinline__ void fold(double (*red)[64], const double s[4], const Thread& t, double* out) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) red[t.q][4 * t.l + j] = s[j];
    __syncthreads();
    if (threadIdx.x < 64) {
        double d = red[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < PIX; ++q) d += red[q][threadIdx.x];
        out[threadIdx.x] = d;
    }
}

// sum over the workgroups of entry e of their partials: lane j its run of workgroups in ascending order, then the wave's tree (lane 0)
__device__ __forceinline__ double partial_sum(const double* part, int wgs, int e) {
    const int lane = (int)threadIdx.x, per = (wgs + WAVE - 1) / WAVE;
    const int b0 = lane * per, b1 = b0 + per < wgs ? b0 + per : wgs;
    double d = 0.0;
    for (int b = b0; b < b1; ++b) d += part[(int64_t)b * STRIDE + e];
    return wave_sum(d);
}

// CENTRED = false: sum c;  true: sum (c - mean)^2
template <bool CENTRED>
__global__ __launch_bounds__(TB) void stats_kernel(const float* __restrict__ c, const double* __restrict__ record, double* __restrict__ part,
                                                   int64_t P, int64_t chunk) {
    __shared__ double red[PIX][64];
    const Thread t = whoami(P, chunk);
    double m[4] = {0.0, 0.0, 0.0, 0.0}, s[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (CENTRED) {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = record[4 * t.l + j];
    }
#pragma unroll 4
    for (int64_t p = t.p0; p < t.p1; p += PIX) {
        const float4 v = ld4(c + p * 64 + 4 * t.l);
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (CENTRED) {
                const double d = (double)x[j] - m[j];
                s[j] += d * d;
            } else {
                s[j] += (double)x[j];
            }
        }
    }
    fold(red, s, t, part + (int64_t)blockIdx.x * STRIDE);
}

// one wave per channel: record[ch] = sum / P
__global__ __launch_bounds__(WAVE) void mean_kernel(const double* __restrict__ part, int wgs, double* __restrict__ record, int64_t P) {
    const int ch = (int)blockIdx.x;
    const double sum = partial_sum(part, wgs, ch);
    if (threadIdx.x == 0) record[ch] = sum / (double)P;
}

// one wave per channel: record[64 + ch] = the biased variance, and torch's update of the buffers
__global__ __launch_bounds__(WAVE) void var_kernel(const double* __restrict__ part, int wgs, double* __restrict__ record, float* running_mean,
                                                   float* running_var, int64_t* num_batches_tracked, double momentum, int64_t P) {
    const int ch = (int)blockIdx.x;
    const double m2 = partial_sum(part, wgs, ch);
    if (threadIdx.x != 0) return;
    const double var = m2 / (double)P;
    record[64 + ch] = var;
    if (running_mean) {
        running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * record[ch]);
        running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * (var * (double)P / (double)(P - 1)));
        if (ch == 0) *num_batches_tracked += 1;
    }
}

template <bool RELU, bool MASK>
__global__ __launch_bounds__(TB) void apply_kernel(const float* c, const double* __restrict__ record, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, double eps, float* y, uint64_t* __restrict__ mask, int64_t P,
                                                   int64_t chunk) {
    const Thread t = whoami(P, chunk);
    double m[4], a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ch = 4 * t.l + j;
        m[j] = record[ch];
        a[j] = (double)gamma[ch] * (1.0 / sqrt(record[64 + ch] + eps));
        b[j] = (double)beta[ch];
    }
    for (int64_t p = t.p0; p < t.p1; p += PIX) {
        const float4 v = ld4(c + p * 64 + 4 * t.l);
        const float x[4] = {v.x, v.y, v.z, v.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = (float)fma(a[j], (double)x[j] - m[j], b[j]);
            if (RELU) o[j] = relu_nan(o[j]);
        }
        st4(y + p * 64 + 4 * t.l, make_float4(o[0], o[1], o[2], o[3]));
        if constexpr (MASK) {
            // bit ch = (y > 0): this lane's four bits at 4 l, ORed over the quarter-wave's 16 lanes (every lane of the wave is here: p0 < p1
            // holds or fails for a whole quarter-wave, and the xor partners stay inside it)
            uint64_t w = (uint64_t)((o[0] > 0.0f ? 1u : 0u) | (o[1] > 0.0f ? 2u : 0u) | (o[2] > 0.0f ? 4u : 0u) | (o[3] > 0.0f ? 8u : 0u)) << (4 * t.l);
#pragma unroll
            for (int s = 1; s < QW; s <<= 1) w |= (uint64_t)__shfl_xor((unsigned long long)w, s, QW);
            if (t.l == 0) mask[p] = w;
        }
    }
}

__global__ __launch_bounds__(TB) void grad_stats_kernel(const float* __restrict__ gy, const float* __restrict__ c, const double* __restrict__ record,
                                                        double* __restrict__ part, int64_t P, int64_t chunk) {
    __shared__ double red[PIX][64];
    const Thread t = whoami(P, chunk);
    double m[4], sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = record[4 * t.l + j];
#pragma unroll 4
    for (int64_t p = t.p0; p < t.p1; p += PIX) {
        const float4 gv = ld4(gy + p * 64 + 4 * t.l), cv = ld4(c + p * 64 + 4 * t.l);
        const float g[4] = {gv.x, gv.y, gv.z, gv.w}, x[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sb[j] += (double)g[j];
            sg[j] += (double)g[j] * ((double)x[j] - m[j]);
        }
    }
    double* mine = part + (int64_t)blockIdx.x * STRIDE;
    fold(red, sb, t, mine);
    fold(red, sg, t, mine + 64);
}

// one wave per channel: grad_record = dbeta[64], dgamma[64], and their fp32 roundings
__global__ __launch_bounds__(WAVE) void grad_sum_kernel(const double* __restrict__ part, int wgs, const double* __restrict__ record, double eps,
                                                        double* __restrict__ grad_record, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int ch = (int)blockIdx.x;
    const double db = partial_sum(part, wgs, ch), dg = partial_sum(part, wgs, 64 + ch);
    if (threadIdx.x != 0) return;
    const double dgam = (1.0 / sqrt(record[64 + ch] + eps)) * dg;
    grad_record[ch] = db;
    grad_record[64 + ch] = dgam;
    dbeta[ch] = (float)db;
    dgamma[ch] = (float)dgam;
}

__global__ __launch_bounds__(TB) void grad_apply_kernel(const float* gy, const float* __restrict__ c, const double* __restrict__ record,
                                                        const double* __restrict__ grad_record, const float* __restrict__ gamma, double eps,
                                                        float* dc, int64_t P, int64_t chunk) {
    const Thread t = whoami(P, chunk);
    double m[4], a[4], k1[4], k2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ch = 4 * t.l + j;
        const double inv = 1.0 / sqrt(record[64 + ch] + eps);
        m[j] = record[ch];
        a[j] = (double)gamma[ch] * inv;
        k1[j] = grad_record[ch] / (double)P;
        k2[j] = grad_record[64 + ch] * inv / (double)P;
    }
#pragma unroll 4
    for (int64_t p = t.p0; p < t.p1; p += PIX) {
        const float4 gv = ld4(gy + p * 64 + 4 * t.l), cv = ld4(c + p * 64 + 4 * t.l);
        const float g[4] = {gv.x, gv.y, gv.z, gv.w}, x[4] = {cv.x, cv.y, cv.z, cv.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)(a[j] * (((double)g[j] - k1[j]) - ((double)x[j] - m[j]) * k2[j]));
        st4(dc + p * 64 + 4 * t.l, make_float4(o[0], o[1], o[2], o[3]));
    }
}

constexpr int64_t RECORD_BYTES = 128 * (int64_t)sizeof(double), CH_BYTES = 64 * (int64_t)sizeof(float);
inline int64_t act_bytes(int64_t P) { return P * 64 * (int64_t)sizeof(float); }
inline int64_t ws_bytes(int64_t P) { return split(P).wgs * STRIDE * (int64_t)sizeof(double); }
// one of the outs shares a byte with another out or with an in
inline bool clash(const void* const* out, const int64_t* out_bytes, int n_out, const void* const* in, const int64_t* in_bytes, int n_in) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (overlaps(out[o], out_bytes[o], in[i], in_bytes[i])) return true;
        for (int p = o + 1; p < n_out; ++p)
            if (overlaps(out[o], out_bytes[o], out[p], out_bytes[p])) return true;
    }
    return false;
}

}  // namespace bn_train
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_bn_train_workspace_bytes(int64_t P) {
    if (!bn_train::size_ok(P)) return 0;
    return (size_t)bn_train::ws_bytes(P);
}

int deqsci_bn_train_stats_f32(const float* c, double* record, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              double momentum, int64_t P, void* workspace, deqsci_stream_t stream) {
    const int buffers = (running_mean != nullptr) + (running_var != nullptr) + (num_batches_tracked != nullptr);
    if (!c || !record || !workspace || (buffers != 0 && buffers != 3)) return DEQSCI_ERR_NULL;
    if (P == 0) return 0;
    if (!bn_train::size_ok(P)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(c) || misaligned(record, 8) || misaligned(workspace, 8) || misaligned(running_mean, 4) || misaligned(running_var, 4) ||
        misaligned(num_batches_tracked, 8))
        return DEQSCI_ERR_ALIGN;
    const void* in[1] = {c};
    const int64_t in_bytes[1] = {bn_train::act_bytes(P)};
    const void* out[5] = {record, workspace, running_mean, running_var, num_batches_tracked};
    const int64_t out_bytes[5] = {bn_train::RECORD_BYTES, bn_train::ws_bytes(P), bn_train::CH_BYTES, bn_train::CH_BYTES, 8};
    if (bn_train::clash(out, out_bytes, 5, in, in_bytes, 1)) return DEQSCI_ERR_UNSUPPORTED;
    const bn_train::Split sp = bn_train::split(P);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(bn_train::stats_kernel<false>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, c, record, part, P, sp.chunk);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(bn_train::mean_kernel, dim3(64), dim3(WAVE), 0, st, part, (int)sp.wgs, record, P);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(bn_train::stats_kernel<true>, dim3((unsigned)sp.wgs), dim3(TB), 0, st, c, record, part, P, sp.chunk);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(bn_train::var_kernel, dim3(64), dim3(WAVE), 0, st, part, (int)sp.wgs, record, running_mean, running_var,
                       num_batches_tracked, momentum, P);
    return launch_status();
}

int deqsci_bn_train_apply_f32(const float* c, const double* record, const float* gamma, const float* beta, double eps, float* y,
                              uint64_t* mask, int relu, int64_t P, deqsci_stream_t stream) {
    if (!c || !record || !gamma || !beta || !y) return DEQSCI_ERR_NULL;
    if (P == 0) return 0;
    if (!bn_train::size_ok(P)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(c) || !aligned16(y) || misaligned(record, 8) || misaligned(gamma, 4) || misaligned(beta, 4) || misaligned(mask, 8))
        return DEQSCI_ERR_ALIGN;
    if (relu != 0 && relu != 1) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t act = bn_train::act_bytes(P);
    const void* in[4] = {record, gamma, beta, y == c ? nullptr : c};                   // (y may BE c; any other overlap is refused)
    const int64_t in_bytes[4] = {bn_train::RECORD_BYTES, bn_train::CH_BYTES, bn_train::CH_BYTES, act};
    const void* out[2] = {y, mask};
    const int64_t out_bytes[2] = {act, P * 8};
    if (bn_train::clash(out, out_bytes, 2, in, in_bytes, 4) || overlaps(mask, P * 8, c, act)) return DEQSCI_ERR_UNSUPPORTED;
    const bn_train::Split sp = bn_train::split(P);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)sp.wgs), block(TB);
    if (relu && mask)
        hipLaunchKernelGGL((bn_train::apply_kernel<true, true>), grid, block, 0, st, c, record, gamma, beta, eps, y, mask, P, sp.chunk);
    else if (relu)
        hipLaunchKernelGGL((bn_train::apply_kernel<true, false>), grid, block, 0, st, c, record, gamma, beta, eps, y, mask, P, sp.chunk);
    else if (mask)
        hipLaunchKernelGGL((bn_train::apply_kernel<false, true>), grid, block, 0, st, c, record, gamma, beta, eps, y, mask, P, sp.chunk);
    else
        hipLaunchKernelGGL((bn_train::apply_kernel<false, false>), grid, block, 0, st, c, record, gamma, beta, eps, y, mask, P, sp.chunk);
    return launch_status();
}

int deqsci_bn_train_grad_stats_f32(const float* gy, const float* c, const double* record, double eps, double* grad_record, float* dgamma,
                                   float* dbeta, int64_t P, void* workspace, deqsci_stream_t stream) {
    if (!gy || !c || !record || !grad_record || !dgamma || !dbeta || !workspace) return DEQSCI_ERR_NULL;
    if (P == 0) return 0;
    if (!bn_train::size_ok(P)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(gy) || !aligned16(c) || misaligned(record, 8) || misaligned(grad_record, 8) || misaligned(dgamma, 4) || misaligned(dbeta, 4) ||
        misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    const int64_t act = bn_train::act_bytes(P);
    const void* in[3] = {gy, c, record};
    const int64_t in_bytes[3] = {act, act, bn_train::RECORD_BYTES};
    const void* out[4] = {grad_record, dgamma, dbeta, workspace};
    const int64_t out_bytes[4] = {bn_train::RECORD_BYTES, bn_train::CH_BYTES, bn_train::CH_BYTES, bn_train::ws_bytes(P)};
    if (bn_train::clash(out, out_bytes, 4, in, in_bytes, 3)) return DEQSCI_ERR_UNSUPPORTED;
    const bn_train::Split sp = bn_train::split(P);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(bn_train::grad_stats_kernel, dim3((unsigned)sp.wgs), dim3(TB), 0, st, gy, c, record, part, P, sp.chunk);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(bn_train::grad_sum_kernel, dim3(64), dim3(WAVE), 0, st, part, (int)sp.wgs, record, eps, grad_record, dgamma, dbeta);
    return launch_status();
}

int deqsci_bn_train_grad_apply_f32(const float* gy, const float* c, const double* record, const double* grad_record, const float* gamma,
                                   double eps, float* dc, int64_t P, deqsci_stream_t stream) {
    if (!gy || !c || !record || !grad_record || !gamma || !dc) return DEQSCI_ERR_NULL;
    if (P == 0) return 0;
    if (!bn_train::size_ok(P)) return DEQSCI_ERR_SHAPE;
    if (!aligned16(gy) || !aligned16(c) || !aligned16(dc) || misaligned(record, 8) || misaligned(grad_record, 8) || misaligned(gamma, 4))
        return DEQSCI_ERR_ALIGN;
    const int64_t act = bn_train::act_bytes(P);
    const void* in[5] = {c, record, grad_record, gamma, dc == gy ? nullptr : gy};        // (dc may BE gy; any other overlap is refused)
    const int64_t in_bytes[5] = {act, bn_train::RECORD_BYTES, bn_train::RECORD_BYTES, bn_train::CH_BYTES, act};
    const void* out[1] = {dc};
    const int64_t out_bytes[1] = {act};
    if (bn_train::clash(out, out_bytes, 1, in, in_bytes, 5)) return DEQSCI_ERR_UNSUPPORTED;
    const bn_train::Split sp = bn_train::split(P);
    hipLaunchKernelGGL(bn_train::grad_apply_kernel, dim3((unsigned)sp.wgs), dim3(TB), 0, static_cast<hipStream_t>(stream), gy, c, record,
                       grad_record, gamma, eps, dc, P, sp.chunk);
    return launch_status();
}

}  // extern "C"
