// The training step's glue for MI355X (gfx950): what the reference does around its solve with MSELoss, loss.item(), skimage's PSNR on the
// host and a dozen elementwise launches per parameter tensor (training/sci_equilibrium_training.py:54-81, torch-1.9 F.adam).
//
//   L1a mse_chunk_kernel   one workgroup = one chunk of CHUNK elements of the batch, taken as ONE row of `total` elements: d = rec - gt,
//                          grad = d * s, dc = clamp(rec, 0, 1) - gt, all in fp32; d * d and dc * dc in fp32 (torch's MSELoss and
//                          harness.psnr square in fp32), summed in float64 per thread, per wave, per workgroup together with the
//                          count of non-finite d -> part[chunk][3]
//   L1b mse_reduce_kernel  one workgroup: the chunk partials in csrc/rows.hpp's stage-2 order (thread i adds chunks i, i + TB, ..., then
//                          block_sums_to) -> stats[0..2]
//   L2  adam_kernel        one Adam step of up to DEQSCI_ADAM_MAX_TENSORS tensors in ONE launch: one workgroup = one chunk of one tensor,
//                          found by a binary search over the prefix sums of the per-tensor chunk counts
//
// Determinism: no atomics, no counters.  L1's sums take the two-stage order of csrc/rows.hpp (tests/rows_order.py: sum_workgroup with
// P = PER_THREAD), whether a group is read as a float4 (rec, gt and grad all 16-byte aligned) or element by element; a NaN or Inf in d
// is counted and enters stats[0] as it is (the reference's loss is NaN there too), and the gradient is written all the same.
// L2 is elementwise: a tensor whose four pointers are all 16-byte aligned is walked as float4 with a scalar tail, any other (a view into
// a flat buffer: 4-byte aligned only) element by element - the same arithmetic.
// HBM-streaming: L1 12 bytes per element, L2 28.
#include "rows.hpp"

namespace deqsci {
namespace train {

using namespace rows;

constexpr int PER_THREAD = 4;                            // float4 per thread and chunk
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                      // 4096 elements per workgroup
static_assert(CHUNK == DEQSCI_TRAIN_CHUNK, "include/deqsci_hip.h states the chunk");
constexpr int NSTAT = 3;

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }   // NaN stays NaN
__device__ __forceinline__ float4 clamp01(float4 v) { return make_float4(clamp01(v.x), clamp01(v.y), clamp01(v.z), clamp01(v.w)); }
__device__ __forceinline__ double bad(float v) { return __builtin_isfinite(v) ? 0.0 : 1.0; }
__device__ __forceinline__ double add4(float4 t, double acc) {
    return (((acc + (double)t.x) + (double)t.y) + (double)t.z) + (double)t.w;
}

__global__ __launch_bounds__(TB) void mse_chunk_kernel(const float* __restrict__ rec, const float* __restrict__ gt, float* __restrict__ grad,
                                                       double* __restrict__ part, int64_t total, float s, int64_t n_chunks) {
    __shared__ double wsum[NW][NSTAT];
    const int tid = threadIdx.x;
    const bool vec = aligned16_all(rec, gt, grad);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double acc[NSTAT] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            if (e >= total) continue;                         // (what lies beyond adds +0.0 in the restated order: skipping it gives the same bits)
            const float4 r = load4(rec, e, total, vec), g = load4(gt, e, total, vec);
            const float4 d = r - g, dc = clamp01(r) - g;      // (load4 reads zeros beyond `total`: both are +0.0 there)
            store4(grad, e, total, vec, s * d);
            acc[0] = add4(d * d, acc[0]);
            acc[1] = add4(dc * dc, acc[1]);
            acc[2] = (((acc[2] + bad(d.x)) + bad(d.y)) + bad(d.z)) + bad(d.w);
        }
        block_sums_to(acc, wsum, part + c * NSTAT);
    }
}

__global__ __launch_bounds__(TB) void mse_reduce_kernel(const double* __restrict__ part, double* __restrict__ stats, int64_t n_chunks) {
    __shared__ double wsum[NW][NSTAT];
    double acc[NSTAT] = {0.0, 0.0, 0.0};
    for (int64_t c = threadIdx.x; c < n_chunks; c += TB) {
#pragma unroll
        for (int k = 0; k < NSTAT; ++k) acc[k] += part[c * NSTAT + k];
    }
    block_sums_to(acc, wsum, stats);
}

inline bool total_ok(int64_t total) { return total >= 0 && total <= ((int64_t)1 << 40); }

// ---- L2.  The table travels BY VALUE in the kernel-argument segment: 64 entries x 48 bytes + 65 prefix sums x 4 bytes + the scalars =
// 3360 bytes, within the 4096 bytes HIP allows a kernel's arguments on AMD devices.  Nothing is staged on the device, so rebuilding the
// table every step (gradients are new tensors after zero_grad) costs neither an allocation nor a synchronisation.
struct AdamArgs {
    deqsci_adam_entry t[DEQSCI_ADAM_MAX_TENSORS];
    uint32_t first[DEQSCI_ADAM_MAX_TENSORS + 1];             // first[i] = chunks of the tensors before i; first[n] = the grid
    int n;
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps;
};
static_assert(sizeof(AdamArgs) <= 4096, "the Adam table must fit the kernel-argument segment");

// One element of torch-1.9's F.adam (the reference's optimizer.step()), in fp32, every operation rounded separately (-ffp-contract=off: no
// FMA is formed) and in exactly this order:
//     m = m * beta1 + g * (1 - beta1)              exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
//     v = v * beta2 + (g * g) * (1 - beta2)        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//     den = sqrtf(v) / bc2s + eps                  (exp_avg_sq.sqrt() / math.sqrt(bias_correction2)).add_(eps)
//     p = p - step_size * (m / den)                param.addcdiv_(exp_avg, denom, value=-step_size)
// The division and the square root are the correctly rounded ones: hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, which the
// Makefile leaves on (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt), and fp32 denormals are kept on gfx950.
struct AdamScalars { float b1, omb1, b2, omb2, eps, bc2s, step_size; };
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamScalars& k) {
    m = m * k.b1 + g * k.omb1;
    v = v * k.b2 + (g * g) * k.omb2;
    const float den = sqrtf(v) / k.bc2s + k.eps;
    p = p - k.step_size * (m / den);
}
__device__ __forceinline__ void adam4(float4& p, float4 g, float4& m, float4& v, const AdamScalars& k) {
    adam1(p.x, g.x, m.x, v.x, k);
    adam1(p.y, g.y, m.y, v.y, k);
    adam1(p.z, g.z, m.z, v.z, k);
    adam1(p.w, g.w, m.w, v.w, k);
}

__global__ __launch_bounds__(TB) void adam_kernel(const AdamArgs a) {
    // the tensor of this chunk: the last i with first[i] <= blockIdx.x (wave-uniform: scalar loads from the argument segment)
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= b) lo = mid; else hi = mid;
    }
    const deqsci_adam_entry& t = a.t[lo];
    float* __restrict__ p = t.param;
    const float* __restrict__ g = t.grad;
    float* __restrict__ m = t.exp_avg;
    float* __restrict__ v = t.exp_avg_sq;
    const int64_t N = t.numel, base = (int64_t)(b - a.first[lo]) * CHUNK;
    const AdamScalars k = {a.beta1, a.one_minus_beta1, a.beta2, a.one_minus_beta2, a.eps, t.bc2s, t.step_size};
    const bool vec = aligned16_all(p, g, m, v);
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const int64_t e = Ch::elem(base, q, threadIdx.x);
        if (e >= N) continue;
        if (vec && e + 4 <= N) {
            float4 pv = ld4(p + e), mv = ld4(m + e), vv = ld4(v + e);
            adam4(pv, ld4(g + e), mv, vv, k);
            st4(p + e, pv);
            st4(m + e, mv);
            st4(v + e, vv);
        } else {
            const int64_t end = e + 4 < N ? e + 4 : N;
            for (int64_t i = e; i < end; ++i) {
                float pi = p[i], mi = m[i], vi = v[i];
                adam1(pi, g[i], mi, vi, k);
                p[i] = pi;
                m[i] = mi;
                v[i] = vi;
            }
        }
    }
}

}  // namespace train
}  // namespace deqsci

using namespace deqsci;

extern "C" {

size_t deqsci_mse_workspace_bytes(int64_t total) {
    if (!train::total_ok(total)) return 0;
    return (size_t)(ceil_div(total, train::CHUNK) * train::NSTAT) * sizeof(double);
}

int deqsci_mse_stats_grad_f32(const float* rec, const float* gt, float* grad, double* stats, int64_t total, float scale, void* workspace,
                              deqsci_stream_t stream) {
    if (!train::total_ok(total) || total == 0) return DEQSCI_ERR_SHAPE;
    if (!rec || !gt || !grad || !stats || !workspace) return DEQSCI_ERR_NULL;
    if (misaligned(rec, 4) || misaligned(gt, 4) || misaligned(grad, 4) || misaligned(stats, 8) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    const int64_t bytes = total * 4, n_chunks = ceil_div(total, train::CHUNK);
    if (overlaps(grad, bytes, rec, bytes) || overlaps(grad, bytes, gt, bytes) || overlaps(stats, 24, grad, bytes) ||
        overlaps(workspace, n_chunks * 24, grad, bytes) || overlaps(workspace, n_chunks * 24, stats, 24))
        return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(train::mse_chunk_kernel, rows::chunk_grid(n_chunks, 1), dim3(TB), 0, st, rec, gt, grad, part, total, scale, n_chunks);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(train::mse_reduce_kernel, dim3(1), dim3(TB), 0, st, part, stats, n_chunks);
    return launch_status();
}

int deqsci_adam_step_f32(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2,
                         float one_minus_beta2, float eps, deqsci_stream_t stream) {
    if (n_tensors < 0 || n_tensors > DEQSCI_ADAM_MAX_TENSORS) return DEQSCI_ERR_UNSUPPORTED;
    if (n_tensors == 0) return 0;
    if (!entries) return DEQSCI_ERR_NULL;
    train::AdamArgs a;
    a.n = n_tensors;
    a.beta1 = beta1;
    a.one_minus_beta1 = one_minus_beta1;
    a.beta2 = beta2;
    a.one_minus_beta2 = one_minus_beta2;
    a.eps = eps;
    uint64_t chunks = 0;
    for (int i = 0; i < DEQSCI_ADAM_MAX_TENSORS; ++i) {
        if (i >= n_tensors) {
            a.t[i] = deqsci_adam_entry{nullptr, nullptr, nullptr, nullptr, 0, 1.0f, 0.0f};
            a.first[i + 1] = (uint32_t)chunks;
            continue;
        }
        const deqsci_adam_entry& t = entries[i];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return DEQSCI_ERR_NULL;
        if (t.numel <= 0 || t.numel > ((int64_t)1 << 40)) return DEQSCI_ERR_SHAPE;
        if (misaligned(t.param, 4) || misaligned(t.grad, 4) || misaligned(t.exp_avg, 4) || misaligned(t.exp_avg_sq, 4)) return DEQSCI_ERR_ALIGN;
        const int64_t bytes = t.numel * 4;
        if (overlaps(t.param, bytes, t.grad, bytes) || overlaps(t.param, bytes, t.exp_avg, bytes) || overlaps(t.param, bytes, t.exp_avg_sq, bytes) ||
            overlaps(t.exp_avg, bytes, t.exp_avg_sq, bytes) || overlaps(t.grad, bytes, t.exp_avg, bytes) || overlaps(t.grad, bytes, t.exp_avg_sq, bytes))
            return DEQSCI_ERR_UNSUPPORTED;
        a.t[i] = t;
        a.first[i] = (uint32_t)chunks;
        chunks += (uint64_t)ceil_div(t.numel, train::CHUNK);
        if (chunks >= ((uint64_t)1 << 31)) return DEQSCI_ERR_UNSUPPORTED;      // the grid's x extent
        a.first[i + 1] = (uint32_t)chunks;
    }
    hipLaunchKernelGGL(train::adam_kernel, dim3((unsigned)chunks), dim3(TB), 0, static_cast<hipStream_t>(stream), a);
    return launch_status();
}

}  // extern "C"
