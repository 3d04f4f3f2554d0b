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
//   L2c adam_clip_kernel   the same body's second instantiation: g * coef in place of g, coef = stats[1] of L3 read on the device, and not
//                          a word written where stats[2] > 0 (a non-finite gradient)
//   L3  grad_norm_*        the global norm of a list of gradients: (a) chunk kernel, one workgroup = one chunk of one tensor, found as L2
//                          finds it: squares in float64 (exact) and the non-finite count -> part[chunk][2]; (b) fold kernel, one
//                          workgroup = one tensor: its chunk partials in L1b's order -> tsum[tensor][2]; (c) final kernel, one workgroup:
//                          thread 0 adds the tensors' sums in list order -> stats[0..2], the per-tensor norms behind them.  (a) and (b)
//                          once per table of DEQSCI_ADAM_MAX_TENSORS tensors, (c) once: 2 tables + 1 launches.
//   L3s grad_scale_kernel  g *= coef for a table of tensors; nothing written where stats[2] > 0 or coef == 1
//
// Determinism: no atomics, no counters.  L1's sums take the two-stage order of csrc/rows.hpp (tests/rows_order.py: sum_workgroup with
// P = PER_THREAD), whether a group is read as a float4 (rec, gt and grad all 16-byte aligned) or element by element; a NaN or Inf in d
// is counted and enters stats[0] as it is (the reference's loss is NaN there too), and the gradient is written all the same.
// L2 is elementwise: a tensor whose four pointers are all 16-byte aligned is walked as float4 with a scalar tail, any other (a view into
// a flat buffer: 4-byte aligned only) element by element - the same arithmetic.  L3's sums take the same two-stage order per tensor and
// then the list order, so tests/clip_ref.py restates them on the host bit for bit.
// HBM-streaming: L1 12 bytes per element, L2 and L2c 28, L3 4, L3s 8.
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

// CLIP: L2c.  stats[1] and stats[2] are wave-uniform scalar loads; the early return leaves every tensor as it was.
template <bool CLIP>
__device__ __forceinline__ void adam_body(const AdamArgs& a, const double* __restrict__ stats) {
    float coef = 1.0f;
    if (CLIP) {
        if (stats[2] > 0.0) return;
        coef = (float)stats[1];                               // (exact: L3 stored an fp32's value)
    }
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
            float4 pv = ld4(p + e), mv = ld4(m + e), vv = ld4(v + e), gv = ld4(g + e);
            if (CLIP) gv = coef * gv;
            adam4(pv, gv, mv, vv, k);
            st4(p + e, pv);
            st4(m + e, mv);
            st4(v + e, vv);
        } else {
            const int64_t end = e + 4 < N ? e + 4 : N;
            for (int64_t i = e; i < end; ++i) {
                float pi = p[i], mi = m[i], vi = v[i], gi = g[i];
                if (CLIP) gi = coef * gi;
                adam1(pi, gi, mi, vi, k);
                p[i] = pi;
                m[i] = mi;
                v[i] = vi;
            }
        }
    }
}

__global__ __launch_bounds__(TB) void adam_kernel(const AdamArgs a) { adam_body<false>(a, nullptr); }
__global__ __launch_bounds__(TB) void adam_clip_kernel(const AdamArgs a, const double* __restrict__ stats) { adam_body<true>(a, stats); }
static_assert(sizeof(AdamArgs) + sizeof(double*) <= 4096, "the Adam table and the stats pointer must fit the kernel-argument segment");

// ---- L3, L3s.  The table of gradients travels by value like AdamArgs (64 x 16 bytes + 65 prefix sums).
constexpr int NNORM = 2;                                     // the sum of squares, the count of non-finite elements
struct GradArgs {
    float* g[DEQSCI_ADAM_MAX_TENSORS];
    int64_t numel[DEQSCI_ADAM_MAX_TENSORS];
    uint32_t first[DEQSCI_ADAM_MAX_TENSORS + 1];             // as AdamArgs::first
    int n;
};
static_assert(sizeof(GradArgs) + 3 * sizeof(void*) <= 4096, "the gradient table must fit the kernel-argument segment");

__device__ __forceinline__ int table_find(const uint32_t* first, int n, uint32_t b) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// (a) part: the table's first chunk partial.  A float squared in double is exact (24-bit significands), so sq4's fma IS square + sum.
__global__ __launch_bounds__(TB) void grad_norm_chunk_kernel(const GradArgs a, double* __restrict__ part) {
    __shared__ double wsum[NW][NNORM];
    const uint32_t b = blockIdx.x;
    const int lo = table_find(a.first, a.n, b);
    const float* __restrict__ g = a.g[lo];
    const int64_t N = a.numel[lo], base = (int64_t)(b - a.first[lo]) * CHUNK;
    const bool vec = aligned16_all(g);
    double acc[NNORM] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const int64_t e = Ch::elem(base, q, threadIdx.x);
        if (e >= N) continue;                                 // (what lies beyond adds +0.0 in the restated order: the same bits)
        const float4 t = load4(g, e, N, vec);                 // zeros beyond N: +0.0 to the sum, finite to the count
        acc[0] = sq4(t, acc[0]);
        acc[1] = (((acc[1] + bad(t.x)) + bad(t.y)) + bad(t.z)) + bad(t.w);
    }
    block_sums_to(acc, wsum, part + (int64_t)b * NNORM);
}

// (b) one workgroup = tensor blockIdx.x of the table; part and tsum: the table's first chunk partial and first tensor sum
__global__ __launch_bounds__(TB) void grad_norm_fold_kernel(const GradArgs a, const double* __restrict__ part, double* __restrict__ tsum) {
    __shared__ double wsum[NW][NNORM];
    const int64_t c0 = a.first[blockIdx.x], c1 = a.first[blockIdx.x + 1];
    double acc[NNORM] = {0.0, 0.0};
    for (int64_t c = c0 + threadIdx.x; c < c1; c += TB) {
#pragma unroll
        for (int k = 0; k < NNORM; ++k) acc[k] += part[c * NNORM + k];
    }
    block_sums_to(acc, wsum, tsum + (int64_t)blockIdx.x * NNORM);
}

// (c) one workgroup.  The division and the square root in double are the correctly rounded ones.
__global__ __launch_bounds__(TB) void grad_norm_final_kernel(const double* __restrict__ tsum, int64_t n, double max_norm, double* __restrict__ stats) {
    for (int64_t i = threadIdx.x; i < n; i += TB) stats[3 + i] = sqrt(tsum[i * NNORM]);
    if (threadIdx.x != 0) return;
    double sum = 0.0, count = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        sum += tsum[i * NNORM];
        count += tsum[i * NNORM + 1];
    }
    const double norm = sqrt(sum), c = max_norm / (norm + 1e-6);
    stats[0] = norm;
    stats[1] = (double)(float)(c >= 1.0 ? 1.0 : c);           // one rounding to fp32; a NaN stays NaN
    stats[2] = count;
}

__global__ __launch_bounds__(TB) void grad_scale_kernel(const GradArgs a, const double* __restrict__ stats) {
    if (stats[2] > 0.0) return;
    const float coef = (float)stats[1];
    if (coef == 1.0f) return;                                 // g * 1 is g
    const uint32_t b = blockIdx.x;
    const int lo = table_find(a.first, a.n, b);
    float* __restrict__ g = a.g[lo];
    const int64_t N = a.numel[lo], base = (int64_t)(b - a.first[lo]) * CHUNK;
    const bool vec = aligned16_all(g);
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const int64_t e = Ch::elem(base, q, threadIdx.x);
        if (e >= N) continue;
        store4(g, e, N, vec, coef * load4(g, e, N, vec));
    }
}

// A table of gradients out of entries[0..n): every entry checked (null, shape, alignment), the chunk prefix sums formed.  -> 0 or the error
inline int grad_table(const deqsci_grad_entry* entries, int n, GradArgs& a, uint64_t& chunks) {
    a.n = n;
    chunks = 0;
    for (int i = 0; i < DEQSCI_ADAM_MAX_TENSORS; ++i) {
        if (i >= n) {
            a.g[i] = nullptr;
            a.numel[i] = 0;
            a.first[i + 1] = (uint32_t)chunks;
            continue;
        }
        const deqsci_grad_entry& t = entries[i];
        if (!t.grad) return DEQSCI_ERR_NULL;
        if (t.numel <= 0 || t.numel > ((int64_t)1 << 40)) return DEQSCI_ERR_SHAPE;
        if (misaligned(t.grad, 4)) return DEQSCI_ERR_ALIGN;
        a.g[i] = t.grad;
        a.numel[i] = t.numel;
        a.first[i] = (uint32_t)chunks;
        chunks += (uint64_t)ceil_div(t.numel, CHUNK);
        if (chunks >= ((uint64_t)1 << 31)) return DEQSCI_ERR_UNSUPPORTED;      // the grid's x extent
        a.first[i + 1] = (uint32_t)chunks;
    }
    return 0;
}

// the chunks of all n tensors, or -1 where an entry is invalid or the workspace would pass 2^40 chunks
inline int64_t grad_chunks(const deqsci_grad_entry* entries, int64_t n) {
    if (n < 0 || n > ((int64_t)1 << 24) || (n > 0 && !entries)) return -1;
    int64_t chunks = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (entries[i].numel <= 0 || entries[i].numel > ((int64_t)1 << 40)) return -1;
        chunks += ceil_div(entries[i].numel, CHUNK);
        if (chunks > ((int64_t)1 << 40)) return -1;
    }
    return chunks;
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

static int adam_launch(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                       float eps, const double* stats, bool clip, deqsci_stream_t stream) {
    if (n_tensors < 0 || n_tensors > DEQSCI_ADAM_MAX_TENSORS) return DEQSCI_ERR_UNSUPPORTED;
    if (n_tensors == 0) return 0;
    if (!entries || (clip && !stats)) return DEQSCI_ERR_NULL;
    if (clip && misaligned(stats, 8)) return DEQSCI_ERR_ALIGN;
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
        if (clip && (overlaps(stats, 24, t.param, bytes) || overlaps(stats, 24, t.exp_avg, bytes) || overlaps(stats, 24, t.exp_avg_sq, bytes) ||
                     overlaps(stats, 24, t.grad, bytes)))
            return DEQSCI_ERR_UNSUPPORTED;
        a.t[i] = t;
        a.first[i] = (uint32_t)chunks;
        chunks += (uint64_t)ceil_div(t.numel, train::CHUNK);
        if (chunks >= ((uint64_t)1 << 31)) return DEQSCI_ERR_UNSUPPORTED;      // the grid's x extent
        a.first[i + 1] = (uint32_t)chunks;
    }
    if (clip)
        hipLaunchKernelGGL(train::adam_clip_kernel, dim3((unsigned)chunks), dim3(TB), 0, static_cast<hipStream_t>(stream), a, stats);
    else
        hipLaunchKernelGGL(train::adam_kernel, dim3((unsigned)chunks), dim3(TB), 0, static_cast<hipStream_t>(stream), a);
    return launch_status();
}

int deqsci_adam_step_f32(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2,
                         float one_minus_beta2, float eps, deqsci_stream_t stream) {
    return adam_launch(entries, n_tensors, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, nullptr, false, stream);
}

int deqsci_adam_step_clipped_f32(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2,
                                 float one_minus_beta2, float eps, const double* stats, deqsci_stream_t stream) {
    return adam_launch(entries, n_tensors, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, stats, true, stream);
}

size_t deqsci_grad_norm_workspace_bytes(const deqsci_grad_entry* entries, int64_t n_tensors) {
    const int64_t chunks = train::grad_chunks(entries, n_tensors);
    if (chunks < 0) return 0;
    return (size_t)((chunks + n_tensors) * train::NNORM) * sizeof(double);
}

int deqsci_grad_norm_f32(const deqsci_grad_entry* entries, int64_t n_tensors, double max_norm, double* stats, void* workspace,
                         deqsci_stream_t stream) {
    if (n_tensors < 0 || n_tensors > ((int64_t)1 << 24)) return DEQSCI_ERR_SHAPE;
    if (!stats || (n_tensors > 0 && (!entries || !workspace))) return DEQSCI_ERR_NULL;
    if (!(max_norm >= 0.0)) return DEQSCI_ERR_UNSUPPORTED;
    if (misaligned(stats, 8) || misaligned(workspace, 8)) return DEQSCI_ERR_ALIGN;
    // every table is checked before the first launch
    const int T = DEQSCI_ADAM_MAX_TENSORS;
    train::GradArgs a;
    uint64_t chunks = 0;
    for (int64_t lo = 0; lo < n_tensors; lo += T)
        if (int e = train::grad_table(entries + lo, (int)(n_tensors - lo < T ? n_tensors - lo : T), a, chunks)) return e;
    const int64_t total_chunks = train::grad_chunks(entries, n_tensors);
    if (total_chunks < 0) return DEQSCI_ERR_SHAPE;
    const int64_t stats_bytes = (3 + n_tensors) * 8, ws_bytes = (total_chunks + n_tensors) * train::NNORM * 8;
    if (overlaps(stats, stats_bytes, workspace, ws_bytes)) return DEQSCI_ERR_UNSUPPORTED;
    for (int64_t i = 0; i < n_tensors; ++i)
        if (overlaps(stats, stats_bytes, entries[i].grad, entries[i].numel * 4) || overlaps(workspace, ws_bytes, entries[i].grad, entries[i].numel * 4))
            return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    double* tsum = part + total_chunks * train::NNORM;
    int64_t chunk0 = 0;
    for (int64_t lo = 0; lo < n_tensors; lo += T) {
        const int n = (int)(n_tensors - lo < T ? n_tensors - lo : T);
        train::grad_table(entries + lo, n, a, chunks);
        hipLaunchKernelGGL(train::grad_norm_chunk_kernel, dim3((unsigned)chunks), dim3(TB), 0, st, a, part + chunk0 * train::NNORM);
        if (int e = launch_status()) return e;
        hipLaunchKernelGGL(train::grad_norm_fold_kernel, dim3((unsigned)n), dim3(TB), 0, st, a, part + chunk0 * train::NNORM, tsum + lo * train::NNORM);
        if (int e = launch_status()) return e;
        chunk0 += (int64_t)chunks;
    }
    hipLaunchKernelGGL(train::grad_norm_final_kernel, dim3(1), dim3(TB), 0, st, tsum, n_tensors, max_norm, stats);
    return launch_status();
}

int deqsci_grad_scale_f32(const deqsci_grad_entry* entries, int64_t n_tensors, const double* stats, deqsci_stream_t stream) {
    if (n_tensors < 0 || n_tensors > ((int64_t)1 << 24)) return DEQSCI_ERR_SHAPE;
    if (n_tensors == 0) return 0;
    if (!entries || !stats) return DEQSCI_ERR_NULL;
    if (misaligned(stats, 8)) return DEQSCI_ERR_ALIGN;
    const int T = DEQSCI_ADAM_MAX_TENSORS;
    train::GradArgs a;
    uint64_t chunks = 0;
    for (int64_t lo = 0; lo < n_tensors; lo += T)
        if (int e = train::grad_table(entries + lo, (int)(n_tensors - lo < T ? n_tensors - lo : T), a, chunks)) return e;
    for (int64_t i = 0; i < n_tensors; ++i)
        if (overlaps(stats, 24, entries[i].grad, entries[i].numel * 4)) return DEQSCI_ERR_UNSUPPORTED;
    for (int64_t lo = 0; lo < n_tensors; lo += T) {
        train::grad_table(entries + lo, (int)(n_tensors - lo < T ? n_tensors - lo : T), a, chunks);
        hipLaunchKernelGGL(train::grad_scale_kernel, dim3((unsigned)chunks), dim3(TB), 0, static_cast<hipStream_t>(stream), a, stats);
        if (int e = launch_status()) return e;
    }
    return 0;
}

}  // extern "C"
