// Jacobian diagnostics of the fixed-point map f(z) = z1 - D(z1), z1 = P z + c, for MI355X (gfx950): what the power iterations of
// deqsci_amd/jacobian.py need beyond the masked layers of the implicit backward (csrc/vjp.hip, csrc/winograd.hip, csrc/ffdnet_edges.hip).
//
//   J1 ffdnet_head_masked_kernel   h = conv3x3(pixel_unshuffle_2(x)) * mask: FFDNet's first layer linearised (forward weights, image
//                                  channels 1..4 - sigma is a constant of the linearisation -, the first ReLU's mask) and, with the
//                                  tail's weight transposed and flipped and the last ReLU's mask, the transpose of its last layer
//                                  (pixel_shuffle's transpose is pixel_unshuffle).  The head stencil of csrc/ffdnet_edges.hip
//                                  (ffdnet_head_kernel) without the sigma plane - 36 weight rows instead of 45 -, without bias and
//                                  ReLU, and with the masked epilogue of conv_c1_to_64_kernel<3>.
//   J2 power_partial_kernel        one workgroup = one (sample, chunk of CHUNK elements): a = sum w^2 and b = sum v_prev w with float64
//                                  products and sums (per thread, per wave, per workgroup) -> part[sample][chunk][2]
//      power_normalise_kernel      every workgroup sums its sample's chunk pairs in ONE fixed order (so all of them hold the same a),
//                                  writes its chunk of v_out = w / sqrt(a), and the workgroup of chunk 0 writes (a, b) to the table.
//                                  a zero or not finite: v_out = 0 and (NaN, NaN) in the table - never a number that looks valid.
//
// Determinism: J2 sums in the two-stage order of csrc/rows.hpp, reading a row as float4 where the row starts are 16-byte aligned and
// element by element elsewhere.  fp32 is scale-free and the vectors are renormalised every step, so no range
// bookkeeping is needed.  HBM-streaming: J2 reads w twice and v_prev once, writes v_out once.
#include "rows.hpp"

namespace deqsci {
namespace jac {

typedef float f32x2 __attribute__((ext_vector_type(2)));
// acc += s.x * w  /  acc += s.y * w on a register pair: ONE v_pk_fma_f32, the broadcast is an operand modifier (csrc/ffdnet_edges.hip)
__device__ __forceinline__ void pk_fma_lo(f32x2& acc, f32x2 s, f32x2 w) {
    acc = __builtin_elementwise_fma(__builtin_shufflevector(s, s, 0, 0), w, acc);
}
__device__ __forceinline__ void pk_fma_hi(f32x2& acc, f32x2 s, f32x2 w) {
    acc = __builtin_elementwise_fma(__builtin_shufflevector(s, s, 1, 1), w, acc);
}

// Mapping as ffdnet_head_kernel: 16 lanes per half-resolution position, each owning 4 output channels with their 4 x 36 weights in
// VGPRs for the whole HD_T x HD_T tile; the (2 HD_T + 4)^2 full-resolution patch sits in LDS (zero outside the image = the zero
// padding of the unshuffled channels) and the 16 lanes of a position read it by broadcast.
template <int HD_T>
__global__ __launch_bounds__(TB) void ffdnet_head_masked_kernel(const float* __restrict__ x, const float* __restrict__ wq,
                                                                const uint32_t* __restrict__ mask, float* __restrict__ h, int H, int W) {
    constexpr int HD_P = 2 * HD_T + 4;            // patch side in full-res pixels
    constexpr int HD_PS = HD_P + 2;               // LDS row stride (even: float2 reads stay 8-B aligned)
    __shared__ __attribute__((aligned(16))) float patch[HD_P * HD_PS];
    const int n = blockIdx.z;
    const int r0 = blockIdx.y * HD_T, c0 = blockIdx.x * HD_T;
    const int H2 = 2 * H, W2 = 2 * W;
    const float* xn = x + (int64_t)n * H2 * W2;
    for (int e = threadIdx.x; e < HD_P * HD_P; e += TB) {
        const int pr = e / HD_P, pc = e % HD_P;
        const int gr = 2 * r0 - 2 + pr, gc = 2 * c0 - 2 + pc;
        patch[pr * HD_PS + pc] = (gr >= 0 && gr < H2 && gc >= 0 && gc < W2) ? xn[(int64_t)gr * W2 + gc] : 0.0f;
    }
    const int cq = threadIdx.x % 16, slot = threadIdx.x / 16;
    f32x2 wl[36], wh[36];                         // [ch*9 + tap] -> output channels 4cq..4cq+3 as two register pairs
#pragma unroll
    for (int k = 0; k < 36; ++k) {
        const float4 t = ld4(wq + (k * 16 + cq) * 4);
        wl[k] = (f32x2){t.x, t.y};
        wh[k] = (f32x2){t.z, t.w};
    }
    __syncthreads();
    float* hn = h + (int64_t)n * H * W * 64;
#pragma unroll 1
    for (int it = 0; it < HD_T * HD_T / 16; ++it) {
        const int q = it * 16 + slot;
        const int lr = q / HD_T, lc = q % HD_T;
        const int r = r0 + lr, c = c0 + lc;
        f32x2 al = {0.0f, 0.0f}, ah = {0.0f, 0.0f};
#pragma unroll
        for (int prow = 0; prow < 6; ++prow) {      // full-res rows 2r-2 .. 2r+3: dr = prow/2 - 1, i = prow%2
            const float* pp = patch + (2 * lr + prow) * HD_PS + 2 * lc;
            f32x2 v[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) v[j] = *reinterpret_cast<const f32x2*>(pp + 2 * j);
#pragma unroll
            for (int pcol = 0; pcol < 6; ++pcol) {  // dc = pcol/2 - 1, j = pcol%2
                const int ch = 2 * (prow % 2) + (pcol % 2);
                const int tap = (prow / 2) * 3 + (pcol / 2);
                if (pcol % 2 == 0) { pk_fma_lo(al, v[pcol / 2], wl[ch * 9 + tap]); pk_fma_lo(ah, v[pcol / 2], wh[ch * 9 + tap]); }
                else { pk_fma_hi(al, v[pcol / 2], wl[ch * 9 + tap]); pk_fma_hi(ah, v[pcol / 2], wh[ch * 9 + tap]); }
            }
        }
        if (r < H && c < W) {                       // couts 4 cq .. 4 cq + 3: half cq >> 3 of the pixel's word
            const uint32_t m = mask[2 * ((int64_t)n * H * W + (int64_t)r * W + c) + (cq >> 3)] >> (4 * (cq & 7));
            const float4 o4 = make_float4((m & 1u) ? al[0] : 0.0f, (m & 2u) ? al[1] : 0.0f, (m & 4u) ? ah[0] : 0.0f, (m & 8u) ? ah[1] : 0.0f);
            st4(hn + ((int64_t)r * W + c) * 64 + 4 * cq, o4);
        }
    }
}

// ---- J2
using namespace rows;

constexpr int PER_THREAD = 4;                            // float4 per thread and row
typedef Chunk<PER_THREAD> Ch;
constexpr int64_t CHUNK = Ch::SIZE;                      // 4096 elements per workgroup

__global__ __launch_bounds__(TB) void power_partial_kernel(const float* __restrict__ w, const float* __restrict__ v_prev,
                                                           double* __restrict__ part, int64_t N, int64_t n_chunks) {
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    const float* wr = w + s * N;
    const float* vr = v_prev ? v_prev + s * N : nullptr;
    const bool vec = aligned16_all(wr, vr);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            const float4 x = load4(wr, e, N, vec);
            const float4 y = vr ? load4(vr, e, N, vec) : f4(0.0f);
            a = sq4(x, a);
            b = dot4(y, x, b);
        }
        a = block_sum(a, wsum);
        b = block_sum(b, wsum);
        if (tid == 0) {
            part[(s * n_chunks + c) * 2] = a;
            part[(s * n_chunks + c) * 2 + 1] = b;
        }
    }
}

// v_out may be w or v_prev themselves (every element is read and written by the same thread; v_prev was consumed by the first stage)
__global__ __launch_bounds__(TB) void power_normalise_kernel(const float* w, float* v_out, const double* __restrict__ part,
                                                             double* __restrict__ table_row, int has_prev, int64_t N, int64_t n_chunks) {
    __shared__ double wsum[NW];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.y;
    // the sample's chunk pairs, thread t summing chunks t, t + TB, ... in order: the same order in every workgroup of the sample
    double a = 0.0, b = 0.0;
    for (int64_t t = tid; t < n_chunks; t += TB) {
        a += part[(s * n_chunks + t) * 2];
        b += part[(s * n_chunks + t) * 2 + 1];
    }
    a = block_sum(a, wsum);
    b = block_sum(b, wsum);
    const bool ok = a > 0.0 && a <= 1.79769313486231570815e308;          // (NaN fails both comparisons)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (blockIdx.x == 0 && tid == 0) {
        table_row[2 * s] = ok ? a : nan;
        table_row[2 * s + 1] = (ok && has_prev) ? b : nan;
    }
    const double rs = ok ? 1.0 / sqrt(a) : 0.0;
    const float* wr = w + s * N;
    float* vo = v_out + s * N;
    const bool vec = aligned16_all(wr, vo);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * CHUNK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            const int64_t e = Ch::elem(base, q, tid);
            const float4 x = load4(wr, e, N, vec);          // the products in float64, rounded to fp32 once
            store4(vo, e, N, vec, ok ? make_float4((float)(x.x * rs), (float)(x.y * rs), (float)(x.z * rs), (float)(x.w * rs)) : f4(0.0f));
        }
    }
}

inline bool sizes_ok(int64_t bsz, int64_t N) {
    // (bsz is the grid's y extent; the element offsets are int64)
    return bsz >= 0 && N >= 0 && bsz <= 65535 && N <= ((int64_t)1 << 40);
}

}  // namespace jac
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int deqsci_ffdnet_head_masked_f32(const float* x, const float* w_packed, const uint64_t* mask, float* h, int64_t n, int64_t H,
                                  int64_t W, deqsci_stream_t stream) {
    if (!x || !w_packed || !mask || !h) return DEQSCI_ERR_NULL;
    if (n <= 0 || H <= 0 || W <= 0) return DEQSCI_ERR_SHAPE;
    if (n > 65535 || H > (1 << 20) || W > (1 << 20)) return DEQSCI_ERR_UNSUPPORTED;
    if (!aligned16(w_packed) || !aligned16(h) || misaligned(mask, 8) || misaligned(x, 4))
        return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t* m32 = reinterpret_cast<const uint32_t*>(mask);
    if (ceil_div(W, 32) * ceil_div(H, 32) * n >= 2 * (int64_t)num_cus()) {
        const dim3 grid((unsigned)ceil_div(W, 32), (unsigned)ceil_div(H, 32), (unsigned)n);
        hipLaunchKernelGGL(jac::ffdnet_head_masked_kernel<32>, grid, dim3(TB), 0, st, x, w_packed, m32, h, (int)H, (int)W);
    } else {                                       // grids that would leave CUs idle: 16 x 16 tiles, as the head itself
        const dim3 grid((unsigned)ceil_div(W, 16), (unsigned)ceil_div(H, 16), (unsigned)n);
        hipLaunchKernelGGL(jac::ffdnet_head_masked_kernel<16>, grid, dim3(TB), 0, st, x, w_packed, m32, h, (int)H, (int)W);
    }
    return launch_status();
}

size_t deqsci_power_workspace_bytes(int64_t bsz, int64_t N) {
    if (!jac::sizes_ok(bsz, N)) return 0;
    return (size_t)(bsz * ceil_div(N, jac::CHUNK)) * 2 * sizeof(double);
}

int deqsci_power_step_f32(const float* w, const float* v_prev, float* v_out, double* table_row, int64_t bsz, int64_t N,
                          void* workspace, deqsci_stream_t stream) {
    if (!jac::sizes_ok(bsz, N)) return DEQSCI_ERR_SHAPE;
    if (bsz == 0 || N == 0) return 0;
    if (!w || !v_out || !table_row || !workspace) return DEQSCI_ERR_NULL;
    if (misaligned(w, 4) || misaligned(v_prev, 4) || misaligned(v_out, 4) || misaligned(table_row, 8) || misaligned(workspace, 8))
        return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_chunks = ceil_div(N, jac::CHUNK);
    double* part = static_cast<double*>(workspace);
    const dim3 grid = rows::chunk_grid(n_chunks, bsz);
    hipLaunchKernelGGL(jac::power_partial_kernel, grid, dim3(TB), 0, st, w, v_prev, part, N, n_chunks);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(jac::power_normalise_kernel, grid, dim3(TB), 0, st, w, v_out, (const double*)part, table_row, v_prev ? 1 : 0, N,
                       n_chunks);
    return launch_status();
}

}  // extern "C"
