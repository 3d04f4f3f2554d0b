// Mask gradients of the SCI operators and of the GAP projection for MI355X (gfx950): what a learnable coded aperture needs.
//
//   G1 gap_update_grad   the backward of K3 (csrc/sci_ops.hip) in one pass: with g the gradient of z1 = z + Phi^T((y - Phi z) / s),
//                            fb = sum_b z_b Phi_b      q = sum_b g_b Phi_b      d = y - fb      r = d / s      t = q / s
//                            gPhi_b = (r g_b) - (t z_b)      gs = -(t r)      gz_b = g_b - (t Phi_b)      gy = t
//   G2 sci_mask_grad     gPhi_b = a v_b: the mask gradient of y = Phi x (a = gy, v = x) and of x = Phi^T y (a = y, v = gx)
//   G3 phi_sum_grad      gPhi_b = (sum_b Phi_b == 0 ? 0 : gs): the backward of O4, cut where the forward substituted 1
//
// Streaming fp32 kernels bounded by HBM bandwidth like K1-K3, and built the same way: HWB only (the layout the autograd wrappers
// use), the tensor read as a flat float4 stream, LP = B/4 adjacent lanes per pixel combined by the wave64 xor-butterfly, one
// coalesced 16-byte access per lane per instruction, every product, sum, difference and quotient rounded separately
// (-ffp-contract=off), fb and q formed exactly as K3 forms fb (dot4_seq + group_sum).  A generic any-B path takes one lane per
// pixel and sums the frames left to right.
// A mask shared by the batch (phi_shared = 1) gets the SUM of the per-sample gradients: the grid's y dimension is 1, the lane that
// owns a pixel quarter walks n = 0 .. bsz-1 in that order and keeps the running sums in registers (the generic G1 path keeps them
// in its own output elements), so the result is deterministic and has one order of operations.  No atomics, no allocation, no
// synchronisation: graph-capturable.
#include "common.hpp"

namespace deqsci {

constexpr int UNR = 4;          // independent float4 positions per lane, as in csrc/sci_ops.hip

// r g - t z per frame of a quad, both products rounded before the difference
__device__ __forceinline__ float4 rg_minus_tz(float r, float4 g, float t, float4 z) { return r * g - t * z; }

template <int LP, int POL>
__global__ __launch_bounds__(TB) void gap_grad_hwb_kernel(const float* __restrict__ z, const float* __restrict__ phi,
                                                          const float* __restrict__ g, const float* __restrict__ y,
                                                          const float* __restrict__ phisum, float* __restrict__ gphi,
                                                          float* __restrict__ gs, float* __restrict__ gz, float* __restrict__ gy,
                                                          int64_t P, int bsz, int phi_shared) {
    const int64_t Q = P * LP;                          // float4 per measurement
    const int64_t n0 = phi_shared ? 0 : blockIdx.y;    // the mask this block writes a gradient for
    const int nn = phi_shared ? bsz : 1;               // measurements summed into it
    const float* ps = phi + n0 * Q * 4;
    const float* ss = phisum + n0 * P;
    const int64_t base = (int64_t)blockIdx.x * (TB * UNR) + threadIdx.x;
    float4 pv[UNR], ap[UNR];
    float sv[UNR], as[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
        const int64_t q = base + j * TB;
        const int64_t qc = q < Q ? q : Q - 1;
        pv[j] = ldp<POL>(ps + qc * 4);
        sv[j] = ss[qc / LP];
    }
    for (int n = 0; n < nn; ++n) {
        const int64_t m = n0 + n;
        const float* zs = z + m * Q * 4;
        const float* gr = g + m * Q * 4;
        const float* ys = y + m * P;
        float4 zv[UNR], gv[UNR];
        float yv[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int64_t q = base + j * TB;
            const int64_t qc = q < Q ? q : Q - 1;
            zv[j] = ldp<POL>(zs + qc * 4);
            gv[j] = ldp<POL>(gr + qc * 4);
            yv[j] = ys[qc / LP];
        }
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int64_t q = base + j * TB;
            const float fb = group_sum<LP>(dot4_seq(zv[j], pv[j]));
            const float qd = group_sum<LP>(dot4_seq(gv[j], pv[j]));
            const float r = (yv[j] - fb) / sv[j];
            const float t = qd / sv[j];
            const float4 tp = rg_minus_tz(r, gv[j], t, zv[j]);
            const float ts = -(t * r);
            if (n == 0) { ap[j] = tp; as[j] = ts; } else { ap[j] = ap[j] + tp; as[j] = as[j] + ts; }
            if (q < Q) {
                if (gz) stp<POL>(gz + m * Q * 4 + q * 4, gv[j] - t * pv[j]);
                if (gy && (q & (LP - 1)) == 0) gy[m * P + q / LP] = t;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
        const int64_t q = base + j * TB;
        if (q < Q) {
            if (gphi) stp<POL>(gphi + n0 * Q * 4 + q * 4, ap[j]);
            if (gs && (q & (LP - 1)) == 0) gs[n0 * P + q / LP] = as[j];
        }
    }
}

template <int LP, int POL>
__global__ __launch_bounds__(TB) void mask_grad_hwb_kernel(const float* __restrict__ a, const float* __restrict__ v,
                                                           float* __restrict__ gphi, int64_t P, int bsz, int phi_shared) {
    const int64_t Q = P * LP;
    const int64_t n0 = phi_shared ? 0 : blockIdx.y;
    const int nn = phi_shared ? bsz : 1;
    const int64_t base = (int64_t)blockIdx.x * (TB * UNR) + threadIdx.x;
    float4 acc[UNR];
    for (int n = 0; n < nn; ++n) {
        const int64_t m = n0 + n;
        const float* vs = v + m * Q * 4;
        const float* as = a + m * P;
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int64_t q = base + j * TB;
            const int64_t qc = q < Q ? q : Q - 1;
            const float4 t = as[qc / LP] * ldp<POL>(vs + qc * 4);
            acc[j] = n == 0 ? t : acc[j] + t;
        }
    }
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
        const int64_t q = base + j * TB;
        if (q < Q) stp<POL>(gphi + n0 * Q * 4 + q * 4, acc[j]);
    }
}

// S in the order of phisum_hwb_kernel (csrc/sci_ops.hip), so that the cut falls exactly where that kernel wrote 1
template <int LP, int POL>
__global__ __launch_bounds__(TB) void phisum_grad_hwb_kernel(const float* __restrict__ phi, const float* __restrict__ gs,
                                                             float* __restrict__ gphi, int64_t P) {
    const int64_t n = blockIdx.y;
    const int64_t Q = P * LP;
    const float* ps = phi + n * Q * 4;
    const float* gr = gs + n * P;
    float* os = gphi + n * Q * 4;
    const int64_t base = (int64_t)blockIdx.x * (TB * UNR) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
        const int64_t q = base + j * TB;
        const int64_t qc = q < Q ? q : Q - 1;
        const float4 p = ldp<POL>(ps + qc * 4);
        const float s = group_sum<LP>(((p.x + p.y) + p.z) + p.w);
        const float v = (s == 0.0f) ? 0.0f : gr[qc / LP];
        if (q < Q) stp<POL>(os + q * 4, f4(v));
    }
}

// ------------------------------------------------------------------------------------------------
// Generic paths: any B, one lane per pixel, frames left to right from frame 0 (the order of generic_kernel in csrc/sci_ops.hip).
// ------------------------------------------------------------------------------------------------
// gphi is read back by the lane that wrote it (the running sum over a shared mask's batch): not __restrict__.
__global__ __launch_bounds__(TB) void gap_grad_generic_kernel(const float* __restrict__ z, const float* __restrict__ phi,
                                                              const float* __restrict__ g, const float* __restrict__ y,
                                                              const float* __restrict__ phisum, float* gphi, float* gs, float* gz,
                                                              float* gy, int64_t P, int B, int bsz, int phi_shared) {
    const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= P) return;
    const int64_t n0 = phi_shared ? 0 : blockIdx.y;
    const int nn = phi_shared ? bsz : 1;
    const float* pp = phi + (n0 * P + p) * B;
    const float s = phisum[n0 * P + p];
    float* op = gphi ? gphi + (n0 * P + p) * B : nullptr;
    float as = 0.0f;
    for (int n = 0; n < nn; ++n) {
        const int64_t m = n0 + n;
        const float* zp = z + (m * P + p) * B;
        const float* gp = g + (m * P + p) * B;
        float fb = zp[0] * pp[0], qd = gp[0] * pp[0];
        for (int b = 1; b < B; ++b) { fb += zp[b] * pp[b]; qd += gp[b] * pp[b]; }
        const float r = (y[m * P + p] - fb) / s;
        const float t = qd / s;
        if (op) {
            for (int b = 0; b < B; ++b) {
                const float tp = r * gp[b] - t * zp[b];
                op[b] = n == 0 ? tp : op[b] + tp;
            }
        }
        const float ts = -(t * r);
        as = n == 0 ? ts : as + ts;
        if (gz) {
            float* o = gz + (m * P + p) * B;
            for (int b = 0; b < B; ++b) o[b] = gp[b] - t * pp[b];
        }
        if (gy) gy[m * P + p] = t;
    }
    if (gs) gs[n0 * P + p] = as;
}

__global__ __launch_bounds__(TB) void mask_grad_generic_kernel(const float* __restrict__ a, const float* __restrict__ v,
                                                               float* __restrict__ gphi, int64_t P, int B, int bsz, int phi_shared) {
    const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= P) return;
    const int64_t n0 = phi_shared ? 0 : blockIdx.y;
    const int nn = phi_shared ? bsz : 1;
    for (int b = 0; b < B; ++b) {
        float acc = a[n0 * P + p] * v[(n0 * P + p) * B + b];
        for (int n = 1; n < nn; ++n) acc += a[(n0 + n) * P + p] * v[((n0 + n) * P + p) * B + b];
        gphi[(n0 * P + p) * B + b] = acc;
    }
}

__global__ __launch_bounds__(TB) void phisum_grad_generic_kernel(const float* __restrict__ phi, const float* __restrict__ gs,
                                                                 float* __restrict__ gphi, int64_t P, int B) {
    const int64_t n = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= P) return;
    const float* pp = phi + (n * P + p) * B;
    float acc = pp[0];
    for (int b = 1; b < B; ++b) acc += pp[b];
    const float v = acc == 0.0f ? 0.0f : gs[n * P + p];
    float* o = gphi + (n * P + p) * B;
    for (int b = 0; b < B; ++b) o[b] = v;
}

static inline bool lp_ok(int64_t B) { return B == 4 || B == 8 || B == 16 || B == 32; }
// the checks of csrc/sci_ops.hip's check_dims, and HWB alone
static inline int check_dims_hwb(int64_t bsz, int64_t H, int64_t W, int64_t B, int layout) {
    if (bsz <= 0 || H <= 0 || W <= 0 || B <= 0) return DEQSCI_ERR_SHAPE;
    if (bsz > 65535 || B > 4096) return DEQSCI_ERR_UNSUPPORTED;
    if (layout != DEQSCI_LAYOUT_HWB) return DEQSCI_ERR_UNSUPPORTED;
    return 0;
}

#define LP_DISPATCH(B, ...)                          \
    switch ((int)(B)) {                              \
        case 4:  { constexpr int LP = 1; __VA_ARGS__; } break; \
        case 8:  { constexpr int LP = 2; __VA_ARGS__; } break; \
        case 16: { constexpr int LP = 4; __VA_ARGS__; } break; \
        default: { constexpr int LP = 8; __VA_ARGS__; } break; \
    }
#define POL_DISPATCH(pol, ...)                                   \
    switch (pol) {                                               \
        case POL_NTL:  { constexpr int POL = POL_NTL; __VA_ARGS__; } break;  \
        case POL_NTS:  { constexpr int POL = POL_NTS; __VA_ARGS__; } break;  \
        case POL_NTLS: { constexpr int POL = POL_NTLS; __VA_ARGS__; } break; \
        default:       { constexpr int POL = POL_DEFAULT; __VA_ARGS__; } break; \
    }

}  // namespace deqsci

using namespace deqsci;

extern "C" {

int deqsci_gap_update_grad_f32(const float* z, const float* phi, const float* g, const float* y, const float* phisum, float* gphi,
                               float* gs, float* gz, float* gy, int64_t bsz, int64_t H, int64_t W, int64_t B, int layout,
                               int phi_shared, deqsci_stream_t stream) {
    if (!z || !phi || !g || !y || !phisum) return DEQSCI_ERR_NULL;
    if (!gphi && !gs && !gz && !gy) return DEQSCI_ERR_NULL;
    if (int e = check_dims_hwb(bsz, H, W, B, layout)) return e;
    if (!aligned16(z) || !aligned16(phi) || !aligned16(g) || !aligned16(y) || !aligned16(phisum) || !aligned16(gphi) ||
        !aligned16(gs) || !aligned16(gz) || !aligned16(gy))
        return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = H * W, nm = phi_shared ? 1 : bsz;            // masks
    // the launch's own bytes: z, g, y per measurement, Phi and Phi_sum per mask, and the outputs that are asked for
    const int64_t bytes = bsz * P * (8 * B + 4) + nm * P * (4 * B + 4) + (gphi ? nm * P * 4 * B : 0) + (gs ? nm * P * 4 : 0) +
                          (gz ? bsz * P * 4 * B : 0) + (gy ? bsz * P * 4 : 0);
    const int pol = pick_policy(bytes, POL_NTLS);
    if (lp_ok(B)) {
        POL_DISPATCH(pol, LP_DISPATCH(B, hipLaunchKernelGGL((gap_grad_hwb_kernel<LP, POL>), dim3(ceil_div(P * LP, TB * UNR), nm), dim3(TB), 0, st, z, phi, g, y, phisum, gphi, gs, gz, gy, P, (int)bsz, phi_shared)));
    } else {
        hipLaunchKernelGGL(gap_grad_generic_kernel, dim3(ceil_div(P, TB), nm), dim3(TB), 0, st, z, phi, g, y, phisum, gphi, gs, gz, gy, P, (int)B, (int)bsz, phi_shared);
    }
    return launch_status();
}

int deqsci_sci_mask_grad_f32(const float* a, const float* v, float* gphi, int64_t bsz, int64_t H, int64_t W, int64_t B, int layout,
                             int phi_shared, deqsci_stream_t stream) {
    if (!a || !v || !gphi) return DEQSCI_ERR_NULL;
    if (int e = check_dims_hwb(bsz, H, W, B, layout)) return e;
    if (!aligned16(a) || !aligned16(v) || !aligned16(gphi)) return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = H * W, nm = phi_shared ? 1 : bsz;
    const int pol = pick_policy(bsz * P * (4 * B + 4) + nm * P * 4 * B, POL_NTLS);
    if (lp_ok(B)) {
        POL_DISPATCH(pol, LP_DISPATCH(B, hipLaunchKernelGGL((mask_grad_hwb_kernel<LP, POL>), dim3(ceil_div(P * LP, TB * UNR), nm), dim3(TB), 0, st, a, v, gphi, P, (int)bsz, phi_shared)));
    } else {
        hipLaunchKernelGGL(mask_grad_generic_kernel, dim3(ceil_div(P, TB), nm), dim3(TB), 0, st, a, v, gphi, P, (int)B, (int)bsz, phi_shared);
    }
    return launch_status();
}

int deqsci_phi_sum_grad_f32(const float* phi, const float* gs, float* gphi, int64_t nb, int64_t H, int64_t W, int64_t B, int layout,
                            deqsci_stream_t stream) {
    if (!phi || !gs || !gphi) return DEQSCI_ERR_NULL;
    if (int e = check_dims_hwb(nb, H, W, B, layout)) return e;
    if (!aligned16(phi) || !aligned16(gs) || !aligned16(gphi)) return DEQSCI_ERR_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = H * W;
    const int pol = pick_policy(nb * P * (8 * B + 4), POL_NTLS);
    if (lp_ok(B)) {
        POL_DISPATCH(pol, LP_DISPATCH(B, hipLaunchKernelGGL((phisum_grad_hwb_kernel<LP, POL>), dim3(ceil_div(P * LP, TB * UNR), nb), dim3(TB), 0, st, phi, gs, gphi, P)));
    } else {
        hipLaunchKernelGGL(phisum_grad_generic_kernel, dim3(ceil_div(P, TB), nb), dim3(TB), 0, st, phi, gs, gphi, P, (int)B);
    }
    return launch_status();
}

}  // extern "C"
