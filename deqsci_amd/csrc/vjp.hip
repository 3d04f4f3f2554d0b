// The implicit backward's ReLU masks (the DEQ hook solves g = J_f(z0)^T g + grad, solvers/new_equilibrium_utils_yaping.py:273-276):
// every vector-Jacobian product through the denoiser is linear in v, and its ReLU decisions are those of ONE forward pass at z0, so
// they are stored once, one bit per unit, and every VJP layer multiplies its output by them (the masked epilogues of csrc/winograd.hip,
// csrc/winograd44.hip and csrc/ffdnet_edges.hip).
//
//   V0 relu_mask_pack_kernel   fp32 channels_last activation (pixels, 64) -> one 64-bit word per pixel, bit c = (a[pixel, c] > 0):
//                              ReLU'(0) = 0 as in PyTorch, so +-0.0 and NaN block.  A wave reads one pixel's 64 channels per step
//                              (256 contiguous bytes), v_cmp + ballot gives the word; lane p keeps the word of pixel p of the wave's
//                              64, and the wave stores its 64 words as one 512-byte run.
#include "common.hpp"

namespace deqsci {
namespace vjp {

constexpr int PIX_PER_WAVE = 64;

__global__ __launch_bounds__(TB) void relu_mask_pack_kernel(const float* __restrict__ a, uint64_t* __restrict__ mask, int64_t n_pix) {
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    const int64_t base = ((int64_t)blockIdx.x * (TB / WAVE) + threadIdx.x / WAVE) * PIX_PER_WAVE;
    if (base >= n_pix) return;
    const int cnt = (int)(n_pix - base < PIX_PER_WAVE ? n_pix - base : PIX_PER_WAVE);
    const float* ab = a + base * 64 + lane;
    uint64_t mine = 0;
#pragma unroll 8
    for (int p = 0; p < PIX_PER_WAVE; ++p) {
        if (p < cnt) {                                        // (uniform)
            const uint64_t w = __builtin_amdgcn_ballot_w64(ab[(int64_t)p * 64] > 0.0f);
            if (lane == p) mine = w;
        }
    }
    if (lane < cnt) mask[base + lane] = mine;
}

}  // namespace vjp
}  // namespace deqsci

using namespace deqsci;

extern "C" int deqsci_relu_mask_pack_f32(const float* a, uint64_t* mask, int64_t n_pixels, deqsci_stream_t stream) {
    if (!a || !mask) return DEQSCI_ERR_NULL;
    if (n_pixels < 0) return DEQSCI_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(a) & 3) != 0 || (reinterpret_cast<uintptr_t>(mask) & 7) != 0) return DEQSCI_ERR_ALIGN;
    if (n_pixels == 0) return 0;
    const int64_t per_block = (int64_t)(TB / WAVE) * vjp::PIX_PER_WAVE;
    if (ceil_div(n_pixels, per_block) > (int64_t)INT32_MAX) return DEQSCI_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vjp::relu_mask_pack_kernel, dim3((unsigned)ceil_div(n_pixels, per_block)), dim3(TB), 0,
                       static_cast<hipStream_t>(stream), a, mask, n_pixels);
    return launch_status();
}
