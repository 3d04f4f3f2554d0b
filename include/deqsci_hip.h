/*
 * deqsci_hip.h - C ABI of libdeqsci_hip.so: the MI355X (gfx950) kernels of the DEQ-SCI
 * reconstruction hot path (SCI sensing operators, GAP projection, Anderson fixed-point
 * bookkeeping).  Plain pointers and sizes only - no torch / C++ types cross this boundary.
 *
 * The reference (IndigoPurple/DEQSCI) is pure Python and has no FFI; each entry point below
 * replaces the ATen expression(s) the reference evaluates at the cited file:line.  The binding a
 * reference maintainer would add is a ctypes stub - see INTEGRATION.md.
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers to contiguous fp32, 16-byte aligned.
 *   - Layouts: DEQSCI_LAYOUT_HWB = (bsz,H,W,B), frames innermost - the reference's API layout
 *     (solvers/equilibrium_solvers_yaping.py:397); DEQSCI_LAYOUT_BHW = (bsz,B,H,W) planar - the
 *     denoiser's (bsz*B,1,H,W) layout (ibid. :415).  y / Phi_sum are always (bsz,H,W).
 *   - phi_shared != 0: Phi (and Phi_sum) carry no batch dimension - one mask for every
 *     measurement of a clip (training/sci_equilibrium_training.py:161-176).
 *   - Ownership: the caller owns every buffer including scratch; no entry point allocates,
 *     frees or synchronises.  Work is enqueued on `stream`; entry points are re-entrant,
 *     hold no global state and are safe under HIP-graph stream capture.
 *   - Return: 0 on success; >0 = hipError_t of the failed launch; <0 = DEQSCI_ERR_*.
 */
#ifndef DEQSCI_HIP_H
#define DEQSCI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEQSCI_LAYOUT_HWB 0
#define DEQSCI_LAYOUT_BHW 1

#define DEQSCI_MAX_M 8            /* largest Anderson history depth (reference uses m=5) */
#define DEQSCI_PART_STRIDE (DEQSCI_MAX_M + 1)

#define DEQSCI_ERR_NULL        (-1)   /* required pointer is NULL                      */
#define DEQSCI_ERR_SHAPE       (-2)   /* non-positive / inconsistent sizes             */
#define DEQSCI_ERR_ALIGN       (-3)   /* pointer not 16-byte aligned                   */
#define DEQSCI_ERR_UNSUPPORTED (-4)   /* m > DEQSCI_MAX_M, unknown layout, ...         */

typedef void* deqsci_stream_t;    /* a hipStream_t (NULL = the legacy default stream) */

const char* deqsci_version(void);
const char* deqsci_error_string(int code);

/* K1  y = Phi x : y[n,h,w] = sum_b x[n,h,w,b] * Phi[n,h,w,b]
 *     replaces A_torch_, utils/cg_utils.py:85-90.  x and phi share `layout`. */
int deqsci_sci_forward_f32(const float* x, const float* phi, float* y,
                           int64_t bsz, int64_t H, int64_t W, int64_t B,
                           int layout, int phi_shared, deqsci_stream_t stream);

/* K2  x = Phi^T y : x[n,h,w,b] = y[n,h,w] * Phi[n,h,w,b]
 *     replaces At_torch_ (utils/cg_utils.py:124-129) and initial_point (:228-229). */
int deqsci_sci_adjoint_f32(const float* y, const float* phi, float* x,
                           int64_t bsz, int64_t H, int64_t W, int64_t B,
                           int layout, int phi_shared, deqsci_stream_t stream);

/* O4  Phi_sum = sum_b Phi with zeros replaced by 1
 *     replaces training/sci_equilibrium_training.py:162-163.  nb = bsz, or 1 for a shared mask. */
int deqsci_phi_sum_f32(const float* phi, float* phisum,
                       int64_t nb, int64_t H, int64_t W, int64_t B,
                       int layout, deqsci_stream_t stream);

/* K3  fused GAP projection  z1 = z + Phi^T((y - Phi z) / Phi_sum)
 *     replaces solvers/equilibrium_solvers_yaping.py:399-400 (5 ATen kernels, 4 temporaries)
 *     and, when layout_out == BHW with layout_in == HWB, also the permute+contiguous at :415/:419.
 *     z and phi are in layout_in; z1 is written in layout_out.  z1 may alias z iff the layouts match. */
int deqsci_gap_update_f32(const float* z, const float* phi, const float* y, const float* phisum,
                          float* z1, int64_t bsz, int64_t H, int64_t W, int64_t B,
                          int layout_in, int layout_out, int phi_shared, deqsci_stream_t stream);

/* ---- mask gradients (csrc/sci_grad.hip): what training a coded aperture needs; not on the reconstruction path ----
 * HWB only (any other layout: DEQSCI_ERR_UNSUPPORTED); outputs must not overlap inputs.  With phi_shared = 1 a mask gradient has ONE
 * mask's shape and holds the sum over the batch, taken n = 0 .. bsz-1 in that order by the lane that owns the element (deterministic).
 *
 * G1  the backward of K3 in one launch.  g (bsz,H,W,B) is the gradient of z1; with fb = sum_b z_b Phi_b, q = sum_b g_b Phi_b (both
 *     formed as K3 forms fb), r = (y - fb) / Phi_sum, t = q / Phi_sum, every operation rounded separately:
 *         gphi_b = r g_b - t z_b     gs = -(t r)     gz_b = g_b - t Phi_b     gy = t
 *     gphi (nm,H,W,B) and gs (nm,H,W) with nm = 1 for a shared mask, else bsz; gz (bsz,H,W,B) and gy (bsz,H,W) per measurement.
 *     Each output pointer may be NULL (that output is skipped); all four NULL is DEQSCI_ERR_NULL. */
int deqsci_gap_update_grad_f32(const float* z, const float* phi, const float* g, const float* y, const float* phisum,
                               float* gphi, float* gs, float* gz, float* gy,
                               int64_t bsz, int64_t H, int64_t W, int64_t B,
                               int layout, int phi_shared, deqsci_stream_t stream);

/* G2  gphi_b = a v_b, a (bsz,H,W), v (bsz,H,W,B): the mask gradient of K1 (a = grad y, v = x) and of K2 (a = y, v = grad x). */
int deqsci_sci_mask_grad_f32(const float* a, const float* v, float* gphi,
                             int64_t bsz, int64_t H, int64_t W, int64_t B,
                             int layout, int phi_shared, deqsci_stream_t stream);

/* G3  the backward of O4: gphi_b = gs where sum_b Phi_b != 0 and 0 where O4 wrote 1 (the sum is formed again in O4's order). */
int deqsci_phi_sum_grad_f32(const float* phi, const float* gs, float* gphi,
                            int64_t nb, int64_t H, int64_t W, int64_t B,
                            int layout, deqsci_stream_t stream);

/* (bsz,H,W,B) <-> (bsz,B,H,W) through an LDS tile; `to_layout` is the layout of `out`. */
int deqsci_transpose_f32(const float* in, float* out,
                         int64_t bsz, int64_t H, int64_t W, int64_t B,
                         int to_layout, deqsci_stream_t stream);

/* K4b out = z1 - noise, z1 and noise planar (BHW), out in layout_out
 *     replaces `z - noise.view(bsz,c,w,h).permute(0,2,3,1)`, equilibrium_solvers_yaping.py:417,420. */
int deqsci_residual_out_f32(const float* z1, const float* noise, float* out,
                            int64_t bsz, int64_t H, int64_t W, int64_t B,
                            int layout_out, deqsci_stream_t stream);

/* ---- Anderson / Picard bookkeeping (solvers/new_equilibrium_utils_yaping.py:153-189, 213-222) ----
 * History buffers F_hist, G_hist are (bsz, m, N) with G = F - X kept instead of X
 * (X_i = F_i - G_i), N = H*W*B in whatever element order the caller iterates in.
 * `deqsci_anderson_chunks(bsz,N)` blocks per sample each emit DEQSCI_PART_STRIDE fp32 partial sums.
 */
int64_t deqsci_anderson_chunks(int64_t bsz, int64_t N);
size_t  deqsci_partials_bytes(int64_t bsz, int64_t N);           /* `partials` buffer            */
size_t  deqsci_gram_bytes(int64_t bsz);                          /* persistent fp64 Gram + norms + arrival
                                                                    ticket; ZERO it once before first use */

/* K4  F_k = z1 - noise (noise may be NULL: F_k = z1);  G_k = F_k - x_cur;  store both into history
 *     slot `slot`; optionally x_next = F_k; per-block partial sums of <G_k,G_j> for j < n_filled and
 *     of |F_k|^2.  replaces :163/:183 stores, the G rows of :177 and the two norms of :184. */
int deqsci_residual_store_f32(const float* z1, const float* noise, const float* x_cur,
                              float* F_hist, float* G_hist, float* x_next, float* partials,
                              int64_t bsz, int64_t N, int m, int slot, int n_filled,
                              deqsci_stream_t stream);

/* K5+K6  finish the reduction (fp64), refresh row/column `slot` of the persistent Gram matrix,
 *     solve the bordered (n+1)x(n+1) system [[0,1^T],[1,GG^T+lam I]] [nu;alpha] = e0 by LU with
 *     partial pivoting, one wavefront per sample, and emit the relative residual
 *     res[0] = |G_k| / (eps + |F_k|) over the whole batch (reference semantics, :184) and
 *     res[1+s] per sample.  replaces torch.bmm + torch.solve + 2x .item() at :178-184.
 *     n = 0 skips the solve (ramp-up / Picard).  alpha is (bsz, DEQSCI_MAX_M). */
int deqsci_anderson_solve_f32(const float* partials, void* gram, float* alpha, float* res,
                              int64_t bsz, int64_t N, int m, int slot, int n_filled, int n,
                              float lam, float eps, deqsci_stream_t stream);

/* The same with the REFERENCE's arithmetic for alpha: gram32 = the n x n block G G^T of the first n history rows as the caller's fp32
 *     GEMM produced it ((bsz, n, n) row-major, rows in slot order: torch.bmm(G[:, :n], G[:, :n]^T), :178), the bordered system formed
 *     and factorised in fp32 (torch.solve = sgesv, :180).  The relative residual still comes from the exact sums.  gram32 NULL = the
 *     entry point above.  Why it exists: DESIGN.md section 5, "Config 2" - the ~5e-6 rounding error of that GEMM at N = 2^19 is worth
 *     +0.02 dB on the reference's 180-iteration FFDNet ensemble. */
int deqsci_anderson_solve_gram_f32(const float* partials, void* gram, float* alpha, float* res,
                                   int64_t bsz, int64_t N, int m, int slot, int n_filled, int n,
                                   float lam, float eps, const float* gram32, deqsci_stream_t stream);

/* The same WITHOUT a GEMM library (anderson_arith = "reference" of the engine and of the drop-in DEQFixedPoint): the new row of G G^T in the
 *     summation order of the fp32 torch.bmm behind tests/golden (MKL sgemm for 5 x N times N x 5: sixteen interleaved fused-multiply-add
 *     chains per entry, chain c over k = c, c + 16, ..., summed pairwise at the end; within one ulp of torch.bmm, tools/gram_on_real_history.py).
 *     On the loop's heavy-tailed residuals that order ABSORBS the small products of a 2^15-step chain: the diagonal comes out 3-7e-6 too small -
 *     a bias, and the thing that moves the reference's chaotic FFDNet ensembles (an unbiased fp32 sum of the same error size
 *     does not).  G_hist = the history K4 wrote (bsz, m, N), partials = K4's block sums of the same call; ref_state = deqsci_gram_ref_bytes(bsz, N)
 *     bytes, caller-owned, 16-byte aligned, ZEROED once and then left alone between calls (it carries the MAX_M x MAX_M fp32 Gram of each sample:
 *     row / column `slot` is refreshed per call, the other rows are what a deterministic GEMM would recompute bit for bit).
 *     deqsci_gram_row_chain16_f32 computes the 16 chain sums of every entry <G_slot, G_j>, j < n_filled, into ref_state: serial = 1 runs the chains
 *     as they are written (N / 16 dependent FMAs, ~220 us at N = 2^19); serial = 0 produces THE SAME BITS in two passes - inside one binade of the
 *     running sum a chain step is S + RN_ulp(p), an integer sum that any number of workgroups can form in any order; only the binade crossings are
 *     walked term by term (csrc/anderson.hip) - and falls back to serial = 1 where N % 4 != 0.  deqsci_anderson_solve_ref_f32 = that (serial = 0),
 *     then the bordered system formed and factorised in fp32 (:180, sgesv); residuals and the float64 Gram of `gram` as by the entry points above. */
size_t deqsci_gram_ref_bytes(int64_t bsz, int64_t N);
int deqsci_gram_row_chain16_f32(const float* G_hist, const float* partials, float* ref_state,
                                int64_t bsz, int64_t N, int m, int slot, int n_filled, int serial,
                                deqsci_stream_t stream);
int deqsci_anderson_solve_ref_f32(const float* G_hist, const float* partials, float* ref_state, void* gram, float* alpha, float* res,
                                  int64_t bsz, int64_t N, int m, int slot, int n_filled, int n,
                                  float lam, float eps, deqsci_stream_t stream);

/* (round 6) K4 and the first of those two passes in ONE launch: deqsci_residual_store_ref_f32 = deqsci_residual_store_f32 (same F / G / x_next, the
 *     same block sums in `partials`, bit for bit) whose blocks also leave the records of deqsci_gram_row_chain16_f32's first pass in ref_state - the
 *     history rows are in the block's registers anyway; the binade a block rounds for comes from its predecessors' block sums, which the blocks
 *     publish to one another inside the launch (csrc/anderson.hip: residual_store_round_kernel).  Only where deqsci_gram_ref_fusable(bsz, N) = 1
 *     (blocks of 2048 elements - N bsz <= 2^25 -, N a whole number of at most 256 of them: 256 x 256 x 8 is exactly that), DEQSCI_ERR_UNSUPPORTED otherwise - then the caller uses the two
 *     entry points above.  deqsci_anderson_apply_solve_ref_f32 = deqsci_anderson_solve_ref_f32 without that first pass: it must follow a
 *     deqsci_residual_store_ref_f32 of the same call (same ref_state, slot, n_filled) on the same stream.  replaces :163,:177-184 like the pair above. */
int deqsci_gram_ref_fusable(int64_t bsz, int64_t N);
int deqsci_residual_store_ref_f32(const float* z1, const float* noise, const float* x_cur,
                                  float* F_hist, float* G_hist, float* x_next, float* partials, float* ref_state,
                                  int64_t bsz, int64_t N, int m, int slot, int n_filled, deqsci_stream_t stream);
int deqsci_anderson_apply_solve_ref_f32(const float* G_hist, const float* partials, float* ref_state, void* gram, float* alpha, float* res,
                                        int64_t bsz, int64_t N, int m, int slot, int n_filled, int n,
                                        float lam, float eps, deqsci_stream_t stream);

/* K7  x_out = beta * sum_i alpha_i F_i + (1-beta) * sum_i alpha_i X_i,  X_i = F_i - G_i   (:182) */
int deqsci_anderson_mix_f32(const float* F_hist, const float* G_hist, const float* alpha,
                            float* x_out, float beta, int n, int64_t bsz, int64_t N, int m,
                            deqsci_stream_t stream);

/* K7+K3  the mix above fused with the GAP projection of its result: writes x_out (the new
 *     iterate X_k, needed for G_k and as the value andersonexp returns) and z1 = GAP(x_out).
 *     History, phi, x_out and z1 all in `layout`. */
int deqsci_anderson_mix_gap_f32(const float* F_hist, const float* G_hist, const float* alpha,
                                float beta, int n, int m,
                                const float* phi, const float* y, const float* phisum,
                                float* x_out, float* z1,
                                int64_t bsz, int64_t H, int64_t W, int64_t B,
                                int layout, int phi_shared, deqsci_stream_t stream);

/* Denoiser epilogue: h = max(h + bias[c], 0) in place (relu = 0: bias only), h (n,c,hw) NCHW-contiguous or
 *     channels_last.  Fuses the BatchNorm(eval)+ReLU of networks/ffdnet/models.py:53-58 - folded into the
 *     preceding conv's weights plus this per-channel bias - into one pass instead of PyTorch's two. */
int deqsci_bias_relu_f32(float* h, const float* bias, int64_t n, int64_t c, int64_t hw,
                         int channels_last, int relu, deqsci_stream_t stream);

/* FFDNet tail: conv3x3(64 -> 4, pad 1, no bias) fused with `upsamplefeatures` (networks/ffdnet/functions.py:62-81,
 *     = pixel_shuffle 2).  h is the channels_last activation (n,H,W,64); w_packed is the (4,64,3,3) weight
 *     re-ordered [half(2)][tap(9)][cin(32)][cout(4)]; out is the planar (n,1,2H,2W) predicted-noise image.
 *     in_bias (64 floats, may be NULL): h is the previous layer's RAW conv output and max(h + in_bias[c], 0)
 *     (its folded BatchNorm bias + ReLU) is applied while the tile is staged - one activation sweep less. */
int deqsci_ffdnet_tail_f32(const float* h, const float* w_packed, const float* in_bias, float* out,
                           int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);

/* The same two stencils without the FFDNet layout layers - SimpleCNN's edge layers
 *     (networks/provable/model/SimpleCNN_models.py:43-57): conv3x3(64 -> 1) from a channels_last (n,H,W,64) activation to
 *     a planar (n,1,H,W) image (w_packed [half(2)][tap(9)][cin(32)], optional in_bias + ReLU on the way in), and
 *     conv3x3(1 -> 64) [+ ReLU] from a planar image to channels_last (w_packed [tap(9)][cout/4(16)][cout%4(4)]). */
int deqsci_conv3x3_c64_to_1_f32(const float* h, const float* w_packed, const float* in_bias, float* out,
                                int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);
int deqsci_conv3x3_c1_to_64_f32(const float* x, const float* w_packed, float* h,
                                int64_t n, int64_t H, int64_t W, int relu, deqsci_stream_t stream);

/* FFDNet head: `concatenate_input_noise_map` (networks/ffdnet/functions.py:16-53: sigma map + 2x2 pixel-unshuffle)
 *     + conv3x3(5 -> 64, pad 1, no bias) + ReLU.  x is the planar (n,1,2H,2W) image, sigma[i*sigma_stride] the noise
 *     level of image i (stride 0 = one value for all), w_packed the (64,5,3,3) weight re-ordered
 *     [ch*9+tap (45)][cout/4 (16)][cout%4 (4)]; h is written as the channels_last (n,H,W,64) activation. */
int deqsci_ffdnet_head_f32(const float* x, const float* w_packed, const float* sigma, int64_t sigma_stride,
                           float* h, int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);

/* conv3x3(64 -> 64, pad 1, stride 1) + per-channel bias + ReLU as Winograd F(2x2,3x3) on the fp32 matrix cores.
 *     x, y channels_last (n,H,W,64), x != y; u_packed = the (64,64,3,3) weight transformed U = G g G^T and ordered
 *     [cin chunk c (8)][xi (16)][wn (2)][q (4)][i (16)][j (2)][s (2)], cout = 32 wn + 16 j + i, cin = 8 c + 2 q + s
 *     (the kernel's MFMA lane order); bias (64, may be NULL); relu 0/1.
 *     The middle layers of FFDNet (networks/ffdnet/models.py:53-58, BatchNorm folded) and SimpleCNN. */
int deqsci_conv3x3_c64_winograd_f32(const float* x, const float* u_packed, const float* bias, float* y,
                                    int64_t n, int64_t H, int64_t W, int relu, deqsci_stream_t stream);

/* The same layer as Winograd F(4x4,3x3): 2.25 instead of 4 multiplications per output, the large-batch kernel (block tiles of
 *     16 x 32 output pixels, one persistent workgroup per CU: it wants >= ~2 block tiles per CU; small launches belong to the
 *     F(2x2,3x3) entry point above).  Same arguments; u_packed = U = G g G^T (6x6 per cout, cin) ordered
 *     [cin chunk c (8)][s (18)][rg (2)][cgp (2)][q (4)][i (16)][j (2)][ks (2)] with transform position (3 rg + s / 6, s % 6),
 *     cout = 32 cgp + 16 j + i, cin = 8 c + 2 q + ks.  Rounding ~1.2e-6 per layer (F(2x2,3x3): 2.1e-7). */
int deqsci_conv3x3_c64_winograd44_f32(const float* x, const float* u_packed, const float* bias, float* y,
                                      int64_t n, int64_t H, int64_t W, int relu, deqsci_stream_t stream);

/* The same kernel between the layers of a stack (FFDNet: 13 of them in a row): activations in "blk32" instead of channels_last -
 *     [n][channel chunk (8)][H][ceil(W/32)][32][8]: planes of 8 channels; inside every block of 32 columns, column m at position
 *     8 ((m+1) & 3) + ((m+1) >> 2) - ((m+1) & 3 == 0), i.e. in the order the kernel stages them (its input fetch becomes two
 *     contiguous 512-byte runs per pixel row, its output stores 256 contiguous bytes per tile row).  in_layout / out_layout:
 *     DEQSCI_ACT_NHWC or DEQSCI_ACT_BLK32, independently (first layer NHWC -> BLK32, last BLK32 -> NHWC); the blk32 buffer holds
 *     n * 8 * H * ceil(W/32) * 256 floats, columns >= W are never read or written.  start_event / stop_event: both NULL, or both
 *     raw hipEvent_t handles that receive the dispatch's begin / end (measurement). */
#define DEQSCI_ACT_NHWC 0
#define DEQSCI_ACT_BLK32 1
int deqsci_conv3x3_c64_winograd44_layout_f32(const float* x, const float* u_packed, const float* bias, float* y,
                                             int64_t n, int64_t H, int64_t W, int relu, int in_layout, int out_layout,
                                             deqsci_stream_t stream, void* start_event, void* stop_event);

/* ---- the same layer as a DIRECT convolution on the f16 matrix cores with fp32-class accuracy (csrc/conv_s16.hip): every operand
 *     is two fp16 pieces (x = hi + lo, 22 significant bits), three f16 MFMAs per product (w_hi x_hi + w_lo x_hi + w_hi x_lo), fp32
 *     accumulation.  x_sp16: the activation as [n][4 cin chunks][2 pieces: hi, lo][2 blocks of 8 channels][H][W][8 halfs] holding
 *     2^e x.  w_packed: 2^w_exp w as [4 chunks][9 taps][2 pieces][2 cout groups of 32][64 lanes][8 halfs] (cout = 32 g + lane % 32,
 *     cin = 16 c + 8 (lane / 32) + j), w_exp the power of two that puts max |w| into [2^13, 2^14).
 *
 *     RANGES.  fp32 (the reference's arithmetic, solvers/equilibrium_solvers_yaping.py:397-420) is scale-free, fp16 is not, so the
 *     exponent e of an sp16 activation follows the data - PER IMAGE of the batch, so that one measurement's result never depends on what
 *     else is in the batch.  Every sp16 activation is described by a pair (amax, exp): `amax` a DEVICE pointer to n floats, amax[i] =
 *     max |x| of image i of that activation - then e(i) = DEQSCI_SP16_TARGET_EXP - floor(log2(amax[i])), i.e. 2^e max|x| in
 *     [2^11, 2^12), derived identically by the kernel that writes the activation and the kernel that reads it - or NULL: the fixed
 *     exponent `exp` for every image (DEQSCI_SP16_DEFAULT_EXP = 8 suits activations of a few units).  `track_amax` (may be NULL): a MEASURING launch - the same arithmetic,
 *     but max |y| of image i of the output is folded into track_amax[i] (n floats; zero them first) and, for the 64->64 layer, y itself
 *     is not written: run a layer once with track_amax = the slots of its output, then again with out_amax = those slots.  Nothing crosses to the host: a captured hipGraph follows
 *     its inputs.  An activation that outgrows fp16 (16 x the measured maximum) becomes inf, never a silently wrong finite number.
 *
 *     Output = relu?(conv + bias): out_f32 = 0 -> sp16 with the range (out_amax, out_exp); out_f32 = 1 -> fp32 channels_last
 *     (n,H,W,64).  Images up to 2^31 / 256 - 33 pixels.  start_event / stop_event: both NULL, or both raw hipEvent_t handles. */
#define DEQSCI_SP16_DEFAULT_EXP 8
#define DEQSCI_SP16_TARGET_EXP 11
int deqsci_conv3x3_c64_split16(const void* x_sp16, const void* w_packed, const float* bias, void* y,
                               int64_t n, int64_t H, int64_t W, int relu, int w_exp, const float* in_amax, int in_exp,
                               const float* out_amax, int out_exp, float* track_amax, int out_f32,
                               deqsci_stream_t stream, void* start_event, void* stop_event);
/* A RUN of n_layers such layers (the denoisers' 13 / 2 middle layers, each feeding the next) in ONE launch: the kernel's persistent
 *     workgroups walk their tiles layer after layer with DATAFLOW synchronisation instead of kernel boundaries - a tile of layer l + 1
 *     waits for layer l of itself and its eight neighbour tiles only (one progress word per tile, agent-scope atomics; activations
 *     stored write-through and fetched with agent-scope loads - no cache maintenance, no grid-wide barrier).  Bit-identical to n_layers
 *     single launches.  Two things it buys: at one measurement per call (8 images of 128 x 128 = one tile per CU, the reference's
 *     usage) the kernel boundary that cost a fifth of a layer; and at any batch size a SLICE of the batch whose activations fit the
 *     Infinity Cache (n x H x W x 256 bytes <= 128 MiB: 32 images of 128 x 128) runs all its layers back to back out of that cache -
 *     the caller slices the batch (pointers into it, range_stride = the batch's images) and launches slice after slice.
 *     layers: DEVICE table of n_layers x { const void* w_packed; const float* bias (may be NULL); int32 w_exp; int32 relu } (24 bytes
 *     each).  Layer l reads x_sp16 (l = 0) or the buffer layer l - 1 wrote, and writes y_even (l even) / y_odd (l odd); all sp16,
 *     none aliasing another.  ranges: n_layers + 1 rows of range slots, range_stride (>= n) floats apart - ranges[l * range_stride + i]
 *     = max |image i of the input of layer l|; NULL: the input holds 2^in_exp x, every output 2^out_exp y.
 *     flags: 32 (n_tiles + 1) 32-bit DEVICE words (n_tiles = n ceil(H/16) ceil(W/32); tile t's word is flags[32 t], a 128-byte line
 *     each), zeroed ONCE by the caller and then left alone: the progress words count on from launch to launch (launches of one shape
 *     may share them when they run one after the other; another shape needs its own).  flags[32 n_tiles] != 0 after a launch = a wait
 *     timed out - a workgroup of the launch was not resident, i.e. somebody else holds CUs of this device - and the output of that
 *     launch is invalid; the launch never hangs, and later launches on the same words do not wait at all (zero the words to rearm).
 *     THE RESIDENCY / TIME-OUT CONTRACT (this launch and deqsci_conv3x3_c64_wino16_stack): the workgroups of a launch wait for ONE ANOTHER, so all
 *     of them must be resident at once.  The launcher asks for min(n_tiles, CUs) workgroups, one per CU by their LDS footprint, after an
 *     occupancy query (DEQSCI_ERR_UNSUPPORTED if the kernel cannot be resident at all on this device) - which holds when the device's CUs
 *     are the caller's: no CU mask, no other process, no concurrent kernel of another stream holding CUs for the length of the launch.  It
 *     is NOT enforced by the hardware queue (no cooperative launch: those cannot be captured into a hipGraph).  A caller who cannot
 *     promise it must read flags[32 n_tiles] after the launch (the Python launchers do, and raise; DEQSCIEngine reads it after the first
 *     stack f-call of a reconstruction and at its end, redoes the call with one launch per layer and stays there for 16 calls) - a
 *     waiting workgroup gives up after ~0.25 s, so a broken promise costs time and an invalid output that says so, never a hang. */
int deqsci_conv3x3_c64_split16_stack(const void* x_sp16, void* y_even, void* y_odd, const void* layers, int n_layers,
                                     int64_t n, int64_t H, int64_t W, const float* ranges, int64_t range_stride, int in_exp, int out_exp,
                                     void* flags, deqsci_stream_t stream, void* start_event, void* stop_event);
/* ---- the same layer with a third fewer matrix-core products (csrc/conv_w16.hip): the split-fp16 arithmetic under Winograd F(2,3) ALONG X
 *     nested in the direct sum ALONG Y - per tap row dy and position xi = 0..3 the weights U[dy][xi] = G g[dy][.] (G of F(2,3), formed in
 *     float64 by the caller), the input transform B^T d of every halo row in the kernel (fp32, then hi + lo), ONE fp32 accumulation chain of
 *     36 MFMAs per position, y[2t] = M0 + M1 + M2, y[2t+1] = M1 - M2 - M3.  18 f16 MFMA products per output and (cin, cout) instead of 27;
 *     per layer against float64 on FFDNet's own data the same 1.3e-7 as the direct kernel (tools/wino16_numerics.py).
 *     Replaces nn.Conv2d(64,64,3,padding=1) + BatchNorm(eval) + ReLU, networks/ffdnet/models.py:53-58 (the 13 middle layers :46-64).
 *     u_packed: 2^w_exp U as [4 cin chunks][2 xi halves][2 xi'][3 dy][2 pieces: hi, lo][2 cout groups of 32][64 lanes][8 halfs]
 *     (xi = 2 half + xi', cout = 32 g + lane % 32, cin = 16 c + 8 (lane / 32) + j), w_exp the power of two that puts max |U| into [2^13, 2^14).
 *     Activations x, y in "p32": the 16 planes of 16-byte pixels of sp16 holding 2^e x as fp32 instead of hi + lo fp16 -
 *     [n][8 blocks of 8 channels][2 halves of 4][H][ceil(W/64) column blocks][2 column parities][32][4 floats]: plane 2 b8 + j = channels
 *     8 b8 + 4 j .. + 3, a row is 64 ceil(W/64) pixels long (the tail of the last block is padding nobody reads), and inside a block of 64
 *     columns the 32 EVEN columns come first, then the 32 odd ones - an F(2,3) tile pair reads and writes whole 128-byte lines (nothing to
 *     join in front of the transform, nothing to split behind the output transform); FFDNet's first and last layer write / read it
 *     (deqsci_ffdnet_head_p32, deqsci_ffdnet_tail_p32).  Ranges (in_amax, in_exp),
 *     (out_amax, out_exp): as for sp16 (B^T d is at most twice max |d|: the headroom against fp16's overflow is 8 x the measured maximum
 *     instead of 16 x).  Output = relu?(conv + bias).  Block tiles of 8 x 64 output pixels, one persistent 512-thread workgroup per CU
 *     (a wave = one output row x 64 couts; 148 KB of LDS). */
int deqsci_conv3x3_c64_wino16(const void* x_p32, const void* u_packed, const float* bias, void* y_p32,
                              int64_t n, int64_t H, int64_t W, int relu, int w_exp, const float* in_amax, int in_exp,
                              const float* out_amax, int out_exp,
                              deqsci_stream_t stream, void* start_event, void* stop_event);
/* A RUN of n_layers such layers in ONE launch: deqsci_conv3x3_c64_split16_stack's contract word for word (layer table, ranges, progress
 *     words, time-out word, residency: never more workgroups than CUs, each of them alone on its CU by its LDS footprint), with
 *     n_tiles = n ceil(H/8) ceil(W/64) and every activation (x, y_even, y_odd) in p32. */
int deqsci_conv3x3_c64_wino16_stack(const void* x_p32, void* y_even, void* y_odd, const void* layers, int n_layers,
                                    int64_t n, int64_t H, int64_t W, const float* ranges, int64_t range_stride, int in_exp, int out_exp,
                                    void* flags, deqsci_stream_t stream, void* start_event, void* stop_event);
/* fp32 channels_last (n,H,W,64) -> sp16 with the range (amax, exp); and, for x = n images of `count` contiguous floats each, max |x| of
 *     image i folded into amax[i] (zero them first): the range of an activation no sp16-writing kernel produced (the denoiser's input
 *     image; a converted fp32 activation). */
int deqsci_f32_to_split16(const float* x_nhwc, void* y_sp16, int64_t n, int64_t H, int64_t W, const float* amax, int exp,
                          deqsci_stream_t stream);
int deqsci_absmax_f32(const float* x, int64_t n, int64_t count, float* amax, deqsci_stream_t stream);
/* SimpleCNN's first layer (conv3x3 1 -> 64 [+ ReLU], deqsci_conv3x3_c1_to_64_f32) writing sp16 with the range (out_amax, out_exp)
 *     instead of fp32 channels_last - no conversion pass in front of a run of split16 layers. */
int deqsci_conv3x3_c1_to_64_sp16(const float* x, const float* w_packed, void* h_sp16, int64_t n, int64_t H, int64_t W, int relu,
                                 const float* out_amax, int out_exp, float* track_amax, deqsci_stream_t stream);
/* ... and writing / reading p32 (in front of / behind a run of deqsci_conv3x3_c64_wino16 layers: SimpleCNN_models.py:43-45, 55-56). */
int deqsci_conv3x3_c1_to_64_p32(const float* x, const float* w_packed, void* h_p32, int64_t n, int64_t H, int64_t W, int relu,
                                const float* out_amax, int out_exp, float* track_amax, deqsci_stream_t stream);
int deqsci_conv3x3_c64_to_1_p32(const void* x_p32, const void* w_packed, float* out, int64_t n, int64_t H, int64_t W,
                                int w_exp, const float* in_amax, int in_exp, deqsci_stream_t stream);
/* The denoisers' last layers (conv3x3 64 -> 4 + pixel shuffle / 64 -> 1, no bias) on the f16 matrix cores with the split-fp16 arithmetic of
 *     deqsci_conv3x3_c64_split16: the 9 taps ride in the matrix N dimension (column = COUT tap + cout), the per-tap products are summed from
 *     LDS.  w_packed: 2^w_exp w as [4 chunks][2 pieces][N tiles][64 lanes][8 halfs]; the input's range is (in_amax, in_exp); fp32 out. */
int deqsci_ffdnet_tail_split16(const void* x_sp16, const void* w_packed, float* out, int64_t n, int64_t H, int64_t W,
                               int w_exp, const float* in_amax, int in_exp, deqsci_stream_t stream);
int deqsci_conv3x3_c64_to_1_split16(const void* x_sp16, const void* w_packed, float* out, int64_t n, int64_t H, int64_t W,
                                    int w_exp, const float* in_amax, int in_exp, deqsci_stream_t stream);
/* FFDNet's first layer (sigma map + pixel-unshuffle + conv3x3 5 -> 64 + ReLU) likewise, writing sp16: K = 45 taps padded to 48, the
 *     activation operand gathered from the image and split on the fly at 2^e_in, e_in(i) from max(in_amax[i], sigma(i)) (in_amax[i] =
 *     max |x| of image i; NULL: in_exp).  w_packed: 2^w_exp w as [3 k steps][2 pieces][2 cout groups][64 lanes][8 halfs], k = 9 ch + tap. */
int deqsci_ffdnet_head_split16(const float* x, const void* w_packed, const float* sigma, int64_t sigma_stride, void* h_sp16,
                               int64_t n, int64_t H, int64_t W, int w_exp, const float* in_amax, int in_exp,
                               const float* out_amax, int out_exp, float* track_amax, deqsci_stream_t stream);

/* FFDNet's first and last layer in front of / behind a run of deqsci_conv3x3_c64_wino16 layers: the entry points above writing / reading
 *     "p32" instead of sp16 (the same planes and ranges, 2^e x unsplit as fp32, the columns of every block of 64 with the parities apart:
 *     see deqsci_conv3x3_c64_wino16).  Same weights (w_packed of deqsci_ffdnet_head_split16 / deqsci_ffdnet_tail_split16), same
 *     arithmetic; the tail splits its operand into hi + lo on the fly.  networks/ffdnet/models.py:46-64, functions.py:16-81. */
int deqsci_ffdnet_head_p32(const float* x, const void* w_packed, const float* sigma, int64_t sigma_stride, void* h_p32,
                           int64_t n, int64_t H, int64_t W, int w_exp, const float* in_amax, int in_exp,
                           const float* out_amax, int out_exp, deqsci_stream_t stream);
int deqsci_ffdnet_tail_p32(const void* x_p32, const void* w_packed, float* out, int64_t n, int64_t H, int64_t W,
                           int w_exp, const float* in_amax, int in_exp, deqsci_stream_t stream);

/* ---- evaluation metric (not on the reconstruction path) ----
 * S1+S2  per-frame mean SSIM of x against y (pytorch_ssim._ssim of the reference: Gaussian window `window`, sigma 1.5, zero
 *     padding of window/2, C1 = 0.01^2, C2 = 0.03^2), one float64 per (measurement, frame): out is (M, B), out[m*B + f].
 *     x and y are (M,H,W,B) (layout HWB) or (M,B,H,W) (layout BHW), fp32, 4-byte aligned; out and workspace 8-byte aligned.
 *     window: odd, 3..15.  valid = 0: mean over all H*W map values ("same", the reference's size_average); valid = 1: mean over
 *     the (H-window+1) x (W-window+1) map values whose window lies inside the image (-2 if there are none).  clamp_x != 0: x is
 *     clamped to [0,1] on load (NaN kept).  A NaN in a frame makes that frame's value NaN.  Deterministic (fixed summation
 *     order, no atomics).  M = 0 or B = 0: nothing is launched.  workspace = deqsci_ssim_workspace_bytes(...) bytes, no
 *     initialisation needed; out and workspace must not overlap x, y or each other (-4).  The workspace query returns
 *     DEQSCI_ERR_* (< 0) for invalid sizes or layout. */
int64_t deqsci_ssim_workspace_bytes(int64_t M, int64_t H, int64_t W, int64_t B, int layout);
int deqsci_ssim_f32(const float* x, const float* y, double* out, int64_t M, int64_t H, int64_t W, int64_t B,
                    int layout, int window, int valid, int clamp_x, void* workspace, deqsci_stream_t stream);

/* Q1+Q2  per-sample squared error of an iterate against the ground truth, the numerator of the per-f-call PSNR trace
 *     (harness.psnr's arithmetic): out[s] = sum_i (clamp(x[s,i]) - gt[s,i])^2, the difference and the square in fp32, the sum
 *     in float64.  x: bsz rows of N fp32, row s at x + s * x_stride (x_stride >= N, in elements: the engine passes a slot of the
 *     Anderson history, F_hist + slot * N with x_stride = m * N); gt (bsz, N) dense; both 4-byte aligned (rows that are both
 *     16-byte aligned are read as float4, the others element by element, in the SAME summation order).  out (bsz) float64 and
 *     workspace 8-byte aligned.  clamp_x != 0: x is clamped to [0,1] on load (NaN kept).  A NaN in a sample makes that sample's
 *     value NaN, no other's.  Deterministic (two stages, fixed summation order, no atomics).  bsz = 0 or N = 0: nothing is
 *     launched.  bsz <= 65535.  workspace = deqsci_sqerr_workspace_bytes(bsz, N) bytes (0 for invalid sizes), no
 *     initialisation needed.  Two launches on `stream`; no allocation, no host synchronisation, graph-capturable. */
size_t deqsci_sqerr_workspace_bytes(int64_t bsz, int64_t N);
int deqsci_sqerr_rows_f32(const float* x, const float* gt, double* out, int64_t bsz, int64_t N, int64_t x_stride, int clamp_x,
                          void* workspace, deqsci_stream_t stream);

/* ---- GAP-TV: a classical baseline and the DEQ's other starting point (not on the DEQ's path) ----
 * T0-T3  the reference's GAP_TV_rec (utils/cg_utils.py:207-224) with scikit-image 0.17.2's denoise_tv_chambolle
 *     (multichannel, each frame a (1,H,W) channel: tau = 1/6), per measurement - a batch of bsz measurements gives what bsz calls
 *     of one give, bit for bit.  y (bsz,H,W), Phi (bsz,H,W,B) or (1,H,W,B) when phi_shared != 0, Phi_sum (bsz,H,W) or (1,H,W):
 *     fp32, 4-byte aligned; out (bsz,H,W,B) fp32.  maxiter GAP iterations of step `step`, each followed by at most n_iter_max
 *     Chambolle iterations of weight `weight` that stop early when |E_prev - E| < eps E_init.  State in fp64.  B <= 128.
 *     stop: NULL or (bsz, maxiter, B) int32, the Chambolle iteration each (measurement, GAP iteration, frame) stopped at, or
 *     n_iter_max if the early stop never fired.  maxiter = 0 returns At(y, Phi).  workspace = deqsci_gaptv_workspace_bytes(...)
 *     bytes, 16-byte aligned, no initialisation needed; out, stop and workspace must not overlap the inputs or each other (-4).
 *     Launches 2 + maxiter (1 + n_iter_max) kernels and one memset on `stream`; no host synchronisation.
 * T0,T2,T3  deqsci_tv_chambolle_f32: the Chambolle denoiser alone on n planes image (n,H,W) fp32 -> out (n,H,W) fp32 with an
 *     explicit tau (1/4 for a 2-D array, 1/6 for a (1,H,W) channel); stop NULL or (n,) int32 as above.  The workspace queries
 *     return DEQSCI_ERR_* (< 0) for invalid sizes. */
int64_t deqsci_gaptv_workspace_bytes(int64_t bsz, int64_t H, int64_t W, int64_t B);
int deqsci_gaptv_f32(const float* y, const float* phi, const float* phi_sum, float* out, int64_t bsz, int64_t H, int64_t W,
                     int64_t B, int phi_shared, int maxiter, double step, double weight, double eps, int n_iter_max, int* stop,
                     void* workspace, deqsci_stream_t stream);
int64_t deqsci_tv_chambolle_workspace_bytes(int64_t n, int64_t H, int64_t W);
int deqsci_tv_chambolle_f32(const float* image, float* out, int64_t n, int64_t H, int64_t W, double weight, double eps,
                            int n_iter_max, double tau, int* stop, void* workspace, deqsci_stream_t stream);

/* ---- the DEQ's implicit backward on the device (not on the reconstruction path) ----
 * The hook of the training forward (solvers/new_equilibrium_utils_yaping.py:273-276) solves g = J_f(z0)^T g + grad, and every
 * J_f^T v = P (v - J_D(z1)^T v) (P = the GAP projection with y = 0, deqsci_gap_update_f32).  J_D^T v of a conv [+BN] + ReLU stack
 * runs the layers backwards with the weights transposed and flipped (BN folded into the scale, no bias), each ReLU replaced by
 * the unit's mask from ONE forward pass at z1: v -> conv3x3(1 -> 64) * mask -> [conv3x3(64 -> 64) * mask] ... ->
 * conv3x3(64 -> 1) (deqsci_conv3x3_c64_to_1_f32 with in_bias NULL).  The masks do not change between the hook's iterations.
 * Same conventions as above: device pointers, caller-owned buffers, no allocation, no host synchronisation, graph-capturable.
 *
 * V0  mask (n_pixels) uint64, 8-byte aligned: bit c of mask[p] = (a[p*64 + c] > 0) for the fp32 channels_last activation a
 *     (n_pixels, 64), 4-byte aligned - ReLU'(0) = 0 as in PyTorch: +-0.0 and NaN give 0.  n_pixels = 0: nothing is launched.
 * V1  the 64 -> 64 layer of deqsci_conv3x3_c64_winograd_f32 (Winograd F(2x2,3x3): same x, u_packed, y, sizes and limits;
 *     channels_last in and out) with output = conv3x3(x) * mask instead of relu(conv3x3(x) + bias): no bias, no ReLU, the mask
 *     (n*H*W words, pixel order of y) as written by V0; 8-byte aligned.  Scale-free fp32 arithmetic: the VJP's inputs change scale
 *     from one iteration to the next.  (F(4x4,3x3) has no masked form: at its 256-register limit the mask reads spill.)
 * V2  the same epilogue on deqsci_conv3x3_c1_to_64_f32: h = conv3x3(x) * mask, x planar (n,1,H,W), h channels_last (n,H,W,64). */
int deqsci_relu_mask_pack_f32(const float* a, uint64_t* mask, int64_t n_pixels, deqsci_stream_t stream);
int deqsci_conv3x3_c64_winograd_masked_f32(const float* x, const float* u_packed, const uint64_t* mask, float* y,
                                           int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);
int deqsci_conv3x3_c1_to_64_masked_f32(const float* x, const float* w_packed, const uint64_t* mask, float* h,
                                       int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);

/* ---- Jacobian diagnostics (deqsci_amd/jacobian.py: the local Lipschitz constant and the spectral radius of f at a point) ----
 * J1  FFDNet's first layer without its sigma channel, bias and ReLU, masked: h = conv3x3(pixel_unshuffle_2(x)) * mask.  x planar
 *     (n,1,2H,2W), w_packed the (64,4,3,3) weight packed as deqsci_ffdnet_head_f32's is but over 36 rows ([ch*9+tap][cout/4][cout%4]),
 *     mask the words of V0 in the pixel order of h (8-byte aligned), h channels_last (n,H,W,64), 16-byte aligned.  With the forward
 *     weights of image channels 1..4 and the first ReLU's mask: the linearised first layer; with the last layer's weight transposed
 *     and flipped and the last ReLU's mask: the transpose of the last layer.  (The other two edge products are
 *     deqsci_ffdnet_tail_f32 with in_bias = NULL.)  Scale-free fp32 arithmetic.
 * J2  one step of a power iteration, per sample: a = |w|^2 and b = <v_prev, w> with float64 products and sums, (a, b) written to
 *     table_row[2 s], table_row[2 s + 1] (the caller passes the row of the current iteration of its float64 table), and
 *     v_out = w / sqrt(a).  a zero or not finite: v_out = 0 and (NaN, NaN) in the table.  v_prev may be NULL (b = NaN); v_out may be
 *     w or v_prev.  w, v_prev, v_out (bsz,N) dense fp32, 4-byte aligned; table_row and workspace 8-byte aligned.  Deterministic
 *     (two stages, fixed summation order, no atomics).  bsz = 0 or N = 0: nothing is launched.  bsz <= 65535.  workspace =
 *     deqsci_power_workspace_bytes(bsz, N) bytes (0 for invalid sizes), no initialisation needed.  Two launches on `stream`; no
 *     allocation, no host synchronisation, graph-capturable. */
int deqsci_ffdnet_head_masked_f32(const float* x, const float* w_packed, const uint64_t* mask, float* h,
                                  int64_t n, int64_t H, int64_t W, deqsci_stream_t stream);
size_t deqsci_power_workspace_bytes(int64_t bsz, int64_t N);
int deqsci_power_step_f32(const float* w, const float* v_prev, float* v_out, double* table_row, int64_t bsz, int64_t N,
                          void* workspace, deqsci_stream_t stream);

/* ---- Broyden's method for g(x) = f(x) - x = 0 (deqsci_amd/broyden.py; the reference's solvers/broyd_equilibrium_utils.py:117-181) ----
 * The history is two planar buffers U, V (bsz, L, N) fp32 with contiguous rows (the reference's Us, VTs), L <= DEQSCI_BROYDEN_MAX_L;
 * dx (the update just taken), gx_old, gx_new, x, x_next, update are (bsz, N) dense fp32.  `table` holds
 * DEQSCI_BROYDEN_TABLE_STRIDE doubles per sample: a_j = <dx, U_j> at [j], b_j = <V_j, dg> at [27 + j], c_j = <V_j, gx_new> at [54 + j]
 * (j < t; the other entries are left alone), |gx_new|^2 at [81], d = <vT, dg> at [82], c_new = <vT, gx_new> at [83]; dg = gx_new - gx_old
 * in fp32, never stored.  workspace = deqsci_broyden_workspace_bytes(bsz, N, L) bytes (0 for invalid sizes), no initialisation needed;
 * deqsci_broyden_chunk() = the elements of a row one workgroup sums.  fp32 pointers 4-byte aligned (float4 accesses where every
 * pointer is 16-byte aligned and N a multiple of 4; the results do not depend on it), table and workspace 8-byte aligned.
 * B1+B2 deqsci_broyden_dots_f32: a_j, b_j, c_j for the t filled rows and |gx_new|^2, float64 products and sums in a fixed two-stage
 *     order -> table.  Two launches.  t = 0 with dx = gx_old = gx_new: just the squared norm.
 * B3+B4 deqsci_broyden_update_f32 (after B1+B2 with the same arguments): vT = -dx + sum_j a_j V_j -> V[slot] (NaN -> 0),
 *     w = dx - (sum_j b_j U_j - dg), U[slot] = w / d (fp32 division, NaN -> 0), d and c_new in float64 from vT before its NaNs are
 *     zeroed -> table, update = gx_new - sum_j c_j U_j over the rows j < max(t, slot + 1) in ascending j with the new row in its place
 *     (a row it replaces, slot < t, does not contribute), x_next = x + update when x_next is given.  The coefficients are rounded to fp32
 *     once, the combinations summed in fp32.  slot == t (the history fills) or slot < t == L (it wraps).  update may be dx or gx_new,
 *     x_next may be x; none of the rows may overlap U or V.  Two launches.
 * No allocation, no host synchronisation, no atomics: graph-capturable and deterministic, and a sample's results do not depend on the
 * rest of the batch.  NULL -> -1; bsz <= 0, N <= 0, L < 1, L > 27, t > L, slot >= L, slot > t, slot < t < L -> -2; misaligned -> -3; bsz > 65535,
 * N > 2^28, aliasing with the history -> -4. */
#define DEQSCI_BROYDEN_MAX_L 27
#define DEQSCI_BROYDEN_TABLE_STRIDE 84
int64_t deqsci_broyden_chunk(void);
size_t deqsci_broyden_workspace_bytes(int64_t bsz, int64_t N, int L);
int deqsci_broyden_dots_f32(const float* U, const float* V, const float* dx, const float* gx_old, const float* gx_new, double* table,
                            void* workspace, int64_t bsz, int64_t N, int L, int t, deqsci_stream_t stream);
int deqsci_broyden_update_f32(float* U, float* V, const float* dx, const float* gx_old, const float* gx_new, const float* x, float* x_next,
                              float* update, double* table, void* workspace, int64_t bsz, int64_t N, int L, int t, int slot,
                              deqsci_stream_t stream);

/* ---- The vector epsilon-algorithm, Aitken's delta-squared extrapolation of x, f(x), f(f(x)) (deqsci_amd/epsilon2.py; the reference's
 * solvers/new_equilibrium_utils_yaping.py:194-211, epsilon2) ----
 * x, f_x, f_fx, x_new are (bsz, N) dense fp32; dx = f_x - x, df = f_fx - f_x, d2 = df - dx are formed in fp32, never stored.  `table` holds
 * DEQSCI_EPSILON2_TABLE_STRIDE doubles per sample: sum dx^2 at [0], sum df^2 at [1], sum d2^2 (without lam) at [2], sum (x_new - x)^2 at [3]
 * (the difference rounded to fp32 first), sum x_new^2 at [4].  workspace = deqsci_epsilon2_workspace_bytes(bsz, N) bytes (0 for invalid
 * sizes), no initialisation needed; deqsci_epsilon2_chunk() = the elements of a row one workgroup sums.  fp32 pointers 4-byte aligned
 * (float4 accesses where every pointer is 16-byte aligned and N a multiple of 4; the results do not depend on it), table and workspace
 * 8-byte aligned.
 * E1+E2 deqsci_epsilon2_norms_f32: the three sums of squares, float64 products and sums in a fixed two-stage order -> table[s][0..2].
 *     Two launches.
 * E3+E2 deqsci_epsilon2_update_f32 (after E1+E2 with the same rows): a = fp32(table[s][0]), b = fp32(table[s][1]),
 *     c = fp32(table[s][2]) + lam (an fp32 sum), x_new = f_x + (df * a - dx * b) / c elementwise in fp32 with every operation rounded
 *     on its own, and the two sums of squares of the result -> table[s][3..4].  x_new may overlap none of x, f_x, f_fx (which may be one
 *     another).  Two launches.
 * No allocation, no host synchronisation, no atomics: graph-capturable and deterministic, and a sample's results do not depend on the
 * rest of the batch.  NULL -> -1; bsz <= 0, N <= 0, N > 2^28 -> -2; misaligned -> -3; bsz > 65535, x_new overlapping an input -> -4. */
#define DEQSCI_EPSILON2_TABLE_STRIDE 5
int64_t deqsci_epsilon2_chunk(void);
size_t deqsci_epsilon2_workspace_bytes(int64_t bsz, int64_t N);
int deqsci_epsilon2_norms_f32(const float* x, const float* f_x, const float* f_fx, double* table, void* workspace, int64_t bsz, int64_t N,
                              deqsci_stream_t stream);
int deqsci_epsilon2_update_f32(const float* x, const float* f_x, const float* f_fx, float* x_new, double* table, void* workspace,
                               int64_t bsz, int64_t N, float lam, deqsci_stream_t stream);

/* ---- the denoiser's weight gradients (deqsci_amd/vjp.py: DenoiserParamGrads; not on the reconstruction path) ----
 * The taped call z = f(z*) of the training forward hands autograd (df/dtheta)^T g; for a bias-free conv3x3 + ReLU stack that is one
 * weight gradient per convolution (torch's cross-correlation, pad 1: a tap outside the image contributes nothing - it is not multiplied,
 * so a NaN beside the border does not spread - and a row end or an image end never pairs with the next row or image).  All tensors fp32;
 * 64-channel activations channels_last (n,H,W,64), scalar images planar (n,1,H,W).
 * W0  dw[co][ci][ky][kx] = sum over img,h,w of g[img,h,w,co] * x[img,h+ky-1,w+kx-1,ci], dense (64,64,3,3): x the layer's input, g the
 *     gradient behind it (both 16-byte aligned).  Exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32): every product is rounded once
 *     and summed in an fp32 fma chain.
 * W1  576 outputs, dense (64,3,3) (= (64,1,3,3) and (1,64,3,3)), s a scalar image, t a 64-channel activation (4-byte aligned):
 *     flip = 0: dw[c][ky][kx] = sum_p t[p,c] * s[p+(ky-1,kx-1)]   (the first layer: s = the image, t = the gradient behind its ReLU)
 *     flip = 1: dw[c][ky][kx] = sum_p s[p] * t[p+(ky-1,kx-1),c]   (the last layer: s = the gradient of the noise, t = the last activation)
 * Both are two launches on `stream`: every workgroup of the first owns a fixed run of pixel tiles, accumulates in fp32 and adds its
 * accumulators to its float64 partial in the workspace at the latest every DEQSCI_WGRAD_CHAIN pixels (so no entry sums more than
 * DEQSCI_WGRAD_CHAIN products in fp32); the second sums the workgroups' partials per entry in float64, in ascending workgroup order, and
 * rounds once.  No atomics, no workgroup waits for another: deterministic bit for bit.  workspace =
 * deqsci_wgrad_workspace_bytes(n, H, W) bytes (0 for invalid sizes; serves both entries), 8-byte aligned, no initialisation needed.
 * No allocation, no host synchronisation, graph-capturable.  NULL -> -1; n < 1 or a non-positive side -> -2; misaligned -> -3; dw or
 * workspace overlapping an input or one another, flip other than 0 / 1, n or a side above 2^20 or n*H*ceil(W/32) >= 2^31 -> -4. */
#define DEQSCI_WGRAD_CHAIN 4096
size_t deqsci_wgrad_workspace_bytes(int64_t n, int64_t H, int64_t W);
int deqsci_wgrad3x3_c64_c64_f32(const float* x, const float* g, float* dw, int64_t n, int64_t H, int64_t W, void* workspace,
                                deqsci_stream_t stream);
int deqsci_wgrad3x3_c1_c64_f32(const float* s, const float* t, float* dw, int flip, int64_t n, int64_t H, int64_t W, void* workspace,
                               deqsci_stream_t stream);

/* ---- the same for a denoiser with a frozen (eval-mode) BatchNorm: FFDNet, conv + BN + ReLU DnCNN (csrc/wgrad_bn.hip).  The contract of W0 /
 * W1 above holds for both: fixed runs of tiles, fp32 accumulators, float64 partials at the latest every DEQSCI_WGRAD_CHAIN pixels, a summing
 * launch in ascending workgroup order that rounds once, deterministic bit for bit, no allocation, no host synchronisation, graph-capturable;
 * a tap outside the image and a pixel beyond a row's end are never multiplied.  workspace = deqsci_wgrad_bn_workspace_bytes(n, H, W) bytes for
 * (n,64,H,W) activations (0 for invalid sizes; serves both entries), 8-byte aligned, no initialisation needed.
 * W0-BN  a middle layer y = relu(scale[co] * conv(x, w) + shift): with R = W0's dw(x, g),
 *            dw[co][ci][ky][kx] = (float)(scale[co] * R),  dsum[co] = sum_p g[p,co],  ddot[co] = sum_{ci,ky,kx} w[co][ci][ky][kx] * R
 *        from W0's entry sums in float64, each rounded once (scale == 1: dw is W0's bit for bit).  x, g as for W0; w dense (64,64,3,3),
 *        scale, dsum, ddot 64 floats.  dbeta = dsum, dgamma = (ddot - mean * dsum) / sqrt(var + eps).
 * W2     FFDNet's edge layers, read through the 2x2 pixel-unshuffle u[p, 2i+j] = img[2h+i, 2w+j] of the planar (n,1,H,W) image (H, W the
 *        FULL-resolution sides; t is (n,64,H/2,W/2) channels_last; the workspace is that of (n, H/2, W/2)):
 *            which = 0: dw (64,5,3,3), dw[c][1+q][tap] = sum_p t[p,c] * u[p+d, q],  dw[c][0][tap] = sum_p sigma[img] * t[p,c] over the p with
 *                       p+d inside the half-resolution image (sigma: sigma_stride = 0 one float, = 1 n floats)
 *            which = 1: dw (4,64,3,3), dw[q][c][tap] = sum_p u[p, q] * t[p+d, c]  (sigma is not read and may be NULL)
 * NULL -> -1; n < 1, a non-positive or (W2) odd side -> -2; misaligned -> -3; an output or the workspace overlapping an input or one another,
 * which other than 0 / 1, sigma_stride other than 0 / 1, sizes beyond W0's limits -> -4. */
size_t deqsci_wgrad_bn_workspace_bytes(int64_t n, int64_t H, int64_t W);
int deqsci_wgrad3x3_c64_c64_bn_f32(const float* x, const float* g, const float* w, const float* scale, float* dw, float* dsum, float* ddot,
                                   int64_t n, int64_t H, int64_t W, void* workspace, deqsci_stream_t stream);
int deqsci_wgrad3x3_shuffle_f32(const float* img, const float* sigma, int64_t sigma_stride, const float* t, float* dw, int which, int64_t n,
                                int64_t H, int64_t W, void* workspace, deqsci_stream_t stream);

/* ---- real spectral normalisation in train mode (csrc/realsn.hip): the power-iteration step of a spectrally normalised 3x3 convolution and
 * the gradient of its normalised weight.  W (C_out, C_in, 3, 3) dense fp32, u (C_out, h, w), v (C_in, h, w) planar fp32.
 * R1 power   n_iters >= 1 times:  t1 = W^T u (the adjoint of the pad-1 convolution),  v = t1 / max(|t1|, eps),  t2 = W v,  u = t2 / max(|t2|, eps);
 *            then cur_sigma = sum(u * (W v)) and weight = W / cur_sigma * sigma_t (fp32, in this order).  u is read and overwritten; v, weight
 *            and record are written: record[0] = |W^T u|, record[1] = |W v|, record[2] = cur_sigma of the last iteration, in float64.
 *            3 n_iters + 1 launches on `stream`.
 * R2 grad    dW = (sigma_t / cur_sigma) * (G - (sum(G * W) / cur_sigma) * C),  C[o,i,ky,kx] = sum_p u[o,p] v[i, p + (ky-1, kx-1)] (zero outside
 *            the map), from R1's u, v and record; G, dW in W's shape.  2 launches.
 * The convolutions and C accumulate in fp32 in a fixed order; the sums of squares, cur_sigma and sum(G * W) in float64 (csrc/rows.hpp), sqrt in
 * float64, then fp32: the rounded norm, max(., eps), the division.  No atomics (bit-equal run to run), no allocation, no host synchronisation.
 * (C_in, C_out) in {(1,64), (64,64), (64,1)}, h, w >= 1, h * w <= 2^20.  workspace = deqsci_realsn_workspace_bytes(C_in, C_out, h, w) bytes
 * (0 for sizes that are refused; serves both entries), 16-byte aligned, no initialisation needed.
 * NULL -> -1; a non-positive size, n_iters < 1 -> -2; a float array or the workspace not 16-byte, record not 8-byte aligned -> -3; another
 * (C_in, C_out), a larger map, an output or the workspace overlapping an input or one another -> -4.  All checked before any launch. */
size_t deqsci_realsn_workspace_bytes(int64_t C_in, int64_t C_out, int64_t h, int64_t w);
int deqsci_realsn_power_f32(const float* W, float* u, float* v, float* weight, double* record, int n_iters, float sigma_t, float eps,
                            int64_t C_in, int64_t C_out, int64_t h, int64_t w, void* workspace, deqsci_stream_t stream);
int deqsci_realsn_grad_f32(const float* G, const float* W, const float* u, const float* v, const double* record, float* dW, float sigma_t,
                           int64_t C_in, int64_t C_out, int64_t h, int64_t w, void* workspace, deqsci_stream_t stream);
/* R3 pack    the normalised weight (C_out, C_in, 3, 3) R1 wrote -> the packs the convolution kernels read, in ONE launch: no host
 *            synchronisation, no host -> device copy, no allocation.  Every output may be NULL (not wanted); the caller owns the buffers.
 *            (64,64): pack = the F(2x2,3x3) pack (64*64*16 floats, the layout of csrc/winograd.hip), pack44 = the F(4x4,3x3) pack
 *                     (64*64*36 floats, csrc/winograd44.hip), pack_t = the F(2x2,3x3) pack of the transposed weight
 *                     wt[co, ci, ky, kx] = weight[ci, co, 2 - ky, 2 - kx], through which a gradient goes down.
 *            (1,64):  pack = the 1 -> 64 stencil's [tap][cout] (576 floats), pack_t = the 64 -> 1 stencil's [half][tap][cin % 32] of wt.
 *            (64,1):  pack = the 64 -> 1 stencil's pack, pack_t = the 1 -> 64 stencil's pack of wt.  pack44 must be NULL for both.
 *            Arithmetic of the Winograd packs: U = G g G^T in float64 from the fp32 weight, G the transform's constants as doubles
 *            (F(2x2,3x3): 1, 1/2; F(4x4,3x3): 1/4, 1/6, 1/12, 1/24, each the double nearest the quotient).  ONE order: first
 *            T[a][k] = (G[a][0] g[0][k] + G[a][1] g[1][k]) + G[a][2] g[2][k], then U[a][b] = (T[a][0] G[b][0] + T[a][1] G[b][1]) + T[a][2] G[b][2];
 *            every product and every sum is rounded by itself (no fused multiply-add), the zero entries of G take part like the others,
 *            and U is rounded to fp32 once.  The edge packs are permutations.  Bit-equal run to run.
 *            NULL weight or all three outputs NULL -> -1; another (C_in, C_out), pack44 for an edge layer -> -4; a pointer not 16-byte
 *            aligned -> -3; an output overlapping the weight or another output -> -4.  All checked before the launch. */
int deqsci_realsn_pack_f32(const float* weight, float* pack, float* pack44, float* pack_t, int64_t C_in, int64_t C_out, deqsci_stream_t stream);

/* ---- BatchNorm2d in TRAIN mode behind a 64 -> 64 convolution (csrc/bn_train.hip): batch statistics, normalisation and their backward on the
 * fp32 channels_last activation (P, 64), P = n H W pixels.  A workgroup owns a fixed run of pixels (DEQSCI_BN_TRAIN_CHUNK, or
 * ceil(P / DEQSCI_BN_TRAIN_MAX_WG) rounded up to 16 where that is more), a thread sums its pixels in float64, the workgroup folds them in a
 * fixed order into one float64 partial, and a closing launch sums the partials in a fixed order: no atomics, bit-equal run to run.
 * record = double[128]: the batch mean [0, 64) and the BIASED batch variance [64, 128);  grad_record = double[128]: dbeta, then dgamma.
 * T1 stats       mean = sum(c) / P;  var = sum((c - mean)^2) / P from a second, centred pass (it keeps its digits under any offset of c).
 *                The closing launch applies torch's update in float64, rounded once: running_mean = (1 - momentum) running_mean +
 *                momentum mean,  running_var = (1 - momentum) running_var + momentum var P / (P - 1),  *num_batches_tracked += 1.
 *                The three buffer pointers may ALL be NULL (no update; some but not all: -1).  4 launches.
 * T2 apply       per channel, float64: inv = 1 / sqrt(var + eps), a = gamma * inv;  per element
 *                    y = (float) fma(a, (double)c - mean, (double)beta)      (one fused multiply-add, rounded once to fp32)
 *                then max(y, 0) where relu = 1 (a NaN stays a NaN).  y may BE c.  mask (NULL: skipped): one word per pixel in
 *                deqsci_relu_mask_pack_f32's format, bit ch = (y > 0), written in the same pass.  1 launch.
 * T3 grad stats  gy = the gradient behind the layer, already masked by its ReLU; c the stored convolution output.  float64 products and sums:
 *                    dbeta = sum gy,   dgamma = inv * sum gy * ((double)c - mean)
 *                kept in grad_record for T4 and rounded once to the fp32 outputs dgamma[64], dbeta[64].  2 launches.
 * T4 grad apply  per channel, float64: k1 = dbeta / P,  k2 = dgamma * inv / P,  a = gamma * inv;  per element
 *                    dc = (float)(a * (((double)gy - k1) - ((double)c - mean) * k2))
 *                (every operation rounded in float64, the result once to fp32).  dc may BE gy.  A pixel the ReLU masked (gy = 0) still
 *                receives the two statistic terms.  1 launch.
 * c, gy, y, dc 16-byte aligned; records, the workspace and num_batches_tracked 8-byte, the rest 4-byte.  workspace =
 * deqsci_bn_train_workspace_bytes(P) bytes (0 for P < 2 or P >= 2^31; T1 and T3), no initialisation needed.  No allocation, no host
 * synchronisation, graph-capturable.  P = 0 launches nothing and returns 0.  NULL -> -1;  P < 0, P = 1 (torch: "Expected more than 1 value
 * per channel when training"), P >= 2^31 -> -2;  misaligned -> -3;  an output or the workspace overlapping an input or another output
 * (other than y == c, dc == gy), relu other than 0 / 1 -> -4. */
#define DEQSCI_BN_TRAIN_CHUNK 128
#define DEQSCI_BN_TRAIN_MAX_WG 1024
size_t deqsci_bn_train_workspace_bytes(int64_t P);
int deqsci_bn_train_stats_f32(const float* c, double* record, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                              double momentum, int64_t P, void* workspace, deqsci_stream_t stream);
int deqsci_bn_train_apply_f32(const float* c, const double* record, const float* gamma, const float* beta, double eps, float* y,
                              uint64_t* mask, int relu, int64_t P, deqsci_stream_t stream);
int deqsci_bn_train_grad_stats_f32(const float* gy, const float* c, const double* record, double eps, double* grad_record, float* dgamma,
                                   float* dbeta, int64_t P, void* workspace, deqsci_stream_t stream);
int deqsci_bn_train_grad_apply_f32(const float* gy, const float* c, const double* record, const double* grad_record, const float* gamma,
                                   double eps, float* dc, int64_t P, deqsci_stream_t stream);

/* ---- the training step's glue (csrc/train.hip): loss, PSNR, NaN check and loss gradient in one pass; Adam for many tensors in one launch ----
 * L1  rec, gt: flat fp32 of `total` elements in the same layout (the batch as ONE row), 4-byte aligned.  Per element, in fp32:
 *     d = rec - gt, grad = d * scale (the caller passes scale = (float)(2.0 / total): the gradient of the mean squared error),
 *     dc = clamp(rec, 0, 1) - gt (NaN kept).  stats[0] = sum d * d, stats[1] = sum dc * dc (squares in fp32, sums in float64),
 *     stats[2] = the number of non-finite d.  A NaN or Inf in d is counted, enters stats[0] as it is, and the gradient is written all
 *     the same.  The loss is stats[0] / total and the batch PSNR 10 log10(total / stats[1]) (harness.psnr's arithmetic).
 *     Deterministic: the two-stage order of csrc/rows.hpp over chunks of DEQSCI_TRAIN_CHUNK elements, stage 2 by one workgroup, no
 *     atomics; the sums do not depend on the pointers' alignment (rec, gt and grad all 16-byte aligned: read as float4).
 *     grad (total) fp32 must not overlap rec or gt; stats: 3 float64, 8-byte aligned; workspace = deqsci_mse_workspace_bytes(total)
 *     bytes (0 for invalid sizes), 8-byte aligned, no initialisation needed; overlaps among the outputs: -4.  total = 0: -2.
 *     Two launches on `stream`; no allocation, no host synchronisation, graph-capturable. */
#define DEQSCI_TRAIN_CHUNK 4096
size_t deqsci_mse_workspace_bytes(int64_t total);
int deqsci_mse_stats_grad_f32(const float* rec, const float* gt, float* grad, double* stats, int64_t total, float scale, void* workspace,
                              deqsci_stream_t stream);

/* L2  one Adam step (torch-1.9 F.adam: no weight decay, no amsgrad) of n_tensors <= DEQSCI_ADAM_MAX_TENSORS tensors in ONE launch.
 *     entries: n_tensors records in HOST memory, read before the call returns (the table travels by value in the kernel's arguments:
 *     64 x 48 bytes + the chunk prefix sums fit the 4096 bytes a HIP kernel's arguments may take, so no device buffer is staged, nothing
 *     allocated and nothing synchronised).  Per element, in fp32, each operation rounded separately, in this order:
 *         m = m * beta1 + g * one_minus_beta1;  v = v * beta2 + (g * g) * one_minus_beta2;
 *         den = sqrtf(v) / bc2s + eps;  p = p - step_size * (m / den)
 *     with bc2s = sqrt(1 - beta2^t) and step_size = lr / (1 - beta1^t) of the entry (t = the tensor's own step count), computed by the
 *     caller in double and passed as floats; division and square root correctly rounded.  param, exp_avg, exp_avg_sq are updated in
 *     place.  Pointers 4-byte aligned (a tensor whose four pointers are 16-byte aligned is walked as float4 with a scalar tail, any
 *     other element by element: the same values); the four ranges of an entry must not overlap (-4).  numel >= 1.  n_tensors = 0:
 *     nothing is launched; more than DEQSCI_ADAM_MAX_TENSORS: -4 (the caller launches once per table). */
#define DEQSCI_ADAM_MAX_TENSORS 64
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float bc2s;
    float step_size;
} deqsci_adam_entry;
int deqsci_adam_step_f32(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2,
                         float one_minus_beta2, float eps, deqsci_stream_t stream);

/* L3  the global gradient norm of n_tensors >= 0 fp32 tensors (ANY number), the clipping coefficient of torch's clip_grad_norm_ and the
 *     count of non-finite elements, all left on the device.  entries: n_tensors records in HOST memory, read before the call returns
 *     (tables of DEQSCI_ADAM_MAX_TENSORS tensors travel by value in the kernels' arguments, as L2's).  The order of summation is fixed:
 *       1. one workgroup = one chunk of DEQSCI_TRAIN_CHUNK elements of one tensor: every element widened to double and squared there
 *          (exact), the chunk summed in the stage-1 order of csrc/rows.hpp (4 float4 per thread), the non-finite elements counted beside;
 *       2. a tensor's chunk partials in L1's stage-2 order (one workgroup per tensor: thread i adds chunks i, i + 256, ..., then the
 *          workgroup's sum);
 *       3. the tensors' sums one after the other in list order, in double, across the tables.
 *     stats (3 + n_tensors float64, 8-byte aligned):
 *       stats[0] = sqrt(sum);  stats[1] = coef = (float)c where c = max_norm / (stats[0] + 1e-6) in double and c >= 1 gives 1 (a NaN
 *       stays NaN), stored as that fp32's value;  stats[2] = the number of non-finite elements;  stats[3 + i] = tensor i's own norm.
 *     A NaN or Inf is counted and enters the sums as it is.  max_norm >= 0 (NaN: -4).  Gradients 4-byte aligned (16-byte aligned ones
 *     are read as float4: the same sums), numel >= 1.  workspace = deqsci_grad_norm_workspace_bytes(entries, n_tensors) bytes (0 for
 *     invalid entries), 8-byte aligned, no initialisation needed; stats and workspace must overlap neither each other nor a gradient (-4).
 *     2 ceil(n_tensors / DEQSCI_ADAM_MAX_TENSORS) + 1 launches on `stream` (chunks and tensors per table, then one workgroup); no
 *     atomics, no allocation, no host synchronisation, graph-capturable.
 * L3s grad = grad * coef in place (one fp32 rounding, as clip_grad_norm_'s grad.mul_) for the listed tensors, with coef = stats[1] read on
 *     the device; nothing is written where stats[2] > 0 (a non-finite gradient) or coef == 1 (the same bits).  One launch per table.
 * L2c L2 with g' = g * coef (one fp32 rounding) in place of g, coef = stats[1] read on the device by every workgroup; where
 *     stats[2] > 0 NOTHING is written for any tensor (param, exp_avg and exp_avg_sq stay untouched).  grad is not written.  With
 *     coef == 1 the step's bits are L2's.  stats: 3 float64, 8-byte aligned, overlapping no tensor of the table (-4); the rest as L2. */
typedef struct {
    float* grad;
    int64_t numel;
} deqsci_grad_entry;
size_t deqsci_grad_norm_workspace_bytes(const deqsci_grad_entry* entries, int64_t n_tensors);
int deqsci_grad_norm_f32(const deqsci_grad_entry* entries, int64_t n_tensors, double max_norm, double* stats, void* workspace,
                         deqsci_stream_t stream);
int deqsci_grad_scale_f32(const deqsci_grad_entry* entries, int64_t n_tensors, const double* stats, deqsci_stream_t stream);
int deqsci_adam_step_clipped_f32(const deqsci_adam_entry* entries, int n_tensors, float beta1, float one_minus_beta1, float beta2,
                                 float one_minus_beta2, float eps, const double* stats, deqsci_stream_t stream);

/* ---- training batches out of raw video (csrc/synth.hip): crop, augment and snapshot synthesis in one launch per 64 samples ----
 * Y1  pool: `pool_bytes` bytes of uint8 frames on the device, every video a contiguous (T,Hv,Wv) block.  table: bsz rows of
 *     DEQSCI_SYNTH_ROW_WORDS int64 in HOST memory, read before the call returns (the rows travel by value in the kernel's arguments,
 *     DEQSCI_SYNTH_MAX_ROWS per launch: nothing staged, nothing allocated, nothing synchronised, no atomics):
 *         {video_offset, T, Hv, Wv, t0, dt, y0, x0, ds, flags}
 *     video_offset = the video's first byte in the pool; dt = the signed, non-zero step in frames (negative: the clip played backwards);
 *     ds >= 1 = the step in pixels; flags = DEQSCI_SYNTH_FLIP_H | _FLIP_V | _TRANSPOSE.  Output pixel (i,j), frame b of a sample:
 *         (Hc,Wc) = transpose ? (W,H) : (H,W);  (r,c) = transpose ? (j,i) : (i,j);  flip_v: r = Hc-1-r;  flip_h: c = Wc-1-c
 *         u = video[t0 + dt b, y0 + ds r, x0 + ds c]
 *         gt[i,j,b] = (float)u / 255.0f;   s = 0, then s = s + mask[i,j,b] * (float)u for b = 0..B-1;   meas[i,j] = s / 255.0f
 *     in fp32, the product and the sum rounded separately, both divisions correctly rounded.  With a mask of zeros and ones and
 *     B <= 64 the sums are integers below 2^24, so gt and meas are the floats nearest u / 255 and sum / 255: what a loader of the
 *     reference's training directory (uint8 patches, float64 sums, / 255 in double) returns.
 *     gt (bsz,H,W,B), meas (bsz,H,W), mask (H,W,B) fp32, 4-byte aligned (float4 accesses where B % 4 == 0 and gt, mask and mask_stride
 *     allow them: the same values); mask_stride = elements from one sample's mask to the next (>= H W B), 0 = one mask for all.
 *     1 <= B <= DEQSCI_SYNTH_MAX_FRAMES, H, W >= 1 (any value).  EVERY row is checked on the host before the first launch: all B source
 *     frames and the four corners of the crop inside the video, the video inside the pool - DEQSCI_ERR_SHAPE otherwise, so the kernel
 *     never reads out of bounds; unknown flag bits, or an output overlapping another buffer: DEQSCI_ERR_UNSUPPORTED.  bsz = 0: nothing
 *     is launched. */
#define DEQSCI_SYNTH_ROW_WORDS 10
#define DEQSCI_SYNTH_MAX_ROWS 64
#define DEQSCI_SYNTH_MAX_FRAMES 64
#define DEQSCI_SYNTH_FLIP_H 1
#define DEQSCI_SYNTH_FLIP_V 2
#define DEQSCI_SYNTH_TRANSPOSE 4
int deqsci_synth_batch_u8(const uint8_t* pool, int64_t pool_bytes, const int64_t* table, int64_t bsz, const float* mask, int64_t mask_stride,
                          float* gt, float* meas, int64_t H, int64_t W, int64_t B, deqsci_stream_t stream);
/* Y0  (n,3) uint8 RGB -> (n) uint8 luma, (77 R + 150 G + 29 B + 128) >> 8 in integer arithmetic (exact); gray must not overlap rgb (-4);
 *     n = 0: nothing is launched. */
int deqsci_rgb_to_gray_u8(const uint8_t* rgb, uint8_t* gray, int64_t n, deqsci_stream_t stream);

/* ---- a reproducible random source and the sensor-noise model on it (csrc/noise.hip) ----
 * The generator is Philox4x32-10 in integer arithmetic.  M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85; one round:
 *         (c0,c1,c2,c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),  then (k0,k1) += (W0,W1);  ten rounds.
 *     The key (k0,k1) is the 64-bit `seed` (low word, high word).  Counter words 0 and 1 are the 64-bit group index g = e >> 2, e the flat
 *     element index inside ONE sample; words 2 and 3 are the sample's 64-bit sequence number seq[sample].  The four output words
 *     x0..x3 of a group serve the elements 4g .. 4g+3, so a value is a function of (seed, seq, e) and of nothing else: not of bsz, not
 *     of the launch geometry, not of which call or which device draws it.
 *     Normals, fp32, with the accurate library functions (logf, sqrtf, sincospif - not the fast intrinsics):
 *         u(x) = ((x >> 9) + 0.5f) * 2^-23   (exact, strictly inside (0,1));   r = sqrtf(-2.0f * logf(u(x0)));   sincospif(2.0f * u(x1), &s, &c)
 *         element 4g = r * c, element 4g+1 = r * s;  x2, x3 give elements 4g+2 and 4g+3 the same way.  |normal| <= sqrt(48 ln 2) < 5.77.
 *     seq: bsz uint64 in HOST memory, read before the call returns (by value in the kernel's arguments, DEQSCI_NOISE_MAX_ROWS samples per
 *     launch); nothing allocated, nothing synchronised, no atomics, every output element written once.  Pointers 4-byte aligned (float4 /
 *     uint4 accesses where n % 4 == 0 and the pointers are 16-byte aligned: the same values).  NULL: -1; bsz < 0, n < 1 or more than 2^40
 *     elements: -2; misaligned: -3; bsz = 0: nothing is launched.
 * N0  out (bsz, ceil(n / 4), 4) uint32: the raw words of every group that serves one of the n elements of a sample.
 * N1  out (bsz, n) fp32 standard normals.
 * N2  out (bsz, n) = y (bsz, n) under the Gaussian approximation of Poisson-Gaussian noise (variance gain y + sigma^2) followed by an ADC of
 *     `bits` bits over [0, full_scale].  fp32, every operation rounded on its own, both divisions and the square root correctly rounded,
 *     in THIS order, nrm the element's normal of N1:
 *         if y is not finite:  o = y                       (NaN and +-Inf pass through untouched, also through the quantiser)
 *         else:  p = fmaxf(y, 0);  v = gain * p;  v = v + sigma * sigma;  d = sqrtf(v);  t = d * nrm;  o = y + t
 *                if bits > 0:  L = 2^bits - 1;  c = o / full_scale;  c = fminf(fmaxf(c, 0), 1);  q = rintf(c * L);  o = (q / L) * full_scale
 *     out == y (exactly in place) is allowed, any other overlap is refused (-4); bits outside 0..16, sigma or gain negative or not finite,
 *     full_scale not positive and finite: -4.  bits = 0: no quantiser (full_scale is then only checked). */
#define DEQSCI_NOISE_MAX_ROWS 64
int deqsci_philox_words_u32(uint32_t* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, deqsci_stream_t stream);
int deqsci_philox_normal_f32(float* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, deqsci_stream_t stream);
int deqsci_sensor_noise_f32(const float* y, float* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, float sigma, float gain,
                            int bits, float full_scale, deqsci_stream_t stream);

/* ---- measurement only (bench.py): the same launch with the dispatch's own begin/end timestamps
 * written to two raw hipEvent_t handles (hipExtLaunchKernelGGL), i.e. the duration rocprofv3 reports,
 * without the marker-packet overhead of events recorded around a launch. */
int deqsci_anderson_mix_gap_timed_f32(const float* F_hist, const float* G_hist, const float* alpha,
                                      float beta, int n, int m,
                                      const float* phi, const float* y, const float* phisum,
                                      float* x_out, float* z1,
                                      int64_t bsz, int64_t H, int64_t W, int64_t B,
                                      int layout, int phi_shared, deqsci_stream_t stream,
                                      void* start_event, void* stop_event);
int deqsci_conv3x3_c64_winograd_timed_f32(const float* x, const float* u_packed, const float* bias, float* y,
                                          int64_t n, int64_t H, int64_t W, int relu, deqsci_stream_t stream,
                                          void* start_event, void* stop_event);
int deqsci_conv3x3_c64_winograd44_timed_f32(const float* x, const float* u_packed, const float* bias, float* y,
                                            int64_t n, int64_t H, int64_t W, int relu, deqsci_stream_t stream,
                                            void* start_event, void* stop_event);
int deqsci_event_create(void** ev);
int deqsci_event_destroy(void* ev);
int deqsci_event_elapsed_ms(void* start_event, void* stop_event, float* ms);   /* after the stream is synchronised */

#ifdef __cplusplus
}
#endif
#endif /* DEQSCI_HIP_H */
