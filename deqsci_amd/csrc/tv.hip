// GAP-TV for MI355X (gfx950): the reference's GAP_TV_rec (utils/cg_utils.py:207-224) with scikit-image 0.17.2's
// denoise_tv_chambolle as its denoiser - a classical baseline and the DEQ's other starting point (ibid. :228-236).
//
//   T0 tv_init_kernel       f = At(y, Phi) (the product in fp32, as the reference's float32 arrays, stored as fp64), y1 = 0;
//                           or, for the bare denoiser, the fp32 planes upcast
//   T1 gap_step_kernel      per pixel: fb = sum_b f_b Phi_b (numpy's summation order), y1 += y - fb,
//                           f_b += step * (((y1 - fb) / Phi_sum) * Phi_b)  - the accelerated GAP step, fp64
//   T2 tv_iter_kernel       ONE Chambolle iteration over every (measurement, frame) plane still iterating: a 64 x 16 tile
//                           with its one-pixel halo staged in LDS, p ping-ponged between two buffers, per-workgroup fp64 sums
//                           of d^2 and |g|; the last workgroup of a plane to arrive folds the plane's sums in a fixed order and
//                           applies the stop rule (per-plane `done` word and stop index).  Workgroups of a stopped plane return
//                           at once, so the `out` of the stopping iteration stays in place.
//   T3 tv_store_kernel      fp64 planes -> fp32, (M,H,W,B) for GAP-TV, (n,H,W) for the bare denoiser
//
// One GAP-TV call is T0, maxiter x (T1 + n_iter_max x T2), T3: no host synchronisation anywhere.
//
// Chambolle (skimage 0.17.2 _denoise_tv_chambolle_nd on a plane; a length-1 leading axis adds nothing but tau = 1/(2 ndim)):
//     i = 0:  out = image, d = 0
//     i > 0:  d = -(p_h + p_w) + p_h[h-1] + p_w[w-1] (terms outside the plane are 0), out = image + d
//     E = (sum d^2 + weight * sum |g|) / (H W),  g = forward differences of out (0 on the last row / column)
//     p = (p - tau g) / (1 + (tau / weight) |g|)
//     i = 0: E_init = E_prev = E;  else stop if |E_prev - E| < eps E_init (returning this iteration's out), else E_prev = E
// Every operation is the reference's, rounded once in fp64 in the same order (-ffp-contract=off); only the plane sums of E are
// summed in another order than numpy's, so E carries a relative difference of ~1e-16 and a stop test can only differ where the
// reference's own margin is that small.
// Determinism: per-thread, per-wave, per-workgroup and per-plane summation orders are fixed; no floating-point atomics.  A plane's
// result does not depend on what else is in the batch.
#include <math.h>

#include "common.hpp"

namespace deqsci {
namespace tv {

constexpr int TW = 64;                 // tile columns: one double per lane of a wave
constexpr int TH = 16;                 // tile rows: four per wave
constexpr int PH = TH + 2, PW = TW + 2;  // staged p: rows r0-1 .. r0+TH, columns c0-1 .. c0+TW
constexpr int OH = TH + 1, OW = TW + 1;  // staged out: rows r0 .. r0+TH, columns c0 .. c0+TW
constexpr int MAX_FRAMES = 128;        // numpy's pairwise sum is restated for one block of <= 128 terms

struct Plane {                          // per-plane state, written by the plane's last workgroup of a launch
    double e_init, e_prev;
    int done, pad;
};

// T0: f[m,b,h,w] = (double)(y[m,h,w] * Phi[m|0,h,w,b]) (mode 0), or f[i] = (double)img[i] (mode 1); y1 = 0
__global__ __launch_bounds__(TB) void tv_init_kernel(const float* __restrict__ y, const float* __restrict__ phi, const float* __restrict__ img,
                                                     double* __restrict__ f, double* __restrict__ y1, int64_t M, int64_t HW, int64_t B,
                                                     int phi_shared) {
    const int64_t n = M * B * HW;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        if (img) { f[i] = (double)img[i]; continue; }
        const int64_t px = i % HW, mb = i / HW, b = mb % B, m = mb / B;
        const float p = phi[((phi_shared ? 0 : m) * HW + px) * B + b];
        f[i] = (double)(y[m * HW + px] * p);
        if (b == 0) y1[m * HW + px] = 0.0;
    }
}

// T1: one accelerated-GAP step per pixel; f (the previous TV output) -> g (the next TV input), planar fp64.  fb is summed in the order of
// numpy's pairwise_sum for one block of B <= 128 terms (what np.sum(f * Phi, axis=3) runs per pixel): B < 8 left to right; otherwise eight
// running sums r_k over b = k, k + 8, ..., folded ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the B % 8 last terms in order.
__global__ __launch_bounds__(TB) void gap_step_kernel(const float* __restrict__ y, const float* __restrict__ phi, const float* __restrict__ phi_sum,
                                                      const double* __restrict__ f, double* __restrict__ g, double* __restrict__ y1,
                                                      int64_t M, int64_t HW, int B, int phi_shared, double step) {
    const int64_t n = M * HW;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        const int64_t px = i % HW, m = i / HW;
        const float* ph = phi + ((phi_shared ? 0 : m) * HW + px) * B;
        const double* fm = f + m * B * HW + px;
        double fb = 0.0;
        int b = 0;
        if (B >= 8) {
            double r[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] = fm[k * HW] * (double)ph[k];
            for (b = 8; b + 8 <= B; b += 8) {
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] += fm[(b + k) * HW] * (double)ph[b + k];
            }
            fb = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        }
        for (; b < B; ++b) fb += fm[b * HW] * (double)ph[b];
        const double yv = y1[i] + ((double)y[i] - fb);
        y1[i] = yv;
        const double r = (yv - fb) / (double)phi_sum[(phi_shared ? 0 : m) * HW + px];
        double* gm = g + m * B * HW + px;
        for (b = 0; b < B; ++b) gm[b * HW] = fm[b * HW] + step * (r * (double)ph[b]);
    }
}

// T2: Chambolle iteration `it` of every plane not yet stopped.  img/out: (planes, H, W) fp64; p_in/p_out: [2][planes][H][W] (h then
// w component); part: [planes][n_tiles][2]; ticket: [planes] (zero between launches); stop: NULL or the per-plane stop words of this
// call, plane q -> stop[(q / group) * group_stride + q % group].
__global__ __launch_bounds__(TB) void tv_iter_kernel(const double* __restrict__ img, double* __restrict__ out, const double* __restrict__ p_in,
                                                     double* __restrict__ p_out, double* __restrict__ part, unsigned* __restrict__ ticket,
                                                     Plane* __restrict__ st, int* __restrict__ stop, int64_t H, int64_t W, int64_t tiles_x,
                                                     int64_t n_tiles, int64_t planes, int64_t group, int64_t group_stride, int it,
                                                     int n_iter_max, double weight, double tau, double tau_w, double eps) {
    __shared__ double lph[PH * PW], lpw[PH * PW], lo[OH * OW];
    __shared__ double wsum[2][TB / WAVE];
    __shared__ int last;

    const int64_t q = blockIdx.x / n_tiles, t = blockIdx.x % n_tiles;
    if (it > 0 && st[q].done) return;                                   // stopped: its out stays
    const int tid = threadIdx.x;
    const int64_t r0 = (t / tiles_x) * TH, c0 = (t % tiles_x) * TW;
    const int64_t HW = H * W, np_ = planes * HW;
    const double* im = img + q * HW;

    if (it > 0) {
        const double* pih = p_in + q * HW;
        const double* piw = p_in + np_ + q * HW;
        for (int i = tid; i < PH * PW; i += TB) {
            const int rr = i / PW, cc = i % PW;
            const int64_t h = r0 - 1 + rr, w = c0 - 1 + cc;
            const bool in = h >= 0 && h < H && w >= 0 && w < W;
            lph[i] = in ? pih[h * W + w] : 0.0;
            lpw[i] = in ? piw[h * W + w] : 0.0;
        }
        __syncthreads();
    }
    // out over the tile plus one row below and one column to the right
    for (int i = tid; i < OH * OW; i += TB) {
        const int rr = i / OW, cc = i % OW;
        const int64_t h = r0 + rr, w = c0 + cc;
        double o = 0.0;
        if (h < H && w < W) {
            o = im[h * W + w];
            if (it > 0) {
                const int k = (rr + 1) * PW + (cc + 1);
                const double d = ((-(lph[k] + lpw[k])) + lph[k - PW]) + lpw[k - 1];
                o = o + d;
            }
        }
        lo[i] = o;
    }
    __syncthreads();

    double sd = 0.0, sn = 0.0;
    const int cc = tid % TW;
    double* poh = p_out + q * HW;
    double* pow_ = p_out + np_ + q * HW;
    double* oq = out + q * HW;
    for (int rr = tid / TW; rr < TH; rr += TB / TW) {
        const int64_t h = r0 + rr, w = c0 + cc;
        if (h >= H || w >= W) continue;
        const double o = lo[rr * OW + cc];
        const double gh = (h < H - 1) ? lo[(rr + 1) * OW + cc] - o : 0.0;
        const double gw = (w < W - 1) ? lo[rr * OW + cc + 1] - o : 0.0;
        const double nrm = sqrt(gh * gh + gw * gw);
        double ph = 0.0, pw = 0.0;
        if (it > 0) {
            const int k = (rr + 1) * PW + (cc + 1);
            ph = lph[k];
            pw = lpw[k];
            const double d = ((-(ph + pw)) + lph[k - PW]) + lpw[k - 1];
            sd += d * d;
        }
        sn += nrm;
        const double den = nrm * tau_w + 1.0;
        poh[h * W + w] = (ph - tau * gh) / den;
        pow_[h * W + w] = (pw - tau * gw) / den;
        oq[h * W + w] = o;
    }
    // workgroup sums in a fixed order: wave butterfly, then the four wave sums in wave order
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        sd += __shfl_xor(sd, o, WAVE);
        sn += __shfl_xor(sn, o, WAVE);
    }
    if ((tid & (WAVE - 1)) == 0) {
        wsum[0][tid / WAVE] = sd;
        wsum[1][tid / WAVE] = sn;
    }
    __syncthreads();
    if (tid == 0) {
        double* pp = part + (q * n_tiles + t) * 2;
        __hip_atomic_store(pp, ((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pp + 1, ((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned a = __hip_atomic_fetch_add(ticket + q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (a == (unsigned)(n_tiles - 1));
    }
    __syncthreads();
    if (!last || tid >= WAVE) return;
    // the plane's last workgroup: one wave folds the tile sums (lane l: tiles l, l + 64, ... in order; then a fixed butterfly)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const double* pq = part + q * n_tiles * 2;
    double ad = 0.0, an = 0.0;
    for (int64_t k = tid; k < n_tiles; k += WAVE) {
        ad += __hip_atomic_load(pq + 2 * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        an += __hip_atomic_load(pq + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        ad += __shfl_xor(ad, o, WAVE);
        an += __shfl_xor(an, o, WAVE);
    }
    if (tid != 0) return;
    __hip_atomic_store(ticket + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double E = (ad + weight * an) / (double)HW;
    int* sp = stop ? stop + (q / group) * group_stride + q % group : nullptr;
    if (it == 0) {
        st[q].e_init = E;
        st[q].e_prev = E;
        st[q].done = 0;
        if (sp && n_iter_max == 1) *sp = n_iter_max;
        return;
    }
    if (fabs(st[q].e_prev - E) < eps * st[q].e_init) {
        st[q].done = 1;
        if (sp) *sp = it;
        return;
    }
    st[q].e_prev = E;
    if (sp && it == n_iter_max - 1) *sp = n_iter_max;
}

// T3: fp64 planes (M,B,H,W) -> fp32 (M,H,W,B) (hwb != 0) or (M*B,H,W)
__global__ __launch_bounds__(TB) void tv_store_kernel(const double* __restrict__ f, float* __restrict__ out, int64_t M, int64_t HW, int64_t B,
                                                      int hwb) {
    const int64_t n = M * HW * B;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
        if (!hwb) { out[i] = (float)f[i]; continue; }
        const int64_t b = i % B, mp = i / B, px = mp % HW, m = mp / HW;      // i indexes the output: consecutive threads write adjacent frames
        out[i] = (float)f[(m * B + b) * HW + px];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
struct Layout {                            // byte offsets into the workspace (every part 16-byte aligned)
    int64_t f, o, p0, p1, y1, part, plane, ticket, total;
};

inline int64_t al16(int64_t v) { return (v + 15) / 16 * 16; }

inline Layout layout_of(int64_t planes, int64_t H, int64_t W, int64_t M) {
    const int64_t N = planes * H * W * 8, nt = ceil_div(H, TH) * ceil_div(W, TW);
    Layout l;
    l.f = 0;
    l.o = l.f + al16(N);
    l.p0 = l.o + al16(N);
    l.p1 = l.p0 + al16(2 * N);
    l.y1 = l.p1 + al16(2 * N);
    l.part = l.y1 + al16(M * H * W * 8);
    l.plane = l.part + al16(planes * nt * 2 * 8);
    l.ticket = l.plane + al16(planes * (int64_t)sizeof(Plane));
    l.total = l.ticket + al16(planes * 4);
    return l;
}

inline int check(int64_t n, int64_t H, int64_t W, int64_t B) {
    if (n < 0 || H < 1 || W < 1 || B < 1) return DEQSCI_ERR_SHAPE;
    if (H > (int64_t)1 << 24 || W > (int64_t)1 << 24 || (n > 0 && n * B > ((int64_t)1 << 40) / (H * W))) return DEQSCI_ERR_SHAPE;
    const int64_t blocks = n * B * ceil_div(H, TH) * ceil_div(W, TW);
    if (blocks >= ((int64_t)1 << 31)) return DEQSCI_ERR_SHAPE;      // T2's one-dimensional grid
    return 0;
}

inline unsigned grid_for(int64_t n) {
    const int64_t b = ceil_div(n, TB);
    return (unsigned)(b < 65536 ? (b > 0 ? b : 1) : 65536);
}

// n_iter_max T2 launches over the planes at ws + l.f; the result at ws + l.o
inline int chambolle(char* ws, const Layout& l, int64_t planes, int64_t H, int64_t W, int64_t group, int64_t group_stride, int* stop,
                     double weight, double eps, int n_iter_max, double tau, hipStream_t st) {
    const int64_t tiles_x = ceil_div(W, TW), n_tiles = ceil_div(H, TH) * tiles_x;
    double* p[2] = {reinterpret_cast<double*>(ws + l.p0), reinterpret_cast<double*>(ws + l.p1)};
    const double tau_w = tau / weight;
    for (int i = 0; i < n_iter_max; ++i) {
        hipLaunchKernelGGL(tv_iter_kernel, dim3((unsigned)(planes * n_tiles)), dim3(TB), 0, st, reinterpret_cast<const double*>(ws + l.f),
                           reinterpret_cast<double*>(ws + l.o), p[i & 1], p[(i + 1) & 1], reinterpret_cast<double*>(ws + l.part),
                           reinterpret_cast<unsigned*>(ws + l.ticket), reinterpret_cast<Plane*>(ws + l.plane), stop, H, W, tiles_x, n_tiles,
                           planes, group, group_stride, i, n_iter_max, weight, tau, tau_w, eps);
        if (int e = launch_status()) return e;
    }
    return 0;
}

inline bool params_ok(double weight, double eps, int n_iter_max, double tau) {
    return weight > 0.0 && isfinite(weight) && eps >= 0.0 && isfinite(eps) && n_iter_max >= 1 && tau > 0.0 && isfinite(tau);
}

}  // namespace tv
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int64_t deqsci_gaptv_workspace_bytes(int64_t bsz, int64_t H, int64_t W, int64_t B) {
    if (int e = tv::check(bsz, H, W, B)) return e;
    if (B > tv::MAX_FRAMES) return DEQSCI_ERR_UNSUPPORTED;
    return tv::layout_of(bsz * B, H, W, bsz).total;
}

int64_t deqsci_tv_chambolle_workspace_bytes(int64_t n, int64_t H, int64_t W) {
    if (int e = tv::check(n, H, W, 1)) return e;
    return tv::layout_of(n, H, W, 0).total;
}

int deqsci_gaptv_f32(const float* y, const float* phi, const float* phi_sum, float* out, int64_t bsz, int64_t H, int64_t W, int64_t B,
                     int phi_shared, int maxiter, double step, double weight, double eps, int n_iter_max, int* stop, void* workspace,
                     deqsci_stream_t stream) {
    if (!y || !phi || !phi_sum || !out || !workspace) return DEQSCI_ERR_NULL;
    if (int e = tv::check(bsz, H, W, B)) return e;
    if (maxiter < 0 || !isfinite(step) || !tv::params_ok(weight, eps, n_iter_max, 1.0)) return DEQSCI_ERR_SHAPE;
    if (B > tv::MAX_FRAMES) return DEQSCI_ERR_UNSUPPORTED;
    if (bsz == 0) return 0;
    if (misaligned(y, 4) || misaligned(phi, 4) || misaligned(phi_sum, 4) || misaligned(out, 4) || misaligned(stop, 4) || misaligned(workspace, 16))
        return DEQSCI_ERR_ALIGN;
    const int64_t HW = H * W, nb = phi_shared ? 1 : bsz;
    const tv::Layout l = tv::layout_of(bsz * B, H, W, bsz);
    const int64_t n_out = bsz * HW * B * 4, n_stop = stop ? bsz * (int64_t)maxiter * B * 4 : 0;
    if (overlaps(workspace, l.total, y, bsz * HW * 4) || overlaps(workspace, l.total, phi, nb * HW * B * 4) ||
        overlaps(workspace, l.total, phi_sum, nb * HW * 4) || overlaps(workspace, l.total, out, n_out) ||
        overlaps(out, n_out, y, bsz * HW * 4) || overlaps(out, n_out, phi, nb * HW * B * 4) ||
        overlaps(out, n_out, phi_sum, nb * HW * 4) ||
        (stop && (overlaps(stop, n_stop, workspace, l.total) || overlaps(stop, n_stop, out, n_out))))
        return DEQSCI_ERR_UNSUPPORTED;

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* f = reinterpret_cast<double*>(ws + l.f);
    double* o = reinterpret_cast<double*>(ws + l.o);
    double* y1 = reinterpret_cast<double*>(ws + l.y1);
    if (hipError_t e = hipMemsetAsync(ws + l.ticket, 0, (size_t)(l.total - l.ticket), st)) return (int)e;
    hipLaunchKernelGGL(tv::tv_init_kernel, dim3(tv::grid_for(bsz * B * HW)), dim3(TB), 0, st, y, phi, nullptr, o, y1, bsz, HW, B, phi_shared);
    if (int e = launch_status()) return e;
    for (int it = 0; it < maxiter; ++it) {
        hipLaunchKernelGGL(tv::gap_step_kernel, dim3(tv::grid_for(bsz * HW)), dim3(TB), 0, st, y, phi, phi_sum, o, f, y1, bsz, HW, (int)B,
                           phi_shared, step);
        if (int e = launch_status()) return e;
        // (a (1,H,W) channel: ndim 3, tau = 1/6)
        if (int e = tv::chambolle(ws, l, bsz * B, H, W, B, (int64_t)maxiter * B, stop ? stop + (int64_t)it * B : nullptr, weight, eps,
                                  n_iter_max, 1.0 / 6.0, st))
            return e;
    }
    hipLaunchKernelGGL(tv::tv_store_kernel, dim3(tv::grid_for(bsz * HW * B)), dim3(TB), 0, st, o, out, bsz, HW, B, 1);
    return launch_status();
}

int deqsci_tv_chambolle_f32(const float* image, float* out, int64_t n, int64_t H, int64_t W, double weight, double eps, int n_iter_max,
                            double tau, int* stop, void* workspace, deqsci_stream_t stream) {
    if (!image || !out || !workspace) return DEQSCI_ERR_NULL;
    if (int e = tv::check(n, H, W, 1)) return e;
    if (!tv::params_ok(weight, eps, n_iter_max, tau)) return DEQSCI_ERR_SHAPE;
    if (n == 0) return 0;
    if (misaligned(image, 4) || misaligned(out, 4) || misaligned(stop, 4) || misaligned(workspace, 16)) return DEQSCI_ERR_ALIGN;
    const tv::Layout l = tv::layout_of(n, H, W, 0);
    const int64_t nb = n * H * W * 4;
    if (overlaps(workspace, l.total, image, nb) || overlaps(workspace, l.total, out, nb) || overlaps(out, nb, image, nb) ||
        (stop && (overlaps(stop, n * 4, workspace, l.total) || overlaps(stop, n * 4, out, nb))))
        return DEQSCI_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (hipError_t e = hipMemsetAsync(ws + l.ticket, 0, (size_t)(l.total - l.ticket), st)) return (int)e;
    hipLaunchKernelGGL(tv::tv_init_kernel, dim3(tv::grid_for(n * H * W)), dim3(TB), 0, st, nullptr, nullptr, image,
                       reinterpret_cast<double*>(ws + l.f), nullptr, n, H * W, (int64_t)1, 0);
    if (int e = launch_status()) return e;
    if (int e = tv::chambolle(ws, l, n, H, W, 1, 1, stop, weight, eps, n_iter_max, tau, st)) return e;
    hipLaunchKernelGGL(tv::tv_store_kernel, dim3(tv::grid_for(n * H * W)), dim3(TB), 0, st, reinterpret_cast<const double*>(ws + l.o), out, n,
                       H * W, (int64_t)1, 0);
    return launch_status();
}

}  // extern "C"
