// Training batches out of raw video for MI355X (gfx950): what the reference's unshipped MATLAB scripts did ahead of time - cut (H,W,B)
// blocks out of videos, turn them, form the snapshot - done per batch on the device, from a pool of uint8 frames, in the training
// loop's own layouts (utils/sci_dataloader.py:218-239 reads the result of those scripts: gt / 255, meas / 255, mask).
//
//   Y0  rgb_to_gray_kernel   (n,3) u8 -> (n) u8, (77 R + 150 G + 29 B + 128) >> 8 in integers; once, when a colour video enters the pool
//   Y1  synth_kernel         one workgroup = one TS x TS tile of one sample's patch, all B frames in runs of FB.  Per run: the source
//                            bytes into an LDS tile [frame][crop row][crop column], lanes along the crop's columns (a row of the video:
//                            the byte reads of a wave fall into whole 32-byte runs at ds = 1, ascending or descending with the flip);
//                            then one thread per output pixel, lanes along j, reads its FB bytes - across the tile when the patch is
//                            transposed, the pitch of 9 words keeps that free of bank conflicts -, writes the pixel's B floats of gt as
//                            one contiguous run and carries s = s + mask_b * u_b in a register; meas = s / 255 after the last run.
//
// Arithmetic (include/deqsci_hip.h states it): fp32, the product and the sum rounded separately (-ffp-contract=off), both divisions the
// correctly rounded ones (hipcc's default; a multiplication by 1/255 differs in 12 096 of the 16 321 integer sums up to 255 x 64).
// Geometry: the launcher folds a descriptor row into a base offset and three signed strides (a flip is a negative stride, a reversed clip
// a negative frame stride), so the kernel has ONE addressing form; the rows travel by value in the kernel arguments (csrc/train.hip's
// Adam table is the precedent), 64 per launch.  Every row is checked against its video and the pool on the host before the first launch.
// No staging buffer, no allocation, no synchronisation, no atomics; every output element is written exactly once.
#include "common.hpp"

namespace deqsci {
namespace synth {

constexpr int TS = 32;                                   // tile side, in pixels
constexpr int FB = 16;                                   // frames per run through the LDS tile
constexpr int PITCH = TS + 4;                            // bytes per tile row: 9 words, odd - a column read (transposed patch) hits 32 banks
constexpr int ROWS_PER_PASS = TB / TS;                   // 8 tile rows per pass of the workgroup
constexpr int PASSES = TS / ROWS_PER_PASS;               // 4 pixels per thread
static_assert(TB % TS == 0 && TS % ROWS_PER_PASS == 0, "the workgroup walks the tile in whole passes");
static_assert(DEQSCI_SYNTH_MAX_FRAMES % FB == 0, "whole runs at the largest B");

struct Row {
    int64_t base;                                        // byte offset in the pool of frame 0, crop row 0, crop column 0
    int64_t fstride;                                     // bytes from frame b to b + 1 (dt Hv Wv: negative for a reversed clip)
    int64_t rstride;                                     // bytes from crop row r to r + 1 (+-ds Wv)
    int32_t cstride;                                     // bytes from crop column c to c + 1 (+-ds)
    int32_t transpose;
};
struct Args {
    Row row[DEQSCI_SYNTH_MAX_ROWS];
    const uint8_t* pool;
    const float* mask;
    float* gt;
    float* meas;
    int64_t mask_stride;                                 // elements from one sample's mask to the next; 0: one shared mask
    int32_t H, W, B, tiles_w;
    int32_t vec;                                         // B % 4 == 0 and gt, mask (and its stride) 16-byte aligned: float4 accesses
};
static_assert(sizeof(Row) == 32, "64 rows of 32 bytes");
static_assert(sizeof(Args) <= 4096, "the descriptor table must fit the kernel-argument segment");

__global__ __launch_bounds__(TB) void synth_kernel(const Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[FB][TS][PITCH];
    const Row& d = a.row[blockIdx.y];
    const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;
    const int ti = (int)(blockIdx.x / (uint32_t)a.tiles_w), tj = (int)(blockIdx.x - (uint32_t)ti * (uint32_t)a.tiles_w);
    const int i0 = ti * TS, j0 = tj * TS;
    const int H = a.H, W = a.W, B = a.B;
    const bool tr = d.transpose != 0;
    const int Hc = tr ? W : H, Wc = tr ? H : W;           // the crop, in the video's orientation
    const int r0 = tr ? j0 : i0, c0 = tr ? i0 : j0;
    const int64_t sample = blockIdx.y, HW = (int64_t)H * W;
    const uint8_t* __restrict__ src = a.pool + d.base;
    const float* __restrict__ mask = a.mask + sample * a.mask_stride;
    float* __restrict__ gt = a.gt + sample * HW * B;
    float* __restrict__ meas = a.meas + sample * HW;
    const int j = j0 + lx, c = c0 + lx;
    float acc[PASSES];
#pragma unroll
    for (int k = 0; k < PASSES; ++k) acc[k] = 0.0f;
    for (int b0 = 0; b0 < B; b0 += FB) {
        const int nb = B - b0 < FB ? B - b0 : FB;
        if (b0) __syncthreads();                          // the last run's readers are done with the tile
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int lr = ly + k * ROWS_PER_PASS, r = r0 + lr;
            if (r < Hc && c < Wc) {
                const uint8_t* p = src + (int64_t)b0 * d.fstride + (int64_t)r * d.rstride + (int64_t)c * d.cstride;
                for (int fb = 0; fb < nb; ++fb) tile[fb][lr][lx] = p[(int64_t)fb * d.fstride];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int li = ly + k * ROWS_PER_PASS, i = i0 + li;
            if (i >= H || j >= W) continue;
            const int lr = tr ? lx : li, lc = tr ? li : lx;
            const int64_t e = ((int64_t)i * W + j) * B + b0;
            float s = acc[k];
            if (a.vec) {
                for (int fb = 0; fb < nb; fb += 4) {      // (B % 4 == 0: nb is a whole number of quads)
                    const float4 m = ld4(mask + e + fb);
                    const float4 u = make_float4((float)tile[fb][lr][lc], (float)tile[fb + 1][lr][lc], (float)tile[fb + 2][lr][lc],
                                                 (float)tile[fb + 3][lr][lc]);
                    st4(gt + e + fb, u / f4(255.0f));
                    s = s + m.x * u.x;
                    s = s + m.y * u.y;
                    s = s + m.z * u.z;
                    s = s + m.w * u.w;
                }
            } else {
                for (int fb = 0; fb < nb; ++fb) {
                    const float u = (float)tile[fb][lr][lc];
                    gt[e + fb] = u / 255.0f;
                    s = s + mask[e + fb] * u;
                }
            }
            acc[k] = s;
        }
    }
#pragma unroll
    for (int k = 0; k < PASSES; ++k) {
        const int i = i0 + ly + k * ROWS_PER_PASS;
        if (i < H && j < W) meas[(int64_t)i * W + j] = acc[k] / 255.0f;
    }
}

__global__ __launch_bounds__(TB) void rgb_to_gray_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ gray, int64_t n) {
    for (int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x; p < n; p += (int64_t)gridDim.x * TB) {
        const uint32_t r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
        gray[p] = (uint8_t)((77u * r + 150u * g + 29u * b + 128u) >> 8);        // at most 255 x 256 + 128: below 2^16
    }
}

constexpr int64_t DIM_MAX = ((int64_t)1 << 31) - 1;      // T, Hv, Wv, |dt|, ds and the coordinates: products of two stay inside int64
inline bool dim_ok(int64_t v) { return v >= 1 && v <= DIM_MAX; }

// One descriptor row {video_offset, T, Hv, Wv, t0, dt, y0, x0, ds, flags} -> its Row, or false when anything it would read lies outside its
// video, or the video outside the pool's `pool_bytes` bytes.
inline int fold_row(const int64_t* q, int64_t pool_bytes, int64_t H, int64_t W, int64_t B, Row* out) {
    const int64_t off = q[0], T = q[1], Hv = q[2], Wv = q[3], t0 = q[4], dt = q[5], y0 = q[6], x0 = q[7], ds = q[8], flags = q[9];
    if (flags < 0 || flags > (DEQSCI_SYNTH_FLIP_H | DEQSCI_SYNTH_FLIP_V | DEQSCI_SYNTH_TRANSPOSE)) return DEQSCI_ERR_UNSUPPORTED;
    if (!dim_ok(T) || !dim_ok(Hv) || !dim_ok(Wv) || !dim_ok(ds) || dt == 0 || dt < -DIM_MAX || dt > DIM_MAX) return DEQSCI_ERR_SHAPE;
    const int64_t frame = Hv * Wv;
    if (off < 0 || off > pool_bytes || T > (pool_bytes - off) / frame) return DEQSCI_ERR_SHAPE;      // the video inside the pool
    const bool tr = (flags & DEQSCI_SYNTH_TRANSPOSE) != 0;
    const int64_t Hc = tr ? W : H, Wc = tr ? H : W;
    if (Hc > Hv || Wc > Wv || t0 < 0 || t0 >= T || y0 < 0 || y0 >= Hv || x0 < 0 || x0 >= Wv) return DEQSCI_ERR_SHAPE;
    const int64_t t_last = t0 + dt * (B - 1), y_last = y0 + ds * (Hc - 1), x_last = x0 + ds * (Wc - 1);     // (each below 2^63: see DIM_MAX)
    if (t_last < 0 || t_last >= T) return DEQSCI_ERR_SHAPE;                                            // all B frames: the first and the last bound the rest
    if (y_last >= Hv || x_last >= Wv) return DEQSCI_ERR_SHAPE;                                         // the four corners
    const bool fh = (flags & DEQSCI_SYNTH_FLIP_H) != 0, fv = (flags & DEQSCI_SYNTH_FLIP_V) != 0;
    out->base = off + t0 * frame + (fv ? y_last : y0) * Wv + (fh ? x_last : x0);
    out->fstride = dt * frame;
    out->rstride = (fv ? -ds : ds) * Wv;
    out->cstride = (int32_t)(fh ? -ds : ds);
    out->transpose = tr ? 1 : 0;
    return 0;
}

}  // namespace synth
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int deqsci_synth_batch_u8(const uint8_t* pool, int64_t pool_bytes, const int64_t* table, int64_t bsz, const float* mask, int64_t mask_stride,
                          float* gt, float* meas, int64_t H, int64_t W, int64_t B, deqsci_stream_t stream) {
    if (bsz < 0 || pool_bytes < 0 || H < 1 || W < 1 || H > synth::DIM_MAX || W > synth::DIM_MAX || B < 1 || B > DEQSCI_SYNTH_MAX_FRAMES)
        return DEQSCI_ERR_SHAPE;
    const int64_t HW = H * W, N = HW * B;
    if (bsz > ((int64_t)1 << 40) / N) return DEQSCI_ERR_SHAPE;
    if (mask_stride != 0 && mask_stride < N) return DEQSCI_ERR_SHAPE;
    if (bsz == 0) return 0;
    if (!pool || !table || !mask || !gt || !meas) return DEQSCI_ERR_NULL;
    if (misaligned(table, 8) || misaligned(mask, 4) || misaligned(gt, 4) || misaligned(meas, 4)) return DEQSCI_ERR_ALIGN;
    const int64_t gt_bytes = bsz * N * 4, meas_bytes = bsz * HW * 4, mask_bytes = ((bsz - 1) * mask_stride + N) * 4;
    if (overlaps(gt, gt_bytes, meas, meas_bytes) || overlaps(gt, gt_bytes, mask, mask_bytes) || overlaps(meas, meas_bytes, mask, mask_bytes) ||
        overlaps(gt, gt_bytes, pool, pool_bytes) || overlaps(meas, meas_bytes, pool, pool_bytes))
        return DEQSCI_ERR_UNSUPPORTED;
    const int64_t tiles_w = ceil_div(W, synth::TS), tiles = tiles_w * ceil_div(H, synth::TS);
    if (tiles >= ((int64_t)1 << 31)) return DEQSCI_ERR_UNSUPPORTED;                                   // the grid's x extent
    synth::Row scratch;
    for (int64_t s = 0; s < bsz; ++s)                                                                  // EVERY row, before the first launch
        if (int e = synth::fold_row(table + s * DEQSCI_SYNTH_ROW_WORDS, pool_bytes, H, W, B, &scratch)) return e;
    synth::Args a;
    a.pool = pool;
    a.mask_stride = mask_stride;
    a.H = (int32_t)H;
    a.W = (int32_t)W;
    a.B = (int32_t)B;
    a.tiles_w = (int32_t)tiles_w;
    a.vec = (B % 4 == 0 && mask_stride % 4 == 0 && aligned16(gt) && aligned16(mask)) ? 1 : 0;
    for (int64_t first = 0; first < bsz; first += DEQSCI_SYNTH_MAX_ROWS) {
        const int64_t n = bsz - first < DEQSCI_SYNTH_MAX_ROWS ? bsz - first : DEQSCI_SYNTH_MAX_ROWS;
        for (int64_t s = 0; s < DEQSCI_SYNTH_MAX_ROWS; ++s) {
            if (s < n) (void)synth::fold_row(table + (first + s) * DEQSCI_SYNTH_ROW_WORDS, pool_bytes, H, W, B, &a.row[s]);
            else a.row[s] = synth::Row{0, 0, 0, 0, 0};
        }
        a.mask = mask + first * mask_stride;
        a.gt = gt + first * N;
        a.meas = meas + first * HW;
        hipLaunchKernelGGL(synth::synth_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(TB), 0, static_cast<hipStream_t>(stream), a);
        if (int e = launch_status()) return e;
    }
    return 0;
}

int deqsci_rgb_to_gray_u8(const uint8_t* rgb, uint8_t* gray, int64_t n, deqsci_stream_t stream) {
    if (n < 0 || n > ((int64_t)1 << 40)) return DEQSCI_ERR_SHAPE;
    if (n == 0) return 0;
    if (!rgb || !gray) return DEQSCI_ERR_NULL;
    if (overlaps(rgb, 3 * n, gray, n)) return DEQSCI_ERR_UNSUPPORTED;
    const int64_t blocks = ceil_div(n, TB), cap = (int64_t)num_cus() * 16;
    hipLaunchKernelGGL(synth::rgb_to_gray_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(TB), 0, static_cast<hipStream_t>(stream),
                       rgb, gray, n);
    return launch_status();
}

}  // extern "C"
