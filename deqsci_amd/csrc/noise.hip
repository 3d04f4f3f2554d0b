// A reproducible random source and the sensor-noise model built on it, for MI355X (gfx950).  The generator is Philox4x32-10 (Salmon et
// al., "Parallel random numbers: as easy as 1, 2, 3", SC11) in plain integer arithmetic: counter-based, so element e of the sample with
// sequence number seq is a function of (seed, seq, e) and of NOTHING else - not of the batch size, the launch geometry or the rank count.
//
//   N0  philox_words    (bsz, groups, 4) uint32: the raw words of group g = e >> 2 of every sample (the integer part, held exactly)
//   N1  philox_normal   (bsz, n) fp32 standard normals, Box-Muller on the words of the element's group
//   N2  sensor_noise    y (bsz, n) -> out (bsz, n): y + sqrt(gain max(y, 0) + sigma^2) normal, then an ADC of `bits` bits over [0, full_scale]
//
// One thread takes one group: ten rounds (40 integer multiplies: a 32 x 32 -> 64 product is a v_mul_lo plus a v_mul_hi), two logf, two
// sqrtf, two sincospif, and its four elements as one float4 where n % 4 == 0 and the pointers are 16-byte aligned, one by one otherwise
// (the same values; the last group of a sample may be partial).  include/deqsci_hip.h states the counter layout and N2's order of
// operations.  The accurate library functions ON PURPOSE: __logf loses hundreds of ulps where u approaches 1, which is where the small
// normals come from.  fp32 with every operation rounded on its own (-ffp-contract=off), both divisions and the square roots the correctly
// rounded ones (hipcc's default).  The per-sample sequence numbers are a HOST array and travel by value in the kernel arguments, 64 per
// launch (csrc/synth.hip's descriptor rows are the precedent).  No allocation, no synchronisation, no atomics; every output element is
// written exactly once, and a thread reads its four inputs before it writes them, so out == y is allowed.
#include "common.hpp"

namespace deqsci {
namespace noise {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;   // the round's two multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;   // the key schedule's increments (golden ratio, sqrt(3) - 1)
constexpr int ROUNDS = 10;
constexpr int WORDS = 0, NORMAL = 1, SENSOR = 2;         // what a launch writes

struct Args {
    uint64_t seq[DEQSCI_NOISE_MAX_ROWS];                 // the samples' sequence numbers: counter words 2 and 3
    const float* y;                                      // SENSOR only
    void* out;                                           // WORDS: uint32 (rows, groups, 4); otherwise float (rows, n)
    uint64_t seed;                                       // the key
    int64_t n, groups;                                   // elements and groups (ceil(n / 4)) per sample
    float sigma, gain, full_scale, levels;               // levels = 2^bits - 1 (exact in fp32 up to 16 bits); 0: no quantiser
};
static_assert(sizeof(Args) <= 4096, "the sequence numbers must fit the kernel-argument segment");

__device__ __forceinline__ uint4 philox4x32_10(uint64_t group, uint64_t seq, uint64_t seed) {
    uint32_t c0 = (uint32_t)group, c1 = (uint32_t)(group >> 32), c2 = (uint32_t)seq, c3 = (uint32_t)(seq >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    return make_uint4(c0, c1, c2, c3);
}

// x -> ((x >> 9) + 0.5) 2^-23: 23 bits, the half and the scaling are all exact in fp32; strictly inside (0,1)
__device__ __forceinline__ float unit(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& na, float& nb) {
    const float r = sqrtf(-2.0f * logf(unit(xa)));
    float s, c;
    sincospif(2.0f * unit(xb), &s, &c);
    na = r * c;
    nb = r * s;
}

__device__ __forceinline__ float4 normals(uint4 w) {
    float4 v;
    box_muller(w.x, w.y, v.x, v.y);
    box_muller(w.z, w.w, v.z, v.w);
    return v;
}

__device__ __forceinline__ bool finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float sensor(float y, float nrm, const Args& a) {
    if (!finite(y)) return y;                            // NaN and +-Inf pass through untouched, also through the quantiser
    const float p = fmaxf(y, 0.0f);
    float v = a.gain * p;
    v = v + a.sigma * a.sigma;
    const float d = sqrtf(v);
    const float t = d * nrm;
    float o = y + t;
    if (a.levels > 0.0f) {
        float c = o / a.full_scale;
        c = fminf(fmaxf(c, 0.0f), 1.0f);
        const float q = rintf(c * a.levels);
        o = (q / a.levels) * a.full_scale;
    }
    return o;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(TB) void philox_kernel(const Args a) {
    const int64_t g = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (g >= a.groups) return;
    const int64_t sample = blockIdx.y;
    const uint4 w = philox4x32_10((uint64_t)g, a.seq[sample], a.seed);
    if (MODE == WORDS) {
        uint32_t* o = static_cast<uint32_t*>(a.out) + (sample * a.groups + g) * 4;
        if (VEC) {
            *reinterpret_cast<uint4*>(o) = w;
        } else {
            o[0] = w.x;
            o[1] = w.y;
            o[2] = w.z;
            o[3] = w.w;
        }
        return;
    }
    const float4 nrm = normals(w);
    const int64_t e = sample * a.n + g * 4;
    float* o = static_cast<float*>(a.out) + e;
    if (VEC) {                                           // n % 4 == 0: every group is whole
        float4 v = nrm;
        if (MODE == SENSOR) {
            const float4 y = ld4(a.y + e);
            v = make_float4(sensor(y.x, nrm.x, a), sensor(y.y, nrm.y, a), sensor(y.z, nrm.z, a), sensor(y.w, nrm.w, a));
        }
        st4(o, v);
    } else {
        const int64_t left = a.n - g * 4;                // >= 1: the last group of a sample may be partial
        const float nr[4] = {nrm.x, nrm.y, nrm.z, nrm.w};
        float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (MODE == SENSOR) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < left) y[k] = a.y[e + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < left) o[k] = MODE == SENSOR ? sensor(y[k], nr[k], a) : nr[k];
    }
}

template <int MODE, bool VEC>
inline int launch_rows(Args& a, const uint64_t* seq, int64_t bsz, int64_t out_stride, hipStream_t stream) {
    const float* y = a.y;
    char* out = static_cast<char*>(a.out);
    const int64_t blocks = ceil_div(a.groups, TB);
    for (int64_t first = 0; first < bsz; first += DEQSCI_NOISE_MAX_ROWS) {
        const int64_t rows = bsz - first < DEQSCI_NOISE_MAX_ROWS ? bsz - first : DEQSCI_NOISE_MAX_ROWS;
        for (int64_t s = 0; s < DEQSCI_NOISE_MAX_ROWS; ++s) a.seq[s] = s < rows ? seq[first + s] : 0;
        a.y = y ? y + first * a.n : nullptr;
        a.out = out + first * out_stride * 4;
        hipLaunchKernelGGL((philox_kernel<MODE, VEC>), dim3((unsigned)blocks, (unsigned)rows), dim3(TB), 0, stream, a);
        if (int e = launch_status()) return e;
    }
    return 0;
}

template <int MODE>
inline int launch(Args& a, const uint64_t* seq, int64_t bsz, int64_t out_stride, bool vec, hipStream_t stream) {
    return vec ? launch_rows<MODE, true>(a, seq, bsz, out_stride, stream) : launch_rows<MODE, false>(a, seq, bsz, out_stride, stream);
}

constexpr int64_t N_MAX = (int64_t)1 << 40;              // elements per call: ceil(n / 4) / 256 workgroups stay far inside the grid's x extent

// the checks the three entry points share; 1: nothing to do (bsz == 0)
inline int check(const void* out, const uint64_t* seq, int64_t bsz, int64_t n) {
    if (bsz < 0 || n < 1 || n > N_MAX || bsz > N_MAX / n) return DEQSCI_ERR_SHAPE;
    if (bsz == 0) return 1;
    if (!out || !seq) return DEQSCI_ERR_NULL;
    if (misaligned(out, 4)) return DEQSCI_ERR_ALIGN;
    return 0;
}

inline Args make_args(const float* y, void* out, int64_t n, uint64_t seed) {
    Args a;
    a.y = y;
    a.out = out;
    a.seed = seed;
    a.n = n;
    a.groups = ceil_div(n, 4);
    a.sigma = a.gain = a.levels = 0.0f;
    a.full_scale = 1.0f;
    return a;
}

inline bool finite_f32(float v) { return v - v == 0.0f; }

}  // namespace noise
}  // namespace deqsci

using namespace deqsci;

extern "C" {

int deqsci_philox_words_u32(uint32_t* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, deqsci_stream_t stream) {
    if (int e = noise::check(out, seq, bsz, n)) return e < 0 ? e : 0;
    noise::Args a = noise::make_args(nullptr, out, n, seed);
    return noise::launch<noise::WORDS>(a, seq, bsz, a.groups * 4, aligned16(out), static_cast<hipStream_t>(stream));
}

int deqsci_philox_normal_f32(float* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, deqsci_stream_t stream) {
    if (int e = noise::check(out, seq, bsz, n)) return e < 0 ? e : 0;
    noise::Args a = noise::make_args(nullptr, out, n, seed);
    return noise::launch<noise::NORMAL>(a, seq, bsz, n, n % 4 == 0 && aligned16(out), static_cast<hipStream_t>(stream));
}

int deqsci_sensor_noise_f32(const float* y, float* out, const uint64_t* seq, int64_t bsz, int64_t n, uint64_t seed, float sigma, float gain,
                            int bits, float full_scale, deqsci_stream_t stream) {
    if (bits < 0 || bits > 16 || !noise::finite_f32(sigma) || sigma < 0.0f || !noise::finite_f32(gain) || gain < 0.0f ||
        !noise::finite_f32(full_scale) || !(full_scale > 0.0f))
        return DEQSCI_ERR_UNSUPPORTED;
    if (int e = noise::check(out, seq, bsz, n)) return e < 0 ? e : 0;
    if (!y) return DEQSCI_ERR_NULL;
    if (misaligned(y, 4)) return DEQSCI_ERR_ALIGN;
    if (y != out && overlaps(y, bsz * n * 4, out, bsz * n * 4)) return DEQSCI_ERR_UNSUPPORTED;      // exactly in place, or apart
    noise::Args a = noise::make_args(y, out, n, seed);
    a.sigma = sigma;
    a.gain = gain;
    a.full_scale = full_scale;
    a.levels = (float)(((int64_t)1 << bits) - 1);
    return noise::launch<noise::SENSOR>(a, seq, bsz, n, n % 4 == 0 && aligned16(y) && aligned16(out), static_cast<hipStream_t>(stream));
}

}  // extern "C"
