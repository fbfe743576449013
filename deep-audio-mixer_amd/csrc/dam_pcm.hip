// dam_pcm.hip -- the last step of "stems in, mix out": planar float audio -> interleaved little-endian PCM as a WAV
// `data` chunk holds it (the callers' sf.write: inference.ipynb cells 9/11, evaluation.py:58-66,
// data/listening_test_data_preparation.py), quantised where the master already is.
//
// Per element (frame n, channel c), B = 16 / 24 / 32:
//   v = (double)x * s                 s = scale[0], scale[c], or no product at all (n_scale = 0); one float64 rounding
//   NaN v -> 0, counted as clipped
//   w = v * 2^(B-1)                   exact
//   dither: w = w + d                 d = u1 - u2, u1 / u2 = high / low 32 bits of r over 2^32,
//                                     r = splitmix64 finaliser of seed * 0xD1342543DE82EF95 + (n * channels + c)
//   q = rint(w) (ties to even), clamped to [-2^(B-1), 2^(B-1) - 1]; every clamped element counts in clip_count[c]
//   DAM_WAV_F32: (float)v, no dither, nothing counted.
// tests/_pcm_ref.py restates this in numpy; the kernel is compared with it byte for byte.  TPDF dither of +-1 LSB as a
// pure function of (seed, element): the bytes do not depend on the launch geometry.
//
// Shape: one read of x, one write of out.  A tile is 256 lanes x V frames, V = 16 bytes of one channel row (4 float32 or
// 2 float64 frames per lane and channel).  The lane's piece of the interleaved output is the contiguous V * channels *
// bytes-per-sample bytes behind lane * that: where this is 4, 8, 12 or 16 bytes (stereo 16-bit from float32: 16) the lane
// packs it in registers and stores it whole -- consecutive lanes, consecutive addresses.  Every other case (24-bit with
// an odd lane piece, channel counts whose lane piece exceeds 16 bytes) is transposed through LDS: samples are written to
// their interleaved place in a tile image, which then leaves as 16-byte vectors.  Only the last partial dword of the whole
// buffer is written bytewise.  The grid strides over tiles.
#include "dam_common.h"

namespace dam {
namespace {

constexpr int PCM_THREADS = 256;

typedef unsigned u32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x3_u __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned u32x2_u __attribute__((ext_vector_type(2), aligned(4)));

template <typename T> struct in16;
template <> struct in16<float> { typedef f32x4_u type; static constexpr int V = 4; };
template <> struct in16<double> { typedef f64x2_u type; static constexpr int V = 2; };

__host__ __device__ constexpr int fmt_bytes(int fmt) { return fmt == DAM_WAV_S16 ? 2 : fmt == DAM_WAV_S24 ? 3 : 4; }

__device__ __forceinline__ unsigned long long mix64_full(unsigned long long z) {       // splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One sample -> its code (the low fmt_bytes(FMT) bytes of the result); `clipped` is set, never cleared.
template <int FMT, typename TI>
__device__ __forceinline__ unsigned encode_one(TI x, bool has_scale, double s, bool dither, unsigned long long base,
                                               unsigned long long e, bool& clipped) {
#pragma clang fp contract(off)
    double v = (double)x;
    if (has_scale) v = v * s;
    if (FMT == DAM_WAV_F32) return __float_as_uint((float)v);
    constexpr int B = FMT == DAM_WAV_S16 ? 16 : FMT == DAM_WAV_S24 ? 24 : 32;
    constexpr double FS = (double)(1ll << (B - 1));
    if (v != v) { clipped = true; return 0u; }
    double w = v * FS;
    if (dither) {
        const unsigned long long r = mix64_full(base + e);
        const double d = (double)(unsigned)(r >> 32) * (1.0 / 4294967296.0) - (double)(unsigned)r * (1.0 / 4294967296.0);
        w = w + d;
    }
    double q = rint(w);
    if (q < -FS) { q = -FS; clipped = true; }
    if (q > FS - 1.0) { q = FS - 1.0; clipped = true; }
    return (unsigned)(int)q;
}

// clip bookkeeping: one LDS add per wave and sample slot that clipped at all (a ballot, nothing when nobody clipped)
__device__ __forceinline__ void count_clipped(bool clipped, unsigned* cnt) {
    const unsigned long long m = __ballot(clipped);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(cnt, (unsigned)__popcll(m));
}

// Lane piece of 4 / 8 / 12 / 16 bytes, packed in registers.
template <typename TI, int FMT, int C>
__global__ __launch_bounds__(PCM_THREADS) void pcm_encode_direct_kernel(const TI* __restrict__ x, int64_t n,
                                                                       const double* __restrict__ scale, int n_scale,
                                                                       int dither, unsigned long long seed,
                                                                       unsigned char* __restrict__ out,
                                                                       unsigned long long* __restrict__ clip_count) {
    constexpr int V = in16<TI>::V, BPS = fmt_bytes(FMT), LB = V * C * BPS, NW = LB / 4;
    static_assert(LB % 4 == 0 && LB <= 16, "lane piece must be whole dwords");
    __shared__ unsigned cnt[C];
    if (threadIdx.x < C) cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = seed * 0xD1342543DE82EF95ull;
    double s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = n_scale ? scale[n_scale == 1 ? 0 : c] : 1.0;
    const int64_t tiles = (n + PCM_THREADS * V - 1) / (PCM_THREADS * V);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t f0 = (t * PCM_THREADS + threadIdx.x) * V;
        const int64_t left = n - f0;                                   // frames this lane owns: min(left, V), may be <= 0
        TI xv[C][V];
        if (left >= V) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const typename in16<TI>::type a = *reinterpret_cast<const typename in16<TI>::type*>(x + (int64_t)c * n + f0);
#pragma unroll
                for (int j = 0; j < V; ++j) xv[c][j] = a[j];
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int j = 0; j < V; ++j) xv[c][j] = j < left ? x[(int64_t)c * n + f0 + j] : (TI)0;
        }
        unsigned w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0u;
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                bool clipped = false;
                const unsigned code = encode_one<FMT, TI>(xv[c][j], n_scale != 0, s[c], dither != 0, base,
                                                          (unsigned long long)(f0 + j) * C + c, clipped);
                if (FMT != DAM_WAV_F32) count_clipped(clipped && j < left, &cnt[c]);
                constexpr unsigned MASK = BPS == 4 ? 0xFFFFFFFFu : (1u << (8 * (BPS & 3))) - 1u;
                const unsigned m = code & MASK;
                const int byte = (j * C + c) * BPS;                    // compile-time after unrolling
                w[byte >> 2] |= m << (8 * (byte & 3));
                if ((byte & 3) + BPS > 4) w[(byte >> 2) + 1] |= m >> (8 * (4 - (byte & 3)));
            }
        unsigned char* o = out + f0 * (C * BPS);
        if (left >= V) {
            if (NW == 4) *reinterpret_cast<u32x4_u*>(o) = u32x4_u{w[0], w[1 % NW], w[2 % NW], w[3 % NW]};
            else if (NW == 3) *reinterpret_cast<u32x3_u*>(o) = u32x3_u{w[0], w[1 % NW], w[2 % NW]};
            else if (NW == 2) *reinterpret_cast<u32x2_u*>(o) = u32x2_u{w[0], w[1 % NW]};
            else *reinterpret_cast<unsigned*>(o) = w[0];
        } else if (left > 0) {                                         // the buffer's end: whole dwords, then its last bytes
            const int nb = (int)left * C * BPS;
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                if (4 * (k + 1) <= nb) reinterpret_cast<unsigned*>(o)[k] = w[k];
                else
                    for (int b = 4 * k; b < nb; ++b) o[b] = (unsigned char)(w[k] >> (8 * (b & 3)));
            }
        }
    }
    if (FMT != DAM_WAV_F32 && clip_count) {
        __syncthreads();
        if (threadIdx.x < C && cnt[threadIdx.x]) atomicAdd(&clip_count[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    }
}

// Any channel count and sample width: the tile's interleaved image is assembled in LDS and leaves as 16-byte vectors.
template <typename TI, int FMT>
__global__ __launch_bounds__(PCM_THREADS) void pcm_encode_lds_kernel(const TI* __restrict__ x, int C, int64_t n,
                                                                    const double* __restrict__ scale, int n_scale,
                                                                    int dither, unsigned long long seed,
                                                                    unsigned char* __restrict__ out,
                                                                    unsigned long long* __restrict__ clip_count) {
    constexpr int V = in16<TI>::V, BPS = fmt_bytes(FMT);
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];          // PCM_THREADS * V * C * BPS bytes
    __shared__ unsigned cnt[8];
    if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = seed * 0xD1342543DE82EF95ull;
    const int frame_bytes = C * BPS;
    const int64_t tile_frames = PCM_THREADS * V;
    const int64_t tiles = (n + tile_frames - 1) / tile_frames;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t t0 = t * tile_frames;
        const int64_t f0 = t0 + (int64_t)threadIdx.x * V;
        const int64_t left = n - f0;
        for (int c = 0; c < C; ++c) {
            const double s = n_scale ? scale[n_scale == 1 ? 0 : c] : 1.0;
            TI xv[V];
            if (left >= V) {
                const typename in16<TI>::type a = *reinterpret_cast<const typename in16<TI>::type*>(x + (int64_t)c * n + f0);
#pragma unroll
                for (int j = 0; j < V; ++j) xv[j] = a[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) xv[j] = j < left ? x[(int64_t)c * n + f0 + j] : (TI)0;
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                bool clipped = false;
                const unsigned code = encode_one<FMT, TI>(xv[j], n_scale != 0, s, dither != 0, base,
                                                          (unsigned long long)(f0 + j) * C + c, clipped);
                if (FMT != DAM_WAV_F32) count_clipped(clipped && j < left, &cnt[c]);
                unsigned char* p = tile + ((int)threadIdx.x * V + j) * frame_bytes + c * BPS;
                if (BPS == 4) *reinterpret_cast<unsigned*>(p) = code;
                else if (BPS == 2) *reinterpret_cast<unsigned short*>(p) = (unsigned short)code;
                else { p[0] = (unsigned char)code; p[1] = (unsigned char)(code >> 8); p[2] = (unsigned char)(code >> 16); }
            }
        }
        __syncthreads();
        const int64_t frames = n - t0 < tile_frames ? n - t0 : tile_frames;
        const int nb = (int)frames * frame_bytes;                      // bytes of this tile; a partial tile is the last one
        unsigned char* o = out + t0 * frame_bytes;                     // a multiple of 1024 * V / 4 bytes: dword aligned
        const int n16 = nb >> 4;
        for (int i = threadIdx.x; i < n16; i += PCM_THREADS)
            reinterpret_cast<u32x4_u*>(o)[i] = reinterpret_cast<const u32x4_u*>(tile)[i];
        const int rest = nb - (n16 << 4);                              // < 16 bytes: dwords, then the buffer's last bytes
        if ((int)threadIdx.x < (rest >> 2))
            reinterpret_cast<unsigned*>(o)[n16 * 4 + threadIdx.x] = reinterpret_cast<const unsigned*>(tile)[n16 * 4 + threadIdx.x];
        if ((int)threadIdx.x < (rest & 3)) {
            const int b = (nb & ~3) + threadIdx.x;
            o[b] = tile[b];
        }
        __syncthreads();
    }
    if (FMT != DAM_WAV_F32 && clip_count && (int)threadIdx.x < C && cnt[threadIdx.x])
        atomicAdd(&clip_count[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

template <typename TI, int FMT, int C>
static void launch_direct(dim3 grid, hipStream_t st, const void* x, int64_t n, const double* scale, int n_scale, int dither,
                          uint64_t seed, void* out, unsigned long long* clip) {
    hipLaunchKernelGGL((pcm_encode_direct_kernel<TI, FMT, C>), grid, dim3(PCM_THREADS), 0, st, (const TI*)x, n, scale, n_scale,
                       dither, (unsigned long long)seed, (unsigned char*)out, clip);
}

template <typename TI, int FMT>
static void launch_fmt(int channels, int64_t n, dim3 grid, hipStream_t st, const void* x, const double* scale, int n_scale,
                       int dither, uint64_t seed, void* out, unsigned long long* clip) {
    constexpr int V = in16<TI>::V, BPS = fmt_bytes(FMT);
    if constexpr ((V * BPS) % 4 == 0 && V * BPS <= 16) {
        if (channels == 1) return launch_direct<TI, FMT, 1>(grid, st, x, n, scale, n_scale, dither, seed, out, clip);
    }
    if constexpr ((V * 2 * BPS) % 4 == 0 && V * 2 * BPS <= 16) {
        if (channels == 2) return launch_direct<TI, FMT, 2>(grid, st, x, n, scale, n_scale, dither, seed, out, clip);
    }
    const size_t lds = (size_t)PCM_THREADS * V * channels * BPS;
    hipLaunchKernelGGL((pcm_encode_lds_kernel<TI, FMT>), grid, dim3(PCM_THREADS), lds, st, (const TI*)x, channels, n, scale,
                       n_scale, dither, (unsigned long long)seed, (unsigned char*)out, clip);
}

__global__ void pcm_zero_kernel(unsigned long long* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0ull;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_pcm_tile_frames(int x_is_f64) {
    return (int64_t)dam::PCM_THREADS * (x_is_f64 ? dam::in16<double>::V : dam::in16<float>::V);
}
extern "C" int dam_pcm_max_blocks(void) { return DAM_PCM_MAX_BLOCKS; }

extern "C" int dam_pcm_encode(const void* x, int x_is_f64, int channels, int64_t n_samples, const double* scale, int n_scale,
                              int format, int dither, uint64_t seed, void* out, int64_t* clip_count, void* stream) {
    using namespace dam;
    if (!x || !out || channels < 1 || channels > DAM_PCM_MAX_CHANNELS || n_samples <= 0) return DAM_ERR_BAD_ARG;
    if (n_scale != 0 && n_scale != 1 && n_scale != channels) return DAM_ERR_BAD_ARG;
    if (n_scale != 0 && !scale) return DAM_ERR_BAD_ARG;
    if (format != DAM_WAV_S16 && format != DAM_WAV_S24 && format != DAM_WAV_S32 && format != DAM_WAV_F32) return DAM_ERR_BAD_ARG;
    if (((uintptr_t)out & 3) || ((uintptr_t)x & (x_is_f64 ? 7 : 3))) return DAM_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    // clip_count is overwritten: zeroed first, then every workgroup that clipped adds its count
    unsigned long long* clip = (unsigned long long*)clip_count;
    if (clip) {
        hipLaunchKernelGGL(pcm_zero_kernel, dim3(1), dim3(64), 0, st, clip, channels);
        DAM_CHECK_LAUNCH();
    }
    if (format == DAM_WAV_F32) dither = 0;
    int64_t blocks = cdiv(n_samples, dam_pcm_tile_frames(x_is_f64));
    if (blocks > DAM_PCM_MAX_BLOCKS) blocks = DAM_PCM_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks);
#define DAM_PCM(TI)                                                                                                       \
    switch (format) {                                                                                                     \
        case DAM_WAV_S16: launch_fmt<TI, DAM_WAV_S16>(channels, n_samples, grid, st, x, scale, n_scale, dither, seed, out, clip); break; \
        case DAM_WAV_S24: launch_fmt<TI, DAM_WAV_S24>(channels, n_samples, grid, st, x, scale, n_scale, dither, seed, out, clip); break; \
        case DAM_WAV_S32: launch_fmt<TI, DAM_WAV_S32>(channels, n_samples, grid, st, x, scale, n_scale, dither, seed, out, clip); break; \
        default: launch_fmt<TI, DAM_WAV_F32>(channels, n_samples, grid, st, x, scale, n_scale, dither, seed, out, clip); break;         \
    }
    if (x_is_f64) { DAM_PCM(double) } else { DAM_PCM(float) }
#undef DAM_PCM
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
