// dam_istft.hip -- inverse STFT (torch.istft, center=True, onesided, Hann synthesis window = analysis window) for gfx950.
//
// Stands for experiments.ipynb cell 53 of the reference (librosa.istft(db_to_amplitude(masked) * phases, hop_length=512))
// and, with the complex front-end of dam_stft.hip, for cells 44 and 50 (the phases of the STFT of the stems' sum).
//
// Overlap-add scheme: a GATHER, no atomics.  A workgroup owns ISTFT_SEG consecutive output samples of one track and
// keeps their numerator and squared-window envelope in registers (one sample per thread and 256-sample row).  It walks the
// frames that reach into its segment in ascending order; each frame is inverted by the whole workgroup in LDS (real-FFT
// pre-twiddle -> n_fft/2-point complex inverse FFT) and every thread adds the samples of that frame that fall on its own
// positions.  Every output sample is therefore the sum of its covering frames in frame order, whatever the batch size or
// the segment it falls in: bit-identical between runs and between batch sizes.  The price is that the n_fft/hop - 1 frames
// straddling a segment border are inverted by both neighbours (2048 / 1024: 9 transforms for 8 frames' worth of output).
#include "dam_fft_lds.h"

namespace dam {
namespace {

constexpr int ISTFT_SEG = 8192;                         // output samples per workgroup
constexpr int ISTFT_ROWS = ISTFT_SEG / FFT_THREADS;     // accumulators per thread

// One spectrum bin as the transform uses it: `spec`, or 10^(0.05 mag_db) on the phase of `spec` ((1, 0) where spec == 0).
__device__ __forceinline__ float2 load_bin(const float2* __restrict__ spec, const float* __restrict__ mag_db, int64_t idx) {
    float2 x = spec[idx];
    if (mag_db) {
        const float db = mag_db[idx];
        // 10^(db/20) = 2^(db * c), c = log2(10)/20 split in two floats so that the exponent carries no rounding of its own
        constexpr float C_HI = 0.16609640419483185f, C_LO = 5.4953625e-10f, LN2 = 0.69314718055994531f;
        const float p = db * C_HI;
        const float r = fmaf(db, C_HI, -p) + db * C_LO;
        const float amp = exp2f(p) * fmaf(LN2, r, 1.0f);
        const float m = fmaxf(fabsf(x.x), fabsf(x.y));
        if (m > 0.f) {
            const float xs = x.x / m, ys = x.y / m;         // scaled first: no overflow or underflow in the norm
            const float inv = 1.0f / sqrtf(xs * xs + ys * ys);
            x = make_float2(amp * (xs * inv), amp * (ys * inv));
        } else {
            x = make_float2(amp, 0.f);
        }
    }
    return x;
}

__global__ __launch_bounds__(FFT_THREADS) void istft_kernel(
    const float2* __restrict__ spec, const float* __restrict__ mag_db, const float* __restrict__ window,
    const float2* __restrict__ tw /* W_nfft^k */, int n_fft, int hop, int n_frames, int64_t length, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M]
    const int tid = threadIdx.x;
    const int M = n_fft >> 1;
    const int64_t track = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * ISTFT_SEG;
    // in the centred (padded) signal frame t covers [t hop, t hop + n_fft) and output sample n sits at n + M
    const int64_t a = s0 + M;
    const int64_t t_first = a - n_fft < 0 ? 0 : (a - n_fft) / hop + 1;              // first t with t hop + n_fft > a
    int64_t t_last = (a + ISTFT_SEG - 1) / hop;                                     // last t with t hop < a + SEG
    if (t_last > n_frames - 1) t_last = n_frames - 1;
    const float2* sp = spec + track * (int64_t)(M + 1) * n_frames;
    const float* db = mag_db ? mag_db + track * (int64_t)(M + 1) * n_frames : nullptr;
    const float scale = 0.5f / (float)M;              // the halves of the real-FFT split and irfft's 1/n_fft (a power of two)
    float acc[ISTFT_ROWS], env[ISTFT_ROWS];
#pragma unroll
    for (int i = 0; i < ISTFT_ROWS; ++i) acc[i] = env[i] = 0.f;

    for (int64_t t = t_first; t <= t_last; ++t) {
        // pre-twiddle: Z[k] = E[k] + i O[k], E = X[k] + conj(X[M-k]), O = (X[k] - conj(X[M-k])) conj(W^k); Z[M-k] = conj(E) + i conj(O)
        for (int k = tid; k <= (M >> 1); k += FFT_THREADS) {
            float2 xk = load_bin(sp, db, (int64_t)k * n_frames + t), xn = load_bin(sp, db, (int64_t)(M - k) * n_frames + t);
            if (k == 0) xk.y = xn.y = 0.f;            // DC and Nyquist: irfft ignores their imaginary parts
            const float2 e = make_float2(xk.x + xn.x, xk.y - xn.y);
            const float2 d = make_float2(xk.x - xn.x, xk.y + xn.y);
            const float2 w = tw[k];
            const float2 o = cmul(d, make_float2(w.x, -w.y));
            buf[k] = make_float2(e.x - o.y, e.y + o.x);
            if (k) buf[M - k] = make_float2(e.x + o.y, o.x - e.y);
        }
        __syncthreads();
        const float* z = reinterpret_cast<const float*>(lds_fft_radix2<true>(buf, buf + M, M, n_fft, tw, tid));
        // x[2n] = Re z[n], x[2n+1] = Im z[n]: sample j of the frame is z[j] read as floats
        const int off = (int)(t * hop - a);                               // frame sample j lands on segment position j + off
#pragma unroll
        for (int i = 0; i < ISTFT_ROWS; ++i) {
            if (FFT_THREADS * (i + 1) <= off || FFT_THREADS * i >= off + n_fft) continue;        // workgroup-uniform
            const int j = tid + FFT_THREADS * i - off;
            if (j >= 0 && j < n_fft) {
                const float w = window[j];
                acc[i] = fmaf(w * scale, z[j], acc[i]);
                env[i] = fmaf(w, w, env[i]);
            }
        }
        __syncthreads();                                                  // the buffers are rewritten by the next frame
    }
    float* o = out + track * length;
#pragma unroll
    for (int i = 0; i < ISTFT_ROWS; ++i) {
        const int64_t n = s0 + tid + FFT_THREADS * i;
        if (n < length) o[n] = env[i] > 1e-11f ? acc[i] / env[i] : 0.f;   // torch.istft's envelope threshold; uncovered samples are 0
    }
}

bool istft_geometry_ok(int n_fft, int hop) {
    return n_fft >= 64 && n_fft <= 16384 && !(n_fft & (n_fft - 1)) && hop >= 1 && hop <= n_fft / 2;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_istft_workspace_bytes(int64_t n_tracks, int64_t n_frames, int n_fft, int hop, int64_t length) {
    if (n_tracks <= 0 || n_frames <= 0 || length <= 0 || !dam::istft_geometry_ok(n_fft, hop)) return -1;
    return 0;                   // the gather keeps its partial sums in registers
}

extern "C" int dam_istft_f32(const float* spec, const float* mag_db, int64_t n_tracks, int64_t n_frames, int n_fft, int hop,
                             int64_t length, const float* window, const float* twiddles, float* out, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    using namespace dam;
    if (n_tracks <= 0 || n_frames <= 0 || length <= 0 || n_fft <= 0 || hop <= 0 || workspace_bytes < 0) return DAM_ERR_BAD_ARG;
    if (!istft_geometry_ok(n_fft, hop)) return DAM_ERR_UNSUPPORTED;
    if (n_tracks > 65535 || n_frames > 0x7fffffff / 2 || cdiv(length, ISTFT_SEG) > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    if (!spec || !window || !twiddles || !out) return DAM_ERR_BAD_ARG;
    (void)workspace;
    const size_t lds = (size_t)n_fft * sizeof(float2);                // two buffers of n_fft/2 complex points
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit
    if (lds > 48 * 1024 && !raise_lds_limit<&istft_kernel>(132 * 1024)) return DAM_ERR_LAUNCH;
    const dim3 grid((unsigned)cdiv(length, ISTFT_SEG), (unsigned)n_tracks);
    hipLaunchKernelGGL(istft_kernel, grid, dim3(FFT_THREADS), lds, (hipStream_t)stream, reinterpret_cast<const float2*>(spec),
                       mag_db, window, reinterpret_cast<const float2*>(twiddles), n_fft, hop, (int)n_frames, length, out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
