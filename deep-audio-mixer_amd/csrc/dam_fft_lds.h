// Workgroup FFT in LDS: the pieces shared by the one-frame-per-workgroup transforms -- the generic dB front-end and the complex
// front-end (dam_stft.hip) and the inverse transform (dam_istft.hip).  The tuned 2048-point kernel shares none of this.
#pragma once
#include "dam_common.h"

namespace dam {

constexpr int FFT_THREADS = 256;

// Channel layouts: interleaved (PLANAR = false: sample p of channel c at trk[CH*p + c], what soundfile / a WAV decoder
// hands over) and planar (PLANAR = true: trk[c*cs + p], the [channels, n] arrays inference_utils.py works on).
// Integer PCM (DAM_PCM_S16 / DAM_PCM_S32: the samples as the WAV file holds them, data/dataset.py:192-196 reads them through
// soundfile, which divides by 2^(bits-1)): every sample is converted to float exactly as that division rounds it, the
// power-of-two scale 2^-(bits-1) rides on the window * gain product (exact), so the result is bit for bit what the float32
// kernel computes from host-converted samples -- without the host conversion and with half the bytes over PCIe for 16 bit.
template <typename PCM> struct pcm_traits { static constexpr bool integer = false; static constexpr float scale = 1.0f; };
template <> struct pcm_traits<int16_t> { static constexpr bool integer = true; static constexpr float scale = 1.0f / 32768.0f; };
template <> struct pcm_traits<int32_t> { static constexpr bool integer = true; static constexpr float scale = 1.0f / 2147483648.0f; };

template <typename PCM>
__device__ __forceinline__ float mean2(PCM a, PCM b) {
    if constexpr (pcm_traits<PCM>::integer) return ((float)a + (float)b) * 0.5f;
    else return (float)((a + b) * (PCM)0.5);
}

template <typename PCM, int CH, bool PLANAR>
__device__ __forceinline__ float mono_at(const PCM* __restrict__ trk, int64_t cs, int64_t p) {
    if (CH == 1) return (float)trk[p];
    if (PLANAR) return mean2<PCM>(trk[p], trk[cs + p]);
    return mean2<PCM>(trk[2 * p], trk[2 * p + 1]);
}

__device__ __forceinline__ int64_t reflect(int64_t p, int64_t n) {
    p = p < 0 ? -p : p;
    return p >= n ? 2 * (n - 1) - p : p;
}

// The frame that starts at sample p0 of the reflect-padded mono signal, packed as M complex points in LDS:
// z[n] = w[2n] g x[2n] + i w[2n+1] g x[2n+1], x = channel mean, summed over n_sum tracks sum_stride apart.  No barrier.
template <typename PCM, int CH, bool PLANAR>
__device__ __forceinline__ void lds_load_frame(float2* z, int M, const PCM* __restrict__ trk, int n_sum, int64_t sum_stride,
                                               int64_t cs, int64_t n_samples, int64_t p0, const float* __restrict__ window,
                                               float g, int tid) {
    for (int n = tid; n < M; n += FFT_THREADS) {
        const int64_t a = reflect(p0 + 2 * n, n_samples), b = reflect(p0 + 2 * n + 1, n_samples);
        float xa = 0.f, xb = 0.f;
        for (int s = 0; s < n_sum; ++s) {
            xa += mono_at<PCM, CH, PLANAR>(trk + s * sum_stride, cs, a);
            xb += mono_at<PCM, CH, PLANAR>(trk + s * sum_stride, cs, b);
        }
        z[n] = make_float2(xa * (window[2 * n] * g), xb * (window[2 * n + 1] * g));
    }
}

// log2(M) autosort (Stockham) radix-2 passes over the M complex points in x[], ping-ponging with y[].
// tw = W_nfft^k = exp(-2 pi i k / n_fft), n_fft = 2 M; INVERSE conjugates it (unnormalised inverse).
// x[] must be complete (barrier passed) on entry; the returned buffer holds the result in natural order, barrier passed.
template <bool INVERSE>
__device__ __forceinline__ float2* lds_fft_radix2(float2* x, float2* y, int M, int n_fft, const float2* __restrict__ tw, int tid) {
    int sshift = 0;                                   // s = 1 << sshift
    for (int n = M; n > 1; n >>= 1, ++sshift) {
        const int m = n >> 1, s = 1 << sshift;
        for (int e = tid; e < (M >> 1); e += FFT_THREADS) {
            const int p = e >> sshift, q = e & (s - 1);
            const float2 a = x[q + s * p], b = x[q + s * (p + m)];
            float2 w = tw[(2 * p * s) & (n_fft - 1)];                       // W_n^p = W_nfft^(2 p s)
            if (INVERSE) w.y = -w.y;
            y[q + s * (2 * p)] = cadd(a, b);
            y[q + s * (2 * p + 1)] = cmul(csub(a, b), w);
        }
        __syncthreads();
        float2* tmp = x; x = y; y = tmp;
    }
    return x;
}

// Real-FFT split: bin k = 0 .. M of the 2M-point transform of the real frame, from the M-point transform Z of its packed form:
// X[k] = E + W^k O, E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2; indices mod M (k = M: W^M = -1, X = E - O).
__device__ __forceinline__ float2 real_fft_bin(const float2* z, int k, int M, const float2* __restrict__ tw) {
    const float2 zk = z[k & (M - 1)], zn = z[(M - k) & (M - 1)];
    const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
    return cadd(e, cmul(tw[k], o));
}

}  // namespace dam
