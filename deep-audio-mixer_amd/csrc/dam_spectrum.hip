// dam_spectrum.hip -- long-term average spectrum (LTAS) in fractional-octave bands of gain-ramped stem sums, and the
// spectral-balance error of candidate mixes against a reference mix (include/dam_hip.h states the definition).
//
// The reference judges a mix by level only (evaluation.py:39-53: per-stem loudness relative to the stems' mean) although the
// model is trained on a spectral objective (model_trainer.py:34-35); its author compares summed-stem spectrograms with the
// mix spectrogram by hand in experiments.ipynb.  This is that comparison as a number: the band powers of "stems x gain
// ramps", time-averaged, relative to their total.  The evaluator expresses every variant of a song as gains on resident
// stems, so the kernel sums the stems with their gains AS IT LOADS a frame -- no mix and no STFT is ever written; what
// leaves a workgroup is one float64 [bands] partial.
//   band power  one workgroup = SPEC_F consecutive frames of one mix: load (stems x gains, channel mean, window) -> the LDS
//               radix-2 FFT of dam_fft_lds.h -> real-FFT split -> |X|^2 added in float64 to the lane's own bins; after the
//               last frame the bins are folded into bands, 64 lanes and one butterfly per band     (frame run, mix) grid
//   reduce      a mix's partials added in ascending workgroup order, divided by the frame count     one workgroup per mix
//   error       mean |L_cand - L_ref| over the bands both spectra hold above -70 dB of their total  one per candidate
// Not tuned beyond its structure: the loader reads sample by sample through runtime strides (any layout, float32 / float64).
#include "dam_common.h"
#include "dam_fft_lds.h"
#include "dam_spectrum_load.h"   // SpecGeo, mix_pair: the loader, shared with dam_specdist.hip

#pragma clang fp contract(off)        // the mix signal and the sums are stated operation by operation; no fused multiply-add

namespace dam {
namespace {

constexpr int SPEC_F = 8;             // frames one workgroup owns: a library constant, never a function of the batch
constexpr int SPEC_MAX_BANDS = 64;

// PER = bins 0 .. M-1 a lane owns (M / 256, at least 1); the Nyquist bin M rides on lane 0.  The running sums are a
// compile-time array so that they stay in registers (32 doubles at n_fft = 16384).  Only PER = 1 (M may be below 256) tests
// k < M: as a test per i the frame-invariant lane masks, one SGPR pair each, were hoisted and 59 SGPRs spilled at PER = 32.
template <typename T, int PER>
__global__ __launch_bounds__(FFT_THREADS) void spectrum_band_power_kernel(
    const T* __restrict__ x, int64_t mix_stride, const double* __restrict__ gains, const float* __restrict__ window,
    const float2* __restrict__ tw /* W_nfft^k */, const int* __restrict__ edges, SpecGeo g, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M]; afterwards M + 1 doubles of bin sums
    const int tid = threadIdx.x, M = g.n_fft >> 1;
    const int r = blockIdx.y, blk = blockIdx.x;
    const T* xr = x + (int64_t)r * mix_stride;
    const double* gr = gains ? gains + (int64_t)r * g.n_stems * g.n_gains : nullptr;
    double acc[PER], nyq = 0.0;
#pragma unroll
    for (int i = 0; i < PER; ++i) acc[i] = 0.0;
    const int t0 = blk * SPEC_F, t1 = t0 + SPEC_F < g.n_frames ? t0 + SPEC_F : g.n_frames;
    for (int t = t0; t < t1; ++t) {
        const int64_t p0 = (int64_t)t * g.hop - M;
        for (int n = tid; n < M; n += FFT_THREADS) {
            const int64_t a = reflect(p0 + 2 * n, g.n_samples), b = reflect(p0 + 2 * n + 1, g.n_samples);
            const float2 xm = mix_pair<T>(xr, gr, g, a, b);
            buf[n] = make_float2(xm.x * window[2 * n], xm.y * window[2 * n + 1]);
        }
        __syncthreads();
        const float2* z = lds_fft_radix2<false>(buf, buf + M, M, g.n_fft, tw, tid);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = tid + FFT_THREADS * i;
            if (PER > 1 || k < M) {                                   // PER > 1: M = 256 PER, every k is a bin
                float2 xk = real_fft_bin(z, k, M, tw);
                if (k == 0) xk.y = 0.f;                               // DC of a real signal
                const double pw = (double)xk.x * (double)xk.x + (double)xk.y * (double)xk.y;
                acc[i] += k == 0 ? pw : 2.0 * pw;
            }
        }
        if (tid == 0) {                                               // Nyquist, real as well
            const float2 xk = real_fft_bin(z, M, M, tw);
            nyq += (double)xk.x * (double)xk.x;
        }
        __syncthreads();                                              // z is read: the next frame (or the bin sums) may land
    }
    double* binsum = reinterpret_cast<double*>(buf);                  // 8 (M + 1) bytes of the 16 M the block holds
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = tid + FFT_THREADS * i;
        if (PER > 1 || k < M) binsum[k] = acc[i];
    }
    if (tid == 0) binsum[M] = nyq;
    __syncthreads();
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    double* out = partial + ((int64_t)r * g.blocks_per_mix + blk) * g.n_bands;
    for (int b = wave; b < g.n_bands; b += FFT_THREADS / WAVE) {      // wave-uniform
        int lo = edges[b], hi = edges[b + 1];
        lo = lo < 0 ? 0 : (lo > M + 1 ? M + 1 : lo);
        hi = hi < 0 ? 0 : (hi > M + 1 ? M + 1 : hi);
        double s = 0.0;
        for (int k = lo + lane; k < hi; k += WAVE) s += binsum[k];
        for (int m = 1; m < WAVE; m <<= 1) s += __shfl_xor(s, m);
        if (lane == 0) out[b] = s;
    }
}

__global__ __launch_bounds__(SPEC_MAX_BANDS) void spectrum_reduce_kernel(const double* __restrict__ partial, int blocks_per_mix,
                                                                        int n_bands, int n_frames, double* __restrict__ power) {
    const int b = threadIdx.x;
    if (b >= n_bands) return;
    const double* p = partial + (int64_t)blockIdx.x * blocks_per_mix * n_bands + b;
    double s = 0.0;
#pragma unroll 8                                                      // eight loads in flight; the additions stay in ascending order
    for (int i = 0; i < blocks_per_mix; ++i) s += p[(int64_t)i * n_bands];
    power[(int64_t)blockIdx.x * n_bands + b] = s / (double)n_frames;
}

__global__ __launch_bounds__(WAVE) void spectrum_balance_error_kernel(const double* __restrict__ ref,
                                                                     const double* __restrict__ cand_all, int n_bands,
                                                                     double* __restrict__ err, int* __restrict__ n_kept) {
    const int b = threadIdx.x;
    const double* cand = cand_all + (int64_t)blockIdx.x * n_bands;
    double tr = 0.0, tc = 0.0;                                        // every lane forms the same ascending sums
    for (int j = 0; j < n_bands; ++j) { tr += ref[j]; tc += cand[j]; }
    const double pr = b < n_bands ? ref[b] : 0.0, pc = b < n_bands ? cand[b] : 0.0;
    const bool keep = b < n_bands && pr >= DAM_SPECTRUM_GATE * tr && pc >= DAM_SPECTRUM_GATE * tc;
    const double d = keep ? fabs(10.0 * log10(pc / tc) - 10.0 * log10(pr / tr)) : 0.0;
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < n_bands; ++j) {                               // ascending b, all 64 lanes in step
        const double dj = __shfl(d, j);
        const int kj = __shfl((int)keep, j);
        if (kj) { sum += dj; ++n; }
    }
    if (b == 0) {
        err[blockIdx.x] = n ? sum / (double)n : __longlong_as_double(0x7ff8000000000000ll);
        n_kept[blockIdx.x] = n;
    }
}

template <typename T, int PER>
int launch_band_power(const void* x, int64_t mix_stride, const double* gains, const float* window, const float* twiddles,
                      const int32_t* edges, const SpecGeo& g, int n_mixes, double* partial, hipStream_t s) {
    const size_t lds = (size_t)g.n_fft * sizeof(float2);              // two images of n_fft/2 complex points
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit (the kernel has no static LDS beside it)
    if (lds > 48 * 1024 && !raise_lds_limit<&spectrum_band_power_kernel<T, PER>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((spectrum_band_power_kernel<T, PER>), dim3((unsigned)g.blocks_per_mix, (unsigned)n_mixes),
                       dim3(FFT_THREADS), lds, s, (const T*)x, mix_stride, gains, window, reinterpret_cast<const float2*>(twiddles),
                       edges, g, partial);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

template <typename T>
int dispatch_band_power(int per, const void* x, int64_t mix_stride, const double* gains, const float* window,
                        const float* twiddles, const int32_t* edges, const SpecGeo& g, int n_mixes, double* partial,
                        hipStream_t s) {
    switch (per) {
        case 1: return launch_band_power<T, 1>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
        case 2: return launch_band_power<T, 2>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
        case 4: return launch_band_power<T, 4>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
        case 8: return launch_band_power<T, 8>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
        case 16: return launch_band_power<T, 16>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
        default: return launch_band_power<T, 32>(x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
    }
}

}  // namespace
}  // namespace dam

extern "C" int dam_spectrum_frames_per_block(void) { return dam::SPEC_F; }
extern "C" int dam_spectrum_max_bands(void) { return dam::SPEC_MAX_BANDS; }

extern "C" int64_t dam_spectrum_workspace_bytes(int n_mixes, int64_t n_samples, int hop, int n_bands) {
    if (n_mixes <= 0 || n_samples <= 0 || hop <= 0 || n_bands <= 0) return 0;
    const int64_t n_frames = 1 + n_samples / hop;
    return (int64_t)n_mixes * dam::cdiv(n_frames, dam::SPEC_F) * n_bands * (int64_t)sizeof(double);
}

extern "C" int dam_spectrum_band_power(const void* x, int x_is_f64, int n_mixes, int n_stems, int channels, int64_t n_samples,
                                       int64_t mix_stride, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride,
                                       const double* gains, int n_gains, const float* window, const float* twiddles, int n_fft,
                                       int hop, const int32_t* edges, int n_bands, double* power, void* workspace,
                                       void* stream) {
    using namespace dam;
    if (!x || !window || !twiddles || !edges || !power || !workspace) return DAM_ERR_BAD_ARG;
    if (n_mixes <= 0 || n_stems <= 0 || n_samples <= 0) return DAM_ERR_BAD_ARG;
    if (channels != 1 && channels != 2) return DAM_ERR_BAD_ARG;
    if (n_fft < 64 || n_fft > 16384 || (n_fft & (n_fft - 1))) return DAM_ERR_BAD_ARG;
    if (hop < 1 || n_samples <= n_fft / 2) return DAM_ERR_BAD_ARG;    // reflect padding needs n > n_fft/2
    if (gains && (n_gains < 1 || n_gains > n_samples)) return DAM_ERR_BAD_ARG;
    if (n_bands < 1 || n_bands > SPEC_MAX_BANDS || n_mixes > 65535) return DAM_ERR_BAD_ARG;
    const int64_t n_frames = 1 + n_samples / hop;
    if (n_frames > 0x7fffffff) return DAM_ERR_BAD_ARG;
    SpecGeo g;
    g.n_samples = n_samples; g.stem_stride = stem_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.n_stems = n_stems; g.channels = channels; g.n_gains = gains ? n_gains : 1;
    g.gseg = n_samples / g.n_gains;
    g.n_fft = n_fft; g.hop = hop; g.n_frames = (int)n_frames; g.n_bands = n_bands;
    g.blocks_per_mix = (int)cdiv(n_frames, SPEC_F);
    g.small = n_samples < 0x7fffffff ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    const int per = n_fft / 2 >= FFT_THREADS ? n_fft / 2 / FFT_THREADS : 1;
    const int rc = x_is_f64 ? dispatch_band_power<double>(per, x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s)
                            : dispatch_band_power<float>(per, x, mix_stride, gains, window, twiddles, edges, g, n_mixes, partial, s);
    if (rc != DAM_OK) return rc;
    hipLaunchKernelGGL(spectrum_reduce_kernel, dim3((unsigned)n_mixes), dim3(SPEC_MAX_BANDS), 0, s, partial, g.blocks_per_mix,
                       n_bands, g.n_frames, power);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_spectrum_balance_error(const double* ref_power, const double* cand_power, int n_variants, int n_bands,
                                          double* err, int32_t* n_kept, void* stream) {
    using namespace dam;
    if (!ref_power || !cand_power || !err || !n_kept || n_variants <= 0 || n_bands < 1 || n_bands > SPEC_MAX_BANDS)
        return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(spectrum_balance_error_kernel, dim3((unsigned)n_variants), dim3(WAVE), 0, (hipStream_t)stream, ref_power,
                       cand_power, n_bands, err, n_kept);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
