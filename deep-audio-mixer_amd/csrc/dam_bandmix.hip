// dam_bandmix.hip -- the band-gain mixer: the audio of per-stem, per-band, per-window gains (what dam_bandfit_solve_grouped
// fits), rendered in one pass over the stems (include/dam_hip.h states the definition).
//
// Two kernels:
//   frames    one workgroup = one frame of one channel.  For every stem in turn: the band fit's transform of the frame (the
//             front-end's LDS FFT, dam_fft_lds.h, read through the gain fit's element strides), the real-FFT split, and
//             acc[k] += e[s][band(k)] * X_s[k] in registers -- thread `tid` owns bins tid, tid + 256, ... below n_fft/2 and
//             lane 0 the real bin n_fft/2.  After the last stem: the mix spectrum packed into its n_fft/2-point form (the
//             pre-twiddle of istft_kernel), the inverse LDS FFT, the synthesis window and irfft's scale, and the frame written
//             to the workspace.  No stem spectrum and no mix spectrum reaches global memory.              (frame, channel) grid
//   gather    one lane = one output sample: the frames that cover it, added in ascending frame order, over the squared-window
//             envelope.  No atomics.                                                              (256 samples, channel) grid
// The bins a thread owns are a template parameter (NB = max(1, n_fft / 512)), so that the running sums are named registers.
// The effective gains of the frame's window, float [S][B + 1] (the last column: the bins outside every band), and the clamped
// edge table sit in 2.3 KB of static LDS beside the transform's two n_fft/2-point buffers.
#include "dam_common.h"
#include "dam_fft_lds.h"

#pragma clang fp contract(off)        // the transform is the band fit's, operation by operation; the fused multiply-adds are written out

namespace dam {
namespace {

constexpr int BM_MAX_S = DAM_GAINFIT_MAX_STEMS;
constexpr int BM_MAX_BANDS = 64;                      // dam_spectrum_max_bands(); checked at the entry
constexpr int BM_GATHER_THREADS = 256;

__device__ __forceinline__ bool finite_f64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

template <typename TX, int NB>
__global__ __launch_bounds__(FFT_THREADS) void bandmix_frames_kernel(
    const TX* __restrict__ x, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, int S, int64_t n_samples,
    const double* __restrict__ gains, const double* __restrict__ fill, const int* __restrict__ edges, int B, int W,
    const float* __restrict__ window, const float2* __restrict__ tw, int n_fft, int hop, int T, float* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M]
    __shared__ float eff[BM_MAX_S][BM_MAX_BANDS + 1];
    __shared__ int edge[BM_MAX_BANDS + 1];
    const int tid = threadIdx.x, M = n_fft >> 1;
    const int t = (int)blockIdx.x, c = (int)blockIdx.y;
    // the frame's window: the gain index of its centre sample (the band fit's w(t))
    const int64_t centre = (int64_t)t * hop < n_samples - 1 ? (int64_t)t * hop : n_samples - 1;
    const int64_t wq = centre / (n_samples / W);
    const int w = wq < W - 1 ? (int)wq : W - 1;
    for (int i = tid; i < S * (B + 1); i += FFT_THREADS) {
        const int s = i / (B + 1), b = i - s * (B + 1);
        const double f = fill[(int64_t)s * W + w];
        double e = finite_f64(f) ? f : 0.0;
        if (b < B) {
            const double g = gains[((int64_t)b * S + s) * W + w];
            if (finite_f64(g)) e = g;
        }
        eff[s][b] = (float)e;
    }
    for (int i = tid; i <= B; i += FFT_THREADS) {
        const int e = edges[i];
        edge[i] = e < 0 ? 0 : e > M + 1 ? M + 1 : e;  // a bad table gives wrong numbers, never an access out of bounds
    }
    __syncthreads();
    // the band of every bin this thread owns: the lowest b with edge[b] <= k < edge[b+1]; B: outside every band
    int band[NB], band_nyq = B;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int k = tid + FFT_THREADS * i;
        int b = 0;
        while (b < B && !(edge[b] <= k && k < edge[b + 1])) ++b;
        band[i] = b;
    }
    if (tid == 0) {
        int b = 0;
        while (b < B && !(edge[b] <= M && M < edge[b + 1])) ++b;
        band_nyq = b;
    }
    float2 acc[NB];
    float acc_nyq = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = make_float2(0.f, 0.f);

    const int64_t p0 = (int64_t)t * hop - M;
    for (int s = 0; s < S; ++s) {
        const TX* trk = x + s * stem_stride + c * channel_stride;
        for (int i = tid; i < M; i += FFT_THREADS) {
            const int64_t a = reflect(p0 + 2 * i, n_samples), b = reflect(p0 + 2 * i + 1, n_samples);
            buf[i] = make_float2((float)trk[a * sample_stride] * window[2 * i], (float)trk[b * sample_stride] * window[2 * i + 1]);
        }
        __syncthreads();
        const float2* z = lds_fft_radix2<false>(buf, buf + M, M, n_fft, tw, tid);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = tid + FFT_THREADS * i;
            if (k < M) {
                float2 xk = real_fft_bin(z, k, M, tw);
                if (k == 0) xk.y = 0.f;               // DC of a real signal
                const float e = eff[s][band[i]];
                acc[i].x = fmaf(e, xk.x, acc[i].x);
                acc[i].y = fmaf(e, xk.y, acc[i].y);
            }
        }
        if (tid == 0) acc_nyq = fmaf(eff[s][band_nyq], real_fft_bin(z, M, M, tw).x, acc_nyq);
        __syncthreads();                              // the buffers are rewritten by the next stem's frame
    }
    // the mix spectrum Y[0 .. M-1] in the first buffer, the real bin M in the unused imaginary part of bin 0
    float2* Y = buf;
    float2* Z = buf + M;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int k = tid + FFT_THREADS * i;
        if (k < M) Y[k] = k == 0 ? make_float2(acc[i].x, acc_nyq) : acc[i];
    }
    __syncthreads();
    // pre-twiddle (istft_kernel's): Z[k] = E[k] + i O[k], E = Y[k] + conj(Y[M-k]), O = (Y[k] - conj(Y[M-k])) conj(W^k)
    for (int k = tid; k <= (M >> 1); k += FFT_THREADS) {
        float2 xk = Y[k], xn = Y[(M - k) & (M - 1)];
        if (k == 0) { xn = make_float2(xk.y, 0.f); xk.y = 0.f; }
        const float2 e = make_float2(xk.x + xn.x, xk.y - xn.y);
        const float2 d = make_float2(xk.x - xn.x, xk.y + xn.y);
        const float2 wk = tw[k];
        const float2 o = cmul(d, make_float2(wk.x, -wk.y));
        Z[k] = make_float2(e.x - o.y, e.y + o.x);
        if (k) Z[M - k] = make_float2(e.x + o.y, o.x - e.y);
    }
    __syncthreads();
    const float* y = reinterpret_cast<const float*>(lds_fft_radix2<true>(Z, Y, M, n_fft, tw, tid));
    // sample j of the frame is y[j]; irfft's 1/n_fft and the halves of the real-FFT split ride on the window (a power of two)
    const float scale = 0.5f / (float)M;
    float* o = frames + ((int64_t)c * T + t) * n_fft;
    for (int j = tid; j < n_fft; j += FFT_THREADS) o[j] = (window[j] * scale) * y[j];
}

// One lane per output sample: its covering frames in ascending order.
__global__ __launch_bounds__(BM_GATHER_THREADS) void bandmix_gather_kernel(const float* __restrict__ frames,
                                                                           const float* __restrict__ window, int n_fft, int hop,
                                                                           int T, int64_t n_samples, float* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BM_GATHER_THREADS + threadIdx.x;
    if (p >= n_samples) return;
    const int c = (int)blockIdx.y;
    const int64_t a = p + (n_fft >> 1);               // the sample's place in the centred signal: frame t covers [t hop, t hop + n_fft)
    const int64_t t_first = a - n_fft < 0 ? 0 : (a - n_fft) / hop + 1;
    int64_t t_last = a / hop;
    if (t_last > T - 1) t_last = T - 1;
    const float* f = frames + (int64_t)c * T * n_fft;
    float acc = 0.f, env = 0.f;
    for (int64_t t = t_first; t <= t_last; ++t) {
        const int j = (int)(a - t * hop);
        const float wj = window[j];
        acc = acc + f[t * n_fft + j];
        env = fmaf(wj, wj, env);
    }
    out[(int64_t)c * n_samples + p] = env > 1e-11f ? acc / env : 0.f;          // torch.istft's envelope threshold
}

int check_args(int64_t n_samples, int channels, int n_fft, int hop) {
    if ((channels != 1 && channels != 2) || n_fft < 64 || n_fft > 16384 || (n_fft & (n_fft - 1)) || hop < 1) return DAM_ERR_BAD_ARG;
    if (n_samples <= n_fft / 2) return DAM_ERR_BAD_ARG;
    if (hop > n_fft / 2) return DAM_ERR_UNSUPPORTED;  // dam_istft_f32's rule: the squared-window envelope must not vanish
    if (1 + n_samples / hop > 0x7fffffff / 2 || cdiv(n_samples, BM_GATHER_THREADS) > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    return DAM_OK;
}

// first frame of window w, as the band fit counts them (dam_bandfit.hip: frame_lo)
int64_t first_frame(int64_t seg, int hop, int T, int W, int w) {
    if (w <= 0) return 0;
    if (w >= W) return T;
    const int64_t t = cdiv((int64_t)w * seg, hop);
    return t < T ? t : T;
}

template <typename TX, int NB>
int launch_frames(const void* x, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, int S, int channels,
                  int64_t n_samples, const double* gains, const double* fill, const int32_t* edges, int B, int W,
                  const float* window, const float* twiddles, int n_fft, int hop, int T, float* frames, hipStream_t s) {
    const size_t lds = (size_t)n_fft * sizeof(float2);        // two buffers of n_fft/2 complex points
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit
    if (lds > 48 * 1024 && !raise_lds_limit<&bandmix_frames_kernel<TX, NB>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((bandmix_frames_kernel<TX, NB>), dim3((unsigned)T, (unsigned)channels), dim3(FFT_THREADS), lds, s,
                       (const TX*)x, stem_stride, sample_stride, channel_stride, S, n_samples, gains, fill, edges, B, W, window,
                       reinterpret_cast<const float2*>(twiddles), n_fft, hop, T, frames);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

#define BM_FRAMES(TX, NB) launch_frames<TX, NB>(x, stem_stride, sample_stride, channel_stride, S, channels, n_samples, gains, fill, \
                                                edges, B, W, window, twiddles, n_fft, hop, T, frames, s)

template <typename TX>
int dispatch_frames(const void* x, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, int S, int channels,
                    int64_t n_samples, const double* gains, const double* fill, const int32_t* edges, int B, int W,
                    const float* window, const float* twiddles, int n_fft, int hop, int T, float* frames, hipStream_t s) {
    switch (n_fft) {                                  // NB = max(1, n_fft / 512): the bins below n_fft/2 a thread owns
        case 16384: return BM_FRAMES(TX, 32);
        case 8192: return BM_FRAMES(TX, 16);
        case 4096: return BM_FRAMES(TX, 8);
        case 2048: return BM_FRAMES(TX, 4);
        case 1024: return BM_FRAMES(TX, 2);
        default: return BM_FRAMES(TX, 1);
    }
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_bandmix_workspace_bytes(int64_t n_samples, int channels, int n_fft, int hop) {
    if (dam::check_args(n_samples, channels, n_fft, hop) != DAM_OK) return 0;
    return (int64_t)sizeof(float) * channels * (1 + n_samples / hop) * n_fft;
}

extern "C" int dam_bandmix_render(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                                  int64_t sample_stride, int64_t channel_stride, const double* gains, const double* fill,
                                  const int32_t* edges, int n_bands, int n_windows, const float* window, const float* twiddles,
                                  int n_fft, int hop, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace dam;
    if (!x || !gains || !fill || !edges || !window || !twiddles || !out || !workspace) return DAM_ERR_BAD_ARG;
    if (n_stems < 1 || n_stems > BM_MAX_S || n_bands < 1 || n_bands > BM_MAX_BANDS || n_bands > dam_spectrum_max_bands())
        return DAM_ERR_BAD_ARG;
    const int rc = check_args(n_samples, channels, n_fft, hop);
    if (rc != DAM_OK) return rc;
    if (n_windows < 1 || n_windows > n_samples) return DAM_ERR_BAD_ARG;
    const int T = (int)(1 + n_samples / hop), S = n_stems, B = n_bands, W = n_windows;
    const int64_t seg = n_samples / W;
    for (int w = 0; w < W; ++w)                       // every window owns a frame, as in the band fit
        if (first_frame(seg, hop, T, W, w + 1) - first_frame(seg, hop, T, W, w) < 1) return DAM_ERR_BAD_ARG;
    if (workspace_bytes < dam_bandmix_workspace_bytes(n_samples, channels, n_fft, hop)) return DAM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* frames = static_cast<float*>(workspace);
    const int st = x_is_f64 ? dispatch_frames<double>(x, stem_stride, sample_stride, channel_stride, S, channels, n_samples, gains,
                                                      fill, edges, B, W, window, twiddles, n_fft, hop, T, frames, s)
                            : dispatch_frames<float>(x, stem_stride, sample_stride, channel_stride, S, channels, n_samples, gains,
                                                     fill, edges, B, W, window, twiddles, n_fft, hop, T, frames, s);
    if (st != DAM_OK) return st;
    hipLaunchKernelGGL(bandmix_gather_kernel, dim3((unsigned)cdiv(n_samples, BM_GATHER_THREADS), (unsigned)channels),
                       dim3(BM_GATHER_THREADS), 0, s, frames, window, n_fft, hop, T, n_samples, out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
