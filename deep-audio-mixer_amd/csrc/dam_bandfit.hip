// dam_bandfit.hip -- the gain fit of dam_gainfit.hip taken per frequency band: the moment matrices of the S stems and the mix
// over the STFT bins of a band and the frames of a window (include/dam_hip.h states the definitions), and the summary of a
// band-wise fit over the bands of a window.  The grouped solve is dam_gainfit.hip's kernel (one group per band).
//
// Two stages, a slab of whole windows at a time (the spectra of a whole song do not fit a reasonable workspace):
//   stft      one workgroup = one frame of one channel of one signal: the front-end's LDS FFT (dam_fft_lds.h, the arithmetic
//             of dam_stft_complex_f32) read through the gain fit's element strides             (frame, signal x channel) grid
//             -> workspace [signal][channel][frame of the slab][bin] float2: a frame's bins are one contiguous row
//   moments   one workgroup = tiles of BF_TILE elements of one (band, window) cell, an element = one (frame, bin) of the cell;
//             (S+1)(S+2)/2 running float64 sums per lane; wave butterfly, wave merge            (cell, tile lane) grid
//   reduce    a cell's tile records added in ascending tile order, both triangles written        one workgroup per cell
// The moment kernel is bound by its reads: (S+1) x channels x 8 bytes per element, every byte once.  S and the channel count
// are template parameters, so that the running sums are named registers.
#include "dam_common.h"
#include "dam_fft_lds.h"

#pragma clang fp contract(off)        // every sum is stated operation by operation; the fused multiply-adds are written out

namespace dam {
namespace {

constexpr int BF_THREADS = 256;
constexpr int BF_PER = 8;                             // elements a lane owns in a full tile
constexpr int BF_TILE = BF_THREADS * BF_PER;          // 2048: a library constant, never a function of the call
constexpr int BF_TILE_BLOCKS = 4;                     // workgroups that share a cell's tiles (tile t on workgroup t % 4)
constexpr int BF_MAX_S = DAM_GAINFIT_MAX_STEMS;
static_assert((BF_MAX_S + 1) * (BF_MAX_S + 2) / 2 <= WAVE, "one lane per pair in the merges");

// first frame of window w: the smallest t with min(t hop, n - 1) / seg >= w (w seg <= n - 1, so the inner min drops out)
__host__ __device__ inline int frame_lo(int64_t seg, int hop, int T, int W, int w) {
    if (w <= 0) return 0;
    if (w >= W) return T;
    const int64_t t = ((int64_t)w * seg + hop - 1) / hop;
    return t < T ? (int)t : T;
}

struct BfGeo {
    int64_t seg;                      // n_samples / W
    int hop, T, W, nbins;             // nbins = n_fft/2 + 1
    int w0, nw, t0, Ts;               // the slab: windows [w0, w0 + nw), frames [t0, t0 + Ts)
    int tmax;                         // tile records per cell in the workspace
};

struct BfCell {
    int e0, nb, ta, nf;               // first bin, bins, first frame, frames
};

__device__ __forceinline__ BfCell cell_of(const int* __restrict__ edges, const BfGeo& g, int b, int w) {
    BfCell c;
    int e0 = edges[b], e1 = edges[b + 1];
    e0 = e0 < 0 ? 0 : e0 > g.nbins ? g.nbins : e0;    // a bad table gives wrong numbers, never an access out of bounds
    e1 = e1 < 0 ? 0 : e1 > g.nbins ? g.nbins : e1;
    c.e0 = e0;
    c.nb = e1 > e0 ? e1 - e0 : 0;
    c.ta = frame_lo(g.seg, g.hop, g.T, g.W, w);
    c.nf = frame_lo(g.seg, g.hop, g.T, g.W, w + 1) - c.ta;
    return c;
}

// One frame of one channel of one signal.  The frame, the FFT and the split are those of stft_complex_kernel (dam_stft.hip) for
// a mono track without a gain; what differs is the addressing (element strides) and the output (a row per frame).
template <typename TX>
__global__ __launch_bounds__(FFT_THREADS) void bandfit_stft_kernel(const TX* __restrict__ x, int64_t signal_stride,
                                                                   int64_t sample_stride, int64_t channel_stride, int channels,
                                                                   int64_t n_samples, const float* __restrict__ window,
                                                                   const float2* __restrict__ tw, int n_fft, int hop, int t0,
                                                                   int Ts, int first_signal, float2* __restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M]
    const int tid = threadIdx.x, M = n_fft >> 1;
    const int sig = (int)blockIdx.y / channels, c = (int)blockIdx.y % channels;
    const TX* trk = x + sig * signal_stride + c * channel_stride;
    const int64_t p0 = (int64_t)(t0 + (int)blockIdx.x) * hop - M;
    for (int i = tid; i < M; i += FFT_THREADS) {
        const int64_t a = reflect(p0 + 2 * i, n_samples), b = reflect(p0 + 2 * i + 1, n_samples);
        buf[i] = make_float2((float)trk[a * sample_stride] * window[2 * i], (float)trk[b * sample_stride] * window[2 * i + 1]);
    }
    __syncthreads();
    const float2* z = lds_fft_radix2<false>(buf, buf + M, M, n_fft, tw, tid);
    float2* o = spec + (((int64_t)(first_signal + sig) * channels + c) * Ts + blockIdx.x) * (M + 1);
    for (int k = tid; k <= M; k += FFT_THREADS) {
        float2 xk = real_fft_bin(z, k, M, tw);
        if (k == 0 || k == M) xk.y = 0.f;             // DC and Nyquist of a real signal
        o[k] = xk;
    }
}

template <int S, int C>
__device__ __forceinline__ void add_element(const float2* __restrict__ p, int64_t plane, double ck,
                                            double (&acc)[(S + 1) * (S + 2) / 2]) {
    float2 u[C][S + 1];
#pragma unroll
    for (int c = 0; c < C; ++c)                       // every load of the element is issued before the first is used
#pragma unroll
        for (int s = 0; s <= S; ++s) u[c][s] = p[(s * C + c) * plane];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int k = 0;
#pragma unroll
        for (int i = 0; i <= S; ++i) {
            const double re = ck * (double)u[c][i].x, im = ck * (double)u[c][i].y;      // (times 1 or 2: exact)
#pragma unroll
            for (int j = i; j <= S; ++j, ++k) {
                acc[k] = __builtin_fma(re, (double)u[c][j].x, acc[k]);
                acc[k] = __builtin_fma(im, (double)u[c][j].y, acc[k]);
            }
        }
    }
}

template <int S, int C>
__global__ __launch_bounds__(BF_THREADS) void bandfit_moments_kernel(const float2* __restrict__ spec, const int* __restrict__ edges,
                                                                     BfGeo g, double* __restrict__ partial) {
    constexpr int NP = (S + 1) * (S + 2) / 2;
    __shared__ double wave_sum[BF_THREADS / WAVE][NP];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)g.nw), wl = (int)(blockIdx.x % (unsigned)g.nw);
    const BfCell cell = cell_of(edges, g, b, g.w0 + wl);
    const unsigned E = (unsigned)cell.nb * (unsigned)cell.nf;         // (the launch side refuses calls where this could wrap)
    const int64_t plane = (int64_t)g.Ts * g.nbins;
    const float2* base = spec + (int64_t)(cell.ta - g.t0) * g.nbins + cell.e0;
    // (workgroup-uniform loop: a cell of few elements leaves the other workgroups of its row without a tile)
    for (unsigned tile = blockIdx.y; (uint64_t)tile * BF_TILE < E; tile += gridDim.y) {
        double acc[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) acc[k] = 0.0;
#pragma clang loop unroll_count(S <= 2 ? 4 : 2)
        for (int i = 0; i < BF_PER; ++i) {
            const unsigned q = tile * BF_TILE + tid + BF_THREADS * i;
            if (q < E) {
                const unsigned ft = q / (unsigned)cell.nb, kb = q - ft * (unsigned)cell.nb;
                const int k = cell.e0 + (int)kb;
                add_element<S, C>(base + (int64_t)ft * g.nbins + kb, plane, k == 0 || k == g.nbins - 1 ? 1.0 : 2.0, acc);
            }
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
#pragma unroll
            for (int m = 1; m < WAVE; m <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], m);
        }
        if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
            for (int k = 0; k < NP; ++k) wave_sum[tid / WAVE][k] = acc[k];
        }
        __syncthreads();
        if (tid < NP)
            partial[((int64_t)blockIdx.x * g.tmax + tile) * NP + tid] =
                ((wave_sum[0][tid] + wave_sum[1][tid]) + wave_sum[2][tid]) + wave_sum[3][tid];
        __syncthreads();                              // wave_sum is rewritten by the workgroup's next tile
    }
}

__global__ __launch_bounds__(WAVE) void bandfit_reduce_kernel(const double* __restrict__ partial, const int* __restrict__ edges,
                                                              BfGeo g, int S, double* __restrict__ moments) {
    const int U = S + 1, NP = U * (U + 1) / 2, k = threadIdx.x;
    if (k >= NP) return;
    const int b = (int)(blockIdx.x / (unsigned)g.nw), w = g.w0 + (int)(blockIdx.x % (unsigned)g.nw);
    const BfCell cell = cell_of(edges, g, b, w);
    const int64_t nt = ((int64_t)cell.nb * cell.nf + BF_TILE - 1) / BF_TILE;
    const double* p = partial + (int64_t)blockIdx.x * g.tmax * NP + k;
    double s = 0.0;                                   // (a cell without an element: a table the kernel had to clamp)
    if (nt > 0) {
        s = p[0];
#pragma unroll 8                                      // eight loads in flight; the additions stay in ascending order
        for (int64_t i = 1; i < nt; ++i) s += p[i * NP];
    }
    int i = 0, row = U, rest = k;                     // pair k of the row-major upper triangle -> (i, j)
    while (rest >= row) { rest -= row; --row; ++i; }
    const int j = i + rest;
    double* m = moments + ((int64_t)b * g.W + w) * U * U;
    m[i * U + j] = s;
    m[j * U + i] = s;
}

// One lane per window: the bands of the window in ascending order.
__global__ __launch_bounds__(WAVE) void bandfit_summary_kernel(const double* __restrict__ residual, const double* __restrict__ target,
                                                               const int* __restrict__ status, int G, int W,
                                                               double* __restrict__ total) {
    const int w = blockIdx.x * WAVE + threadIdx.x;
    if (w >= W) return;
    double num = 0.0, den = 0.0;
    for (int b = 0; b < G; ++b) {
        const double Y = target[(int64_t)b * W + w];
        if (!(Y > 0.0)) continue;                     // a silent band adds nothing
        const double rho = status[(int64_t)b * W + w] > 0 ? residual[(int64_t)b * W + w] : 1.0;
        num = num + rho * Y;
        den = den + Y;
    }
    total[w] = den > 0.0 ? num / den : __longlong_as_double(0x7ff8000000000000ll);
}

template <int S>
void launch_moments(int channels, dim3 grid, const float2* spec, const int* edges, const BfGeo& g, double* partial, hipStream_t s) {
    if (channels == 2)
        hipLaunchKernelGGL((bandfit_moments_kernel<S, 2>), grid, dim3(BF_THREADS), 0, s, spec, edges, g, partial);
    else
        hipLaunchKernelGGL((bandfit_moments_kernel<S, 1>), grid, dim3(BF_THREADS), 0, s, spec, edges, g, partial);
}

void dispatch_moments(int S, int channels, dim3 grid, const float2* spec, const int* edges, const BfGeo& g, double* partial,
                      hipStream_t s) {
    switch (S) {
        case 1: return launch_moments<1>(channels, grid, spec, edges, g, partial, s);
        case 2: return launch_moments<2>(channels, grid, spec, edges, g, partial, s);
        case 3: return launch_moments<3>(channels, grid, spec, edges, g, partial, s);
        case 4: return launch_moments<4>(channels, grid, spec, edges, g, partial, s);
        case 5: return launch_moments<5>(channels, grid, spec, edges, g, partial, s);
        case 6: return launch_moments<6>(channels, grid, spec, edges, g, partial, s);
        case 7: return launch_moments<7>(channels, grid, spec, edges, g, partial, s);
        default: return launch_moments<8>(channels, grid, spec, edges, g, partial, s);
    }
}

template <typename TX>
int launch_stft(const void* x, int64_t signal_stride, int64_t sample_stride, int64_t channel_stride, int n_signals, int channels,
                int64_t n_samples, const float* window, const float* twiddles, int n_fft, int hop, int t0, int Ts, int first_signal,
                float2* spec, hipStream_t s) {
    const size_t lds = (size_t)n_fft * sizeof(float2);        // two buffers of n_fft/2 complex points
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit
    if (lds > 48 * 1024 && !raise_lds_limit<&bandfit_stft_kernel<TX>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((bandfit_stft_kernel<TX>), dim3((unsigned)Ts, (unsigned)(n_signals * channels)), dim3(FFT_THREADS), lds, s,
                       (const TX*)x, signal_stride, sample_stride, channel_stride, channels, n_samples, window,
                       reinterpret_cast<const float2*>(twiddles), n_fft, hop, t0, Ts, first_signal, spec);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// How a call is cut into slabs of whole windows: a function of the arguments alone, so that the size query and the entry agree.
struct BfPlan {
    int64_t seg, frame_bytes, slab_frames;            // slab_frames: frames the spectra region holds
    int T, nbins, nf_max, nw_max, tmax;               // longest window in frames, most windows of a slab, tile records per cell
    int64_t partial_bytes, spectra_bytes;
};

int make_plan(int n_windows, int64_t n_samples, int n_stems, int channels, int n_fft, int hop, int n_bands, int64_t slab_bytes,
              BfPlan* plan) {
    if (n_stems < 1 || n_stems > BF_MAX_S || (channels != 1 && channels != 2)) return DAM_ERR_BAD_ARG;
    if (n_fft < 64 || n_fft > 16384 || (n_fft & (n_fft - 1)) || hop < 1 || n_samples <= n_fft / 2) return DAM_ERR_BAD_ARG;
    if (n_windows < 1 || n_windows > n_samples || n_bands < 1 || n_bands > dam_spectrum_max_bands() || slab_bytes < 0) return DAM_ERR_BAD_ARG;
    const int64_t frames = 1 + n_samples / hop;
    if (frames > 0x7fffffff / 2) return DAM_ERR_UNSUPPORTED;
    BfPlan p;
    p.seg = n_samples / n_windows;
    p.T = (int)frames;
    p.nbins = n_fft / 2 + 1;
    p.frame_bytes = (int64_t)(n_stems + 1) * channels * p.nbins * (int64_t)sizeof(float2);
    p.nf_max = 0;
    for (int w = 0; w < n_windows; ++w) {
        const int nf = frame_lo(p.seg, hop, p.T, n_windows, w + 1) - frame_lo(p.seg, hop, p.T, n_windows, w);
        if (nf < 1) return DAM_ERR_BAD_ARG;           // a window that owns no frame has no moments
        if (nf > p.nf_max) p.nf_max = nf;
    }
    if ((int64_t)p.nbins * p.nf_max > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    const int64_t cap = (slab_bytes ? slab_bytes : (int64_t)DAM_BANDFIT_SLAB_BYTES) / p.frame_bytes;
    p.slab_frames = cap > p.nf_max ? (cap < p.T ? cap : p.T) : p.nf_max;
    p.nw_max = 0;
    for (int w0 = 0; w0 < n_windows;) {               // greedy: as many whole windows as fit, at least one
        int w1 = w0 + 1;
        const int t0 = frame_lo(p.seg, hop, p.T, n_windows, w0);
        while (w1 < n_windows && frame_lo(p.seg, hop, p.T, n_windows, w1 + 1) - t0 <= p.slab_frames) ++w1;
        if (w1 - w0 > p.nw_max) p.nw_max = w1 - w0;
        w0 = w1;
    }
    p.tmax = (int)cdiv((int64_t)p.nbins * p.nf_max, BF_TILE);
    if ((int64_t)n_bands * p.nw_max > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    p.partial_bytes = (int64_t)n_bands * p.nw_max * p.tmax * ((n_stems + 1) * (n_stems + 2) / 2) * (int64_t)sizeof(double);
    p.spectra_bytes = p.slab_frames * p.frame_bytes;
    *plan = p;
    return DAM_OK;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_bandfit_tile_elements(void) { return dam::BF_TILE; }

extern "C" int64_t dam_bandfit_workspace_bytes(int n_windows, int64_t n_samples, int n_stems, int channels, int n_fft, int hop,
                                                    int n_bands, int64_t slab_bytes) {
    dam::BfPlan p;
    if (dam::make_plan(n_windows, n_samples, n_stems, channels, n_fft, hop, n_bands, slab_bytes, &p) != DAM_OK) return 0;
    return p.partial_bytes + p.spectra_bytes;
}

extern "C" int dam_bandfit_moments(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples,
                                        int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, const void* y,
                                        int y_is_f64, int64_t y_sample_stride, int64_t y_channel_stride, const float* window,
                                        const float* twiddles, int n_fft, int hop, const int32_t* edges, int n_bands, int n_windows,
                                        int64_t slab_bytes, double* moments, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !y || !window || !twiddles || !edges || !moments || !workspace) return DAM_ERR_BAD_ARG;
    BfPlan p;
    const int rc = make_plan(n_windows, n_samples, n_stems, channels, n_fft, hop, n_bands, slab_bytes, &p);
    if (rc != DAM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    float2* spec = reinterpret_cast<float2*>(static_cast<char*>(workspace) + p.partial_bytes);
    BfGeo g;
    g.seg = p.seg; g.hop = hop; g.T = p.T; g.W = n_windows; g.nbins = p.nbins; g.tmax = p.tmax;
    for (int w0 = 0; w0 < n_windows;) {               // the slabs of make_plan, one after the other on the stream
        int w1 = w0 + 1;
        const int t0 = frame_lo(p.seg, hop, p.T, n_windows, w0);
        while (w1 < n_windows && frame_lo(p.seg, hop, p.T, n_windows, w1 + 1) - t0 <= p.slab_frames) ++w1;
        g.w0 = w0; g.nw = w1 - w0; g.t0 = t0; g.Ts = frame_lo(p.seg, hop, p.T, n_windows, w1) - t0;
        int st = x_is_f64 ? launch_stft<double>(x, stem_stride, sample_stride, channel_stride, n_stems, channels, n_samples, window,
                                                twiddles, n_fft, hop, g.t0, g.Ts, 0, spec, s)
                          : launch_stft<float>(x, stem_stride, sample_stride, channel_stride, n_stems, channels, n_samples, window,
                                               twiddles, n_fft, hop, g.t0, g.Ts, 0, spec, s);
        if (st != DAM_OK) return st;
        st = y_is_f64 ? launch_stft<double>(y, 0, y_sample_stride, y_channel_stride, 1, channels, n_samples, window, twiddles,
                                            n_fft, hop, g.t0, g.Ts, n_stems, spec, s)
                      : launch_stft<float>(y, 0, y_sample_stride, y_channel_stride, 1, channels, n_samples, window, twiddles, n_fft,
                                           hop, g.t0, g.Ts, n_stems, spec, s);
        if (st != DAM_OK) return st;
        const unsigned cells = (unsigned)(n_bands * g.nw);
        dispatch_moments(n_stems, channels, dim3(cells, (unsigned)(p.tmax < BF_TILE_BLOCKS ? p.tmax : BF_TILE_BLOCKS)), spec, edges,
                         g, partial, s);
        DAM_CHECK_LAUNCH();
        hipLaunchKernelGGL(bandfit_reduce_kernel, dim3(cells), dim3(WAVE), 0, s, partial, edges, g, n_stems, moments);
        DAM_CHECK_LAUNCH();
        w0 = w1;
    }
    return DAM_OK;
}

extern "C" int dam_bandfit_summary(const double* residual, const double* target, const int32_t* status, int n_groups,
                                        int n_windows, double* total, void* stream) {
    using namespace dam;
    if (!residual || !target || !status || !total || n_groups < 1 || n_windows < 1) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(bandfit_summary_kernel, dim3((unsigned)cdiv(n_windows, WAVE)), dim3(WAVE), 0, (hipStream_t)stream, residual,
                       target, status, n_groups, n_windows, total);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
