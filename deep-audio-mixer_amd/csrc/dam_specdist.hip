// dam_specdist.hip -- the log-spectrogram distance of gain mixes: the training criterion (model_trainer.py:34-35, a mean
// squared error between dB spectrograms) measured on the mix that is actually rendered, frame by frame and bin by bin, of
// R candidate mixes "stems x gain ramps" against one reference mix (include/dam_hip.h, "Spectrogram distance", states the
// definition).  As in the band spectrum the stems are summed with their gains AS a frame is loaded; no mix and no spectrogram
// is written, what leaves a workgroup is one float64 (sum d, sum d^2) record per (row, frame, band).
//   frames   one workgroup = one frame t, all R rows: the reference frame is loaded and transformed once, every lane keeps
//            the reference levels of its own bins in registers; then per row: load (stems x row gains) -> LDS FFT -> levels
//            -> (d, d^2) as doubles over the FFT buffer -> bands folded by the four waves -> record       grid = frames
//   cells    a cell's frame records added in ascending t from +0.0; the geometry counts                   (window, row) grid
//   summary  mse / bias / centred rms per row: total, per band, per window                               one workgroup per row
// T (R + 1) transforms instead of the 2 T R of a pairwise comparison.  Not tuned beyond its structure.
#include "dam_common.h"
#include "dam_fft_lds.h"
#include "dam_specdist_frame.h"  // level_db, transform_frame: shared with the gradient (dam_specgrad.hip)
#include "dam_spectrum_load.h"   // SpecGeo, mix_pair: the loader of the band spectrum

#pragma clang fp contract(off)        // levels, differences and sums are stated operation by operation

namespace dam {
namespace {

constexpr int DIST_MAX_BANDS = 64;    // dam_spectrum_max_bands(): the cell kernel gives a band a lane

struct DistGeo {
    int n_rows, n_bands;
    float amin2, floor_db;
};

// The levels of the bins a lane owns (tid + 256 i; PER = 1 tests k < M, as the band spectrum does) and, on lane 0, Nyquist.
template <int PER>
__device__ __forceinline__ void own_levels(const float2* z, int M, const float2* __restrict__ tw, int tid, const DistGeo& d,
                                           float (&lev)[PER], float& nyq) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = tid + FFT_THREADS * i;
        lev[i] = 0.f;
        if (PER > 1 || k < M) {
            float2 xk = real_fft_bin(z, k, M, tw);
            if (k == 0) xk.y = 0.f;                                   // DC of a real signal
            lev[i] = level_db(xk.x * xk.x + xk.y * xk.y, d.amin2, d.floor_db);
        }
    }
    nyq = 0.f;
    if (tid == 0) {                                                   // Nyquist, real as well
        const float2 xk = real_fft_bin(z, M, M, tw);
        nyq = level_db(xk.x * xk.x, d.amin2, d.floor_db);
    }
}

template <typename TC, typename TR, int PER>
__global__ __launch_bounds__(FFT_THREADS) void specdist_frame_kernel(
    const TC* __restrict__ x, const double* __restrict__ gains, const TR* __restrict__ xref, const double* __restrict__ ref_gains,
    const float* __restrict__ window, const float2* __restrict__ tw /* W_nfft^k */, const int* __restrict__ edges, SpecGeo g,
    SpecGeo gref, DistGeo d, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M] (+ 16 bytes); between transforms M + 1 double2
    const int tid = threadIdx.x, M = g.n_fft >> 1, t = blockIdx.x;
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int64_t p0 = (int64_t)t * g.hop - M;
    double2* dd = reinterpret_cast<double2*>(buf);                    // (d, d^2) of bin k at dd[k], k = 0 .. M

    float lref[PER], lref_nyq;
    {
        const float2* z = transform_frame<TR>(buf, xref, ref_gains, gref, p0, window, tw, tid);
        own_levels<PER>(z, M, tw, tid, d, lref, lref_nyq);
    }
    __syncthreads();                                                  // z is read: the first candidate frame may land
    for (int r = 0; r < d.n_rows; ++r) {
        const double* gr = gains ? gains + (int64_t)r * g.n_stems * g.n_gains : nullptr;
        const float2* z = transform_frame<TC>(buf, x, gr, g, p0, window, tw, tid);
        float lc[PER], lc_nyq;
        own_levels<PER>(z, M, tw, tid, d, lc, lc_nyq);
        __syncthreads();                                              // every lane has read z: the doubles may land on it
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = tid + FFT_THREADS * i;
            if (PER > 1 || k < M) {
                const double df = (double)lc[i] - (double)lref[i];
                dd[k] = make_double2(df, df * df);
            }
        }
        if (tid == 0) {
            const double df = (double)lc_nyq - (double)lref_nyq;
            dd[M] = make_double2(df, df * df);
        }
        __syncthreads();
        double* out = partial + (((int64_t)r * g.n_frames + t) * d.n_bands) * 2;
        for (int b = wave; b < d.n_bands; b += FFT_THREADS / WAVE) {  // wave-uniform
            int lo = edges[b], hi = edges[b + 1];
            lo = lo < 0 ? 0 : (lo > M + 1 ? M + 1 : lo);
            hi = hi < 0 ? 0 : (hi > M + 1 ? M + 1 : hi);
            double s1 = 0.0, s2 = 0.0;
            for (int k = lo + lane; k < hi; k += WAVE) {
                const double2 v = dd[k];
                s1 += v.x;
                s2 += v.y;
            }
            for (int m = 1; m < WAVE; m <<= 1) {
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (lane == 0) {
                out[2 * b] = s1;
                out[2 * b + 1] = s2;
            }
        }
        __syncthreads();                                              // dd is read: the next row's frame may land
    }
}

// First frame of window w (w = n_windows: the frame count): the frames whose centre sample min(t hop, n - 1) has gain
// index w, i.e. t >= ceil(w (n / W) / hop).
__device__ __forceinline__ int window_first_frame(int w, int n_windows, int64_t seg, int hop, int n_frames) {
    if (w <= 0) return 0;
    if (w >= n_windows) return n_frames;
    const int64_t f = ((int64_t)w * seg + hop - 1) / hop;
    return f < n_frames ? (int)f : n_frames;
}

// One lane per band, one workgroup per (window, row): the cell's frame records in ascending t from +0.0.
__global__ __launch_bounds__(DIST_MAX_BANDS) void specdist_cell_kernel(const double* __restrict__ partial,
                                                                      const int* __restrict__ edges, int n_bands, int n_windows,
                                                                      int n_frames, int64_t seg, int hop, int n_fft,
                                                                      double* __restrict__ sums, int64_t* __restrict__ count) {
    const int b = threadIdx.x, w = blockIdx.x, r = blockIdx.y;
    if (b >= n_bands) return;
    const int t0 = window_first_frame(w, n_windows, seg, hop, n_frames);
    const int t1 = window_first_frame(w + 1, n_windows, seg, hop, n_frames);
    const double2* p = reinterpret_cast<const double2*>(partial) + ((int64_t)r * n_frames + t0) * n_bands + b;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8                                                      // eight loads in flight; the additions stay in ascending order
    for (int t = t0; t < t1; ++t) {
        const double2 v = p[(int64_t)(t - t0) * n_bands];
        s1 += v.x;
        s2 += v.y;
    }
    double* o = sums + ((((int64_t)r * n_bands + b) * n_windows + w) * 2);
    o[0] = s1;
    o[1] = s2;
    if (r == 0) {
        const int top = n_fft / 2 + 1;
        int lo = edges[b], hi = edges[b + 1];
        lo = lo < 0 ? 0 : (lo > top ? top : lo);
        hi = hi < 0 ? 0 : (hi > top ? top : hi);
        count[(int64_t)b * n_windows + w] = (int64_t)(t1 - t0) * (hi > lo ? hi - lo : 0);
    }
}

__device__ __forceinline__ void summary_store(double* o, double s1, double s2, int64_t n) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (n <= 0) { o[0] = nan; o[1] = nan; o[2] = nan; return; }
    const double mse = s2 / (double)n, bias = s1 / (double)n;
    const double v = mse - bias * bias;
    o[0] = mse;
    o[1] = bias;
    o[2] = sqrt(v > 0.0 ? v : (v == v ? 0.0 : v));                   // max(0, v); a NaN stays one
}

// out[r][0] the total, out[r][1 + b] band b, out[r][1 + B + w] window w.  A band adds its cells in ascending window, a window
// in ascending band, each on a lane of its own; the total then adds the bands' sums in ascending band -- the longest serial walk
// is max(B, W) cells, not B W.
__global__ __launch_bounds__(FFT_THREADS) void specdist_summary_kernel(const double* __restrict__ sums,
                                                                      const int64_t* __restrict__ count, int n_bands,
                                                                      int n_windows, double* __restrict__ out) {
    __shared__ double band_s1[DIST_MAX_BANDS], band_s2[DIST_MAX_BANDS];
    __shared__ int64_t band_n[DIST_MAX_BANDS];
    const int r = blockIdx.x, n_out = 1 + n_bands + n_windows;
    const double* s = sums + (int64_t)r * n_bands * n_windows * 2;
    for (int o = 1 + threadIdx.x; o < n_out; o += FFT_THREADS) {
        const bool band = o <= n_bands;
        const int b0 = band ? o - 1 : 0, b1 = band ? o : n_bands;
        const int w0 = band ? 0 : o - 1 - n_bands, w1 = band ? n_windows : o - n_bands;
        double s1 = 0.0, s2 = 0.0;
        int64_t n = 0;
        for (int b = b0; b < b1; ++b)
            for (int w = w0; w < w1; ++w) {
                const int64_t c = (int64_t)b * n_windows + w;
                s1 += s[2 * c];
                s2 += s[2 * c + 1];
                n += count[c];
            }
        if (band) { band_s1[o - 1] = s1; band_s2[o - 1] = s2; band_n[o - 1] = n; }     // (B <= 64 < 256: the first pass)
        summary_store(out + ((int64_t)r * n_out + o) * 3, s1, s2, n);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s1 = 0.0, s2 = 0.0;
        int64_t n = 0;
        for (int b = 0; b < n_bands; ++b) { s1 += band_s1[b]; s2 += band_s2[b]; n += band_n[b]; }
        summary_store(out + (int64_t)r * n_out * 3, s1, s2, n);
    }
}

struct DistCall {
    const void *x, *xref;
    const double *gains, *ref_gains;
    const float *window, *twiddles;
    const int32_t* edges;
    SpecGeo g, gref;
    DistGeo d;
    double* partial;
    hipStream_t s;
};

template <typename TC, typename TR, int PER>
int launch_frames(const DistCall& c) {
    // two images of n_fft/2 complex points, and the 16 bytes by which n_fft/2 + 1 (d, d^2) pairs exceed them
    const size_t lds = (size_t)(c.g.n_fft / 2 + 1) * sizeof(double2);
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit (the kernel has no static LDS beside it)
    if (lds > 48 * 1024 && !raise_lds_limit<&specdist_frame_kernel<TC, TR, PER>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((specdist_frame_kernel<TC, TR, PER>), dim3((unsigned)c.g.n_frames), dim3(FFT_THREADS), lds, c.s,
                       (const TC*)c.x, c.gains, (const TR*)c.xref, c.ref_gains, c.window,
                       reinterpret_cast<const float2*>(c.twiddles), c.edges, c.g, c.gref, c.d, c.partial);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

template <typename TC, typename TR>
int dispatch_frames(int per, const DistCall& c) {
    switch (per) {
        case 1: return launch_frames<TC, TR, 1>(c);
        case 2: return launch_frames<TC, TR, 2>(c);
        case 4: return launch_frames<TC, TR, 4>(c);
        case 8: return launch_frames<TC, TR, 8>(c);
        case 16: return launch_frames<TC, TR, 16>(c);
        default: return launch_frames<TC, TR, 32>(c);
    }
}

bool fill_geo(SpecGeo& g, int n_stems, int channels, int64_t n, int64_t stem_stride, int64_t sample_stride,
              int64_t channel_stride, const double* gains, int n_gains, int n_fft, int hop, int n_frames, int n_bands) {
    if (n_stems <= 0 || (channels != 1 && channels != 2)) return false;
    if (gains && (n_gains < 1 || n_gains > n)) return false;
    g.n_samples = n; g.stem_stride = stem_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.n_stems = n_stems; g.channels = channels; g.n_gains = gains ? n_gains : 1;
    g.gseg = n / g.n_gains;
    g.n_fft = n_fft; g.hop = hop; g.n_frames = n_frames; g.n_bands = n_bands; g.blocks_per_mix = n_frames;
    g.small = n < 0x7fffffff ? 1 : 0;
    return true;
}

// The geometry rules the sums entry and the workspace size share -> frames, or 0 where the entry refuses.
int64_t checked_frames(int n_rows, int64_t n, int n_fft, int hop, int n_bands, int n_windows) {
    if (n_rows < 1 || n_rows > 65535 || n <= 0) return 0;
    if (n_fft < 64 || n_fft > 16384 || (n_fft & (n_fft - 1))) return 0;
    if (hop < 1 || n <= n_fft / 2) return 0;                          // reflect padding needs n > n_fft/2
    if (n_bands < 1 || n_bands > DIST_MAX_BANDS) return 0;
    if (n_windows < 1 || n_windows > n) return 0;
    const int64_t n_frames = 1 + n / hop;
    if (n_frames > 0x7fffffff / 2 || n_windows > n_frames) return 0;
    const int64_t seg = n / n_windows;
    for (int64_t w = 1, prev = 0; w <= n_windows; ++w) {              // every window owns a frame
        int64_t f = w == n_windows ? n_frames : cdiv(w * seg, hop);
        f = f < n_frames ? f : n_frames;
        if (f <= prev) return 0;
        prev = f;
    }
    return n_frames;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_specdist_workspace_bytes(int n_rows, int64_t n_samples, int n_fft, int hop, int n_bands, int n_windows) {
    const int64_t n_frames = dam::checked_frames(n_rows, n_samples, n_fft, hop, n_bands, n_windows);
    return (int64_t)n_rows * n_frames * n_bands * 2 * (int64_t)sizeof(double);
}

extern "C" int dam_specdist_sums(const void* x, int x_is_f64, int n_rows, int n_stems, int channels, int64_t n_samples,
                                 int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, const double* gains,
                                 int n_gains, const void* ref, int ref_is_f64, int ref_stems, int ref_channels,
                                 int64_t ref_stem_stride, int64_t ref_sample_stride, int64_t ref_channel_stride,
                                 const double* ref_gains, int ref_n_gains, const float* window, const float* twiddles, int n_fft,
                                 int hop, float amin, const int32_t* edges, int n_bands, int n_windows, double* sums,
                                 int64_t* count, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !ref || !window || !twiddles || !edges || !sums || !count || !workspace) return DAM_ERR_BAD_ARG;
    if (!(amin > 0.f)) return DAM_ERR_BAD_ARG;
    const int64_t n_frames = checked_frames(n_rows, n_samples, n_fft, hop, n_bands, n_windows);
    if (n_frames <= 0) return DAM_ERR_BAD_ARG;
    DistCall c;
    if (!fill_geo(c.g, n_stems, channels, n_samples, stem_stride, sample_stride, channel_stride, gains, n_gains, n_fft, hop,
                  (int)n_frames, n_bands))
        return DAM_ERR_BAD_ARG;
    if (!fill_geo(c.gref, ref_stems, ref_channels, n_samples, ref_stem_stride, ref_sample_stride, ref_channel_stride, ref_gains,
                  ref_n_gains, n_fft, hop, (int)n_frames, n_bands))
        return DAM_ERR_BAD_ARG;
    c.x = x; c.xref = ref; c.gains = gains; c.ref_gains = ref_gains; c.window = window; c.twiddles = twiddles; c.edges = edges;
    c.d.n_rows = n_rows; c.d.n_bands = n_bands;
    c.d.amin2 = amin * amin;
    c.d.floor_db = (float)(20.0 * log10((double)amin));
    c.partial = static_cast<double*>(workspace);
    c.s = (hipStream_t)stream;
    const int per = n_fft / 2 >= FFT_THREADS ? n_fft / 2 / FFT_THREADS : 1;
    const int rc = x_is_f64 ? (ref_is_f64 ? dispatch_frames<double, double>(per, c) : dispatch_frames<double, float>(per, c))
                            : (ref_is_f64 ? dispatch_frames<float, double>(per, c) : dispatch_frames<float, float>(per, c));
    if (rc != DAM_OK) return rc;
    hipLaunchKernelGGL(specdist_cell_kernel, dim3((unsigned)n_windows, (unsigned)n_rows), dim3(DIST_MAX_BANDS), 0, c.s, c.partial,
                       edges, n_bands, n_windows, (int)n_frames, n_samples / n_windows, hop, n_fft, sums, count);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_specdist_summary(const double* sums, const int64_t* count, int n_rows, int n_bands, int n_windows,
                                    double* out, void* stream) {
    using namespace dam;
    if (!sums || !count || !out || n_rows < 1 || n_bands < 1 || n_bands > DIST_MAX_BANDS || n_windows < 1)
        return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(specdist_summary_kernel, dim3((unsigned)n_rows), dim3(FFT_THREADS), 0, (hipStream_t)stream, sums, count,
                       n_bands, n_windows, out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
