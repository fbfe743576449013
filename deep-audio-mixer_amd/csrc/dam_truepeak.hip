// dam_truepeak.hip -- inter-sample ("true") peak of every (track, channel) row of a batch, and the gain clamp built on it.
//
// The output chain ends in dam_pcm_encode, which can only count the samples it had to clip.  This file measures, before
// the encoder runs, how high the reconstructed waveform goes -- ITU-R BS.1770 Annex 2 / EBU R128 "true peak": the signal
// oversampled 4x, the largest magnitude of the original and the interpolated values -- and turns it into a ceiling on a
// gain that is still on the device (the -20 LUFS gain of dam_loudness_target_gains): min(gain, ceiling / true peak).
//
// Interpolator: 49-tap Hann-windowed sinc, h[k] = sinc((k - 24) / 4) * 0.5 * (1 - cos(2 pi k / 48)), k = 0..48
// (dam_true_peak_taps_host).  Phase 0 is the identity (h[24] = 1, h[24 +- 4m] = 0); the phases p = 1, 2, 3 have 12 taps:
//   y_p[i] = sum_{j=-6..5} x[i - j] * h[24 + p + 4 j]        x = 0 outside [0, n), i in [0, n)
//   TP = max(max_i |x[i]|, max_{p,i} |y_p[i]|)
// tests/_truepeak_ref.py restates this in numpy.  y_p[i] lies between x[i] and x[i+1]: it reads x[i-5 .. i+6].
//
// Shape: a workgroup takes tiles of TP_TILE consecutive samples of one row.  256 lanes fill an LDS image of the tile plus
// its halo (5 samples before, 6 after, zero outside the row) with coalesced loads -- the float32/float64 conversion and the
// optional gain product (double)x * gains[t][min(n / (n / n_gains), n_gains-1)] happen here, as in the batched meter --
// while the loads of the workgroup's next tile are already in flight.  Lane l then owns the TP_RUN consecutive samples
// behind l * TP_RUN: 19 LDS reads give it the 12-value window of each of its 8 samples, 36 FMAs per sample in a fixed order
// (j = -6 .. 5 per phase).  The image is padded by one double per 8 so that the lanes' stride is 9 doubles = 18 banks:
// conflict-free for ds_read_b64.  Running maxima of |x| and |y_p| per lane, a wave reduction, one (sample peak, true peak)
// pair per workgroup to the workspace; a second launch takes the maximum of each row's pairs.  max() of values that are
// each computed in a fixed order: a row's result does not depend on the grid, the tile walk or the rest of the batch.
// No atomics.  fmax() drops a NaN operand, so a NaN sample (and the interpolated values it poisons) is skipped; an
// infinite sample gives an infinite peak.  Non-finite input is outside the contract.
#include "dam_common.h"
#include "dam_truepeak_fir.h"

#include <math.h>

namespace dam {
namespace {

constexpr int TP_MAX_BLOCKS = 2048;                    // workgroups of one launch (256 CUs x 8)

struct TpGeo {
    int64_t n_samples;
    int64_t track_stride, sample_stride, channel_stride;      // elements
    int64_t gseg;                                             // n_samples / n_gains
    int channels, n_gains;
};

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

template <typename T, bool GAINS>
__global__ __launch_bounds__(TP_THREADS) void true_peak_tile_kernel(const T* __restrict__ x, TpGeo g, TpTaps taps,
                                                                    const double* __restrict__ gains,
                                                                    double* __restrict__ partial /* [row][gridDim.x][2] */) {
    __shared__ double img[TP_LDS];
    __shared__ double red[TP_THREADS / WAVE][2];
    const int t = threadIdx.x;
    const int row = blockIdx.y, track = row / g.channels, ch = row - track * g.channels;
    const T* xr = x + track * g.track_stride + ch * g.channel_stride;
    const double* gr = GAINS ? gains + (int64_t)track * g.n_gains : nullptr;

    // image element e = k * 256 + t of tile `tile` is sample tile * TP_TILE - TP_BEFORE + e of the row
    T next[TP_LOADS];
    auto fetch = [&](int64_t tile) {
        const int64_t n0 = tile * TP_TILE - TP_BEFORE + t;
#pragma unroll
        for (int k = 0; k < TP_LOADS; ++k) {
            const int64_t n = n0 + k * TP_THREADS;
            bool in = n < g.n_samples;
            if (k == 0) in = in && n >= 0;                                      // only the first piece can precede the row
            if (k == TP_LOADS - 1) in = in && t < TP_SPAN - k * TP_THREADS;     // only the last piece is partial
            next[k] = in ? xr[n * g.sample_stride] : (T)0;
        }
    };

    double m_sample = 0.0, m_inter = 0.0;
    const int64_t tiles = (g.n_samples + TP_TILE - 1) / TP_TILE;
    int64_t tile = blockIdx.x;
    if (tile < tiles) fetch(tile);
    for (; tile < tiles; tile += gridDim.x) {
        __syncthreads();                               // the previous image has been consumed
        const int64_t first = tile * TP_TILE - TP_BEFORE;
        // gain index of sample n: min(n / gseg, n_gains - 1).  A segment at least as long as the image is crossed at most
        // once inside it: one (uniform) division per tile; shorter segments divide per element.
        int64_t gi0 = 0, gcross = 0;
        if (GAINS) {
            gi0 = (first > 0 ? first : 0) / g.gseg;
            gcross = (gi0 + 1) * g.gseg;
        }
#pragma unroll
        for (int k = 0; k < TP_LOADS; ++k) {
            const int e = k * TP_THREADS + t;
            if (k < TP_LOADS - 1 || e < TP_SPAN) {
                double v = (double)next[k];
                if (GAINS) {                           // (halo elements outside the row are zero: any valid index will do)
                    const int64_t n = first + e;
                    int64_t gi = g.gseg >= TP_SPAN ? (n >= gcross ? gi0 + 1 : gi0) : (n > 0 ? n : 0) / g.gseg;
                    if (gi > g.n_gains - 1) gi = g.n_gains - 1;
                    v = v * gr[gi];
                }
                img[e + (e >> 3)] = v;
            }
        }
        __syncthreads();
        if (tile + gridDim.x < tiles) fetch(tile + gridDim.x);

        double w[TP_RUN + TP_BEFORE + TP_AFTER];
        tp_window(img, t, w);
        const int64_t left = g.n_samples - (tile * TP_TILE + (int64_t)t * TP_RUN);      // samples of the row from i0 on
#pragma unroll
        for (int r = 0; r < TP_RUN; ++r) {
            double y0, y1, y2;
            tp_phases(w, r, taps, y0, y1, y2);
            if (r < left) {                            // (a sample past the row's end is zero, but its y_p is not)
                m_sample = fmax(m_sample, fabs(w[r + TP_BEFORE]));
                m_inter = fmax(m_inter, fmax(fabs(y0), fmax(fabs(y1), fabs(y2))));
            }
        }
    }
    m_sample = wave_max(m_sample);
    m_inter = wave_max(m_inter);
    if ((t & (WAVE - 1)) == 0) { red[t / WAVE][0] = m_sample; red[t / WAVE][1] = m_inter; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int i = 1; i < TP_THREADS / WAVE; ++i) { m_sample = fmax(m_sample, red[i][0]); m_inter = fmax(m_inter, red[i][1]); }
        double* p = partial + ((int64_t)row * gridDim.x + blockIdx.x) * 2;
        p[0] = m_sample;
        p[1] = fmax(m_sample, m_inter);
    }
}

// one wave per row: the maximum of its n_part pairs
__global__ __launch_bounds__(WAVE) void true_peak_reduce_kernel(const double* __restrict__ partial, int n_part,
                                                                double* __restrict__ sample_peak, double* __restrict__ true_peak) {
    const int row = blockIdx.x;
    const double* p = partial + (int64_t)row * n_part * 2;
    double ms = 0.0, mt = 0.0;
    for (int i = threadIdx.x; i < n_part; i += WAVE) { ms = fmax(ms, p[2 * i]); mt = fmax(mt, p[2 * i + 1]); }
    ms = wave_max(ms);
    mt = wave_max(mt);
    if (threadIdx.x == 0) {
        if (sample_peak) sample_peak[row] = ms;
        true_peak[row] = mt;
    }
}

// gains[i] = min(gains[i], ceiling / max_q peaks[i][q]), numpy's minimum / max: a NaN operand gives NaN
__global__ __launch_bounds__(256) void peak_limit_gains_kernel(double* __restrict__ gains, const double* __restrict__ peaks,
                                                               int n_gains, int peaks_per_gain, double ceiling_lin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_gains) return;
    const double* p = peaks + (int64_t)i * peaks_per_gain;
    double m = p[0];
    for (int q = 1; q < peaks_per_gain; ++q) {
        const double v = p[q];
        if (v > m || v != v) m = v;
    }
    const double c = ceiling_lin / m, gval = gains[i];
    gains[i] = (c < gval || c != c) ? c : gval;
}

static int tp_blocks_per_row(int64_t rows, int64_t n_samples) {
    const int64_t tiles = cdiv(n_samples, TP_TILE);
    int64_t share = TP_MAX_BLOCKS / rows;
    if (share < 1) share = 1;
    return (int)(tiles < share ? tiles : share);
}

}  // namespace
}  // namespace dam

extern "C" int dam_true_peak_taps_host(double* h49) {
    if (!h49) return DAM_ERR_BAD_ARG;
    const double pi = 3.14159265358979323846;
    for (int k = 0; k <= 24; ++k) {
        const double xk = (k - 24) / 4.0, w = 0.5 * (1.0 - cos(2.0 * pi * k / 48.0));
        double s = 1.0;
        if (k != 24) s = (24 - k) % 4 == 0 ? 0.0 : sin(pi * xk) / (pi * xk);          // sinc of a non-zero integer: exactly 0
        h49[k] = h49[48 - k] = s * w;                                                  // symmetric by construction
    }
    return DAM_OK;
}

extern "C" int64_t dam_true_peak_tile_samples(void) { return dam::TP_TILE; }
extern "C" int dam_true_peak_max_blocks(void) { return dam::TP_MAX_BLOCKS; }

extern "C" int64_t dam_true_peak_workspace_bytes(int n_tracks, int64_t n_samples, int channels) {
    if (n_tracks <= 0 || n_samples <= 0 || channels <= 0) return 0;
    const int64_t rows = (int64_t)n_tracks * channels;
    return rows * dam::tp_blocks_per_row(rows, n_samples) * 2 * (int64_t)sizeof(double);
}

extern "C" int dam_true_peak_batch(const void* x, int x_is_f64, int n_tracks, int64_t n_samples, int channels,
                                   int64_t track_stride, int64_t sample_stride, int64_t channel_stride, const double* gains,
                                   int n_gains, double* sample_peak, double* true_peak, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !true_peak || !workspace) return DAM_ERR_BAD_ARG;
    if (n_tracks <= 0 || n_samples <= 0 || channels <= 0) return DAM_ERR_BAD_ARG;
    if (gains && (n_gains <= 0 || n_gains > n_samples)) return DAM_ERR_BAD_ARG;
    const int64_t rows = (int64_t)n_tracks * channels;
    if (rows > 65535) return DAM_ERR_BAD_ARG;
    const TpTaps taps = tp_taps_host();
    TpGeo g;
    g.n_samples = n_samples;
    g.track_stride = track_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.channels = channels; g.n_gains = gains ? n_gains : 1;
    g.gseg = n_samples / g.n_gains;
    const int bx = tp_blocks_per_row(rows, n_samples);
    hipStream_t st = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(workspace);
    const dim3 grid((unsigned)bx, (unsigned)rows);
#define DAM_TP(T, G)                                                                                                     \
    hipLaunchKernelGGL((true_peak_tile_kernel<T, G>), grid, dim3(TP_THREADS), 0, st, reinterpret_cast<const T*>(x), g, taps,   \
                       gains, partial)
    if (x_is_f64) { if (gains) DAM_TP(double, true); else DAM_TP(double, false); }
    else { if (gains) DAM_TP(float, true); else DAM_TP(float, false); }
#undef DAM_TP
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(true_peak_reduce_kernel, dim3((unsigned)rows), dim3(WAVE), 0, st, partial, bx, sample_peak, true_peak);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_peak_limit_gains(double* gains, const double* peaks, int n_gains, int peaks_per_gain, double ceiling_lin,
                                    void* stream) {
    using namespace dam;
    if (!gains || !peaks || n_gains <= 0 || peaks_per_gain <= 0 || !(ceiling_lin > 0.0)) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(peak_limit_gains_kernel, dim3((unsigned)cdiv(n_gains, 256)), dim3(256), 0, (hipStream_t)stream, gains,
                       peaks, n_gains, peaks_per_gain, ceiling_lin);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
