// dam_limiter.hip -- look-ahead true-peak limiter: a time-varying gain that keeps the reconstructed waveform of a row set
// (the channels of one master) under a ceiling where dam_peak_limit_gains can only turn the whole song down.
//
// Definition (include/dam_hip.h states it in full; tests/_limiter_ref.py restates it in numpy).  All float64, closed form,
// no recurrence and no state: every output sample is a function of a bounded input window.
//   xs[c][i] = (double)x[c][i] * s                                    s = pre_gain of the row set, 1 if none
//   d[i]     = max_c max(|xs[c][i]|, |y_1[c][i]|, |y_2[c][i]|, |y_3[c][i]|)       y_p: the meter's phases (dam_truepeak_fir.h)
//   r[i]     = min(1, ceil / d[i])                                    1 where d = 0 and outside [0, n)
//   m[j]     = min_{k in [j-H, j+L]} r[k]                             hold and look-ahead: exact, order-free
//   g[i]     = (sum_{j=i-L..i} m[j], j ascending) / (double)(L+1)     attack / release ramp: its own sum per sample
//   out[c][i] = xs[c][i] * g[i]
//
// Two launches and a reduction.  limiter_demand_kernel is the meter's tile kernel with the maximum taken across the
// channels per sample instead of across the samples per row: it writes r[n] (8 B per sample) to the workspace.  Recomputing
// the demand over the halo inside the apply kernel instead would redo 36 FMAs per channel on L + H + L extra samples of
// every 2048 (x1.65 at the 44.1 kHz defaults, x3.5 at the caps) to save 16 B per sample of traffic.
// limiter_apply_kernel: one workgroup owns LIM_TILE consecutive samples of one row set.  It stages r over
// [t0 - L - H, t0 + T + L) in LDS (every r a g of the tile depends on), forms the doubling min-table there (level k holds
// the minimum over 2^k consecutive values; two LDS images, ping-pong, one barrier per level) and from two overlapping
// table entries m over [t0 - L, t0 + T).  Lane l owns the 8 consecutive samples behind 8 l: it walks m[8l - L .. 8l + 7]
// once, ascending, adding each value to those of its 8 sums whose window holds it -- L + 8 LDS reads for 8 sums, each sum
// still L + 1 terms in the order j = i-L .. i.  m is padded like the meter's image (e + e / 8: lane stride 9 doubles).
// A tile whose staged r are all 1.0 skips table and sums: g = (L+1) * 1.0 / (L+1) = 1.0 exactly either way.
// Each workgroup leaves min g and #{g < 1} of its samples in the workspace; limiter_stats_kernel reduces them per row set
// (a minimum and an integer sum: order-free).  No atomics.  Nothing depends on the grid or on the other row sets.
#include "dam_common.h"
#include "dam_truepeak_fir.h"

#include <math.h>

namespace dam {
namespace {

constexpr int LIM_THREADS = TP_THREADS;
constexpr int LIM_RUN = TP_RUN;
constexpr int LIM_TILE = TP_TILE;                      // samples per workgroup, of both kernels
constexpr int LIM_MAX_LOOKAHEAD = 512;
constexpr int LIM_MAX_HOLD = 4096;                     // at the caps: 2 x 7168 doubles = 112 KiB of LDS, one workgroup per CU

struct LimGeo {
    int64_t n_samples;
    int64_t set_stride, sample_stride, channel_stride;        // elements
    int channels, L, H;
    double ceiling;
};

// elements of one of the two LDS images: r over the tile and its halo, or m padded by one double per 8
__host__ __device__ constexpr int lim_image_elems(int L, int H) {
    const int span = LIM_TILE + 2 * L + H, mpad = (LIM_TILE + L) + ((LIM_TILE + L) >> 3) + 1;
    return span > mpad ? span : mpad;
}

// dynamic LDS of the apply kernel: the two images, one double and one int per wave for the statistics
__host__ __device__ constexpr int lim_lds_bytes(int L, int H) {
    return 2 * lim_image_elems(L, H) * (int)sizeof(double) + (LIM_THREADS / WAVE) * (int)(sizeof(double) + sizeof(int));
}

template <typename T>
__global__ __launch_bounds__(LIM_THREADS) void limiter_demand_kernel(const T* __restrict__ x, LimGeo g, TpTaps taps,
                                                                      const double* __restrict__ pre_gain,
                                                                      double* __restrict__ req /* [set][n] */) {
    __shared__ double img[TP_LDS];
    const int t = threadIdx.x, set = blockIdx.y;
    const double s = pre_gain ? pre_gain[set] : 1.0;
    const int64_t first = (int64_t)blockIdx.x * LIM_TILE - TP_BEFORE;
    double d[LIM_RUN];
#pragma unroll
    for (int r = 0; r < LIM_RUN; ++r) d[r] = 0.0;
    for (int c = 0; c < g.channels; ++c) {
        const T* xr = x + set * g.set_stride + c * g.channel_stride;
        if (c) __syncthreads();                        // the previous channel's image has been consumed
#pragma unroll
        for (int k = 0; k < TP_LOADS; ++k) {
            const int e = k * LIM_THREADS + t;
            const int64_t n = first + e;
            if (e < TP_SPAN) img[e + (e >> 3)] = (n >= 0 && n < g.n_samples) ? (double)xr[n * g.sample_stride] * s : 0.0;
        }
        __syncthreads();
        double w[TP_RUN + TP_BEFORE + TP_AFTER];
        tp_window(img, t, w);
#pragma unroll
        for (int r = 0; r < LIM_RUN; ++r) {
            double y0, y1, y2;
            tp_phases(w, r, taps, y0, y1, y2);
            d[r] = fmax(d[r], fmax(fmax(fabs(w[r + TP_BEFORE]), fabs(y0)), fmax(fabs(y1), fabs(y2))));
        }
    }
    const int64_t i0 = (int64_t)blockIdx.x * LIM_TILE + (int64_t)t * LIM_RUN;
    double* rr = req + (int64_t)set * g.n_samples;
#pragma unroll
    for (int r = 0; r < LIM_RUN; ++r)
        if (i0 + r < g.n_samples) rr[i0 + r] = fmin(1.0, g.ceiling / d[r]);        // d = 0: ceiling / 0 = +inf -> 1
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(LIM_THREADS) void limiter_apply_kernel(const TIn* __restrict__ x, LimGeo g,
                                                                     const double* __restrict__ pre_gain,
                                                                     const double* __restrict__ req, TOut* __restrict__ out,
                                                                     double* __restrict__ part_min, int64_t* __restrict__ part_cnt) {
    extern __shared__ double lim_lds[];                // two images, then the waves' partial statistics
    const int t = threadIdx.x, set = blockIdx.y;
    const int L = g.L, H = g.H;
    const int span = LIM_TILE + 2 * L + H, image = lim_image_elems(L, H);
    const int64_t t0 = (int64_t)blockIdx.x * LIM_TILE;
    const double* rr = req + (int64_t)set * g.n_samples;

    // image element e is r[t0 - L - H + e]
    double* cur = lim_lds;
    double* nxt = lim_lds + image;
    double* red_min = lim_lds + 2 * image;
    int* red_cnt = reinterpret_cast<int*>(red_min + LIM_THREADS / WAVE);
    int below = 0;
    for (int e = t; e < span; e += LIM_THREADS) {
        const int64_t i = t0 - L - H + e;
        const double v = (i >= 0 && i < g.n_samples) ? rr[i] : 1.0;
        below |= v < 1.0;
        cur[e] = v;
    }
    double gain[LIM_RUN];
    if (__syncthreads_or(below)) {
        // table of span h: entry e = min r over [e, e + h); doubled until 2 h > W = L + H + 1
        const int W = L + H + 1;
        int h = 1;
        for (; 2 * h <= W; h *= 2) {
            for (int e = t; e < span; e += LIM_THREADS) nxt[e] = e + h < span ? fmin(cur[e], cur[e + h]) : cur[e];
            __syncthreads();
            double* swap = cur; cur = nxt; nxt = swap;
        }
        // m[t0 - L + u] = min r over image elements [u, u + W): two entries of span h, h <= W < 2 h
        for (int u = t; u < LIM_TILE + L; u += LIM_THREADS) nxt[u + (u >> 3)] = fmin(cur[u], cur[u + W - h]);
        __syncthreads();
        // the lane's samples are i0 + r, i0 = t0 + 8 t; m[i0 - L + q] is element 8 t + q, at 9 t + q + q / 8
        const double* m = nxt + t * (LIM_RUN + 1);
        double acc[LIM_RUN];
#pragma unroll
        for (int r = 0; r < LIM_RUN; ++r) acc[r] = 0.0;
        // sample r sums q = r .. r + L, ascending.  q in [7, L] belongs to all 8 sums.
        auto edge = [&](int q) {
            const double v = m[q + (q >> 3)];
#pragma unroll
            for (int r = 0; r < LIM_RUN; ++r)
                if (q >= r && q <= r + L) acc[r] += v;
        };
        for (int q = 0; q < LIM_RUN - 1; ++q) edge(q);
#pragma unroll 4
        for (int q = LIM_RUN - 1; q <= L; ++q) {
            const double v = m[q + (q >> 3)];
#pragma unroll
            for (int r = 0; r < LIM_RUN; ++r) acc[r] += v;
        }
        for (int q = L + 1 > LIM_RUN - 1 ? L + 1 : LIM_RUN - 1; q < L + LIM_RUN; ++q) edge(q);
        const double terms = (double)(L + 1);
#pragma unroll
        for (int r = 0; r < LIM_RUN; ++r) gain[r] = acc[r] / terms;
    } else {
#pragma unroll
        for (int r = 0; r < LIM_RUN; ++r) gain[r] = 1.0;
    }

    const int64_t i0 = t0 + (int64_t)t * LIM_RUN;
    const int64_t left = g.n_samples - i0;             // samples of the row from i0 on
    double lo = 1.0;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < LIM_RUN; ++r)
        if (r < left) { lo = fmin(lo, gain[r]); cnt += gain[r] < 1.0; }
    const double s = pre_gain ? pre_gain[set] : 1.0;
    for (int c = 0; c < g.channels; ++c) {
        const TIn* xr = x + set * g.set_stride + c * g.channel_stride + i0 * g.sample_stride;
        TOut* o = out + ((int64_t)set * g.channels + c) * g.n_samples + i0;
#pragma unroll
        for (int r = 0; r < LIM_RUN; ++r)
            if (r < left) o[r] = (TOut)(((double)xr[r * g.sample_stride] * s) * gain[r]);
    }

#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off));
        cnt += __shfl_xor(cnt, off);
    }
    if ((t & (WAVE - 1)) == 0) { red_min[t / WAVE] = lo; red_cnt[t / WAVE] = cnt; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int i = 1; i < LIM_THREADS / WAVE; ++i) { lo = fmin(lo, red_min[i]); cnt += red_cnt[i]; }
        const int64_t p = (int64_t)set * gridDim.x + blockIdx.x;
        part_min[p] = lo;
        part_cnt[p] = cnt;
    }
}

// one workgroup per row set: the minimum and the sum of its tiles' partials
__global__ __launch_bounds__(LIM_THREADS) void limiter_stats_kernel(const double* __restrict__ part_min,
                                                                     const int64_t* __restrict__ part_cnt, int64_t tiles,
                                                                     double* __restrict__ min_gain, int64_t* __restrict__ n_limited) {
    __shared__ double red_min[LIM_THREADS];
    __shared__ int64_t red_cnt[LIM_THREADS];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * tiles;
    double lo = 1.0;
    int64_t cnt = 0;
    for (int64_t i = t; i < tiles; i += LIM_THREADS) { lo = fmin(lo, part_min[p0 + i]); cnt += part_cnt[p0 + i]; }
    red_min[t] = lo;
    red_cnt[t] = cnt;
    __syncthreads();
    for (int w = LIM_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) { red_min[t] = fmin(red_min[t], red_min[t + w]); red_cnt[t] += red_cnt[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        if (min_gain) min_gain[blockIdx.x] = red_min[0];
        if (n_limited) n_limited[blockIdx.x] = red_cnt[0];
    }
}

template <typename TIn, typename TOut>
static int launch_apply(dim3 grid, int lds, hipStream_t st, const void* x, const LimGeo& g, const double* pre_gain,
                        const double* req, void* out, double* part_min, int64_t* part_cnt) {
    if (lds > 64 * 1024 && !raise_lds_limit<&limiter_apply_kernel<TIn, TOut>>(lim_lds_bytes(LIM_MAX_LOOKAHEAD, LIM_MAX_HOLD)))
        return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((limiter_apply_kernel<TIn, TOut>), grid, dim3(LIM_THREADS), lds, st, reinterpret_cast<const TIn*>(x), g,
                       pre_gain, req, reinterpret_cast<TOut*>(out), part_min, part_cnt);
    return DAM_OK;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_limiter_tile_samples(void) { return dam::LIM_TILE; }
extern "C" int dam_limiter_max_lookahead(void) { return dam::LIM_MAX_LOOKAHEAD; }
extern "C" int dam_limiter_max_hold(void) { return dam::LIM_MAX_HOLD; }

extern "C" int64_t dam_limiter_workspace_bytes(int n_sets, int64_t n_samples) {
    if (n_sets <= 0 || n_samples <= 0) return 0;
    return (int64_t)n_sets * (n_samples + 2 * dam::cdiv(n_samples, dam::LIM_TILE)) * 8;
}

extern "C" int dam_limiter_apply(const void* x, int x_is_f64, int n_sets, int64_t n_samples, int channels, int64_t set_stride,
                                 int64_t sample_stride, int64_t channel_stride, const double* pre_gain, double ceiling_lin,
                                 int lookahead, int hold, void* out, int out_is_f64, double* min_gain, int64_t* n_limited,
                                 void* workspace, void* stream) {
    using namespace dam;
    if (!x || !out || !workspace) return DAM_ERR_BAD_ARG;
    if (n_sets <= 0 || n_samples <= 0 || channels <= 0) return DAM_ERR_BAD_ARG;
    if (n_sets > 65535) return DAM_ERR_BAD_ARG;
    if (!(ceiling_lin > 0.0)) return DAM_ERR_BAD_ARG;
    if (lookahead < 1 || lookahead > LIM_MAX_LOOKAHEAD || hold < 1 || hold > LIM_MAX_HOLD) return DAM_ERR_BAD_ARG;
    LimGeo g;
    g.n_samples = n_samples;
    g.set_stride = set_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.channels = channels; g.L = lookahead; g.H = hold;
    g.ceiling = ceiling_lin;
    const int64_t tiles = cdiv(n_samples, LIM_TILE);
    if (tiles > 0x7fffffff) return DAM_ERR_BAD_ARG;
    double* req = reinterpret_cast<double*>(workspace);
    double* part_min = req + (int64_t)n_sets * n_samples;
    int64_t* part_cnt = reinterpret_cast<int64_t*>(part_min + (int64_t)n_sets * tiles);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)n_sets);
    const TpTaps taps = tp_taps_host();
    if (x_is_f64)
        hipLaunchKernelGGL(limiter_demand_kernel<double>, grid, dim3(LIM_THREADS), 0, st, reinterpret_cast<const double*>(x), g,
                           taps, pre_gain, req);
    else
        hipLaunchKernelGGL(limiter_demand_kernel<float>, grid, dim3(LIM_THREADS), 0, st, reinterpret_cast<const float*>(x), g,
                           taps, pre_gain, req);
    DAM_CHECK_LAUNCH();
    const int lds = lim_lds_bytes(lookahead, hold);
    int rc;
    if (x_is_f64)
        rc = out_is_f64 ? launch_apply<double, double>(grid, lds, st, x, g, pre_gain, req, out, part_min, part_cnt)
                        : launch_apply<double, float>(grid, lds, st, x, g, pre_gain, req, out, part_min, part_cnt);
    else
        rc = out_is_f64 ? launch_apply<float, double>(grid, lds, st, x, g, pre_gain, req, out, part_min, part_cnt)
                        : launch_apply<float, float>(grid, lds, st, x, g, pre_gain, req, out, part_min, part_cnt);
    if (rc != DAM_OK) return rc;
    DAM_CHECK_LAUNCH();
    if (min_gain || n_limited) {
        hipLaunchKernelGGL(limiter_stats_kernel, dim3((unsigned)n_sets), dim3(LIM_THREADS), 0, st, part_min, part_cnt, tiles,
                           min_gain, n_limited);
        DAM_CHECK_LAUNCH();
    }
    return DAM_OK;
}
