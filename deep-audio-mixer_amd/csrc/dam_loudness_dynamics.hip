// dam_loudness_dynamics.hip -- loudness over time: momentary / short-term loudness curves (EBU R128: 400 ms and 3 s
// windows), the loudness range of EBU Tech 3342 and a per-window loudness-profile error (include/dam_hip.h).
//
// The reference has no code for any of this: it only calls `pyln.Meter(sr).integrated_loudness` (evaluation.py:39-46), one
// number per stem, which cannot tell a mix that rides a stem correctly from one that is too loud in the verses and too quiet
// in the choruses.  The samples are not touched here: the K-weighted hop energies e[c][j] come from
// dam_loudness_block_energy_batch (dam_loudness.hip) with 100 ms block bounds; what follows works on a few thousand
// doubles per track.
//   window  p_i = (sum_c G_c sum_{k<w} e[c][i+k]) / w, every value its own fixed-order sum           (window, track) grid
//   stats   absolute gate, relative gate at 0.01 * the gated mean, the 10 % / 95 % order statistics  one workgroup per track
//   error   mean |candidate profile - reference profile| over the windows where every stem is audible  one per variant
// The order statistics are an MSB-first radix SELECT over order-preserving 64-bit keys of the gated powers, 4 bits a pass,
// both ranks in the same 16 passes over the curve in global memory (a one-hour track is 36 000 doubles: L2-resident).  It is
// exact on the input doubles, needs neither a sort nor LDS or workspace in proportion to the curve, and so has no length cap.
// float64, no atomics: bin counts are per-lane registers, summed by wave shuffles and four LDS words per bin.
#include "dam_common.h"

#pragma clang fp contract(off)        // the sums below are stated operation by operation in the header; no fused multiply-add

namespace dam {
namespace {

constexpr int DYN_THREADS = 256;
constexpr int DYN_WAVES = DYN_THREADS / WAVE;
constexpr int DYN_RADIX_BITS = 4, DYN_BINS = 1 << DYN_RADIX_BITS;

__device__ __forceinline__ double dyn_lufs(double p) { return -0.691 + 10.0 * log10(p); }

__global__ __launch_bounds__(DYN_THREADS) void dyn_window_power_kernel(const double* __restrict__ e, int channels, int n_hops,
                                                                      int w, int n_windows, double* __restrict__ power,
                                                                      double* __restrict__ lufs) {
    const double G[5] = {1.0, 1.0, 1.0, 1.41, 1.41};
    const int i = blockIdx.x * DYN_THREADS + threadIdx.x, track = blockIdx.y;
    if (i >= n_windows) return;
    const double* et = e + (int64_t)track * channels * n_hops + i;
    double p = 0.0;
    for (int c = 0; c < channels; ++c) {
        double s = 0.0;
        for (int k = 0; k < w; ++k) s += et[(int64_t)c * n_hops + k];
        p += G[c] * s;
    }
    p = p / (double)w;
    power[(int64_t)track * n_windows + i] = p;
    if (lufs) lufs[(int64_t)track * n_windows + i] = dyn_lufs(p);
}

// order-preserving 64-bit key of a double (a < b  <=>  key(a) < key(b), -0.0 below +0.0) and its inverse
__device__ __forceinline__ uint64_t dyn_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dyn_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ unsigned dyn_wave_sum(unsigned v) {
    for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(DYN_THREADS) void dyn_curve_stats_kernel(const double* __restrict__ power, int n_windows,
                                                                     double* __restrict__ out /* [tracks][6] */) {
    __shared__ double red[3][DYN_THREADS];                 // gated sum, gated count, maximum
    __shared__ unsigned bins[DYN_WAVES][2][DYN_BINS];      // per wave: the bin counts of the two ranks
    const int t = threadIdx.x, lane = t % WAVE, wave = t / WAVE;
    const double* p = power + (int64_t)blockIdx.x * n_windows;

    // absolute gate: mean of the kept powers in kw_gate_kernel's order; the ungated maximum on the way
    double sum = 0.0, cnt = 0.0, mx = 0.0;
    for (int j = t; j < n_windows; j += DYN_THREADS) {
        const double v = p[j];
        if (v >= DAM_LOUDNESS_ABS_GATE_POWER) { sum += v; cnt += 1.0; }
        mx = v > mx ? v : mx;
    }
    red[0][t] = sum; red[1][t] = cnt; red[2][t] = mx;
    __syncthreads();
    for (int w = DYN_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] = red[2][t + w] > red[2][t] ? red[2][t + w] : red[2][t];
        }
        __syncthreads();
    }
    const double m = red[0][0] / red[1][0];                // an empty gate: 0/0 = NaN, and then nothing passes `>= thr`
    const double thr = 0.01 * m;
    mx = red[2][0];

    // radix select of the ranks k[0] (10 %) and k[1] (95 %) among the powers that pass both gates.  prefix[r] holds the
    // bits of rank r's key found so far; a pass counts, for either rank, the keys that share its prefix by their next 4 bits.
    uint64_t prefix[2] = {0, 0};
    int64_t k[2] = {0, 0};
    unsigned n = 0;
    for (int pass = 0; pass < 64 / DYN_RADIX_BITS; ++pass) {
        const int shift = 64 - DYN_RADIX_BITS * (pass + 1);
        const uint64_t himask = pass ? ~0ull << (shift + DYN_RADIX_BITS) : 0ull;
        unsigned c0[DYN_BINS], c1[DYN_BINS];
#pragma unroll
        for (int b = 0; b < DYN_BINS; ++b) { c0[b] = 0; c1[b] = 0; }
        for (int j = t; j < n_windows; j += DYN_THREADS) {
            const double v = p[j];
            if (!(v >= DAM_LOUDNESS_ABS_GATE_POWER && v >= thr)) continue;
            const uint64_t key = dyn_key(v);
            const unsigned d = (unsigned)(key >> shift) & (DYN_BINS - 1);
            const bool in0 = (key & himask) == prefix[0], in1 = (key & himask) == prefix[1];
#pragma unroll
            for (int b = 0; b < DYN_BINS; ++b) {
                c0[b] += (in0 && d == (unsigned)b) ? 1u : 0u;
                c1[b] += (in1 && d == (unsigned)b) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int b = 0; b < DYN_BINS; ++b) {
            const unsigned s0 = dyn_wave_sum(c0[b]), s1 = dyn_wave_sum(c1[b]);
            if (lane == 0) { bins[wave][0][b] = s0; bins[wave][1][b] = s1; }
        }
        __syncthreads();
        if (pass == 0) {                                   // every key shares the empty prefix: the bins add up to n
            for (int b = 0; b < DYN_BINS; ++b)
                for (int q = 0; q < DYN_WAVES; ++q) n += bins[q][0][b];
            if (n) {
                k[0] = ((int64_t)(n - 1) * 10 + 50) / 100;
                k[1] = ((int64_t)(n - 1) * 95 + 50) / 100;
            }
        }
        if (n == 0) break;                                 // (uniform: every thread read the same counts)
        for (int r = 0; r < 2; ++r) {                      // the bin that holds rank k[r]; k[r] becomes the rank inside it
            int64_t below = 0;
            int digit = DYN_BINS - 1;
            bool found = false;
            for (int b = 0; b < DYN_BINS; ++b) {
                int64_t c = 0;
                for (int q = 0; q < DYN_WAVES; ++q) c += bins[q][r][b];
                if (!found && k[r] < below + c) { digit = b; found = true; }
                if (!found) below += c;
            }
            k[r] -= below;
            prefix[r] |= (uint64_t)digit << shift;
        }
        __syncthreads();                                   // bins are rewritten by the next pass
    }

    if (t == 0) {
        double* o = out + (int64_t)blockIdx.x * 6;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double l_lo = n ? dyn_lufs(dyn_unkey(prefix[0])) : nan, l_hi = n ? dyn_lufs(dyn_unkey(prefix[1])) : nan;
        o[0] = n ? l_hi - l_lo : 0.0;
        o[1] = l_lo;
        o[2] = l_hi;
        o[3] = dyn_lufs(m) - 20.0;
        o[4] = (double)n;
        o[5] = dyn_lufs(mx);
    }
}

__global__ __launch_bounds__(DYN_THREADS) void dyn_profile_error_kernel(const double* __restrict__ ref,
                                                                       const double* __restrict__ cand_all, int n_stems,
                                                                       int n_windows, double* __restrict__ err,
                                                                       double* __restrict__ active) {
    __shared__ double red[2][DYN_THREADS];
    const int t = threadIdx.x;
    const double* cand = cand_all + (int64_t)blockIdx.x * n_stems * n_windows;
    double sum = 0.0, cnt = 0.0;
    for (int i = t; i < n_windows; i += DYN_THREADS) {
        bool live = true;
        double mr = 0.0, mc = 0.0;
        for (int s = 0; s < n_stems; ++s) {
            const double r = ref[(int64_t)s * n_windows + i], c = cand[(int64_t)s * n_windows + i];
            live = live && r >= -70.0 && c >= -70.0;
            mr += r; mc += c;
        }
        if (!live) continue;
        mr = mr / (double)n_stems; mc = mc / (double)n_stems;
        double a = 0.0;
        for (int s = 0; s < n_stems; ++s)
            a += fabs((cand[(int64_t)s * n_windows + i] - mc) - (ref[(int64_t)s * n_windows + i] - mr));
        sum += a; cnt += 1.0;
    }
    red[0][t] = sum; red[1][t] = cnt;
    __syncthreads();
    for (int w = DYN_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        err[blockIdx.x] = red[0][0] / (red[1][0] * (double)n_stems);      // no active window: 0/0 = NaN
        active[blockIdx.x] = red[1][0];
    }
}

}  // namespace
}  // namespace dam

// Momentary (w = 4) / short-term (w = 30) power and loudness of every 100 ms hop (EBU R128 / Tech 3341 windows).
extern "C" int dam_loudness_window_power(const double* e, int n_tracks, int channels, int n_hops, int w, double* power,
                                         double* lufs, void* stream) {
    using namespace dam;
    if (!e || !power || n_tracks <= 0 || channels <= 0 || channels > 5 || w <= 0 || n_hops < w) return DAM_ERR_BAD_ARG;
    if (n_tracks > 65535) return DAM_ERR_UNSUPPORTED;
    const int n_windows = n_hops - w + 1;
    hipLaunchKernelGGL(dyn_window_power_kernel, dim3((unsigned)cdiv(n_windows, DYN_THREADS), (unsigned)n_tracks),
                       dim3(DYN_THREADS), 0, (hipStream_t)stream, e, channels, n_hops, w, n_windows, power, lufs);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// Loudness range (EBU Tech 3342: -70 LUFS / -20 LU gates, 10th and 95th percentile) and the maximum of a power curve.
extern "C" int dam_loudness_curve_stats(const double* power, int n_tracks, int n_windows, double* out, void* stream) {
    using namespace dam;
    if (!power || !out || n_tracks <= 0 || n_windows <= 0) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(dyn_curve_stats_kernel, dim3((unsigned)n_tracks), dim3(DYN_THREADS), 0, (hipStream_t)stream, power,
                       n_windows, out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// The per-window form of evaluation.py:39-53 (evaluate_loudness + _calculate_diff_between_loudness_dicts).
extern "C" int dam_loudness_profile_error(const double* ref_lufs, const double* cand_lufs, int n_variants, int n_stems,
                                          int n_windows, double* err, double* active, void* stream) {
    using namespace dam;
    if (!ref_lufs || !cand_lufs || !err || !active || n_variants <= 0 || n_stems <= 0 || n_windows <= 0) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(dyn_profile_error_kernel, dim3((unsigned)n_variants), dim3(DYN_THREADS), 0, (hipStream_t)stream, ref_lufs,
                       cand_lufs, n_stems, n_windows, err, active);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
