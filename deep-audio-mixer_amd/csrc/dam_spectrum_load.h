// The mix-signal loader shared by the band spectrum (dam_spectrum.hip) and the spectrogram distance (dam_specdist.hip):
// xm of include/dam_hip.h ("Band spectrum": Mix signal) for the two samples of one complex point of a packed frame.
#pragma once
#include "dam_common.h"

#pragma clang fp contract(off)        // the mix signal is stated operation by operation; no fused multiply-add

namespace dam {

struct SpecGeo {
    int64_t n_samples, stem_stride, sample_stride, channel_stride;
    int64_t gseg;                     // n_samples / n_gains
    int n_stems, channels, n_gains, n_fft, hop, n_frames, n_bands, blocks_per_mix;
    int small;                        // n_samples < 2^31: the gain index is a 32-bit division
};

// xm[a], xm[b] of the header for the two samples of one complex point: the stems' channel means times their gains, summed in
// double in ascending s, rounded to float once.  The stems are taken two at a time, every load of the two (both samples, both
// channels, the gains) issued before the first is used (stem index clamped, the surplus value dropped): with one load per
// dependent addition a frame's loader was a chain of exposed memory latencies at two waves per SIMD.  Four at a time ran the
// kernel out of SGPRs (frame-invariant offsets per stem: 10 spilled), two do not.  The order of the additions is the plain loop's.
constexpr int SPEC_STEMS_AT_ONCE = 2;

__device__ __forceinline__ int64_t gain_index(const SpecGeo& g, int64_t p) {
    int64_t gi = g.small ? (int64_t)((uint32_t)p / (uint32_t)g.gseg) : p / g.gseg;
    return gi > g.n_gains - 1 ? g.n_gains - 1 : gi;
}

template <typename T>
__device__ __forceinline__ float2 mix_pair(const T* __restrict__ xr, const double* __restrict__ gr, const SpecGeo& g, int64_t a,
                                           int64_t b) {
    const bool ramp = gr && g.n_gains > 1;
    const int64_t gia = ramp ? gain_index(g, a) : 0, gib = ramp ? gain_index(g, b) : 0;
    const T* pa = xr + a * g.sample_stride;
    const T* pb = xr + b * g.sample_stride;
    const bool stereo = g.channels == 2;
    double acc_a = 0.0, acc_b = 0.0;
    for (int s0 = 0; s0 < g.n_stems; s0 += SPEC_STEMS_AT_ONCE) {
        T a0[SPEC_STEMS_AT_ONCE], a1[SPEC_STEMS_AT_ONCE], b0[SPEC_STEMS_AT_ONCE], b1[SPEC_STEMS_AT_ONCE];
        double ga[SPEC_STEMS_AT_ONCE], gb[SPEC_STEMS_AT_ONCE];
#pragma unroll
        for (int j = 0; j < SPEC_STEMS_AT_ONCE; ++j) {
            const int s = s0 + j < g.n_stems ? s0 + j : g.n_stems - 1;
            const int64_t o = s * g.stem_stride;
            a0[j] = pa[o];
            b0[j] = pb[o];
            a1[j] = stereo ? pa[o + g.channel_stride] : (T)0;
            b1[j] = stereo ? pb[o + g.channel_stride] : (T)0;
            ga[j] = gr ? gr[(int64_t)s * g.n_gains + gia] : 1.0;
            gb[j] = gr ? gr[(int64_t)s * g.n_gains + gib] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < SPEC_STEMS_AT_ONCE; ++j) {
            if (s0 + j < g.n_stems) {
                double ma = stereo ? ((double)a0[j] + (double)a1[j]) * 0.5 : (double)a0[j];
                double mb = stereo ? ((double)b0[j] + (double)b1[j]) * 0.5 : (double)b0[j];
                if (gr) { ma = ma * ga[j]; mb = mb * gb[j]; }
                acc_a = s0 + j ? acc_a + ma : ma;
                acc_b = s0 + j ? acc_b + mb : mb;
            }
        }
    }
    return make_float2((float)acc_a, (float)acc_b);
}

}  // namespace dam
