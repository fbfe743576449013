// The true-peak interpolator's device pieces, shared by the meter (dam_truepeak.hip) and the limiter's demand kernel
// (dam_limiter.hip): the 18 distinct taps, the padded LDS image of a tile and its halo, and the three interpolated phases
// of one sample in the fixed order j = -6 .. 5.  One definition, so that the limiter's demand IS the meter's y_p.
#pragma once
#include "dam_common.h"

namespace dam {

constexpr int TP_THREADS = 256;
constexpr int TP_RUN = 8;                              // consecutive samples per lane
constexpr int TP_TILE = TP_THREADS * TP_RUN;           // samples per tile
constexpr int TP_BEFORE = 5, TP_AFTER = 6;             // halo: y_p[i] reads x[i-5 .. i+6]
constexpr int TP_SPAN = TP_TILE + TP_BEFORE + TP_AFTER;
constexpr int TP_LOADS = (TP_SPAN + TP_THREADS - 1) / TP_THREADS;
constexpr int TP_LDS = TP_SPAN + (TP_SPAN >> 3) + 1;   // image element e lives at e + e / 8

// The taps are symmetric (h49[k] == h49[48 - k], by construction in dam_true_peak_taps_host), so phase 3 is phase 1
// reversed and phase 2 is its own mirror: 18 distinct values, which stay in scalar registers.
struct TpTaps {
    double a[12];                                      // a[j+6] = h49[24 + 1 + 4 j]; h49[24 + 3 + 4 j] = a[5 - j]
    double b[6];                                       // b[j+6] = h49[24 + 2 + 4 j] for j < 0; = b[5 - j] for j >= 0
};

static inline TpTaps tp_taps_host() {
    double h[49];
    dam_true_peak_taps_host(h);
    TpTaps taps;
    for (int j = -6; j <= 5; ++j) taps.a[j + 6] = h[24 + 1 + 4 * j];
    for (int j = -6; j < 0; ++j) taps.b[j + 6] = h[24 + 2 + 4 * j];
    return taps;
}

// The lane's window out of the padded image: w[k] = x[i0 - 5 + k], i0 = the lane's first sample; element t * 8 + k sits at
// t * 9 + k + k / 8 (a lane stride of 9 doubles = 18 banks: conflict-free for ds_read_b64).
__device__ __forceinline__ void tp_window(const double* img, int t, double (&w)[TP_RUN + TP_BEFORE + TP_AFTER]) {
    const double* base = img + t * (TP_RUN + 1);
#pragma unroll
    for (int k = 0; k < TP_RUN + TP_BEFORE + TP_AFTER; ++k) w[k] = base[k + (k >> 3)];
}

// y_1, y_2, y_3 of the lane's sample r: x[i - j] = w[r + 5 - j], j = -6 reads w[r + 11], j = 5 reads w[r]
__device__ __forceinline__ void tp_phases(const double (&w)[TP_RUN + TP_BEFORE + TP_AFTER], int r, const TpTaps taps,
                                          double& y0, double& y1, double& y2) {
    y0 = w[r + 11] * taps.a[0], y1 = w[r + 11] * taps.b[0], y2 = w[r + 11] * taps.a[11];
#pragma unroll
    for (int q = 1; q < 12; ++q) {
        y0 = fma(w[r + 11 - q], taps.a[q], y0);
        y1 = fma(w[r + 11 - q], taps.b[q < 6 ? q : 11 - q], y1);
        y2 = fma(w[r + 11 - q], taps.a[11 - q], y2);
    }
}

}  // namespace dam
