// The frame and level code shared by the spectrogram distance (dam_specdist.hip) and its gradient in the gains
// (dam_specgrad.hip): both must form the same float32 levels from the same float32 frames, operation for operation.
#pragma once
#include "dam_common.h"
#include "dam_fft_lds.h"
#include "dam_spectrum_load.h"   // SpecGeo, mix_pair: the loader of the band spectrum

#pragma clang fp contract(off)        // levels are stated operation by operation

namespace dam {

// The front-end's power_to_db (dam_stft.hip), from the power p = |X|^2.
__device__ __forceinline__ float level_db(float p, float amin2, float floor_db) {
    return p <= amin2 ? floor_db : 3.01029995663981195f * __log2f(p);
}

// The frame of one mix at sample p0 (reflect-padded), windowed, packed as M complex points into buf; then transformed.
template <typename T>
__device__ __forceinline__ const float2* transform_frame(float2* buf, const T* __restrict__ x, const double* __restrict__ gr,
                                                         const SpecGeo& g, int64_t p0, const float* __restrict__ window,
                                                         const float2* __restrict__ tw, int tid) {
    const int M = g.n_fft >> 1;
    for (int n = tid; n < M; n += FFT_THREADS) {
        const int64_t a = reflect(p0 + 2 * n, g.n_samples), b = reflect(p0 + 2 * n + 1, g.n_samples);
        const float2 xm = mix_pair<T>(x, gr, g, a, b);
        buf[n] = make_float2(xm.x * window[2 * n], xm.y * window[2 * n + 1]);
    }
    __syncthreads();
    return lds_fft_radix2<false>(buf, buf + M, M, g.n_fft, tw, tid);
}

}  // namespace dam
