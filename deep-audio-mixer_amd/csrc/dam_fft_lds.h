// Workgroup FFT in LDS, shared by the complex forward front-end (dam_stft.hip) and the inverse transform (dam_istft.hip).
#pragma once
#include "dam_common.h"

namespace dam {

constexpr int FFT_THREADS = 256;

// log2(M) autosort (Stockham) radix-2 passes over the M complex points in x[], ping-ponging with y[] (the scheme of
// stft_generic_kernel).  tw = W_nfft^k = exp(-2 pi i k / n_fft), n_fft = 2 M; INVERSE conjugates it (unnormalised inverse).
// x[] must be complete (barrier passed) on entry; the returned buffer holds the result in natural order, barrier passed.
template <bool INVERSE>
__device__ __forceinline__ float2* lds_fft_radix2(float2* x, float2* y, int M, int n_fft, const float2* __restrict__ tw, int tid) {
    int sshift = 0;                                   // s = 1 << sshift
    for (int n = M; n > 1; n >>= 1, ++sshift) {
        const int m = n >> 1, s = 1 << sshift;
        for (int e = tid; e < (M >> 1); e += FFT_THREADS) {
            const int p = e >> sshift, q = e & (s - 1);
            const float2 a = x[q + s * p], b = x[q + s * (p + m)];
            float2 w = tw[(2 * p * s) & (n_fft - 1)];                       // W_n^p = W_nfft^(2 p s)
            if (INVERSE) w.y = -w.y;
            y[q + s * (2 * p)] = cadd(a, b);
            y[q + s * (2 * p + 1)] = cmul(csub(a, b), w);
        }
        __syncthreads();
        float2* tmp = x; x = y; y = tmp;
    }
    return x;
}

}  // namespace dam
