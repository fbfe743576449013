// dam_align.hip -- the time offset of stems against a mix, by block cross-correlation on the device, and the sample shift that
// removes it (include/dam_hip.h states the definitions).
//
// The gain fit compares sample by sample, so it can only be trusted on a target that is aligned with the stems: a real mix (a
// dataset's own mix file, a bounce with plug-in delay, a file trimmed by hand as experiments.ipynb's last cell does) is not,
// and a handful of samples of offset rotate the phase of everything above a few kHz.  This is the measurement of that offset
// and its removal; estimate -> shift -> fit never comes to the host.
//   cross spectrum  one workgroup = AL_F consecutive half-overlapped frames of one (stem, mix) pair: the mix frame (N samples)
//                   and the zero-padded stem frame (N/2 samples) go through the LDS radix-2 FFT of dam_fft_lds.h, conj(A) Y is
//                   added in float64 to the lane's own bins; the energies of both signals ride along   (frame run, stem) grid
//   reduce          a pair's workgroup records added in ascending workgroup order                       (record slice, stem) grid
//   finish          weighting, float32 LDS inverse transform of the spectrum scaled to unit peak, peak search, parabola
//                                                                                                     one workgroup per pair
//   shift           out[s][p] = x[s][p - lag[s]], lag read from device memory                          (sample run, stem) grid
// The mix frame is transformed by every stem's workgroup: sharing it would need S sets of per-lane float64 bin sums (4 x 32
// doubles per stem at N = 16384) or a second LDS image, and neither fits.  Not tuned beyond its structure: the loader reads
// sample by sample through runtime strides (any layout, float32 / float64 stems and mix independently).
#include "dam_common.h"
#include "dam_fft_lds.h"

#pragma clang fp contract(off)        // the sums are stated operation by operation; no fused multiply-add

namespace dam {
namespace {

constexpr int AL_F = 8;               // frames one workgroup owns: a library constant, never a function of the batch
constexpr int AL_MAX_LAG = 4096;
constexpr int AL_MAX_S = 8;
constexpr int AL_STASH_PER = 32;      // bins per lane from which the mix frame's bins are kept in the workspace
constexpr int AL_SCRATCH = 4096;      // bytes of the finish kernel's dynamic LDS behind the two FFT images

struct AlGeo {
    int64_t n_samples, stem_stride, sample_stride, channel_stride, y_sample_stride, y_channel_stride;
    int channels, n_fft, n_frames, blocks_per_pair;
};

int align_fft_size(int max_lag) {
    if (max_lag < 1 || max_lag > AL_MAX_LAG) return 0;
    int p = 1;
    while (p < max_lag) p <<= 1;
    return 4 * p < 64 ? 64 : 4 * p;
}

// doubles of one record: re[0 .. M], im[0 .. M], E_a, E_y
__host__ __device__ inline int64_t record_doubles(int n_fft) { return 2 * (int64_t)(n_fft / 2 + 1) + 2; }

// doubles of one workgroup's slice for the mix frame's bins (N/2 float2), where the cross-spectrum kernel keeps them there
inline int64_t stash_doubles(int n_fft) { return n_fft / 2 / FFT_THREADS >= AL_STASH_PER ? n_fft / 2 : 0; }

__device__ __forceinline__ double al_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the mono signal of the header at sample p; 0 outside [0, n)
template <typename T>
__device__ __forceinline__ float mono_sample(const T* __restrict__ trk, int64_t ps, int64_t cs, bool stereo, int64_t p, int64_t n) {
    if (p < 0 || p >= n) return 0.f;
    const T* q = trk + p * ps;
    return stereo ? (float)(((double)q[0] + (double)q[cs]) * 0.5) : (float)q[0];
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

// PER = bins 0 .. M-1 a lane owns (M / 256, at least 1); the Nyquist bin M rides on lane 0.  The running sums and the mix
// frame's bins are compile-time arrays so that they stay in registers.  At PER = 32 (N = 16384) the 2 x 32 float64 sums are 128
// registers, and the kernel spilled some 290 more in two ways, each of which alone left it spilling: the mix frame's 32 bins
// held across the stem's transform, and the frame-invariant LDS / twiddle addresses and twiddle values of all 32 bins, hoisted
// out of the frame loop.  So there (STASH) the mix frame's bins wait in the workgroup's own slice of the workspace, written and
// read back by the same lane (64 KB each way per frame, beside 192 KB of samples), and the lane's first bin is made opaque
// in every frame so that nothing derived from it is loop-invariant.
template <typename TX, typename TY, int PER>
__global__ __launch_bounds__(FFT_THREADS) void align_cross_spectrum_kernel(const TX* __restrict__ x, const TY* __restrict__ y,
                                                                           const float2* __restrict__ tw /* W_N^k */, AlGeo g,
                                                                           double* __restrict__ partial, float2* stash) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M]; afterwards eight doubles of wave sums
    const int tid = threadIdx.x, M = g.n_fft >> 1, Q = M >> 1;        // M = H = N/2 samples of hop, Q = N/4
    const int blk = blockIdx.x, s = blockIdx.y;
    const TX* xs = x + (int64_t)s * g.stem_stride;
    const bool stereo = g.channels == 2;
    constexpr bool STASH = PER >= AL_STASH_PER;
    float2* ystash = stash + ((int64_t)s * g.blocks_per_pair + blk) * M;
    double cre[PER], cim[PER], nyq = 0.0, ea = 0.0, ey = 0.0;
#pragma unroll
    for (int i = 0; i < PER; ++i) cre[i] = cim[i] = 0.0;
    const int t0 = blk * AL_F, t1 = t0 + AL_F < g.n_frames ? t0 + AL_F : g.n_frames;
    for (int t = t0; t < t1; ++t) {
        const int64_t p0 = (int64_t)t * M;
        // the mix frame y[p0 - N/4 + j], j in [0, N); its energy over the frame's own samples p0 .. p0 + H - 1
        for (int n = tid; n < M; n += FFT_THREADS) {
            const int64_t p = p0 - Q + 2 * n;
            const float a = mono_sample<TY>(y, g.y_sample_stride, g.y_channel_stride, stereo, p, g.n_samples);
            const float b = mono_sample<TY>(y, g.y_sample_stride, g.y_channel_stride, stereo, p + 1, g.n_samples);
            buf[n] = make_float2(a, b);
            if (2 * n >= Q && 2 * n < Q + M) {
                ey += (double)a * (double)a;
                ey += (double)b * (double)b;
            }
        }
        __syncthreads();
        const float2* z = lds_fft_radix2<false>(buf, buf + M, M, g.n_fft, tw, tid);
        float2 yk[STASH ? 1 : PER];
        float ynyq = 0.f;
        int k0 = tid;
        if (STASH) asm volatile("" : "+v"(k0));
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + FFT_THREADS * i;
            float2 v = make_float2(0.f, 0.f);
            if (PER > 1 || k < M) {                                   // PER > 1: M = 256 PER, every k is a bin
                v = real_fft_bin(z, k, M, tw);
                if (k == 0) v.y = 0.f;                                // DC of a real signal
            }
            if (STASH) ystash[k] = v;                                 // read back below by the lane that wrote it
            else yk[i] = v;
        }
        if (tid == 0) ynyq = real_fft_bin(z, M, M, tw).x;             // Nyquist, real as well
        __syncthreads();                                              // z is read: the stem frame may land
        // the stem frame a[p0 + j], j in [0, H), zeros above
        for (int n = tid; n < M; n += FFT_THREADS) {
            float a = 0.f, b = 0.f;
            if (n < Q) {
                const int64_t p = p0 + 2 * n;
                a = mono_sample<TX>(xs, g.sample_stride, g.channel_stride, stereo, p, g.n_samples);
                b = mono_sample<TX>(xs, g.sample_stride, g.channel_stride, stereo, p + 1, g.n_samples);
                ea += (double)a * (double)a;
                ea += (double)b * (double)b;
            }
            buf[n] = make_float2(a, b);
        }
        __syncthreads();
        z = lds_fft_radix2<false>(buf, buf + M, M, g.n_fft, tw, tid);
        if (STASH) asm volatile("" : "+v"(k0));
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = k0 + FFT_THREADS * i;
            if (PER > 1 || k < M) {
                float2 ak = real_fft_bin(z, k, M, tw);
                if (k == 0) ak.y = 0.f;
                const float2 v = STASH ? ystash[k] : yk[STASH ? 0 : i];
                // conj(A) Y: float32 x float32 is exact in float64, so each line rounds twice (the sum, the accumulation)
                cre[i] += (double)ak.x * (double)v.x + (double)ak.y * (double)v.y;
                cim[i] += (double)ak.x * (double)v.y - (double)ak.y * (double)v.x;
            }
        }
        if (tid == 0) nyq += (double)real_fft_bin(z, M, M, tw).x * (double)ynyq;
        __syncthreads();                                              // z is read: the next frame (or the wave sums) may land
    }
    double* rec = partial + ((int64_t)s * g.blocks_per_pair + blk) * record_doubles(g.n_fft);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = tid + FFT_THREADS * i;
        if (PER > 1 || k < M) {
            rec[k] = cre[i];
            rec[M + 1 + k] = cim[i];
        }
    }
    double* wsum = reinterpret_cast<double*>(buf);                    // 64 of the 16 M >= 512 bytes the block holds
    ea = wave_sum_f64(ea);
    ey = wave_sum_f64(ey);
    if ((tid & (WAVE - 1)) == 0) {
        wsum[tid / WAVE] = ea;
        wsum[4 + tid / WAVE] = ey;
    }
    __syncthreads();
    if (tid == 0) {
        rec[M] = nyq;
        rec[2 * M + 1] = 0.0;
        rec[2 * M + 2] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        rec[2 * M + 3] = ((wsum[4] + wsum[5]) + wsum[6]) + wsum[7];
    }
}
static_assert(FFT_THREADS == 4 * WAVE, "four wave sums per energy");

__global__ __launch_bounds__(FFT_THREADS) void align_reduce_kernel(const double* __restrict__ partial, int blocks_per_pair,
                                                                   int64_t rec, double* __restrict__ spec) {
    const int64_t e = (int64_t)blockIdx.x * FFT_THREADS + threadIdx.x;
    if (e >= rec) return;
    const double* p = partial + (int64_t)blockIdx.y * blocks_per_pair * rec + e;
    double s = p[0];
#pragma unroll 8                                                      // eight loads in flight; the additions stay in ascending order
    for (int i = 1; i < blocks_per_pair; ++i) s += p[(int64_t)i * rec];
    spec[(int64_t)blockIdx.y * rec + e] = s;
}

// bin k of the weighted spectrum, times `inv` (one over its largest magnitude), as the float32 the inverse transform takes
__device__ __forceinline__ float2 weighted_bin(const double* __restrict__ re, const double* __restrict__ im, int k, int M, bool phat,
                                               double floor_, double inv) {
    const double a = re[k], b = (k == 0 || k == M) ? 0.0 : im[k];
    const double w = phat ? inv / (sqrt(a * a + b * b) + floor_) : inv;
    return make_float2((float)(a * w), (float)(b * w));
}

// |v1| at lag l1 before |v2| at lag l2: the larger magnitude, then the smaller |lag|, then the negative lag
__device__ __forceinline__ bool peak_before(float v1, int l1, float v2, int l2) {
    if (v1 != v2) return v1 > v2;
    const int a1 = l1 < 0 ? -l1 : l1, a2 = l2 < 0 ? -l2 : l2;
    return a1 != a2 ? a1 < a2 : l1 < l2;
}

__global__ __launch_bounds__(FFT_THREADS) void align_finish_kernel(const double* __restrict__ spec, const float2* __restrict__ tw,
                                                                   int n_fft, int L, int phat, int* __restrict__ lag,
                                                                   double* __restrict__ frac, double* __restrict__ peak,
                                                                   int* __restrict__ sign, int* __restrict__ status,
                                                                   double* __restrict__ curve) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M], then AL_SCRATCH bytes
    const int tid = threadIdx.x, M = n_fft >> 1, Q = M >> 1, s = blockIdx.x;
    const double* re = spec + (int64_t)s * record_doubles(n_fft);
    const double* im = re + M + 1;
    const double ea = re[2 * M + 2], ey = re[2 * M + 3];
    double* sd = reinterpret_cast<double*>(buf + 2 * M);              // [0..3] wave sums, [4..7] wave maxima
    float* best_v = reinterpret_cast<float*>(sd + 8);                 // [256]
    int* best_l = reinterpret_cast<int*>(best_v + FFT_THREADS);       // [256]
    static_assert(8 * sizeof(double) + FFT_THREADS * (sizeof(float) + sizeof(int)) <= AL_SCRATCH, "finish scratch");
    // sum and maximum of |C[k]|, k = 0 .. M: lane l takes k = l, l + 256, ... ascending
    double sum = 0.0, mx = 0.0;
    for (int k = tid; k <= M; k += FFT_THREADS) {
        const double a = re[k], b = (k == 0 || k == M) ? 0.0 : im[k];
        const double m = sqrt(a * a + b * b);
        sum += m;
        mx = m > mx ? m : mx;
    }
    sum = wave_sum_f64(sum);
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const double o = __shfl_xor(mx, m);
        mx = o > mx ? o : mx;
    }
    if ((tid & (WAVE - 1)) == 0) {
        sd[tid / WAVE] = sum;
        sd[4 + tid / WAVE] = mx;
    }
    __syncthreads();
    const double total = ((sd[0] + sd[1]) + sd[2]) + sd[3];
    const double m01 = sd[4] > sd[5] ? sd[4] : sd[5], m23 = sd[6] > sd[7] ? sd[6] : sd[7];
    const double cmax = m01 > m23 ? m01 : m23;
    double* crow = curve ? curve + (int64_t)s * (2 * L + 1) : nullptr;
    if (!(ea > 0.0) || !(ey > 0.0) || !(cmax > 0.0)) {                // (workgroup-uniform) nothing to correlate
        if (crow)
            for (int i = tid; i <= 2 * L; i += FFT_THREADS) crow[i] = 0.0;
        if (tid == 0) {
            lag[s] = 0; frac[s] = 0.0; sign[s] = 0; status[s] = 0; peak[s] = al_nan();
        }
        return;
    }
    const double floor_ = DAM_ALIGN_PHAT_FLOOR * (total / (double)(M + 1));
    // the largest magnitude of the weighted spectrum: |C| / (|C| + floor) grows with |C|
    const double wmax = phat ? cmax / (cmax + floor_) : cmax;
    const double inv = 1.0 / wmax;
    // pre-twiddle: Z[k] = E[k] + i O[k], E = X[k] + conj(X[M-k]), O = (X[k] - conj(X[M-k])) conj(W^k); Z[M-k] = conj(E) + i conj(O)
    for (int k = tid; k <= Q; k += FFT_THREADS) {
        const float2 xk = weighted_bin(re, im, k, M, phat, floor_, inv), xn = weighted_bin(re, im, M - k, M, phat, floor_, inv);
        const float2 e = make_float2(xk.x + xn.x, xk.y - xn.y);
        const float2 d = make_float2(xk.x - xn.x, xk.y + xn.y);
        const float2 w = tw[k];
        const float2 o = cmul(d, make_float2(w.x, -w.y));
        buf[k] = make_float2(e.x - o.y, e.y + o.x);
        if (k) buf[M - k] = make_float2(e.x + o.y, o.x - e.y);
    }
    __syncthreads();
    // sample j of the N-point inverse is z[j] read as floats, times the halves of the split and irfft's 1/N: 0.5 / M
    const float* z = reinterpret_cast<const float*>(lds_fft_radix2<true>(buf, buf + M, M, n_fft, tw, tid));
    const double back = wmax * (0.5 / (double)M);
    float bv = -1.f;
    int bl = 0;
    for (int i = tid; i <= 2 * L; i += FFT_THREADS) {
        const int l = i - L;
        const float v = z[Q + l];
        if (crow) crow[i] = (double)v * back;
        if (peak_before(fabsf(v), l, bv, bl)) { bv = fabsf(v); bl = l; }
    }
    best_v[tid] = bv;
    best_l[tid] = bl;
    __syncthreads();
    if (tid != 0) return;                                             // not hot: one lane folds the 256 candidates
    for (int j = 1; j < FFT_THREADS; ++j)
        if (peak_before(best_v[j], best_l[j], bv, bl)) { bv = best_v[j]; bl = best_l[j]; }
    const double c1 = (double)z[Q + bl] * back, y1 = fabs(c1);
    double fr = 0.0;
    if (bl > -L && bl < L) {
        const double y0 = fabs((double)z[Q + bl - 1] * back), y2 = fabs((double)z[Q + bl + 1] * back);
        const double den = (y0 - 2.0 * y1) + y2;
        if (den < 0.0) fr = 0.5 * (y0 - y2) / den;
    }
    lag[s] = bl;
    frac[s] = fr;
    sign[s] = c1 > 0.0 ? 1 : -1;
    status[s] = 1;
    peak[s] = phat ? y1 : y1 / sqrt(ea * ey);
}

template <typename T>
__global__ __launch_bounds__(256) void align_shift_kernel(const T* __restrict__ x, int64_t n, int channels, int64_t ss, int64_t ps,
                                                          int64_t cs, const int* __restrict__ lag, T* __restrict__ out, int64_t oss,
                                                          int64_t ops, int64_t ocs) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int s = blockIdx.y;
    const int64_t q = p - (int64_t)lag[s];
    const bool in = q >= 0 && q < n;
    const T* src = x + s * ss + (in ? q : 0) * ps;
    T* dst = out + s * oss + p * ops;
    const T a = in ? src[0] : (T)0;
    if (channels == 2) {
        const T b = in ? src[cs] : (T)0;
        dst[ocs] = b;
    }
    dst[0] = a;
}

template <typename TX, typename TY, int PER>
int launch_cross(const void* x, const void* y, const float* twiddles, const AlGeo& g, int n_stems, double* partial, float2* stash,
                 hipStream_t s) {
    const size_t lds = (size_t)g.n_fft * sizeof(float2);              // two images of N/2 complex points
    // 8192 / 16384-point frames: beyond the default dynamic-LDS limit (the kernel has no static LDS beside it)
    if (lds > 48 * 1024 && !raise_lds_limit<&align_cross_spectrum_kernel<TX, TY, PER>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((align_cross_spectrum_kernel<TX, TY, PER>), dim3((unsigned)g.blocks_per_pair, (unsigned)n_stems),
                       dim3(FFT_THREADS), lds, s, (const TX*)x, (const TY*)y, reinterpret_cast<const float2*>(twiddles), g, partial,
                       stash);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

template <typename TX, typename TY>
int dispatch_cross(int per, const void* x, const void* y, const float* twiddles, const AlGeo& g, int n_stems, double* partial,
                   float2* stash, hipStream_t s) {
    switch (per) {
        case 1: return launch_cross<TX, TY, 1>(x, y, twiddles, g, n_stems, partial, stash, s);
        case 2: return launch_cross<TX, TY, 2>(x, y, twiddles, g, n_stems, partial, stash, s);
        case 4: return launch_cross<TX, TY, 4>(x, y, twiddles, g, n_stems, partial, stash, s);
        case 8: return launch_cross<TX, TY, 8>(x, y, twiddles, g, n_stems, partial, stash, s);
        case 16: return launch_cross<TX, TY, 16>(x, y, twiddles, g, n_stems, partial, stash, s);
        default: return launch_cross<TX, TY, 32>(x, y, twiddles, g, n_stems, partial, stash, s);
    }
}

}  // namespace
}  // namespace dam

extern "C" int dam_align_max_lag(void) { return dam::AL_MAX_LAG; }
extern "C" int dam_align_frames_per_block(void) { return dam::AL_F; }
extern "C" int dam_align_fft_size(int max_lag) { return dam::align_fft_size(max_lag); }

extern "C" int64_t dam_align_workspace_bytes(int n_stems, int64_t n_samples, int max_lag) {
    const int n_fft = dam::align_fft_size(max_lag);
    if (!n_fft || n_stems < 1 || n_stems > dam::AL_MAX_S || n_samples < 1) return 0;
    const int64_t blocks = dam::cdiv(dam::cdiv(n_samples, n_fft / 2), dam::AL_F);
    return (int64_t)n_stems * ((blocks + 1) * dam::record_doubles(n_fft) + blocks * dam::stash_doubles(n_fft)) * (int64_t)sizeof(double);
}

extern "C" int dam_align_estimate(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                                  int64_t sample_stride, int64_t channel_stride, const void* y, int y_is_f64,
                                  int64_t y_sample_stride, int64_t y_channel_stride, int max_lag, int weighting,
                                  const float* twiddles, int32_t* lag, double* frac, double* peak, int32_t* sign, int32_t* status,
                                  double* curve, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !y || !twiddles || !lag || !frac || !peak || !sign || !status || !workspace) return DAM_ERR_BAD_ARG;
    if (n_stems < 1 || n_stems > AL_MAX_S || (channels != 1 && channels != 2) || n_samples < 1) return DAM_ERR_BAD_ARG;
    if (weighting != DAM_ALIGN_PLAIN && weighting != DAM_ALIGN_PHAT) return DAM_ERR_BAD_ARG;
    const int n_fft = align_fft_size(max_lag);
    if (!n_fft) return DAM_ERR_BAD_ARG;
    const int64_t n_frames = cdiv(n_samples, n_fft / 2);
    if (n_frames > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    AlGeo g;
    g.n_samples = n_samples; g.stem_stride = stem_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.y_sample_stride = y_sample_stride; g.y_channel_stride = y_channel_stride;
    g.channels = channels; g.n_fft = n_fft; g.n_frames = (int)n_frames;
    g.blocks_per_pair = (int)cdiv(n_frames, AL_F);
    hipStream_t s = (hipStream_t)stream;
    const int64_t rec = record_doubles(n_fft);
    double* partial = static_cast<double*>(workspace);
    double* spec = partial + (int64_t)n_stems * g.blocks_per_pair * rec;
    float2* stash = reinterpret_cast<float2*>(spec + (int64_t)n_stems * rec);
    const int per = n_fft / 2 >= FFT_THREADS ? n_fft / 2 / FFT_THREADS : 1;
    int rc;
    if (x_is_f64)
        rc = y_is_f64 ? dispatch_cross<double, double>(per, x, y, twiddles, g, n_stems, partial, stash, s)
                      : dispatch_cross<double, float>(per, x, y, twiddles, g, n_stems, partial, stash, s);
    else
        rc = y_is_f64 ? dispatch_cross<float, double>(per, x, y, twiddles, g, n_stems, partial, stash, s)
                      : dispatch_cross<float, float>(per, x, y, twiddles, g, n_stems, partial, stash, s);
    if (rc != DAM_OK) return rc;
    hipLaunchKernelGGL(align_reduce_kernel, dim3((unsigned)cdiv(rec, FFT_THREADS), (unsigned)n_stems), dim3(FFT_THREADS), 0, s,
                       partial, g.blocks_per_pair, rec, spec);
    DAM_CHECK_LAUNCH();
    const size_t lds = (size_t)n_fft * sizeof(float2) + AL_SCRATCH;
    if (lds > 48 * 1024 && !raise_lds_limit<&align_finish_kernel>(136 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL(align_finish_kernel, dim3((unsigned)n_stems), dim3(FFT_THREADS), lds, s, spec,
                       reinterpret_cast<const float2*>(twiddles), n_fft, max_lag, weighting == DAM_ALIGN_PHAT ? 1 : 0, lag, frac,
                       peak, sign, status, curve);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_align_shift(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                               int64_t sample_stride, int64_t channel_stride, const int32_t* lag, void* out,
                               int64_t out_stem_stride, int64_t out_sample_stride, int64_t out_channel_stride, void* stream) {
    using namespace dam;
    if (!x || !lag || !out) return DAM_ERR_BAD_ARG;
    if (n_stems < 1 || n_stems > AL_MAX_S || (channels != 1 && channels != 2) || n_samples < 1) return DAM_ERR_BAD_ARG;
    const int64_t blocks = cdiv(n_samples, 256);
    if (blocks > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (x_is_f64)
        hipLaunchKernelGGL(align_shift_kernel<double>, dim3((unsigned)blocks, (unsigned)n_stems), dim3(256), 0, s, (const double*)x,
                           n_samples, channels, stem_stride, sample_stride, channel_stride, lag, (double*)out, out_stem_stride,
                           out_sample_stride, out_channel_stride);
    else
        hipLaunchKernelGGL(align_shift_kernel<float>, dim3((unsigned)blocks, (unsigned)n_stems), dim3(256), 0, s, (const float*)x,
                           n_samples, channels, stem_stride, sample_stride, channel_stride, lag, (float*)out, out_stem_stride,
                           out_sample_stride, out_channel_stride);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
