// dam_specgrad.hip -- the gradient of the spectrogram distance in the gains: d J_r / d g[r][s][j] of J_r = sum_t sum_k d_r[t][k]^2,
// the criterion of dam_specdist.hip with every bin at weight 1, for R candidate mixes "stems x gain ramps" of every clip against
// the clip's reference mix (include/dam_hip.h, "Spectrogram distance: gradient", states the definition).  The adjoint of a frame
// is one more transform of the same size in the same LDS plus S dot products with the samples the forward load has just pulled
// through the cache; neither a mix nor a spectrogram nor a signal gradient is written.
//   frames   one workgroup = frame t of one clip, all R rows: the reference frame is transformed once, every lane keeps the
//            reference levels of its own bins in registers; then per row: load (stems x row gains) -> LDS FFT -> levels, d ->
//            u = (40 / ln 10) d X / p packed for the inverse -> inverse LDS FFT -> times the window -> per stem the dot products
//            with the stem's channel means, split by gain segment -> one record per (row, frame)        grid = (frames, clips)
//   reduce   a gain node adds the records of the frames that touch it in ascending t from +0.0; (S1, S2) likewise over all
//            frames; one wave per output entry, the run of frames from the geometry            grid = (S n_gains + 1, rows, clips)
// T (1 + 2 R) transforms.  Not tuned beyond its structure.
#include "dam_common.h"
#include "dam_fft_lds.h"
#include "dam_specdist_frame.h"  // level_db, transform_frame: the forward half is the distance's, operation for operation
#include "dam_spectrum_load.h"   // SpecGeo, gain_index

#pragma clang fp contract(off)        // levels, differences, products and sums are stated operation by operation

namespace dam {
namespace {

constexpr int GRAD_WAVES = FFT_THREADS / WAVE;
constexpr int GRAD_PART_DOUBLES = 2 * GRAD_WAVES * 2;                 // [parity][wave][2]: the cross-wave partials, 128 bytes
constexpr double GRAD_SCALE = 40.0 / 2.302585092994045684;            // 40 / ln 10

struct GradGeo {
    int64_t x_clip_stride, ref_clip_stride;
    int n_rows;
    float amin2, floor_db;
};

// The two partial sums of every wave -> out[0], out[1] on thread 0: an xor-butterfly over the 64 lanes, distances 1 .. 32, then
// the four waves added as ((w0 + w1) + w2) + w3 through part[step & 1].  One barrier: two areas alternate, and the barrier of the
// next step lies between thread 0's reads of an area and the next writes to it.
__device__ __forceinline__ void block_sum2(double a, double b, double* part, int& step, int tid, double* out) {
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (int m = 1; m < WAVE; m <<= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    double* p = part + (step & 1) * (GRAD_WAVES * 2);
    if (lane == 0) {
        p[2 * wave] = a;
        p[2 * wave + 1] = b;
    }
    __syncthreads();
    if (tid == 0) {
        double s0 = p[0], s1 = p[1];
#pragma unroll
        for (int w = 1; w < GRAD_WAVES; ++w) {
            s0 += p[2 * w];
            s1 += p[2 * w + 1];
        }
        out[0] = s0;
        out[1] = s1;
    }
    ++step;
}

template <typename TC, typename TR, int PER>
__global__ __launch_bounds__(FFT_THREADS) void specgrad_frame_kernel(
    const TC* __restrict__ x, const double* __restrict__ gains, const TR* __restrict__ xref, const double* __restrict__ ref_gains,
    const float* __restrict__ window, const float2* __restrict__ tw /* W_nfft^k */, SpecGeo g, SpecGeo gref, GradGeo d,
    double* __restrict__ records) {
    extern __shared__ __attribute__((aligned(16))) float2 buf[];      // [2][M] points, then GRAD_PART_DOUBLES doubles
    const int tid = threadIdx.x, M = g.n_fft >> 1, t = blockIdx.x, S = g.n_stems;
    const int64_t clip = blockIdx.y;
    const int64_t p0 = (int64_t)t * g.hop - M;
    double* part = reinterpret_cast<double*>(buf + 2 * M);
    int step = 0;

    x += clip * d.x_clip_stride;
    xref += clip * d.ref_clip_stride;
    if (gains) gains += clip * d.n_rows * S * g.n_gains;
    if (ref_gains) ref_gains += clip * gref.n_stems * gref.n_gains;
    // the first of the (at most two) gain segments the frame touches: that of its first sample, clamped into the signal
    const int64_t start = p0 < 0 ? 0 : (p0 > g.n_samples - 1 ? g.n_samples - 1 : p0);
    const int64_t seg0 = g.n_gains > 1 ? gain_index(g, start) : 0;
    // gain_index(q) > seg0  <=>  q >= split (no division per sample); beyond every sample where there is no second segment
    const int64_t split = seg0 < g.n_gains - 1 ? (seg0 + 1) * g.gseg : 0x7fffffffffffffffll;

    float lref[PER], lref_nyq = 0.f;
    {
        const float2* z = transform_frame<TR>(buf, xref, ref_gains, gref, p0, window, tw, tid);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = tid + FFT_THREADS * i;
            lref[i] = 0.f;
            if (PER > 1 || k < M) {
                float2 xk = real_fft_bin(z, k, M, tw);
                if (k == 0) xk.y = 0.f;                               // DC of a real signal
                lref[i] = level_db(xk.x * xk.x + xk.y * xk.y, d.amin2, d.floor_db);
            }
        }
        if (tid == 0) {                                               // Nyquist, real as well
            const float2 xk = real_fft_bin(z, M, M, tw);
            lref_nyq = level_db(xk.x * xk.x, d.amin2, d.floor_db);
        }
    }
    __syncthreads();                                                  // z is read: the first candidate frame may land
    for (int r = 0; r < d.n_rows; ++r) {
        const double* gr = gains ? gains + (int64_t)r * S * g.n_gains : nullptr;
        double* rec = records + (((clip * d.n_rows + r) * g.n_frames + t) * (S + 1)) * 2;
        const float2* z = transform_frame<TC>(buf, x, gr, g, p0, window, tw, tid);
        // u_k of the lane's own bins, written as v_k (v_0 = 2 u_0 and v_M = 2 u_M share point 0) into the image z is NOT in
        float2* v = z == buf ? buf + M : buf;
        float2* pk = z == buf ? buf : buf + M;                        // the packed input of the inverse lands over z
        double s1 = 0.0, s2 = 0.0;
        float u0 = 0.f;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = tid + FFT_THREADS * i;
            if (PER > 1 || k < M) {
                float2 xk = real_fft_bin(z, k, M, tw);
                if (k == 0) xk.y = 0.f;
                const float p = xk.x * xk.x + xk.y * xk.y;
                const double df = (double)level_db(p, d.amin2, d.floor_db) - (double)lref[i];
                s1 += df;
                s2 += df * df;
                const float c = p <= d.amin2 ? 0.f : (float)(GRAD_SCALE * df / (double)p);      // a floored level has no derivative
                if (k == 0) u0 = c * xk.x;
                else v[k] = make_float2(c * xk.x, c * xk.y);
            }
        }
        if (tid == 0) {
            const float2 xk = real_fft_bin(z, M, M, tw);
            const float p = xk.x * xk.x;
            const double df = (double)level_db(p, d.amin2, d.floor_db) - (double)lref_nyq;
            s1 += df;
            s2 += df * df;
            const float c = p <= d.amin2 ? 0.f : (float)(GRAD_SCALE * df / (double)p);
            v[0] = make_float2(2.f * u0, 2.f * (c * xk.x));
        }
        __syncthreads();                                              // v is complete, z is read
        // pre-twiddle of the inverse real transform (dam_istft.hip): Z[k] = E + i O, E = V[k] + conj V[M-k],
        // O = (V[k] - conj V[M-k]) conj(W^k); Z[M-k] = conj(E) + i conj(O)
        for (int k = tid; k <= (M >> 1); k += FFT_THREADS) {
            float2 vk = v[k], vn = v[(M - k) & (M - 1)];
            if (k == 0) { vn = make_float2(vk.y, 0.f); vk.y = 0.f; }
            const float2 e = make_float2(vk.x + vn.x, vk.y - vn.y);
            const float2 dd = make_float2(vk.x - vn.x, vk.y + vn.y);
            const float2 w = tw[k];
            const float2 o = cmul(dd, make_float2(w.x, -w.y));
            pk[k] = make_float2(e.x - o.y, e.y + o.x);
            if (k) pk[M - k] = make_float2(e.x + o.y, o.x - e.y);
        }
        __syncthreads();
        float* zt = reinterpret_cast<float*>(lds_fft_radix2<true>(pk, v, M, g.n_fft, tw, tid));
        // z_t[i] = w[i] y[i], y = half the unnormalised inverse; a lane touches its own positions tid + 256 j only from here on
        for (int i = tid; i < g.n_fft; i += FFT_THREADS) zt[i] = window[i] * (0.5f * zt[i]);
        const bool stereo = g.channels == 2;
        for (int s = 0; s < S; ++s) {
            const TC* xs = x + (int64_t)s * g.stem_stride;
            double a0 = 0.0, a1 = 0.0;
            for (int i = tid; i < g.n_fft; i += FFT_THREADS) {
                const int64_t q = reflect(p0 + i, g.n_samples);
                const TC* ps = xs + q * g.sample_stride;
                const double m = stereo ? ((double)ps[0] + (double)ps[g.channel_stride]) * 0.5 : (double)ps[0];
                const double zm = (double)zt[i] * m;
                if (q >= split) a1 += zm;
                else a0 += zm;
            }
            block_sum2(a0, a1, part, step, tid, rec + 2 * s);
        }
        block_sum2(s1, s2, part, step, tid, rec + 2 * S);             // its barrier: zt is read, the next row's frame may land
    }
}

// First frame whose first sample (t hop - n_fft/2) lies in gain segment j or beyond; j = n_gains: the frame count.
__device__ __forceinline__ int segment_first_frame(int j, int n_gains, int64_t seg, int hop, int M, int n_frames) {
    if (j <= 0) return 0;
    if (j >= n_gains) return n_frames;
    const int64_t f = ((int64_t)j * seg + M + hop - 1) / hop;
    return f < n_frames ? (int)f : n_frames;
}

// Lane i's value on every lane; i is a constant once the loop around it is unrolled (v_readlane, no LDS round trip).
__device__ __forceinline__ double lane_value(double v, int i) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}

// The records [t][.] at stride `stride`, t = t0 .. t1-1, added in ascending t from +0.0: the wave loads 64 at a time, every
// lane then adds them in order (all lanes hold the sum).  Frames before tm give their second value, the others their first.
// PAIR: both values of a record, two sums.  A block of 64 is padded with +0.0, which no sum that began at +0.0 can tell.
template <bool PAIR>
__device__ __forceinline__ double2 walk(const double* __restrict__ p, int64_t stride, int t0, int tm, int t1, int lane) {
    double a = 0.0, b = 0.0;
    for (int base = t0; base < t1; base += WAVE) {
        const int t = base + lane;
        double va = 0.0, vb = 0.0;
        if (t < t1) {
            const double* q = p + (int64_t)t * stride;
            if (PAIR) { va = q[0]; vb = q[1]; }
            else va = q[t < tm ? 1 : 0];
        }
#pragma unroll
        for (int i = 0; i < WAVE; ++i) {
            a += lane_value(va, i);
            if (PAIR) b += lane_value(vb, i);
        }
    }
    return make_double2(a, b);
}

__global__ __launch_bounds__(WAVE) void specgrad_reduce_kernel(const double* __restrict__ records, int n_stems, int n_gains,
                                                              int n_frames, int64_t seg, int hop, int n_fft,
                                                              double* __restrict__ grad, double* __restrict__ value) {
    const int e = blockIdx.x, r = blockIdx.y, lane = threadIdx.x, M = n_fft >> 1;
    const int64_t row = (int64_t)blockIdx.z * gridDim.y + r, stride = (int64_t)(n_stems + 1) * 2;
    const double* p = records + row * n_frames * stride;
    if (e == n_stems * n_gains) {
        const double2 s = walk<true>(p + 2 * n_stems, stride, 0, 0, n_frames, lane);
        if (lane == 0) {
            value[2 * row] = s.x;
            value[2 * row + 1] = s.y;
        }
        return;
    }
    const int s = e / n_gains, j = e - s * n_gains;
    // node j: the frames that begin in segment j-1 and reach into j (their second value), then those that begin in j
    const int tm = segment_first_frame(j, n_gains, seg, hop, M, n_frames);
    const int t1 = segment_first_frame(j + 1, n_gains, seg, hop, M, n_frames);
    int t0 = 0;
    if (j > 0) {
        const int64_t f = ((int64_t)j * seg - M + 1 + hop - 1) / hop;  // first t with t hop - n_fft/2 + n_fft - 1 >= j seg
        t0 = f < tm ? (int)f : tm;
    }
    const double sum = walk<false>(p + 2 * s, stride, t0, tm, t1, lane).x;
    if (lane == 0) grad[(row * n_stems + s) * n_gains + j] = sum;
}

struct GradCall {
    const void *x, *xref;
    const double *gains, *ref_gains;
    const float *window, *twiddles;
    SpecGeo g, gref;
    GradGeo d;
    int n_clips;
    double* records;
    hipStream_t s;
};

template <typename TC, typename TR, int PER>
int launch_frames(const GradCall& c) {
    // two images of n_fft/2 complex points and the cross-wave partials behind them
    const size_t lds = (size_t)c.g.n_fft * sizeof(float2) + GRAD_PART_DOUBLES * sizeof(double);
    // 8192 / 16384-point windows: beyond the default dynamic-LDS limit (the kernel has no static LDS beside it)
    if (lds > 48 * 1024 && !raise_lds_limit<&specgrad_frame_kernel<TC, TR, PER>>(132 * 1024)) return DAM_ERR_LAUNCH;
    hipLaunchKernelGGL((specgrad_frame_kernel<TC, TR, PER>), dim3((unsigned)c.g.n_frames, (unsigned)c.n_clips), dim3(FFT_THREADS),
                       lds, c.s, (const TC*)c.x, c.gains, (const TR*)c.xref, c.ref_gains, c.window,
                       reinterpret_cast<const float2*>(c.twiddles), c.g, c.gref, c.d, c.records);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

template <typename TC, typename TR>
int dispatch_frames(int per, const GradCall& c) {
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
              int64_t channel_stride, const double* gains, int n_gains, int n_fft, int hop, int n_frames) {
    if (n_stems <= 0 || (channels != 1 && channels != 2)) return false;
    if (gains && (n_gains < 1 || n_gains > n)) return false;
    g.n_samples = n; g.stem_stride = stem_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.n_stems = n_stems; g.channels = channels; g.n_gains = gains ? n_gains : 1;
    g.gseg = n / g.n_gains;
    g.n_fft = n_fft; g.hop = hop; g.n_frames = n_frames; g.n_bands = 1; g.blocks_per_mix = n_frames;
    g.small = n < 0x7fffffff ? 1 : 0;
    return true;
}

// The geometry rules the entry and the workspace size share -> frames, or 0 where the entry refuses.
int64_t checked_frames(int n_clips, int n_rows, int64_t n, int n_fft, int hop) {
    if (n_clips < 1 || n_clips > 65535 || n_rows < 1 || n_rows > 65535 || n <= 0) return 0;
    if (n_fft < 64 || n_fft > 16384 || (n_fft & (n_fft - 1))) return 0;
    if (hop < 1 || n <= n_fft / 2) return 0;                          // reflect padding needs n > n_fft/2
    const int64_t n_frames = 1 + n / hop;
    if (n_frames > 0x7fffffff / 2) return 0;
    return n_frames;
}

// A frame may touch two gain segments at most.
bool segments_supported(int64_t n, int n_gains, int n_fft) { return n_gains <= 1 || n / n_gains >= n_fft; }

}  // namespace
}  // namespace dam

extern "C" int64_t dam_specgrad_workspace_bytes(int n_clips, int n_rows, int n_stems, int64_t n_samples, int n_fft, int hop,
                                                int n_gains) {
    const int64_t n_frames = dam::checked_frames(n_clips, n_rows, n_samples, n_fft, hop);
    if (n_frames <= 0 || n_stems < 1 || n_gains < 0 || n_gains > n_samples || !dam::segments_supported(n_samples, n_gains, n_fft))
        return 0;
    return (int64_t)n_clips * n_rows * n_frames * (n_stems + 1) * 2 * (int64_t)sizeof(double);
}

extern "C" int dam_specgrad(const void* x, int x_is_f64, int n_clips, int n_rows, int n_stems, int channels, int64_t n_samples,
                            int64_t x_clip_stride, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride,
                            const double* gains, int n_gains, const void* ref, int ref_is_f64, int ref_stems, int ref_channels,
                            int64_t ref_clip_stride, int64_t ref_stem_stride, int64_t ref_sample_stride,
                            int64_t ref_channel_stride, const double* ref_gains, int ref_n_gains, const float* window,
                            const float* twiddles, int n_fft, int hop, float amin, double* value, double* grad, void* workspace,
                            void* stream) {
    using namespace dam;
    if (!x || !ref || !window || !twiddles || !value || !grad || !workspace) return DAM_ERR_BAD_ARG;
    if (!(amin > 0.f)) return DAM_ERR_BAD_ARG;
    const int64_t n_frames = checked_frames(n_clips, n_rows, n_samples, n_fft, hop);
    if (n_frames <= 0) return DAM_ERR_BAD_ARG;
    GradCall c;
    if (!fill_geo(c.g, n_stems, channels, n_samples, stem_stride, sample_stride, channel_stride, gains, n_gains, n_fft, hop,
                  (int)n_frames))
        return DAM_ERR_BAD_ARG;
    if (!fill_geo(c.gref, ref_stems, ref_channels, n_samples, ref_stem_stride, ref_sample_stride, ref_channel_stride, ref_gains,
                  ref_n_gains, n_fft, hop, (int)n_frames))
        return DAM_ERR_BAD_ARG;
    if (!segments_supported(n_samples, c.g.n_gains, n_fft)) return DAM_ERR_UNSUPPORTED;
    if ((int64_t)n_stems * c.g.n_gains + 1 > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    c.x = x; c.xref = ref; c.gains = gains; c.ref_gains = ref_gains; c.window = window; c.twiddles = twiddles;
    c.d.x_clip_stride = x_clip_stride; c.d.ref_clip_stride = ref_clip_stride;
    c.d.n_rows = n_rows;
    c.d.amin2 = amin * amin;
    c.d.floor_db = (float)(20.0 * log10((double)amin));
    c.n_clips = n_clips;
    c.records = static_cast<double*>(workspace);
    c.s = (hipStream_t)stream;
    const int per = n_fft / 2 >= FFT_THREADS ? n_fft / 2 / FFT_THREADS : 1;
    const int rc = x_is_f64 ? (ref_is_f64 ? dispatch_frames<double, double>(per, c) : dispatch_frames<double, float>(per, c))
                            : (ref_is_f64 ? dispatch_frames<float, double>(per, c) : dispatch_frames<float, float>(per, c));
    if (rc != DAM_OK) return rc;
    hipLaunchKernelGGL(specgrad_reduce_kernel, dim3((unsigned)(n_stems * c.g.n_gains + 1), (unsigned)n_rows, (unsigned)n_clips),
                       dim3(WAVE), 0, c.s, c.records, n_stems, c.g.n_gains, (int)n_frames, c.g.gseg, hop, n_fft, grad, value);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
