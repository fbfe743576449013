// dam_loudness.hip -- ITU-R BS.1770 K-weighting + 400 ms block energies.
//
// Replaces what the reference gets from pyloudnorm (third-party, not vendored; `pyln.Meter(sr).integrated_loudness`):
// data/dataset.py:115-130 (compute_mean_loudness), evaluation.py:39-46,59-66 (per-stem and mix loudness),
// models/baselines/mean_loudness_model.py:10-20.  The device part is everything that touches samples: the two-biquad
// K-weighting filter (scipy.signal.lfilter, transposed direct form II, float64) and the mean square of every gating
// block.  The gating itself (two thresholds over a few thousand block energies) stays on the host (loudness.py).
//
// An IIR filter is a linear recurrence; it is made parallel exactly, not by warm-up: the signal is cut into chunks,
//   pass 1  every chunk is filtered from a zero state            -> its zero-state end state            (parallel)
//   scan    s_in[c+1] = T s_in[c] + s_end0[c], T = (4x4 state transition)^L obtained by running the zero-input filter
//           from the four unit states                           -> the true state entering every chunk (two-level scan,
//           one workgroup per channel)
//   pass 2  every chunk is filtered again from its true entry state; y^2 is stored                       (parallel)
//   blocks  z[ch][j] = sum y^2 over [lo_j, hi_j) / (hi_j - lo_j nominal length)                          (parallel)
// float64 throughout (the reference filters float64 arrays); HBM-bound.
#include "dam_common.h"

namespace dam {
namespace {

struct KwCoef { double b[2][3], a[2][2]; };      // stage 0 = high shelf, stage 1 = high pass; a0 == 1

// one sample through both stages (transposed direct form II, the same recurrence as scipy's lfilter)
__device__ __forceinline__ double kw_step(const KwCoef& k, double x, double (&s)[4]) {
    const double y0 = k.b[0][0] * x + s[0];
    s[0] = k.b[0][1] * x - k.a[0][0] * y0 + s[1];
    s[1] = k.b[0][2] * x - k.a[0][1] * y0;
    const double y1 = k.b[1][0] * y0 + s[2];
    s[2] = k.b[1][1] * y0 - k.a[1][0] * y1 + s[3];
    s[3] = k.b[1][2] * y0 - k.a[1][1] * y1;
    return y1;
}

template <typename T>
__device__ __forceinline__ double kw_load(const T* x, int64_t n, int64_t sample_stride) { return (double)x[n * sample_stride]; }

// pass 1 (PASS == 1): end state of chunk c filtered from zero;  pass 2: y^2 from the true entry state
template <typename T, int PASS>
__global__ __launch_bounds__(64) void kw_chunk_kernel(const T* __restrict__ x, int64_t n_samples, int64_t sample_stride,
                                                      int64_t channel_stride, KwCoef k, int L, int64_t n_chunks,
                                                      double* __restrict__ state /* [ch][n_chunks][4] */,
                                                      double* __restrict__ ysq /* [ch][n_samples] */) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int ch = blockIdx.y;
    if (c >= n_chunks) return;
    const T* xc = x + ch * channel_stride;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double* st = state + ((int64_t)ch * n_chunks + c) * 4;
    if (PASS == 2) { s[0] = st[0]; s[1] = st[1]; s[2] = st[2]; s[3] = st[3]; }
    const int64_t lo = c * L, hi = lo + L < n_samples ? lo + L : n_samples;
    for (int64_t n = lo; n < hi; ++n) {
        const double y = kw_step(k, kw_load(xc, n, sample_stride), s);
        if (PASS == 2) ysq[(int64_t)ch * n_samples + n] = y * y;
    }
    if (PASS == 1) { st[0] = s[0]; st[1] = s[1]; st[2] = s[2]; st[3] = s[3]; }
}

// state[c] := true entry state of chunk c (in place: on input state[c] is the zero-state END state of chunk c).
// One workgroup per channel, two levels: thread t owns K consecutive chunks; it first propagates a zero entry state
// through them, thread 0 chains the 256 results with T^K, then every thread replays its chunks from its true entry state.
__global__ __launch_bounds__(256) void kw_scan_kernel(KwCoef k, int L, int64_t n_chunks, double* __restrict__ state) {
    __shared__ double Tm[4][4];          // Tm[r][q]: component r of the state after L zero-input samples from unit state q
    __shared__ double TK[4][4];          // the same after K chunks
    __shared__ double seg[256][4];       // per thread: end state of its K chunks from a zero entry, then its true entry state
    const int ch = blockIdx.x, t = threadIdx.x;
    const int64_t K = (n_chunks + 255) / 256;
    if (t < 4) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[t] = 1.0;
        for (int n = 0; n < L; ++n) kw_step(k, 0.0, s);
        for (int r = 0; r < 4; ++r) Tm[r][t] = s[r];
    }
    __syncthreads();
    if (t < 4) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        v[t] = 1.0;
        for (int64_t i = 0; i < K; ++i) {
            double w[4];
            for (int r = 0; r < 4; ++r) w[r] = Tm[r][0] * v[0] + Tm[r][1] * v[1] + Tm[r][2] * v[2] + Tm[r][3] * v[3];
            for (int r = 0; r < 4; ++r) v[r] = w[r];
        }
        for (int r = 0; r < 4; ++r) TK[r][t] = v[r];
    }
    double* st = state + (int64_t)ch * n_chunks * 4;
    const int64_t c0 = t * K, c1 = c0 + K < n_chunks ? c0 + K : n_chunks;
    double cur[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t c = c0; c < c1; ++c) {
        double nxt[4];
        for (int r = 0; r < 4; ++r)
            nxt[r] = st[c * 4 + r] + (Tm[r][0] * cur[0] + Tm[r][1] * cur[1] + Tm[r][2] * cur[2] + Tm[r][3] * cur[3]);
        for (int r = 0; r < 4; ++r) cur[r] = nxt[r];
    }
    // threads whose range is short or empty: pad with zero-input chunks so that every segment spans exactly K chunks
    for (int64_t c = (c1 > c0 ? c1 : c0); c < c0 + K; ++c) {
        double nxt[4];
        for (int r = 0; r < 4; ++r) nxt[r] = Tm[r][0] * cur[0] + Tm[r][1] * cur[1] + Tm[r][2] * cur[2] + Tm[r][3] * cur[3];
        for (int r = 0; r < 4; ++r) cur[r] = nxt[r];
    }
    for (int r = 0; r < 4; ++r) seg[t][r] = cur[r];
    __syncthreads();
    if (t == 0) {
        double e[4] = {0.0, 0.0, 0.0, 0.0};          // entry state of segment 0
        for (int i = 0; i < 256; ++i) {
            double nxt[4];
            for (int r = 0; r < 4; ++r)
                nxt[r] = seg[i][r] + (TK[r][0] * e[0] + TK[r][1] * e[1] + TK[r][2] * e[2] + TK[r][3] * e[3]);
            for (int r = 0; r < 4; ++r) { seg[i][r] = e[r]; e[r] = nxt[r]; }
        }
    }
    __syncthreads();
    for (int r = 0; r < 4; ++r) cur[r] = seg[t][r];
    for (int64_t c = c0; c < c1; ++c) {
        double end0[4], nxt[4];
        for (int r = 0; r < 4; ++r) end0[r] = st[c * 4 + r];
        for (int r = 0; r < 4; ++r) nxt[r] = end0[r] + (Tm[r][0] * cur[0] + Tm[r][1] * cur[1] + Tm[r][2] * cur[2] + Tm[r][3] * cur[3]);
        for (int r = 0; r < 4; ++r) { st[c * 4 + r] = cur[r]; cur[r] = nxt[r]; }
    }
}

// z[ch][j] = sum_{n in [lo_j, hi_j)} ysq[ch][n] * inv_len      (hi_j may exceed n_samples: clipped, like a numpy slice)
__global__ __launch_bounds__(256) void kw_block_energy_kernel(const double* __restrict__ ysq, int64_t n_samples,
                                                              const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                              int n_blocks, double inv_len, double* __restrict__ z) {
    __shared__ double red[256];
    const int j = blockIdx.x, ch = blockIdx.y;
    const int64_t a = lo[j], b = hi[j] < n_samples ? hi[j] : n_samples;
    const double* y = ysq + (int64_t)ch * n_samples;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t n = a + threadIdx.x;
    for (; n + 768 < b; n += 1024) { s0 += y[n]; s1 += y[n + 256]; s2 += y[n + 512]; s3 += y[n + 768]; }
    for (; n < b; n += 256) s0 += y[n];
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) z[(int64_t)ch * n_blocks + j] = red[0] * inv_len;
}

constexpr int KW_CHUNK = 1024;

}  // namespace
}  // namespace dam

// RBJ biquads exactly as pyloudnorm 0.1.x builds its "K-weighting" (iirfilter.py): high shelf G = 4 dB, Q = 1/sqrt(2),
// fc = 1500 Hz; high pass Q = 0.5, fc = 38 Hz; both normalised by a0.  coef12 = {b0,b1,b2,a0(=1),a1,a2} x 2 stages.
extern "C" int dam_loudness_kweight_coeffs(double rate, double* coef12) {
    if (!coef12 || !(rate > 0.0)) return DAM_ERR_BAD_ARG;
    const double pi = 3.14159265358979323846;
    {
        const double G = 4.0, Q = 1.0 / sqrt(2.0), fc = 1500.0;
        const double A = pow(10.0, G / 40.0), w0 = 2.0 * pi * (fc / rate), alpha = sin(w0) / (2.0 * Q);
        const double b0 = A * ((A + 1) + (A - 1) * cos(w0) + 2 * sqrt(A) * alpha);
        const double b1 = -2 * A * ((A - 1) + (A + 1) * cos(w0));
        const double b2 = A * ((A + 1) + (A - 1) * cos(w0) - 2 * sqrt(A) * alpha);
        const double a0 = (A + 1) - (A - 1) * cos(w0) + 2 * sqrt(A) * alpha;
        const double a1 = 2 * ((A - 1) - (A + 1) * cos(w0));
        const double a2 = (A + 1) - (A - 1) * cos(w0) - 2 * sqrt(A) * alpha;
        coef12[0] = b0 / a0; coef12[1] = b1 / a0; coef12[2] = b2 / a0; coef12[3] = 1.0; coef12[4] = a1 / a0; coef12[5] = a2 / a0;
    }
    {
        const double Q = 0.5, fc = 38.0;
        const double w0 = 2.0 * pi * (fc / rate), alpha = sin(w0) / (2.0 * Q);
        const double b0 = (1 + cos(w0)) / 2, b1 = -(1 + cos(w0)), b2 = (1 + cos(w0)) / 2;
        const double a0 = 1 + alpha, a1 = -2 * cos(w0), a2 = 1 - alpha;
        coef12[6] = b0 / a0; coef12[7] = b1 / a0; coef12[8] = b2 / a0; coef12[9] = 1.0; coef12[10] = a1 / a0; coef12[11] = a2 / a0;
    }
    return DAM_OK;
}

extern "C" int64_t dam_loudness_workspace_bytes(int64_t n_samples, int channels) {
    if (n_samples <= 0 || channels <= 0) return 0;
    const int64_t n_chunks = dam::cdiv(n_samples, dam::KW_CHUNK);
    return (int64_t)channels * (n_chunks * 4 + n_samples) * (int64_t)sizeof(double);
}

extern "C" int dam_loudness_block_energy(const void* x, int x_is_f64, int64_t n_samples, int channels, int64_t sample_stride,
                                         int64_t channel_stride, const double* coef12_host, const int64_t* blk_lo,
                                         const int64_t* blk_hi, int n_blocks, double block_len, double* z, void* workspace,
                                         void* stream) {
    using namespace dam;
    if (!x || !coef12_host || !blk_lo || !blk_hi || !z || !workspace) return DAM_ERR_BAD_ARG;
    if (n_samples <= 0 || channels <= 0 || channels > 65535 || n_blocks <= 0 || !(block_len > 0.0)) return DAM_ERR_BAD_ARG;
    KwCoef k;
    for (int s = 0; s < 2; ++s) {
        if (coef12_host[s * 6 + 3] != 1.0) return DAM_ERR_BAD_ARG;        // normalised sections only
        for (int i = 0; i < 3; ++i) k.b[s][i] = coef12_host[s * 6 + i];
        k.a[s][0] = coef12_host[s * 6 + 4]; k.a[s][1] = coef12_host[s * 6 + 5];
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_chunks = cdiv(n_samples, KW_CHUNK);
    double* state = reinterpret_cast<double*>(workspace);
    double* ysq = state + (int64_t)channels * n_chunks * 4;
    const dim3 grid((unsigned)cdiv(n_chunks, 64), (unsigned)channels);
    if (x_is_f64) {
        hipLaunchKernelGGL((kw_chunk_kernel<double, 1>), grid, dim3(64), 0, st, reinterpret_cast<const double*>(x), n_samples,
                           sample_stride, channel_stride, k, KW_CHUNK, n_chunks, state, ysq);
    } else {
        hipLaunchKernelGGL((kw_chunk_kernel<float, 1>), grid, dim3(64), 0, st, reinterpret_cast<const float*>(x), n_samples,
                           sample_stride, channel_stride, k, KW_CHUNK, n_chunks, state, ysq);
    }
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(kw_scan_kernel, dim3(channels), dim3(256), 0, st, k, KW_CHUNK, n_chunks, state);
    DAM_CHECK_LAUNCH();
    if (x_is_f64) {
        hipLaunchKernelGGL((kw_chunk_kernel<double, 2>), grid, dim3(64), 0, st, reinterpret_cast<const double*>(x), n_samples,
                           sample_stride, channel_stride, k, KW_CHUNK, n_chunks, state, ysq);
    } else {
        hipLaunchKernelGGL((kw_chunk_kernel<float, 2>), grid, dim3(64), 0, st, reinterpret_cast<const float*>(x), n_samples,
                           sample_stride, channel_stride, k, KW_CHUNK, n_chunks, state, ysq);
    }
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(kw_block_energy_kernel, dim3(n_blocks, channels), dim3(256), 0, st, ysq, n_samples, blk_lo, blk_hi,
                       n_blocks, 1.0 / block_len, z);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// =====================================================================================================================
// Batched form: every (track, channel) row of a batch in one set of launches, block energies without the y^2 image, the
// gating and the loudness-normalisation gain on the device.  Nothing below synchronises with the host.
//
//   bounds  the 2 n_blocks block bounds lo_j / hi_j merged into one sorted list bnd[] (stable: a lo before an equal hi); the
//           samples between two consecutive bounds form a SEGMENT, and block j is the segments pos_lo[j]+1 .. pos_hi[j]
//   pass 1  as above, one wave per 64 consecutive chunks of a row; the wave stages 64 samples of each of its chunks through
//           LDS (one coalesced row of 64 consecutive samples per load instruction; the loads of the next tile are in
//           flight while the lanes filter the current one).  The optional gain ramp is applied as the sample leaves LDS:
//           (double)x * gains[track][min(n / (n_samples / n_gains), n_gains-1)], the product dam_gain_ramp_apply stores.
//   scan    kw_scan_kernel, one workgroup per row
//   pass 2  the same walk from the true entry state; the lane sums y^2 per (segment, chunk) PIECE and stores piece
//           (segment k, chunk c) at piece[row][k + c] -- k and c both grow with the sample index, so k + c is distinct for
//           every non-empty piece -- 8 bytes per piece instead of 8 bytes per sample
//   blocks  z[row][j] = (sum of the pieces of block j, ascending sample order, one thread) / block_len
// No atomics; a row's launch geometry depends on n_samples alone, so its result does not depend on the rest of the batch.
namespace dam {
namespace {

constexpr int KW_TILE = 64;                       // samples of every chunk staged per step
constexpr int KW_ROWS = 64;                       // chunks per wave (one per lane)
constexpr int64_t KW_NEVER = INT64_MAX;

struct KwBatchGeo {
    int64_t n_samples, n_chunks;
    int64_t track_stride, sample_stride, channel_stride;      // elements
    int channels, n_gains;
    int n_bounds;                                             // 2 * n_blocks
    int64_t piece_stride;                                     // n_bounds + n_chunks + 1
};

// bnd[pos] of every lo_j / hi_j in the stable merge of the two nondecreasing sequences.  pos < 2 n_blocks for any input.
__global__ __launch_bounds__(256) void kw_bounds_merge_kernel(const int64_t* __restrict__ lo, const int64_t* __restrict__ hi,
                                                              int n_blocks, int64_t* __restrict__ bnd,
                                                              int* __restrict__ pos_lo, int* __restrict__ pos_hi) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_blocks) return;
    const int64_t l = lo[j], h = hi[j];
    int a = 0, b = n_blocks;                      // number of hi values <  lo_j
    while (a < b) { const int m = (a + b) >> 1; if (hi[m] < l) a = m + 1; else b = m; }
    const int pl = j + a;
    a = 0; b = n_blocks;                          // number of lo values <= hi_j
    while (a < b) { const int m = (a + b) >> 1; if (lo[m] <= h) a = m + 1; else b = m; }
    const int ph = j + a;
    bnd[pl] = l; bnd[ph] = h;
    pos_lo[j] = pl; pos_hi[j] = ph;
}

template <typename T, int PASS>
__global__ __launch_bounds__(64) void kw_batch_chunk_kernel(const T* __restrict__ x, KwBatchGeo g, KwCoef k,
                                                            const double* __restrict__ gains /* [tracks][n_gains] or null */,
                                                            const int64_t* __restrict__ bnd,
                                                            double* __restrict__ state /* [row][n_chunks][4] */,
                                                            double* __restrict__ piece /* [row][piece_stride] */) {
    __shared__ T tile[KW_ROWS][KW_TILE + 1];      // +1: lane c walks row c, consecutive rows fall on consecutive banks
    const int lane = threadIdx.x;
    const int row = blockIdx.y, track = row / g.channels, ch = row - track * g.channels;
    const int64_t c0 = (int64_t)blockIdx.x * KW_ROWS, c = c0 + lane;
    const T* xr = x + track * g.track_stride + ch * g.channel_stride;
    const bool live = c < g.n_chunks;
    const int64_t lo = c * KW_CHUNK, hi = live ? (lo + KW_CHUNK < g.n_samples ? lo + KW_CHUNK : g.n_samples) : lo;

    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double* st = state + ((int64_t)row * g.n_chunks + c) * 4;
    if (PASS == 2 && live) { s[0] = st[0]; s[1] = st[1]; s[2] = st[2]; s[3] = st[3]; }

    // gain ramp: gain index of sample n is min(n / gseg, n_gains - 1); followed incrementally, one division per crossing
    const int64_t gseg = gains ? g.n_samples / g.n_gains : 1;
    const double* gr = gains ? gains + (int64_t)track * g.n_gains : nullptr;
    double gain = 1.0;
    int64_t gnext = gains ? lo : KW_NEVER;        // first sample refreshes it

    // pass 2: current segment kseg = #{bounds <= n}, the next bound, and the running sum of the piece
    int kseg = 0;
    int64_t bnext = KW_NEVER;
    double acc = 0.0;
    double* pr = piece + (int64_t)row * g.piece_stride + c;
    if (PASS == 2 && live) {
        int a = 0, b = g.n_bounds;
        while (a < b) { const int m = (a + b) >> 1; if (bnd[m] <= lo) a = m + 1; else b = m; }
        kseg = a;
        bnext = kseg < g.n_bounds ? bnd[kseg] : KW_NEVER;
    }

    // sample (c0 + r) * KW_CHUNK + t * KW_TILE + lane of the row, 0 outside the signal (a chunk past the last one starts
    // at or after n_samples, so the one comparison covers both)
    T next[KW_ROWS];
    const int64_t rstep = (int64_t)KW_CHUNK * g.sample_stride;
    auto fetch = [&](int t) {
        const int64_t n0 = c0 * KW_CHUNK + t * KW_TILE + lane;
        const T* p = xr + n0 * g.sample_stride;
#pragma unroll
        for (int r = 0; r < KW_ROWS; ++r)
            next[r] = n0 + (int64_t)r * KW_CHUNK < g.n_samples ? p[r * rstep] : (T)0;
    };
    fetch(0);
    for (int t = 0; t < KW_CHUNK / KW_TILE; ++t) {
        __syncthreads();                           // the previous tile has been consumed
#pragma unroll
        for (int r = 0; r < KW_ROWS; ++r) tile[r][lane] = next[r];
        __syncthreads();
        if (t + 1 < KW_CHUNK / KW_TILE) fetch(t + 1);
        const int64_t base = lo + (int64_t)t * KW_TILE;
        const int cnt = hi - base >= KW_TILE ? KW_TILE : (hi > base ? (int)(hi - base) : 0);
        for (int i = 0; i < cnt; ++i) {
            const int64_t n = base + i;
            if (n >= gnext) {
                int64_t gi = n / gseg;
                if (gi >= g.n_gains - 1) { gi = g.n_gains - 1; gnext = KW_NEVER; } else gnext = (gi + 1) * gseg;
                gain = gr[gi];
            }
            const double y = kw_step(k, (double)tile[lane][i] * gain, s);
            if (PASS == 2) {
                if (n >= bnext) {                  // sample n opens a later segment: the open piece is complete
                    pr[kseg] = acc;
                    acc = 0.0;
                    do { ++kseg; bnext = kseg < g.n_bounds ? bnd[kseg] : KW_NEVER; } while (bnext <= n);
                }
                acc += y * y;
            }
        }
    }
    if (live) {
        if (PASS == 1) { st[0] = s[0]; st[1] = s[1]; st[2] = s[2]; st[3] = s[3]; }
        else pr[kseg] = acc;                      // (hi > lo for every live chunk: the open piece holds a sample)
    }
}

// z[row][j]: the pieces of block j in ascending sample order.  Segment k holds the samples [bnd[k-1], bnd[k]).
__global__ __launch_bounds__(256) void kw_batch_block_sum_kernel(const double* __restrict__ piece, KwBatchGeo g,
                                                                 const int64_t* __restrict__ bnd, const int* __restrict__ pos_lo,
                                                                 const int* __restrict__ pos_hi, int n_blocks, double inv_len,
                                                                 double* __restrict__ z) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, row = blockIdx.y;
    if (j >= n_blocks) return;
    const double* pr = piece + (int64_t)row * g.piece_stride;
    double sum = 0.0;
    for (int kk = pos_lo[j] + 1; kk <= pos_hi[j]; ++kk) {
        int64_t a = bnd[kk - 1], b = bnd[kk] < g.n_samples ? bnd[kk] : g.n_samples;
        if (a < 0) a = 0;
        if (a >= b) continue;
        for (int64_t c = a / KW_CHUNK; c <= (b - 1) / KW_CHUNK; ++c) sum += pr[kk + c];
    }
    z[(int64_t)row * n_blocks + j] = sum * inv_len;
}

// Two-stage gating of one track per workgroup, loudness.gated_loudness: l_j = -0.691 + 10 log10(sum_i G_i z[i][j]);
// stage 1 keeps l_j >= -70, Gamma_r = loudness of the stage-1 channel means - 10; stage 2 keeps l_j > Gamma_r and l_j > -70;
// an empty stage-1 set makes Gamma_r NaN (0/0) and so stage 2 empty, an empty stage-2 set gives log10(0) = -inf.
// Fixed-order sums: thread t takes blocks t, t + 256, ..., then a tree over the 256 partials.
__device__ __forceinline__ double kw_block_loudness(const double* __restrict__ z, int channels, int n_blocks, int j) {
    const double G[5] = {1.0, 1.0, 1.0, 1.41, 1.41};
    double w = 0.0;
    for (int i = 0; i < channels; ++i) w += G[i] * z[(int64_t)i * n_blocks + j];
    return -0.691 + 10.0 * log10(w);
}

__global__ __launch_bounds__(256) void kw_gate_kernel(const double* __restrict__ z_all, int channels, int n_blocks,
                                                      double* __restrict__ lufs) {
    __shared__ double red[6][256];                 // five channel sums and the count
    __shared__ double gamma_r;
    const double G[5] = {1.0, 1.0, 1.0, 1.41, 1.41};
    const int t = threadIdx.x;
    const double* z = z_all + (int64_t)blockIdx.x * channels * n_blocks;
    for (int stage = 0; stage < 2; ++stage) {
        double sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
        const double gr = stage ? gamma_r : 0.0;
        for (int j = t; j < n_blocks; j += 256) {
            const double l = kw_block_loudness(z, channels, n_blocks, j);
            const bool keep = stage ? (l > gr && l > -70.0) : (l >= -70.0);
            if (keep) {
                for (int i = 0; i < channels; ++i) sum[i] += z[(int64_t)i * n_blocks + j];
                cnt += 1.0;
            }
        }
        for (int i = 0; i < 5; ++i) red[i][t] = sum[i];
        red[5][t] = cnt;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w) for (int i = 0; i < 6; ++i) red[i][t] += red[i][t + w];
            __syncthreads();
        }
        if (t == 0) {
            double w = 0.0;
            for (int i = 0; i < channels; ++i) {
                double m = red[i][0] / red[5][0];                       // mean of an empty set: 0/0 = NaN
                if (stage && m != m) m = 0.0;                           // np.nan_to_num
                w += G[i] * m;
            }
            const double l = -0.691 + 10.0 * log10(w);
            if (stage) lufs[blockIdx.x] = l; else gamma_r = l - 10.0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void kw_target_gains_kernel(const double* __restrict__ lufs, const double* __restrict__ target,
                                                              int n, double* __restrict__ gains) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gains[i] = pow(10.0, (target[i] - lufs[i]) / 20.0);
}

struct KwBatchWs { double* state; double* piece; int64_t* bnd; int* pos_lo; int* pos_hi; int64_t bytes; };
static KwBatchWs kw_batch_ws(void* base, int64_t rows, int64_t n_chunks, int n_blocks) {
    KwBatchWs w;
    const int64_t piece_stride = 2 * (int64_t)n_blocks + n_chunks + 1;
    w.state = reinterpret_cast<double*>(base);
    w.piece = w.state + rows * n_chunks * 4;
    w.bnd = reinterpret_cast<int64_t*>(w.piece + rows * piece_stride);
    w.pos_lo = reinterpret_cast<int*>(w.bnd + 2 * (int64_t)n_blocks);
    w.pos_hi = w.pos_lo + n_blocks;
    w.bytes = (rows * n_chunks * 4 + rows * piece_stride + 2 * (int64_t)n_blocks) * 8 + 2 * (int64_t)n_blocks * 4;
    return w;
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_loudness_batch_workspace_bytes(int n_tracks, int64_t n_samples, int channels, int n_blocks) {
    if (n_tracks <= 0 || n_samples <= 0 || channels <= 0 || n_blocks <= 0) return 0;
    return dam::kw_batch_ws(nullptr, (int64_t)n_tracks * channels, dam::cdiv(n_samples, dam::KW_CHUNK), n_blocks).bytes;
}

extern "C" int dam_loudness_block_energy_batch(const void* x, int x_is_f64, int n_tracks, int64_t n_samples, int channels,
                                               int64_t track_stride, int64_t sample_stride, int64_t channel_stride,
                                               const double* gains, int n_gains, const double* coef12_host,
                                               const int64_t* blk_lo, const int64_t* blk_hi, int n_blocks, double block_len,
                                               double* z, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !coef12_host || !blk_lo || !blk_hi || !z || !workspace) return DAM_ERR_BAD_ARG;
    if (n_tracks <= 0 || n_samples <= 0 || channels <= 0 || n_blocks <= 0 || !(block_len > 0.0)) return DAM_ERR_BAD_ARG;
    if (gains && (n_gains <= 0 || n_gains > n_samples)) return DAM_ERR_BAD_ARG;
    const int64_t rows = (int64_t)n_tracks * channels;
    if (rows > 65535 || n_blocks > (1 << 29)) return DAM_ERR_UNSUPPORTED;
    KwCoef k;
    for (int s = 0; s < 2; ++s) {
        if (coef12_host[s * 6 + 3] != 1.0) return DAM_ERR_BAD_ARG;        // normalised sections only
        for (int i = 0; i < 3; ++i) k.b[s][i] = coef12_host[s * 6 + i];
        k.a[s][0] = coef12_host[s * 6 + 4]; k.a[s][1] = coef12_host[s * 6 + 5];
    }
    hipStream_t st = (hipStream_t)stream;
    KwBatchGeo g;
    g.n_samples = n_samples; g.n_chunks = cdiv(n_samples, KW_CHUNK);
    g.track_stride = track_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.channels = channels; g.n_gains = gains ? n_gains : 1;
    g.n_bounds = 2 * n_blocks;
    g.piece_stride = (int64_t)g.n_bounds + g.n_chunks + 1;
    const KwBatchWs w = kw_batch_ws(workspace, rows, g.n_chunks, n_blocks);
    const dim3 bgrid((unsigned)cdiv(n_blocks, 256));
    hipLaunchKernelGGL(kw_bounds_merge_kernel, bgrid, dim3(256), 0, st, blk_lo, blk_hi, n_blocks, w.bnd, w.pos_lo, w.pos_hi);
    DAM_CHECK_LAUNCH();
    const dim3 grid((unsigned)cdiv(g.n_chunks, KW_ROWS), (unsigned)rows);
#define DAM_KW_PASS(P)                                                                                                   \
    if (x_is_f64)                                                                                                        \
        hipLaunchKernelGGL((kw_batch_chunk_kernel<double, P>), grid, dim3(64), 0, st, reinterpret_cast<const double*>(x), g, k, \
                           gains, w.bnd, w.state, w.piece);                                                              \
    else                                                                                                                 \
        hipLaunchKernelGGL((kw_batch_chunk_kernel<float, P>), grid, dim3(64), 0, st, reinterpret_cast<const float*>(x), g, k,   \
                           gains, w.bnd, w.state, w.piece)
    DAM_KW_PASS(1);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(kw_scan_kernel, dim3((unsigned)rows), dim3(256), 0, st, k, KW_CHUNK, g.n_chunks, w.state);
    DAM_CHECK_LAUNCH();
    DAM_KW_PASS(2);
#undef DAM_KW_PASS
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(kw_batch_block_sum_kernel, dim3((unsigned)cdiv(n_blocks, 256), (unsigned)rows), dim3(256), 0, st, w.piece,
                       g, w.bnd, w.pos_lo, w.pos_hi, n_blocks, 1.0 / block_len, z);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_loudness_gate(const double* z, int n_tracks, int channels, int n_blocks, double* lufs, void* stream) {
    using namespace dam;
    if (!z || !lufs || n_tracks <= 0 || channels <= 0 || channels > 5 || n_blocks <= 0) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(kw_gate_kernel, dim3((unsigned)n_tracks), dim3(256), 0, (hipStream_t)stream, z, channels, n_blocks, lufs);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_loudness_target_gains(const double* lufs, const double* target, int n, double* gains, void* stream) {
    using namespace dam;
    if (!lufs || !target || !gains || n <= 0) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(kw_target_gains_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, lufs, target, n,
                       gains);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
