// dam_compressor.hip -- feed-forward compressor with attack and release: the recurrence the look-ahead limiter leaves out.
//
// Definition (include/dam_hip.h states it in full; tests/_compressor_ref.py restates it in numpy).  All float64:
//   xs[c][i] = (double)x[c][i] * s                       s = pre_gain of the row set, 1 if none
//   d[i]     = max_c |xs[c][i]|                          one detector for the channels of a set (stereo link)
//   c[i]     = static curve of d[i], dB of reduction     0 exactly, no logarithm, where d <= knee_start
//   p[i]     = max(c[i], aR p[i-1])                      release: peak hold with exponential decay      p[-1] = 0
//   q[i]     = fma(aA, q[i-1], (1 - aA) p[i])            attack: one pole on p                           q[-1] = 0
//   out[c][i] = xs[c][i] * (exp(-(q[i] * ln10/20)) * M)
//
// Both recurrences are scans over closed families of maps of the state:
//   y -> max(c, a y):  (c2, a2) o (c1, a1) = (max(c2, a2 c1), a2 a1), identity (0, 1)   (c >= 0, y >= 0)
//   y -> A y + B:      (B2, A2) o (B1, A1) = (fma(A2, B1, B2), A2 A1), identity (0, 1)
// so a row is cut into chunks of CMP_CHUNK samples, one lane per chunk, CMP_THREADS chunks per workgroup:
//   1. compressor_curve_kernel: d and c per sample, coalesced; c goes to the workspace (8 B per sample) and to LDS, where
//      every lane walks its chunk from p = 0.  The chunk maps (p_end, aR^K) are scanned across the workgroup: every chunk
//      keeps the map of the chunks before it in the tile, the tile keeps its total.  #{d > knee_start} per tile.
//   2. compressor_scan_kernel<Release>: one workgroup per row set walks the tile totals, 256 at a time with a carry, and
//      leaves every tile's entry state.
//   3. compressor_attack_kernel: c again, p from its true entry state max(C_before, A_before * tile entry), q from 0:
//      the chunk maps (q_end, aA^K), scanned as in 1.
//   4. compressor_scan_kernel<Attack>.
//   5. compressor_apply_kernel: p and q from their true entry states; q goes to LDS, then the workgroup applies the gain
//      coalesced, one exp per sample, and writes out (and q where asked).  max q per tile.
//   6. compressor_stats_kernel: the maximum and the integer sum of the tiles' partials per row set.
// Every scan combines in an order that is a function of the element's position in its row set only: a shuffle scan over
// the 64 lanes of a wave, the four wave totals folded left to right, the tiles' carry left to right.  Chunks that start
// behind the row hold the identity; the row's last chunk is walked over c = 0 behind the row's end, which nothing reads
// (no chunk follows it).  Entry states depend on earlier chunks only, so a prefix of the output depends on that prefix of
// the input only.  Where c = 0 so far every state is 0.0 exactly: q = fma(aA, 0, (1 - aA) 0) = 0, exp(-0) = 1.
// No atomics, no host synchronisation, nothing depends on the grid or on the other row sets.
#include "dam_common.h"

#include <math.h>

namespace dam {
namespace {

constexpr int CMP_THREADS = 256;                       // chunks of one workgroup
constexpr int CMP_CHUNK = 16;                          // samples of one lane: part of the definition of the rounding
constexpr int CMP_TILE = CMP_THREADS * CMP_CHUNK;      // samples of one workgroup
constexpr int CMP_LOADS = CMP_TILE / CMP_THREADS;
constexpr int CMP_ROW = CMP_CHUNK + 1;                 // doubles between two lanes' chunks in LDS: 34 l mod 64, conflict-free
constexpr int CMP_WAVES = CMP_THREADS / WAVE;
constexpr int CMP_MAX_TAU = 1 << 17;                   // samples of the longest time constant
constexpr double CMP_LN10_20 = 0.11512925464970228;    // ln(10) / 20

struct CmpGeo {
    int64_t n_samples, tiles;
    int64_t set_stride, sample_stride, channel_stride;         // elements
    int channels;
    double threshold, slope, knee, knee_start;                 // dB, 1 - 1/R, dB, linear
    double a_att, one_minus_a_att, a_rel, makeup;
    double a_att_chunk, a_rel_chunk;                           // a^CMP_CHUNK by CMP_CHUNK - 1 multiplications
};

// per row set: c [n], then per chunk the maps before it in its tile, then per tile totals, entry states and partials
struct CmpWorkspace {
    double* c;
    double *rel_c, *rel_a, *att_b, *att_a;                     // [sets][tiles * CMP_THREADS]
    double *tile_rel_c, *tile_rel_a, *entry_rel;               // [sets][tiles]
    double *tile_att_b, *tile_att_a, *entry_att;
    double* part_max;
    int64_t* part_cnt;
};

struct Release {            // y -> max(c, a y), held as (u, v) = (c, a)
    static __device__ __forceinline__ void compose(double& u, double& v, double eu, double ev) {       // (u, v) o (eu, ev)
        u = fmax(u, v * eu);
        v = v * ev;
    }
    static __device__ __forceinline__ double apply(double u, double v, double y) { return fmax(u, v * y); }
};
struct Attack {             // y -> A y + B, held as (u, v) = (B, A)
    static __device__ __forceinline__ void compose(double& u, double& v, double eu, double ev) {
        u = fma(v, eu, u);
        v = v * ev;
    }
    static __device__ __forceinline__ double apply(double u, double v, double y) { return fma(v, y, u); }
};

// (u, v): lane t's map on entry, the composition of the maps of lanes 0 .. t-1 on exit (the identity for lane 0);
// (tu, tv): the composition of all CMP_THREADS maps.  sh: 2 * CMP_WAVES doubles, free again on return.
template <class Op>
__device__ __forceinline__ void block_scan(double& u, double& v, double& tu, double& tv, double* sh) {
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {         // after the step: lanes [max(0, lane - 2 off + 1), lane]
        const double eu = __shfl_up(u, off), ev = __shfl_up(v, off);
        if (lane >= off) Op::compose(u, v, eu, ev);
    }
    if (lane == WAVE - 1) { sh[w] = u; sh[CMP_WAVES + w] = v; }
    double xu = __shfl_up(u, 1), xv = __shfl_up(v, 1);  // exclusive within the wave
    if (lane == 0) { xu = 0.0; xv = 1.0; }
    __syncthreads();
    double bu = 0.0, bv = 1.0;                         // the waves before this one, left to right
    tu = 0.0; tv = 1.0;
#pragma unroll
    for (int k = 0; k < CMP_WAVES; ++k) {
        double ku = sh[k], kv = sh[CMP_WAVES + k];
        Op::compose(ku, kv, tu, tv);
        tu = ku; tv = kv;
        if (k + 1 == w) { bu = tu; bv = tv; }
    }
    Op::compose(xu, xv, bu, bv);
    u = xu; v = xv;
    __syncthreads();
}

__device__ __forceinline__ double cmp_curve(double d, const CmpGeo& g) {
    if (!(d > g.knee_start)) return 0.0;
    const double o = 20.0 * log10(d) - g.threshold;
    if (g.knee > 0.0 && o < 0.5 * g.knee) {
        const double t = fmax(o + 0.5 * g.knee, 0.0);
        return g.slope * (t * t) / (2.0 * g.knee);
    }
    return g.slope * fmax(o, 0.0);
}

// c of the tile from the workspace into the LDS image, 0 behind the row
__device__ __forceinline__ void load_curve(const double* __restrict__ cw, int64_t t0, int64_t n, double* img) {
#pragma unroll
    for (int k = 0; k < CMP_LOADS; ++k) {
        const int e = k * CMP_THREADS + threadIdx.x;
        img[e + e / CMP_CHUNK] = t0 + e < n ? cw[t0 + e] : 0.0;
    }
}

template <typename T>
__global__ __launch_bounds__(CMP_THREADS) void compressor_curve_kernel(const T* __restrict__ x, CmpGeo g,
                                                                        const double* __restrict__ pre_gain, CmpWorkspace ws) {
    __shared__ double img[CMP_THREADS * CMP_ROW];
    __shared__ double sh[2 * CMP_WAVES];
    __shared__ int red[CMP_WAVES];
    const int t = threadIdx.x, set = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * CMP_TILE;
    const double s = pre_gain ? pre_gain[set] : 1.0;
    const T* xs = x + set * g.set_stride;
    double* cw = ws.c + (int64_t)set * g.n_samples;
    int over = 0;
#pragma unroll
    for (int k = 0; k < CMP_LOADS; ++k) {
        const int e = k * CMP_THREADS + t;
        const int64_t i = t0 + e;
        double c = 0.0;
        if (i < g.n_samples) {
            double d = 0.0;
            for (int ch = 0; ch < g.channels; ++ch) d = fmax(d, fabs((double)xs[i * g.sample_stride + ch * g.channel_stride] * s));
            over += d > g.knee_start;
            c = cmp_curve(d, g);
            cw[i] = c;
        }
        img[e + e / CMP_CHUNK] = c;
    }
    __syncthreads();
    const double* m = img + t * CMP_ROW;
    double p = 0.0;
#pragma unroll
    for (int i = 0; i < CMP_CHUNK; ++i) p = fmax(m[i], g.a_rel * p);
    const bool live = t0 + (int64_t)t * CMP_CHUNK < g.n_samples;
    double u = live ? p : 0.0, v = live ? g.a_rel_chunk : 1.0, tu, tv;
    block_scan<Release>(u, v, tu, tv, sh);
    const int64_t tile = (int64_t)set * g.tiles + blockIdx.x;
    ws.rel_c[tile * CMP_THREADS + t] = u;
    ws.rel_a[tile * CMP_THREADS + t] = v;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) over += __shfl_xor(over, off);
    if ((t & (WAVE - 1)) == 0) red[t / WAVE] = over;
    __syncthreads();
    if (t == 0) {
        ws.tile_rel_c[tile] = tu;
        ws.tile_rel_a[tile] = tv;
        int64_t cnt = 0;
#pragma unroll
        for (int k = 0; k < CMP_WAVES; ++k) cnt += red[k];
        ws.part_cnt[tile] = cnt;
    }
}

// one workgroup per row set: entry[k] = the state behind tiles 0 .. k-1 of a row that starts from 0
template <class Op>
__global__ __launch_bounds__(CMP_THREADS) void compressor_scan_kernel(const double* __restrict__ tile_u,
                                                                       const double* __restrict__ tile_v, int64_t tiles,
                                                                       double* __restrict__ entry) {
    __shared__ double sh[2 * CMP_WAVES];
    const int64_t base = (int64_t)blockIdx.x * tiles;
    double carry = 0.0;
    for (int64_t k0 = 0; k0 < tiles; k0 += CMP_THREADS) {
        const int64_t k = k0 + threadIdx.x;
        double u = k < tiles ? tile_u[base + k] : 0.0, v = k < tiles ? tile_v[base + k] : 1.0, tu, tv;
        block_scan<Op>(u, v, tu, tv, sh);
        if (k < tiles) entry[base + k] = Op::apply(u, v, carry);
        carry = Op::apply(tu, tv, carry);
    }
}

__global__ __launch_bounds__(CMP_THREADS) void compressor_attack_kernel(CmpGeo g, CmpWorkspace ws) {
    __shared__ double img[CMP_THREADS * CMP_ROW];
    __shared__ double sh[2 * CMP_WAVES];
    const int t = threadIdx.x, set = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * CMP_TILE;
    load_curve(ws.c + (int64_t)set * g.n_samples, t0, g.n_samples, img);
    __syncthreads();
    const int64_t tile = (int64_t)set * g.tiles + blockIdx.x, chunk = tile * CMP_THREADS + t;
    const double* m = img + t * CMP_ROW;
    double p = Release::apply(ws.rel_c[chunk], ws.rel_a[chunk], ws.entry_rel[tile]), q = 0.0;
#pragma unroll
    for (int i = 0; i < CMP_CHUNK; ++i) {
        p = fmax(m[i], g.a_rel * p);
        q = fma(g.a_att, q, g.one_minus_a_att * p);
    }
    const bool live = t0 + (int64_t)t * CMP_CHUNK < g.n_samples;
    double u = live ? q : 0.0, v = live ? g.a_att_chunk : 1.0, tu, tv;
    block_scan<Attack>(u, v, tu, tv, sh);
    ws.att_b[chunk] = u;
    ws.att_a[chunk] = v;
    if (t == 0) {
        ws.tile_att_b[tile] = tu;
        ws.tile_att_a[tile] = tv;
    }
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(CMP_THREADS) void compressor_apply_kernel(const TIn* __restrict__ x, CmpGeo g,
                                                                        const double* __restrict__ pre_gain, CmpWorkspace ws,
                                                                        TOut* __restrict__ out, double* __restrict__ reduction) {
    __shared__ double img[CMP_THREADS * CMP_ROW];
    __shared__ double red[CMP_WAVES];
    const int t = threadIdx.x, set = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * CMP_TILE;
    load_curve(ws.c + (int64_t)set * g.n_samples, t0, g.n_samples, img);
    __syncthreads();
    const int64_t tile = (int64_t)set * g.tiles + blockIdx.x, chunk = tile * CMP_THREADS + t;
    double* m = img + t * CMP_ROW;
    double p = Release::apply(ws.rel_c[chunk], ws.rel_a[chunk], ws.entry_rel[tile]);
    double q = Attack::apply(ws.att_b[chunk], ws.att_a[chunk], ws.entry_att[tile]);
    const int64_t left = g.n_samples - (t0 + (int64_t)t * CMP_CHUNK);          // samples of the row from the chunk's first on
    double hi = 0.0;
#pragma unroll
    for (int i = 0; i < CMP_CHUNK; ++i) {
        p = fmax(m[i], g.a_rel * p);
        q = fma(g.a_att, q, g.one_minus_a_att * p);
        m[i] = q;                                      // the lane's own element: read above, written here
        if (i < left) hi = fmax(hi, q);                // (behind the row q may still rise towards p)
    }
    __syncthreads();
    const double s = pre_gain ? pre_gain[set] : 1.0;
    const TIn* xs = x + set * g.set_stride;
    TOut* o = out + (int64_t)set * g.channels * g.n_samples;
    double* r = reduction ? reduction + (int64_t)set * g.n_samples : nullptr;
#pragma unroll
    for (int k = 0; k < CMP_LOADS; ++k) {
        const int e = k * CMP_THREADS + t;
        const int64_t i = t0 + e;
        if (i < g.n_samples) {
            const double qi = img[e + e / CMP_CHUNK];
            const double gain = exp(-(qi * CMP_LN10_20)) * g.makeup;
            for (int ch = 0; ch < g.channels; ++ch)
                o[ch * g.n_samples + i] = (TOut)(((double)xs[i * g.sample_stride + ch * g.channel_stride] * s) * gain);
            if (r) r[i] = qi;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) hi = fmax(hi, __shfl_xor(hi, off));
    if ((t & (WAVE - 1)) == 0) red[t / WAVE] = hi;
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int k = 1; k < CMP_WAVES; ++k) hi = fmax(hi, red[k]);
        ws.part_max[tile] = hi;
    }
}

// one workgroup per row set: the maximum and the sum of its tiles' partials (order-free)
__global__ __launch_bounds__(CMP_THREADS) void compressor_stats_kernel(const double* __restrict__ part_max,
                                                                        const int64_t* __restrict__ part_cnt, int64_t tiles,
                                                                        double* __restrict__ max_reduction,
                                                                        int64_t* __restrict__ n_over) {
    __shared__ double red_max[CMP_THREADS];
    __shared__ int64_t red_cnt[CMP_THREADS];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * tiles;
    double hi = 0.0;
    int64_t cnt = 0;
    for (int64_t i = t; i < tiles; i += CMP_THREADS) { hi = fmax(hi, part_max[p0 + i]); cnt += part_cnt[p0 + i]; }
    red_max[t] = hi;
    red_cnt[t] = cnt;
    __syncthreads();
    for (int w = CMP_THREADS / 2; w >= 1; w >>= 1) {
        if (t < w) { red_max[t] = fmax(red_max[t], red_max[t + w]); red_cnt[t] += red_cnt[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        if (max_reduction) max_reduction[blockIdx.x] = red_max[0];
        if (n_over) n_over[blockIdx.x] = red_cnt[0];
    }
}

static CmpWorkspace carve(void* workspace, int64_t n_sets, int64_t n, int64_t tiles) {
    CmpWorkspace ws;
    double* p = reinterpret_cast<double*>(workspace);
    const int64_t chunks = n_sets * tiles * CMP_THREADS, all_tiles = n_sets * tiles;
    ws.c = p; p += n_sets * n;
    ws.rel_c = p; p += chunks;
    ws.rel_a = p; p += chunks;
    ws.att_b = p; p += chunks;
    ws.att_a = p; p += chunks;
    ws.tile_rel_c = p; p += all_tiles;
    ws.tile_rel_a = p; p += all_tiles;
    ws.entry_rel = p; p += all_tiles;
    ws.tile_att_b = p; p += all_tiles;
    ws.tile_att_a = p; p += all_tiles;
    ws.entry_att = p; p += all_tiles;
    ws.part_max = p; p += all_tiles;
    ws.part_cnt = reinterpret_cast<int64_t*>(p);
    return ws;
}

static double chunk_power(double a) {
    double r = a;
    for (int i = 1; i < CMP_CHUNK; ++i) r *= a;
    return r;
}

// alpha = exp(-1 / tau) within (0, 1), tau at most CMP_MAX_TAU samples (1e-9: log(a) of an a that close to 1 is good to
// ulp(1) / (1 - a) = 1.5e-11 relative at the cap)
static bool alpha_ok(double a) { return a > 0.0 && a < 1.0 && -1.0 / log(a) <= (double)CMP_MAX_TAU * (1.0 + 1e-9); }

template <typename TIn, typename TOut>
static void launch_apply(dim3 grid, hipStream_t st, const void* x, const CmpGeo& g, const double* pre_gain, const CmpWorkspace& ws,
                         void* out, double* reduction) {
    hipLaunchKernelGGL((compressor_apply_kernel<TIn, TOut>), grid, dim3(CMP_THREADS), 0, st, reinterpret_cast<const TIn*>(x), g,
                       pre_gain, ws, reinterpret_cast<TOut*>(out), reduction);
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_compressor_chunk_samples(void) { return dam::CMP_CHUNK; }
extern "C" int64_t dam_compressor_tile_samples(void) { return dam::CMP_TILE; }
extern "C" int64_t dam_compressor_max_time_samples(void) { return dam::CMP_MAX_TAU; }

extern "C" int64_t dam_compressor_workspace_bytes(int n_sets, int64_t n_samples) {
    if (n_sets <= 0 || n_samples <= 0) return 0;
    const int64_t tiles = dam::cdiv(n_samples, dam::CMP_TILE);
    return (int64_t)n_sets * (n_samples + tiles * (4 * dam::CMP_THREADS + 8)) * 8;
}

extern "C" int dam_compressor_apply(const void* x, int x_is_f64, int n_sets, int64_t n_samples, int channels, int64_t set_stride,
                                    int64_t sample_stride, int64_t channel_stride, const double* pre_gain, double threshold_db,
                                    double ratio, double knee_db, double knee_start, double alpha_attack, double alpha_release,
                                    double makeup_lin, void* out, int out_is_f64, double* reduction, double* max_reduction,
                                    int64_t* n_over, void* workspace, void* stream) {
    using namespace dam;
    if (!x || !out || !workspace) return DAM_ERR_BAD_ARG;
    if (n_sets <= 0 || n_samples < 1 || channels <= 0) return DAM_ERR_BAD_ARG;
    if (n_sets > 65535) return DAM_ERR_BAD_ARG;
    if (!(ratio >= 1.0) || !(knee_db >= 0.0) || !isfinite(knee_db) || !isfinite(threshold_db)) return DAM_ERR_BAD_ARG;
    if (!(knee_start > 0.0) || !isfinite(knee_start)) return DAM_ERR_BAD_ARG;
    if (!(fabs(20.0 * log10(knee_start) - (threshold_db - 0.5 * knee_db)) <= 1e-9)) return DAM_ERR_BAD_ARG;
    if (!alpha_ok(alpha_attack) || !alpha_ok(alpha_release)) return DAM_ERR_BAD_ARG;
    if (!(makeup_lin > 0.0) || !isfinite(makeup_lin)) return DAM_ERR_BAD_ARG;
    const int64_t tiles = cdiv(n_samples, CMP_TILE);
    if (tiles > 0x7fffffff) return DAM_ERR_BAD_ARG;
    CmpGeo g;
    g.n_samples = n_samples; g.tiles = tiles;
    g.set_stride = set_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.channels = channels;
    g.threshold = threshold_db; g.slope = 1.0 - 1.0 / ratio; g.knee = knee_db; g.knee_start = knee_start;
    g.a_att = alpha_attack; g.one_minus_a_att = 1.0 - alpha_attack; g.a_rel = alpha_release; g.makeup = makeup_lin;
    g.a_att_chunk = chunk_power(alpha_attack); g.a_rel_chunk = chunk_power(alpha_release);
    const CmpWorkspace ws = carve(workspace, n_sets, n_samples, tiles);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)n_sets), block(CMP_THREADS), sets((unsigned)n_sets);
    if (x_is_f64)
        hipLaunchKernelGGL(compressor_curve_kernel<double>, grid, block, 0, st, reinterpret_cast<const double*>(x), g, pre_gain, ws);
    else
        hipLaunchKernelGGL(compressor_curve_kernel<float>, grid, block, 0, st, reinterpret_cast<const float*>(x), g, pre_gain, ws);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(compressor_scan_kernel<Release>, sets, block, 0, st, ws.tile_rel_c, ws.tile_rel_a, tiles, ws.entry_rel);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(compressor_attack_kernel, grid, block, 0, st, g, ws);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(compressor_scan_kernel<Attack>, sets, block, 0, st, ws.tile_att_b, ws.tile_att_a, tiles, ws.entry_att);
    DAM_CHECK_LAUNCH();
    if (x_is_f64) {
        if (out_is_f64) launch_apply<double, double>(grid, st, x, g, pre_gain, ws, out, reduction);
        else launch_apply<double, float>(grid, st, x, g, pre_gain, ws, out, reduction);
    } else {
        if (out_is_f64) launch_apply<float, double>(grid, st, x, g, pre_gain, ws, out, reduction);
        else launch_apply<float, float>(grid, st, x, g, pre_gain, ws, out, reduction);
    }
    DAM_CHECK_LAUNCH();
    if (max_reduction || n_over) {
        hipLaunchKernelGGL(compressor_stats_kernel, sets, block, 0, st, ws.part_max, ws.part_cnt, tiles, max_reduction, n_over);
        DAM_CHECK_LAUNCH();
    }
    return DAM_OK;
}
