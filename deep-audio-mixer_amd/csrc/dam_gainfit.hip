// dam_gainfit.hip -- the gains a reference mix used, fitted per stem and window on the device, and the distance of candidate
// gain curves from them (include/dam_hip.h states the definitions).
//
// The evaluation judges a mix by level, by level over time and by tone -- all three indirect: the model predicts per-stem
// gains over time, and a windowed least-squares fit of "stems x gains ~ reference mix" says what gains the reference used.
//   moments   one workgroup = GF_TILE consecutive samples of one window: the (S+1)(S+2)/2 products of the S stems and the
//             target, added in float64 to the lane's own running sums; wave butterfly, wave merge    (window, tile) grid
//   reduce    a window's tile records added in ascending tile order, both triangles written          one workgroup per window
//   solve     windows pooled, normalised to unit diagonal, Cholesky on the active stems              one workgroup per window
//   error     mean |d - window mean of d| of d = 20 log10(cand / fit)                                one per candidate
// The moments kernel is the only one that sees the samples; it reads every element once through runtime strides (any layout,
// float32 / float64 stems and target independently).  S and the channel count are template parameters: the running sums are
// named registers (an accumulator array indexed at run time would live in scratch).
#include "dam_common.h"

#pragma clang fp contract(off)        // every sum is stated operation by operation; the one fused multiply-add is written out

namespace dam {
namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_PER = 32;                            // samples a lane owns in a full tile
constexpr int64_t GF_TILE = GF_THREADS * GF_PER;      // 8192: a library constant, never a function of the call
constexpr int GF_MAX_S = DAM_GAINFIT_MAX_STEMS;
constexpr int GF_MAX_U = GF_MAX_S + 1;
static_assert(GF_MAX_U * (GF_MAX_U + 1) / 2 <= WAVE, "one lane per pair in the merges");

struct GfGeo {
    int64_t n_samples, stem_stride, sample_stride, channel_stride, y_sample_stride, y_channel_stride;
    int64_t seg;                      // n_samples / W
    int W, tmax;                      // tmax: tiles of the longest (the last) window = records per window in the workspace
};

__device__ __forceinline__ int64_t window_length(const GfGeo& g, int w) {
    return w == g.W - 1 ? g.n_samples - (int64_t)w * g.seg : g.seg;
}

template <typename TX, typename TY, int S, int C>
__device__ __forceinline__ void add_sample(const TX* __restrict__ x, const TY* __restrict__ y, const GfGeo& g, int64_t p,
                                           double (&acc)[(S + 1) * (S + 2) / 2]) {
    double u[C][S + 1];
    const TX* xp = x + p * g.sample_stride;
    const TY* yp = y + p * g.y_sample_stride;
#pragma unroll
    for (int c = 0; c < C; ++c) {                     // every load of the sample is issued before the first is used
#pragma unroll
        for (int s = 0; s < S; ++s) u[c][s] = (double)xp[s * g.stem_stride + c * g.channel_stride];
        u[c][S] = (double)yp[c * g.y_channel_stride];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int k = 0;
#pragma unroll
        for (int i = 0; i <= S; ++i)
#pragma unroll
            for (int j = i; j <= S; ++j, ++k) acc[k] = __builtin_fma(u[c][i], u[c][j], acc[k]);
    }
}

template <typename TX, typename TY, int S, int C>
__global__ __launch_bounds__(GF_THREADS) void gainfit_moments_kernel(const TX* __restrict__ x, const TY* __restrict__ y, GfGeo g,
                                                                     double* __restrict__ partial) {
    constexpr int NP = (S + 1) * (S + 2) / 2;
    __shared__ double wave_sum[GF_THREADS / WAVE][NP];
    const int tid = threadIdx.x;
    const int w = (int)(blockIdx.x / (unsigned)g.tmax), t = (int)(blockIdx.x % (unsigned)g.tmax);
    const int64_t start = (int64_t)w * g.seg, L = window_length(g, w);
    const int64_t q0 = (int64_t)t * GF_TILE;
    if (q0 >= L) return;                              // (workgroup-uniform: a shorter window has fewer tiles than the last)
    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
    if (L - q0 >= GF_TILE) {
        // (S + 1) C loads per sample; the unroll keeps some 20 to 40 of them in flight per lane
#pragma clang loop unroll_count(S <= 2 ? 8 : S <= 4 ? 4 : 2)
        for (int i = 0; i < GF_PER; ++i) add_sample<TX, TY, S, C>(x, y, g, start + q0 + tid + (int64_t)GF_THREADS * i, acc);
    } else {
        for (int64_t q = q0 + tid; q < L; q += GF_THREADS) add_sample<TX, TY, S, C>(x, y, g, start + q, acc);
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], m);
    }
    if ((tid & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < NP; ++k) wave_sum[tid / WAVE][k] = acc[k];
    }
    __syncthreads();
    if (tid < NP)
        partial[((int64_t)w * g.tmax + t) * NP + tid] = ((wave_sum[0][tid] + wave_sum[1][tid]) + wave_sum[2][tid]) + wave_sum[3][tid];
}

__global__ __launch_bounds__(WAVE) void gainfit_reduce_kernel(const double* __restrict__ partial, GfGeo g, int S,
                                                              double* __restrict__ moments) {
    const int U = S + 1, NP = U * (U + 1) / 2, k = threadIdx.x, w = blockIdx.x;
    if (k >= NP) return;
    const int64_t nt = (window_length(g, w) + GF_TILE - 1) / GF_TILE;
    const double* p = partial + (int64_t)w * g.tmax * NP + k;
    double s = p[0];
#pragma unroll 8                                      // eight loads in flight; the additions stay in ascending order
    for (int64_t i = 1; i < nt; ++i) s += p[i * NP];
    int i = 0, row = U, rest = k;                     // pair k of the row-major upper triangle -> (i, j)
    while (rest >= row) { rest -= row; --row; ++i; }
    const int j = i + rest;
    double* m = moments + (int64_t)w * U * U;
    m[i * U + j] = s;
    m[j * U + i] = s;
}

__device__ __forceinline__ double gf_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One workgroup per (group, window): blockIdx.x = group * W + w.  A group is one run of W windows with its own moments
// [W][S+1][S+1], gains [S][W], residual / target / status [W]; windows are pooled within their group only.  dam_gainfit_solve is
// the call with one group and no target.
__global__ __launch_bounds__(WAVE) void gainfit_solve_kernel(const double* __restrict__ moments, int W, int S, int pool,
                                                             double ridge, double* __restrict__ gains,
                                                             double* __restrict__ residual, double* __restrict__ target,
                                                             int* __restrict__ status) {
    __shared__ double A[GF_MAX_U * GF_MAX_U];
    __shared__ double R[GF_MAX_S * GF_MAX_S];         // the normalised matrix, then its Cholesky factor (lower triangle)
    __shared__ double d[GF_MAX_S], hv[GF_MAX_S], gv[GF_MAX_S];
    __shared__ int idx[GF_MAX_S];
    const int w = (int)(blockIdx.x % (unsigned)W), U = S + 1, UU = U * U;
    const int64_t group = blockIdx.x / (unsigned)W;
    moments += group * W * UU;
    gains += group * S * W;
    residual += group * W;
    status += group * W;
    const int64_t v0 = (int64_t)w - pool > 0 ? (int64_t)w - pool : 0;
    const int64_t v1 = (int64_t)w + pool < W - 1 ? (int64_t)w + pool : W - 1;
    for (int e = threadIdx.x; e < UU; e += WAVE) {
        double s = moments[v0 * UU + e];
        for (int64_t v = v0 + 1; v <= v1; ++v) s += moments[v * UU + e];
        A[e] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;                     // not hot: the elimination is one lane's plain loops
    const double Y = A[S * U + S];
    int na = 0;
    for (int s = 0; s < S; ++s) {
        const double gss = A[s * U + s];
        if (gss > 0.0 && gss >= DAM_GAINFIT_GATE * Y) idx[na++] = s;
    }
    int st = na;
    if (Y == 0.0 || na == 0) {
        st = 0;
    } else {
        for (int a = 0; a < na; ++a) d[a] = sqrt(A[idx[a] * U + idx[a]]);
        for (int i = 0; i < na; ++i)
            for (int j = 0; j < na; ++j) R[i * GF_MAX_S + j] = A[idx[i] * U + idx[j]] / (d[i] * d[j]) + (i == j ? ridge : 0.0);
        for (int j = 0; j < na && st > 0; ++j) {
            double piv = R[j * GF_MAX_S + j];
            for (int k = 0; k < j; ++k) piv -= R[j * GF_MAX_S + k] * R[j * GF_MAX_S + k];
            if (!(piv > DAM_GAINFIT_PIVOT)) { st = -1; break; }
            const double ljj = sqrt(piv);
            R[j * GF_MAX_S + j] = ljj;
            for (int i = j + 1; i < na; ++i) {
                double v = R[i * GF_MAX_S + j];
                for (int k = 0; k < j; ++k) v -= R[i * GF_MAX_S + k] * R[j * GF_MAX_S + k];
                R[i * GF_MAX_S + j] = v / ljj;
            }
        }
    }
    for (int s = 0; s < S; ++s) gv[s] = 0.0;
    if (st > 0) {
        for (int i = 0; i < na; ++i) {
            double v = A[idx[i] * U + S] / d[i];
            for (int k = 0; k < i; ++k) v -= R[i * GF_MAX_S + k] * hv[k];
            hv[i] = v / R[i * GF_MAX_S + i];
        }
        for (int i = na - 1; i >= 0; --i) {
            double v = hv[i];
            for (int k = i + 1; k < na; ++k) v -= R[k * GF_MAX_S + i] * hv[k];
            hv[i] = v / R[i * GF_MAX_S + i];
        }
        for (int s = 0; s < S; ++s) gains[(int64_t)s * W + w] = gf_nan();
        for (int a = 0; a < na; ++a) {
            gv[idx[a]] = hv[a] / d[a];
            gains[(int64_t)idx[a] * W + w] = gv[idx[a]];
        }
        double bg = 0.0, gGg = 0.0;
        for (int i = 0; i < S; ++i) bg += A[i * U + S] * gv[i];
        for (int i = 0; i < S; ++i) {
            double t = 0.0;
            for (int j = 0; j < S; ++j) t += A[i * U + j] * gv[j];
            gGg += gv[i] * t;
        }
        const double r = (Y - 2.0 * bg + gGg) / Y;
        residual[w] = r > 0.0 ? r : 0.0;
    } else {
        for (int s = 0; s < S; ++s) gains[(int64_t)s * W + w] = gf_nan();
        residual[w] = gf_nan();
    }
    status[w] = st;
    if (target) target[group * W + w] = Y;
}

// Lane j of the 64 takes window c0 + j of a run of 64 and leaves its contributions in LDS; lane s < S then adds stem s's, and
// lane GF_MAX_S the variant's, in the order of the header (windows ascending, stems ascending within a window).
__global__ __launch_bounds__(WAVE) void gainfit_gain_error_kernel(const double* __restrict__ fit, const double* __restrict__ cand_all,
                                                                  int S, int W, int n_cand, double* __restrict__ err,
                                                                  double* __restrict__ err_stem, int* __restrict__ n_kept) {
    __shared__ double contrib[WAVE][GF_MAX_S];
    __shared__ unsigned mask[WAVE];
    const int lane = threadIdx.x, v = blockIdx.x;
    const double* cand = cand_all + (int64_t)v * S * n_cand;
    double sum = 0.0;
    int count = 0;
    for (int c0 = 0; c0 < W; c0 += WAVE) {
        const int w = c0 + lane;
        unsigned kept = 0;
        if (w < W) {
            double dv[GF_MAX_S], mu = 0.0;
            int nk = 0;
#pragma unroll
            for (int s = 0; s < GF_MAX_S; ++s) {
                dv[s] = 0.0;
                if (s < S) {
                    const double f = fit[(int64_t)s * W + w], c = cand[(int64_t)s * n_cand + (n_cand == 1 ? 0 : w)];
                    if (isfinite(f) && isfinite(c) && f > 0.0 && c > 0.0) {
                        dv[s] = 20.0 * log10(c / f);
                        mu += dv[s];
                        kept |= 1u << s;
                        ++nk;
                    }
                }
            }
            if (nk < 2) kept = 0;
            else mu = mu / (double)nk;
#pragma unroll
            for (int s = 0; s < GF_MAX_S; ++s) contrib[lane][s] = kept >> s & 1u ? fabs(dv[s] - mu) : 0.0;
        }
        mask[lane] = kept;
        __syncthreads();
        const int run = W - c0 < WAVE ? W - c0 : WAVE;
        // (an entry that is not kept holds +0.0: adding it changes no sum, and the loops have no branch to wait for)
        if (lane < S) {
#pragma unroll 8
            for (int j = 0; j < run; ++j) {
                sum += contrib[j][lane];
                count += (int)(mask[j] >> lane & 1u);
            }
        } else if (lane == GF_MAX_S) {
#pragma unroll 2
            for (int j = 0; j < run; ++j) {
#pragma unroll
                for (int s = 0; s < GF_MAX_S; ++s) sum += contrib[j][s];
                count += __popc(mask[j]);
            }
        }
        __syncthreads();
    }
    const double mean = count ? sum / (double)count : gf_nan();
    if (lane < S) err_stem[(int64_t)v * S + lane] = mean;
    if (lane == GF_MAX_S) {
        err[v] = mean;
        n_kept[v] = count;
    }
}

template <typename TX, typename TY, int S>
void launch_moments(const void* x, const void* y, const GfGeo& g, int channels, unsigned blocks, double* partial, hipStream_t s) {
    if (channels == 2)
        hipLaunchKernelGGL((gainfit_moments_kernel<TX, TY, S, 2>), dim3(blocks), dim3(GF_THREADS), 0, s, (const TX*)x, (const TY*)y, g, partial);
    else
        hipLaunchKernelGGL((gainfit_moments_kernel<TX, TY, S, 1>), dim3(blocks), dim3(GF_THREADS), 0, s, (const TX*)x, (const TY*)y, g, partial);
}

template <typename TX, typename TY>
void dispatch_moments(int S, const void* x, const void* y, const GfGeo& g, int channels, unsigned blocks, double* partial,
                      hipStream_t s) {
    switch (S) {
        case 1: return launch_moments<TX, TY, 1>(x, y, g, channels, blocks, partial, s);
        case 2: return launch_moments<TX, TY, 2>(x, y, g, channels, blocks, partial, s);
        case 3: return launch_moments<TX, TY, 3>(x, y, g, channels, blocks, partial, s);
        case 4: return launch_moments<TX, TY, 4>(x, y, g, channels, blocks, partial, s);
        case 5: return launch_moments<TX, TY, 5>(x, y, g, channels, blocks, partial, s);
        case 6: return launch_moments<TX, TY, 6>(x, y, g, channels, blocks, partial, s);
        case 7: return launch_moments<TX, TY, 7>(x, y, g, channels, blocks, partial, s);
        default: return launch_moments<TX, TY, 8>(x, y, g, channels, blocks, partial, s);
    }
}

// tiles of the longest window of the call (the last one)
int64_t max_tiles(int W, int64_t n_samples) {
    const int64_t seg = n_samples / W;
    return cdiv(n_samples - (int64_t)(W - 1) * seg, GF_TILE);
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_gainfit_tile_samples(void) { return dam::GF_TILE; }

extern "C" int64_t dam_gainfit_workspace_bytes(int n_windows, int64_t n_samples, int n_stems) {
    if (n_windows < 1 || n_samples < n_windows || n_stems < 1 || n_stems > dam::GF_MAX_S) return 0;
    return (int64_t)n_windows * dam::max_tiles(n_windows, n_samples) * ((n_stems + 1) * (n_stems + 2) / 2) * (int64_t)sizeof(double);
}

extern "C" int dam_gainfit_moments(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                                   int64_t sample_stride, int64_t channel_stride, const void* y, int y_is_f64,
                                   int64_t y_sample_stride, int64_t y_channel_stride, int n_windows, double* moments,
                                   void* workspace, void* stream) {
    using namespace dam;
    if (!x || !y || !moments || !workspace) return DAM_ERR_BAD_ARG;
    if (n_stems < 1 || n_stems > GF_MAX_S || (channels != 1 && channels != 2)) return DAM_ERR_BAD_ARG;
    if (n_samples < 1 || n_windows < 1 || n_windows > n_samples) return DAM_ERR_BAD_ARG;
    GfGeo g;
    g.n_samples = n_samples; g.stem_stride = stem_stride; g.sample_stride = sample_stride; g.channel_stride = channel_stride;
    g.y_sample_stride = y_sample_stride; g.y_channel_stride = y_channel_stride;
    g.seg = n_samples / n_windows; g.W = n_windows;
    const int64_t tmax = max_tiles(n_windows, n_samples);
    if (tmax * n_windows > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    g.tmax = (int)tmax;
    const unsigned blocks = (unsigned)(tmax * n_windows);
    hipStream_t s = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    if (x_is_f64) {
        if (y_is_f64) dispatch_moments<double, double>(n_stems, x, y, g, channels, blocks, partial, s);
        else dispatch_moments<double, float>(n_stems, x, y, g, channels, blocks, partial, s);
    } else {
        if (y_is_f64) dispatch_moments<float, double>(n_stems, x, y, g, channels, blocks, partial, s);
        else dispatch_moments<float, float>(n_stems, x, y, g, channels, blocks, partial, s);
    }
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(gainfit_reduce_kernel, dim3((unsigned)n_windows), dim3(WAVE), 0, s, partial, g, n_stems, moments);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_gainfit_solve(const double* moments, int n_windows, int n_stems, int pool, double ridge, double* gains,
                                 double* residual, int32_t* status, void* stream) {
    using namespace dam;
    if (!moments || !gains || !residual || !status) return DAM_ERR_BAD_ARG;
    if (n_windows < 1 || n_stems < 1 || n_stems > GF_MAX_S || pool < 0 || !(ridge >= 0.0)) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(gainfit_solve_kernel, dim3((unsigned)n_windows), dim3(WAVE), 0, (hipStream_t)stream, moments, n_windows,
                       n_stems, pool, ridge, gains, residual, (double*)nullptr, status);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bandfit_solve_grouped(const double* moments, int n_groups, int n_windows, int n_stems, int pool, double ridge,
                                         double* gains, double* residual, double* target, int32_t* status, void* stream) {
    using namespace dam;
    if (!moments || !gains || !residual || !target || !status) return DAM_ERR_BAD_ARG;
    if (n_groups < 1 || n_windows < 1 || n_stems < 1 || n_stems > GF_MAX_S || pool < 0 || !(ridge >= 0.0)) return DAM_ERR_BAD_ARG;
    if ((int64_t)n_groups * n_windows > 0x7fffffff) return DAM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gainfit_solve_kernel, dim3((unsigned)((int64_t)n_groups * n_windows)), dim3(WAVE), 0, (hipStream_t)stream,
                       moments, n_windows, n_stems, pool, ridge, gains, residual, target, status);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_gainfit_gain_error(const double* fit, const double* cand, int n_variants, int n_stems, int n_windows,
                                      int n_cand, double* err, double* err_stem, int32_t* n_kept, void* stream) {
    using namespace dam;
    if (!fit || !cand || !err || !err_stem || !n_kept) return DAM_ERR_BAD_ARG;
    if (n_variants < 1 || n_windows < 1 || n_stems < 1 || n_stems > GF_MAX_S) return DAM_ERR_BAD_ARG;
    if (n_cand != 1 && n_cand != n_windows) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(gainfit_gain_error_kernel, dim3((unsigned)n_variants), dim3(WAVE), 0, (hipStream_t)stream, fit, cand,
                       n_stems, n_windows, n_cand, err, err_stem, n_kept);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
