// dam_bn.hip -- BatchNorm2d (training and eval mode) forward / backward on NHWC float32, HBM-bound kernels.
//
// Replaces nn.BatchNorm2d + F.relu (+ residual add) of models/model_resnet.py:12-27,65,97 (eps 1e-5,
// momentum 0.1) and models/model_scalar_1s.py:174-186 / model_scalar_2s.py:32-44 (eps 1e-3, momentum 0.9),
// including the running-statistics update and the autograd backward reached from model_trainer.py:36.
//
//   * statistics: every workgroup streams a contiguous pixel range with 16-byte loads (a thread owns 4
//     channels), keeps SHIFTED sums (x - K, K = first value seen) so that mean^2 >> var cannot cancel,
//     converts to (n, mean, M2) and the partials are merged with Chan's formula (in double in the finalize
//     kernel): deterministic, no atomics, matches a two-pass CPU BatchNorm;
//   * finalize also updates running_mean / running_var (unbiased) / num_batches_tracked exactly like
//     torch, and emits scale = gamma*invstd, shift = beta - mean*scale for the fused consumers
//     (bn_apply below, or the convolution kernels' load prologue);
//   * apply: y = relu?(x*scale + shift (+ r  or  + r*rscale + rshift))  -- the residual variant covers
//     both BasicBlock shortcuts (identity, or the shortcut conv's own BatchNorm folded in);
//   * backward: one reduction pass (sum dz, sum dz*xhat; dz = dy * (y > 0)) and one apply pass
//     dx = c1*dz + c2*x + c3 with per-channel constants.
#include <type_traits>
#include "dam_common.h"

namespace dam {
namespace {

constexpr int BN_MAX_PARTS = 1024;
static_assert(BN_MAX_PARTS == BN_BWD_RECORDS_MAX, "records a data-gradient epilogue may leave");

struct BnLaunch { int threads, q, r, parts; int64_t ppb; };

inline BnLaunch bn_plan(int64_t P, int C, int max_parts = BN_MAX_PARTS) {
    BnLaunch l;
    l.q = C / 4;
    l.r = 256 / l.q;
    if (l.r < 1) l.r = 1;
    l.threads = l.q * l.r;
    int64_t parts = cdiv(P, (int64_t)l.r * 16);          // ~16 pixels (two batches of 8 loads) per thread
    if (parts > max_parts) {
        // a consumer that merges the records itself wants few of them (fa_max_parts): the workgroups grow instead, so that the
        // pass still has >= 2048 waves to cover the memory latency (170 workgroups of 4 waves ran a 34 MB pair pass 8 us slower)
        parts = max_parts;
        while (l.threads < 1024 && parts * l.threads < 131072 && (size_t)(l.r * 2) * C * 3 * sizeof(float) <= 48 * 1024) {
            l.r *= 2;
            l.threads *= 2;
        }
    }
    if (parts < 1) parts = 1;
    l.ppb = cdiv(P, parts);
    l.parts = (int)cdiv(P, l.ppb);
    return l;
}

// The tail of every record producer: thread (cq, pr) holds NV values for each of its 4 channels; they go to LDS [R][C][NV], a
// tree merges the R pixel rows (all threads active; fixed order -> deterministic) and row 0 stores the workgroup's record
// [C][NV] (store_sc1: dam_common.h).  Merge::step(a, b) folds record b into record a.
struct RecAdd {
    template <int NV>
    static __device__ __forceinline__ void step(float* a, const float* b) {
#pragma unroll
        for (int k = 0; k < NV; ++k) a[k] += b[k];
    }
};
struct RecChan {        // (n, mean, M2) records
    template <int NV>
    static __device__ __forceinline__ void step(float* a, const float* b) {
        static_assert(NV == 3, "(n, mean, M2)");
        const float na = a[0], nb = b[0];
        if (nb != 0.f) {
            const float nn = na + nb, d = b[1] - a[1];
            a[1] += d * (nb / nn);
            a[2] += b[2] + d * d * (na * nb / nn);
            a[0] = nn;
        }
    }
};
template <int NV, typename Merge>
__device__ __forceinline__ void record_tail(float* sm, const float (&v)[NV][4], int C, int cq, int pr, int R,
                                            float* __restrict__ record /* this workgroup's [C][NV] */) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float* o = sm + ((size_t)pr * C + cq * 4 + i) * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = v[k][i];
    }
    __syncthreads();
    int span = 1;
    while (span < R) span <<= 1;
    for (int stride = span >> 1; stride >= 1; stride >>= 1) {
        if (pr < stride && pr + stride < R) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                Merge::template step<NV>(sm + ((size_t)pr * C + cq * 4 + i) * NV, sm + ((size_t)(pr + stride) * C + cq * 4 + i) * NV);
        }
        __syncthreads();
    }
    if (pr == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cq * 4 + i;
#pragma unroll
            for (int k = 0; k < NV; ++k) store_sc1(record + (size_t)c * NV + k, sm[(size_t)c * NV + k]);
        }
    }
}

// gridDim.y == 2: a second tensor of the same shape (x2 -> partial2) in the same launch (dam_bn_stats_pair_f32).
__global__ void bn_stats_partial_kernel(const float* __restrict__ x, int64_t P, int C, int Q, int R, int64_t ppb,
                                        float* __restrict__ partial /* [parts][C][3] */,
                                        const float* __restrict__ x2, float* __restrict__ partial2) {
    extern __shared__ __attribute__((aligned(16))) float sm[];    // [R][C][3]
    if (blockIdx.y) { x = x2; partial = partial2; }
    const int cq = threadIdx.x % Q, pr = threadIdx.x / Q;
    const int64_t lo = blockIdx.x * ppb, hi = (lo + ppb < P) ? lo + ppb : P;
    float k[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    int n = 0;
    constexpr int U = 8;      // loads in flight per thread: the kernel is a pure stream, latency must be covered by MLP
    for (int64_t p = lo + pr; p < hi; p += (int64_t)R * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t q = p + (int64_t)u * R;
            v[u] = q < hi ? *reinterpret_cast<const float4*>(x + q * C + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (n == 0) { k[0] = v[0].x; k[1] = v[0].y; k[2] = v[0].z; k[3] = v[0].w; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + (int64_t)u * R < hi) {
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = e[i] - k[i];
                    s1[i] += d;
                    s2[i] = fmaf(d, d, s2[i]);
                }
                ++n;
            }
        }
    }
    float v[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float md = n ? s1[i] / n : 0.f;
        v[0][i] = (float)n;
        v[1][i] = k[i] + md;
        v[2][i] = n ? fmaxf(s2[i] - s1[i] * md, 0.f) : 0.f;
    }
    record_tail<3, RecChan>(sm, v, C, cq, pr, R, partial + (size_t)blockIdx.x * C * 3);
}

// One wave per channel: lanes merge a strided subset of the partials (Chan), then a shuffle tree merges the lanes.
__global__ __launch_bounds__(64) void bn_stats_finalize_kernel(const float* __restrict__ partial, int parts, int C,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         float* __restrict__ running_mean, float* __restrict__ running_var,
                                         long long* __restrict__ num_batches, float momentum, float eps,
                                         float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                         float* __restrict__ scale, float* __restrict__ shift, const BnFinArgs second,
                                         const float* __restrict__ partial2) {
    if (blockIdx.y) {       // second BatchNorm of a pair launch
        partial = partial2; gamma = second.gamma; beta = second.beta; running_mean = second.running_mean;
        running_var = second.running_var; num_batches = second.num_batches; momentum = second.momentum; eps = second.eps;
        save_mean = second.save_mean; save_invstd = second.save_invstd; scale = second.scale; shift = second.shift;
    }
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c == 0 && lane == 0 && num_batches) *num_batches += 1;
    // the channel's parameters and running statistics are requested together with the records: read behind the reduction
    // (lane 0 only) they were a second memory round trip in a kernel that is nothing but round trips
    const float gam_c = gamma[c], bet_c = beta[c];
    const float rm_c = running_mean ? running_mean[c] : 0.f, rv_c = running_mean ? running_var[c] : 0.f;
    // Every lane requests ALL its records (<= 16: parts <= 1024) before it touches the first: the records come from other
    // XCDs' workgroups, each load is a memory-side round trip, and a load-merge-load chain made this 5 us kernel cost 5-7 us.
    // Merging is two plain wave reductions instead of a chain of Chan updates (no divide per record):
    //   N = sum n_i,  mu = sum n_i mean_i / N,  M2 = sum (m2_i + n_i (mean_i - mu)^2).
    constexpr int U = 16;
    float rn[U], rmn[U], rq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = lane + 64 * u;
        const float* o = partial + ((size_t)(p < parts ? p : 0) * C + c) * 3;
        rn[u] = o[0]; rmn[u] = o[1]; rq[u] = o[2];
        if (p >= parts) rn[u] = 0.f;
    }
    double na = 0, sa = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) { na += (double)rn[u]; sa += (double)rn[u] * (double)rmn[u]; }
    for (int p = lane + 64 * U; p < parts; p += 64) {        // more than 1024 records: not produced by this library
        const float* o = partial + ((size_t)p * C + c) * 3;
        na += (double)o[0]; sa += (double)o[0] * (double)o[1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { na += __shfl_xor(na, off); sa += __shfl_xor(sa, off); }
    const double ma = sa / na;
    double qa = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) { const double d = (double)rmn[u] - ma; qa += (double)rq[u] * (rn[u] != 0.f ? 1.0 : 0.0) + (double)rn[u] * d * d; }
    for (int p = lane + 64 * U; p < parts; p += 64) {
        const float* o = partial + ((size_t)p * C + c) * 3;
        const double d = (double)o[1] - ma;
        qa += (double)o[2] + (double)o[0] * d * d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) qa += __shfl_xor(qa, off);
    if (lane != 0) return;
    const double var = qa / na;
    const float mean = (float)ma;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    const float sc = gam_c * invstd;
    scale[c] = sc;
    shift[c] = bet_c - mean * sc;
    if (running_mean) {
        const double unbiased = na > 1 ? qa / (na - 1) : var;
        running_mean[c] = (1.f - momentum) * rm_c + momentum * mean;
        running_var[c] = (1.f - momentum) * rv_c + momentum * (float)unbiased;
    }
}

__global__ void bn_eval_affine_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                      float eps, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                      float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float invstd = 1.0f / sqrtf(running_var[c] + eps);
    const float sc = gamma[c] * invstd;
    save_mean[c] = running_mean[c];
    save_invstd[c] = invstd;
    scale[c] = sc;
    shift[c] = beta[c] - running_mean[c] * sc;
}

__global__ void bn_apply_kernel(const float* __restrict__ x, int64_t nquads, int Q, const float* __restrict__ scale,
                                const float* __restrict__ shift, const float* __restrict__ res,
                                const float* __restrict__ rscale, const float* __restrict__ rshift, int relu,
                                float* __restrict__ y, unsigned char* __restrict__ sign_bits) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nquads; e += (int64_t)gridDim.x * blockDim.x) {
        const int cq = (int)(e % Q);
        const float4 v = reinterpret_cast<const float4*>(x)[e];
        const float4 sc = reinterpret_cast<const float4*>(scale)[cq], sh = reinterpret_cast<const float4*>(shift)[cq];
        float4 o = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
        if (res) {
            float4 r = reinterpret_cast<const float4*>(res)[e];
            if (rscale) {
                const float4 a = reinterpret_cast<const float4*>(rscale)[cq], b = reinterpret_cast<const float4*>(rshift)[cq];
                r = make_float4(fmaf(r.x, a.x, b.x), fmaf(r.y, a.y, b.y), fmaf(r.z, a.z, b.z), fmaf(r.w, a.w, b.w));
            }
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        reinterpret_cast<float4*>(y)[e] = o;
        // one byte per channel quad: bit i = (y[4e + i] > 0) -- the ReLU mask the backward passes want, 1/16 of the bytes of y
        if (sign_bits) sign_bits[e] = (unsigned char)((o.x > 0.f) | ((o.y > 0.f) << 1) | ((o.z > 0.f) << 2) | ((o.w > 0.f) << 3));
    }
}

__device__ __forceinline__ float4 sign_quad(unsigned b) {       // sign byte -> (1 or 0) x 4
    return make_float4((float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)((b >> 3) & 1u));
}

// ---- backward.  One family for NB = 1 BatchNorm, or NB = 2 that share dy and the ReLU mask (a residual block's bn2 and its
// shortcut BatchNorm, both fed by the block's output gradient): dy and the mask are read once per pass instead of twice, two
// launches instead of four.  Same sums in the same order for either NB: the pair is bitwise two single calls.
struct BnBwdSide {            // one BatchNorm of a backward launch (device pointers)
    const float* x;
    const float* gamma;
    const float* mean;
    const float* invstd;
    float* dx;
    float* dgamma;
    float* dbeta;
};
template <int NB>
struct BnBwdSides { BnBwdSide s[NB]; };

// partial[blk][c] = (sum dz, sum dz*xhat of every side)
// MASK: 3 = from the sign bytes written by bn_apply (one byte per channel quad: y_mask then points at bytes);
// MASK: 0 none, 1 from y_mask (saved output), 2 recomputed as fma(x, mscale, mshift) > 0 -- the forward's own expression, so
// the bits agree and the saved activation is not read at all (NB = 1 only: the pair's mask is the block output's, 1 or 3)
template <int MASK, int NB>
__global__ void bn_bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ y_mask, const BnBwdSides<NB> sd,
                                      int64_t P, int C, int Q, int R, int64_t ppb, const float* __restrict__ mscale,
                                      const float* __restrict__ mshift, float* __restrict__ partial /* [parts][C][1 + NB] */) {
    extern __shared__ __attribute__((aligned(16))) float sm[];    // [R][C][1 + NB]
    const int cq = threadIdx.x % Q, pr = threadIdx.x / Q;
    const int64_t lo = blockIdx.x * ppb, hi = (lo + ppb < P) ? lo + ppb : P;
    float4 mu[NB], is[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        mu[s] = reinterpret_cast<const float4*>(sd.s[s].mean)[cq];
        is[s] = reinterpret_cast<const float4*>(sd.s[s].invstd)[cq];
    }
    float4 msc = make_float4(0.f, 0.f, 0.f, 0.f), msh = msc;
    if (MASK == 2) { msc = reinterpret_cast<const float4*>(mscale)[cq]; msh = reinterpret_cast<const float4*>(mshift)[cq]; }
    float acc[1 + NB][4] = {};      // [0]: sum dz, [1 + s]: sum dz * xhat of side s
    // 12 loads in flight per thread: 3 streams x 4 pieces for one BatchNorm, 4 x 3 for a pair.  With 4 x 4 the pair needs more than
    // the 128 registers a kernel without launch bounds gets, and every form of it spilled addresses inside this loop (a reload
    // waits for all the loads requested before it): 17 - 18 us per launch of the C3 step against 14.4 us for this one
    // (profiles/r06_bn_pair_kernel_variants.txt).  A thread adds its pixels in the same order for any U.
    constexpr int U = NB == 1 ? 4 : 3;
    for (int64_t p = lo + pr; p < hi; p += (int64_t)R * U) {
        float4 gv[U], mv[U], xv[NB][U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t q = p + (int64_t)u * R;
            const bool ok = q < hi;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            // `if (ok)` around the loads, not `ok ? *p : z` per stream: the compiler turns that form into a select between p
            // and a copy of z in scratch (32 bytes per lane for one BatchNorm, 80 - 96 for two, and 87 registers without a mask:
            // five waves per SIMD where this form has six; profiles/r06_dam_bn_resource_usage_*.txt)
            gv[u] = z; mv[u] = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
            for (int s = 0; s < NB; ++s) xv[s][u] = z;
            if (ok) {
                gv[u] = *reinterpret_cast<const float4*>(dy + q * C + cq * 4);
#pragma unroll
                for (int s = 0; s < NB; ++s) xv[s][u] = *reinterpret_cast<const float4*>(sd.s[s].x + q * C + cq * 4);
                if (MASK == 1) mv[u] = *reinterpret_cast<const float4*>(y_mask + q * C + cq * 4);
            }
            if (MASK == 3) mv[u] = sign_quad(ok ? reinterpret_cast<const unsigned char*>(y_mask)[q * Q + cq] : 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 g = gv[u];
            float4 m = mv[u];
            if (MASK == 2) {
                const float4 v = xv[0][u];
                m = make_float4(fmaf(v.x, msc.x, msh.x), fmaf(v.y, msc.y, msh.y), fmaf(v.z, msc.z, msh.z), fmaf(v.w, msc.w, msh.w));
            }
            g.x = m.x > 0.f ? g.x : 0.f; g.y = m.y > 0.f ? g.y : 0.f; g.z = m.z > 0.f ? g.z : 0.f; g.w = m.w > 0.f ? g.w : 0.f;
            acc[0][0] += g.x; acc[0][1] += g.y; acc[0][2] += g.z; acc[0][3] += g.w;
#pragma unroll
            for (int s = 0; s < NB; ++s) {
                const float4 v = xv[s][u];
                float* b = acc[1 + s];
                b[0] = fmaf(g.x, (v.x - mu[s].x) * is[s].x, b[0]); b[1] = fmaf(g.y, (v.y - mu[s].y) * is[s].y, b[1]);
                b[2] = fmaf(g.z, (v.z - mu[s].z) * is[s].z, b[2]); b[3] = fmaf(g.w, (v.w - mu[s].w) * is[s].w, b[3]);
            }
        }
    }
    record_tail<1 + NB, RecAdd>(sm, acc, C, cq, pr, R, partial + (size_t)blockIdx.x * C * (1 + NB));
}

__device__ __forceinline__ double wave_sum64_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// One wave per channel sums NV record columns [parts][C][NV] in double: lane 0 ends up with the totals in s[].  Every lane
// requests ALL its records (<= 16: parts <= 1024) before the first add (see bn_stats_finalize_kernel).
template <int NV>
__device__ __forceinline__ void wave_record_sums(const float* __restrict__ partial, int parts, int C, int c, double (&s)[NV]) {
    const int lane = threadIdx.x;
    constexpr int U = 16;
    float r[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int p = lane + 64 * u;
        const float* o = partial + ((size_t)(p < parts ? p : 0) * C + c) * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) r[u][k] = p < parts ? o[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] = 0;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < NV; ++k) s[k] += (double)r[u][k];
    for (int p = lane + 64 * U; p < parts; p += 64)        // more than 1024 records: not produced by this library
#pragma unroll
        for (int k = 0; k < NV; ++k) s[k] += partial[((size_t)p * C + c) * NV + k];
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] = wave_sum64_f64(s[k]);
}

// One wave per channel.
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int parts, int C, double count,
                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ invstd, int training, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ coef /* [3][C] */) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const float gam_c = gamma[c], inv_c = invstd[c], mean_c = mean[c];      // (requested with the records, see bn_stats_finalize_kernel)
    double s[2];
    wave_record_sums<2>(partial, parts, C, c, s);
    if (lane != 0) return;
    const double s1 = s[0], s2 = s[1];
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
    const double g = (double)gam_c * inv_c;
    double c2 = 0, c3 = 0;
    if (training) {
        c2 = -g * inv_c * s2 / count;
        c3 = -g * s1 / count - c2 * mean_c;
    }
    coef[c] = (float)g; coef[C + c] = (float)c2; coef[2 * C + c] = (float)c3;
}

template <int MASK>
__global__ void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ y_mask,
                                    const float* __restrict__ x, int64_t nquads, int Q, int C,
                                    const float* __restrict__ coef, const float* __restrict__ mscale,
                                    const float* __restrict__ mshift, float* __restrict__ dx) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nquads; e += (int64_t)gridDim.x * blockDim.x) {
        const int cq = (int)(e % Q);
        float4 g = reinterpret_cast<const float4*>(dy)[e];
        const float4 v = reinterpret_cast<const float4*>(x)[e];
        if (MASK != 0) {
            float4 m;
            if (MASK == 1) {
                m = reinterpret_cast<const float4*>(y_mask)[e];
            } else if (MASK == 3) {
                m = sign_quad(reinterpret_cast<const unsigned char*>(y_mask)[e]);
            } else {
                const float4 sc = reinterpret_cast<const float4*>(mscale)[cq], sh = reinterpret_cast<const float4*>(mshift)[cq];
                m = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
            }
            g.x = m.x > 0.f ? g.x : 0.f; g.y = m.y > 0.f ? g.y : 0.f; g.z = m.z > 0.f ? g.z : 0.f; g.w = m.w > 0.f ? g.w : 0.f;
        }
        const float4 c1 = reinterpret_cast<const float4*>(coef)[cq], c2 = reinterpret_cast<const float4*>(coef + C)[cq],
                     c3 = reinterpret_cast<const float4*>(coef + 2 * C)[cq];
        float4 o;
        o.x = fmaf(c1.x, g.x, fmaf(c2.x, v.x, c3.x)); o.y = fmaf(c1.y, g.y, fmaf(c2.y, v.y, c3.y));
        o.z = fmaf(c1.z, g.z, fmaf(c2.z, v.z, c3.z)); o.w = fmaf(c1.w, g.w, fmaf(c2.w, v.w, c3.w));
        reinterpret_cast<float4*>(dx)[e] = o;
    }
}

// out[c] = sum over pixels of x[p][c] (conv bias gradient); reuses the bwd partial layout with one column.
__global__ void channel_sum_partial_kernel(const float* __restrict__ x, int64_t P, int C, int Q, int R, int64_t ppb,
                                           float* __restrict__ partial) {
    extern __shared__ float sm[];
    const int cq = threadIdx.x % Q, pr = threadIdx.x / Q;
    const int64_t lo = blockIdx.x * ppb, hi = (lo + ppb < P) ? lo + ppb : P;
    float a[1][4] = {};
    constexpr int U = 8;
    for (int64_t p = lo + pr; p < hi; p += (int64_t)R * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t q = p + (int64_t)u * R;
            v[u] = q < hi ? *reinterpret_cast<const float4*>(x + q * C + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { a[0][0] += v[u].x; a[0][1] += v[u].y; a[0][2] += v[u].z; a[0][3] += v[u].w; }
    }
    record_tail<1, RecAdd>(sm, a, C, cq, pr, R, partial + (size_t)blockIdx.x * C);
}
__global__ __launch_bounds__(64) void channel_sum_finalize_kernel(const float* __restrict__ partial, int parts, int C, int n_real,
                                            float* __restrict__ out) {
    double s[1];
    wave_record_sums<1>(partial, parts, C, blockIdx.x, s);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)s[0];
}

// ================================================================================================================================
// Finalize INSIDE the elementwise consumer (round 4).  A finalize launch is 4.6-5 us whatever it does and a ResNet18 step had fifty of
// them; round 3's attempt to merge the records in every workgroup of the 4096-workgroup apply launches lost to the table traffic
// (every workgroup re-read every channel's records: ~6 M cache-line requests per launch).  What makes it pay:
//   * the grid is what the chip holds (<= 512 workgroups), each workgroup walks a contiguous pixel range, and
//   * a workgroup only merges the channels it applies: workgroup (slice, range) owns CS = 16 or 32 channels, so its table is
//     parts x CS records (<= ~100 KB, usually 20-60), requested in one burst behind the workgroup's first data loads;
//   * the merge is one pass in double around a pivot (record 0's mean): N = sum n, S = sum n (mean - m0),
//     Q = sum (M2 + n (mean - m0)^2); mean = m0 + S / N, M2 = Q - S^2 / N -- the shifted-data form of the pooled variance, exact to
//     double rounding (no Chan chain, no second pass over the records);
//   * range 0 of every slice writes what later kernels read (save_mean, save_invstd, scale, shift, the running statistics;
//     dgamma / dbeta in the backward form).
// The records' producers ran in earlier launches (the kernel boundary is the synchronisation), so plain loads are fine.
// ================================================================================================================================
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
constexpr int FA_THREADS = 256;
constexpr int FA_U = 4;                 // pixel pieces per thread, stream and register set (two sets: the next batch's loads are
                                        // requested before the current batch is computed and stored)

// grid of the fused launches: at most this many workgroups over all slices
constexpr int FA_WGS = 512;

struct FaPlan { int cs, nslices, nranges, q, ppi; int64_t ppr; };

// CS: the whole row for thin layers (one 128-byte line per pixel at 32 channels), 16-channel slices above that (64-byte pieces:
// the wide layers' tensors are small and L2 resident; what matters there is the table a workgroup has to merge)
inline int fa_cs(int C) { return C <= 32 ? C : 16; }
inline FaPlan fa_plan(int64_t P, int C) {
    FaPlan f;
    f.cs = fa_cs(C);
    f.nslices = C / f.cs;
    f.q = f.cs / 4;
    f.ppi = FA_THREADS / f.q;
    int64_t want = P / ((int64_t)f.ppi * FA_U * 2);       // >= two batches of loads per thread
    const int64_t cap = FA_WGS / f.nslices > 0 ? FA_WGS / f.nslices : 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    f.ppr = cdiv(P, want);
    f.nranges = (int)cdiv(P, f.ppr);
    return f;
}
// a slice table beyond this costs a workgroup more to read than the finalize launch it replaces (measured: 110 KB tables made the
// 129 x 17 stage's fused launch 5 us slower than finalize + apply, 74 KB ones broke even)
constexpr int FA_TABLE_BYTES_MAX = 80 * 1024;
inline bool fa_table_ok(int C, int parts, int rec_floats) { return (int64_t)parts * fa_cs(C) * rec_floats * 4 <= FA_TABLE_BYTES_MAX; }
// The FORWARD form pays more per record (12 bytes, a divide-free but longer merge, sqrt) and its launches on the full-resolution
// stages measured 2-3 us SLOWER than finalize + apply (48 KB tables x 512 workgroups = 24 MB of table reads in front of a 35 us
// stream), the small stages' about equal: it is taken only for tables up to FA_FWD_TABLE_KB KB per workgroup --
// the backward forms win 1.5-2.5 us per launch on every stage and are taken up to FA_TABLE_BYTES_MAX.
constexpr int FA_FWD_TABLE_KB = 24;
inline bool fa_fwd_table_ok(int C, int parts) {
    return fa_table_ok(C, parts, 3) && (int64_t)parts * fa_cs(C) * 12 <= (int64_t)FA_FWD_TABLE_KB * 1024;
}

// Sums NV per-record values over the slice's records: thread (c = tid % CS, i = tid / CS) takes records i, i + TPC, ...; every
// record of a thread is requested before the first is used (<= 16 per thread and round: one round trip for tables up to 256
// records of 16 channels); tid < CS ends up with the channel's totals in acc[].  `term(rec, v)`: one record (NR floats) -> NV addends.
template <int NR, int NV, typename F>
__device__ __forceinline__ void fa_slice_sums(const float* __restrict__ partial, int parts, int C, int ch, int CS, double* red,
                                              double (&acc)[NV], F term) {
    const int tid = threadIdx.x, TPC = FA_THREADS / CS, i0 = tid / CS;
    constexpr int RU = 16;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0;
    for (int p0 = i0; p0 < parts; p0 += TPC * RU) {
        float rec[RU][NR];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int p = p0 + u * TPC;
            const float* o = partial + ((size_t)(p < parts ? p : i0) * C + ch) * NR;
#pragma unroll
            for (int k = 0; k < NR; ++k) rec[u][k] = o[k];
        }
#pragma unroll
        for (int u = 0; u < RU; ++u)
            if (p0 + u * TPC < parts) {
                double v[NV];
                term(rec[u], v);
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += v[k];
            }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) red[tid * NV + k] = acc[k];
    __syncthreads();
    if (tid < CS)
        for (int i = 1; i < TPC; ++i)
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] += red[(tid + i * CS) * NV + k];
}

// The fused kernels' stream over a workgroup's pixel range.  Two register sets alternate: load(set, p0) requests a batch,
// emit(set, p0) computes and stores it.  The set is a type (FaSet<0> / FaSet<1>), so that it indexes the callers' register
// arrays as a compile-time constant and both sets stay in registers.  The caller has already requested set 0 at p0.
template <int S> using FaSet = std::integral_constant<int, S>;
template <typename Load, typename Emit>
__device__ __forceinline__ void fa_stream(int64_t p0, int64_t hi, int64_t step, Load load, Emit emit) {
    for (;;) {
        if (p0 + step < hi) load(FaSet<1>{}, p0 + step);
        emit(FaSet<0>{}, p0);
        p0 += step;
        if (p0 >= hi) break;
        if (p0 + step < hi) load(FaSet<0>{}, p0 + step);
        emit(FaSet<1>{}, p0);
        p0 += step;
        if (p0 >= hi) break;
    }
}

__global__ __launch_bounds__(FA_THREADS) void bn_fin_apply_kernel(const float* __restrict__ partial, int parts, int C, int CS,
                                                                   const BnFinArgs fin, const float* __restrict__ x, int64_t P,
                                                                   int64_t ppr, const float* __restrict__ res,
                                                                   const float* __restrict__ rscale, const float* __restrict__ rshift,
                                                                   int relu, float* __restrict__ y, unsigned char* __restrict__ sign_bits) {
    __shared__ double red[FA_THREADS * 3];
    __shared__ __attribute__((aligned(16))) float tab[2 * 32];
    const int tid = threadIdx.x, slice = blockIdx.y, q = CS / 4, tq = tid % q, tp = tid / q, ppi = FA_THREADS / q;
    const int Q = C / 4, cq = slice * q + tq;
    const int64_t lo = blockIdx.x * ppr, hi = (lo + ppr < P) ? lo + ppr : P;
    const int64_t step = (int64_t)ppi * FA_U;
    float4 xv[2][FA_U], rv[2][FA_U];
    auto load = [&](auto set, int64_t p0) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int u = 0; u < FA_U; ++u) {
            const int64_t p = p0 + (int64_t)u * ppi;
            xv[S][u] = p < hi ? reinterpret_cast<const float4*>(x)[p * Q + cq] : zero4();
            if (res) rv[S][u] = p < hi ? reinterpret_cast<const float4*>(res)[p * Q + cq] : zero4();
        }
    };
    // the first pieces are requested before the records: the table's round trip hides behind them
    load(FaSet<0>{}, lo + tp);
    float4 ra = make_float4(1.f, 1.f, 1.f, 1.f), rb = zero4();
    if (rscale) { ra = reinterpret_cast<const float4*>(rscale)[cq]; rb = reinterpret_cast<const float4*>(rshift)[cq]; }
    {
        const int cl = tid % CS, ch = slice * CS + cl;
        const float m0 = partial[(size_t)ch * 3 + 1];
        const float gam = fin.gamma[ch], bet = fin.beta[ch];
        const bool writer = blockIdx.x == 0 && tid < CS;
        const float rm = (writer && fin.running_mean) ? fin.running_mean[ch] : 0.f, rvv = (writer && fin.running_mean) ? fin.running_var[ch] : 0.f;
        double acc[3];
        fa_slice_sums<3, 3>(partial, parts, C, ch, CS, red, acc, [m0](const float (&r)[3], double (&v)[3]) {
            const double n = (double)r[0], d = (double)r[1] - (double)m0;
            v[0] = n; v[1] = n * d; v[2] = n != 0.0 ? (double)r[2] + n * d * d : 0.0;
        });
        if (tid < CS) {
            const double na = acc[0], ds = acc[1] / na, qa = acc[2] - acc[1] * ds;
            const double var = qa / na;
            const float mean = (float)((double)m0 + ds);
            const float invstd = (float)(1.0 / sqrt((var > 0 ? var : 0.0) + (double)fin.eps));
            const float sc = gam * invstd, sh = bet - mean * sc;
            tab[cl] = sc; tab[CS + cl] = sh;
            if (writer) {
                fin.save_mean[ch] = mean; fin.save_invstd[ch] = invstd; fin.scale[ch] = sc; fin.shift[ch] = sh;
                if (fin.running_mean) {
                    const double unbiased = na > 1 ? (qa > 0 ? qa : 0.0) / (na - 1) : var;
                    fin.running_mean[ch] = (1.f - fin.momentum) * rm + fin.momentum * mean;
                    fin.running_var[ch] = (1.f - fin.momentum) * rvv + fin.momentum * (float)unbiased;
                }
                if (ch == 0 && fin.num_batches) *fin.num_batches += 1;
            }
        }
        __syncthreads();
    }
    const float4 sc = *reinterpret_cast<const float4*>(tab + tq * 4), sh = *reinterpret_cast<const float4*>(tab + CS + tq * 4);
    fa_stream(lo + tp, hi, step, load, [&](auto set, int64_t p0) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int u = 0; u < FA_U; ++u) {
            const int64_t p = p0 + (int64_t)u * ppi;
            if (p < hi) {
                const float4 v = xv[S][u];
                float4 o = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
                if (res) {
                    float4 r = rv[S][u];
                    if (rscale) r = make_float4(fmaf(r.x, ra.x, rb.x), fmaf(r.y, ra.y, rb.y), fmaf(r.z, ra.z, rb.z), fmaf(r.w, ra.w, rb.w));
                    o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
                }
                if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                reinterpret_cast<float4*>(y)[p * Q + cq] = o;
                if (sign_bits)
                    sign_bits[p * Q + cq] = (unsigned char)((o.x > 0.f) | ((o.y > 0.f) << 1) | ((o.z > 0.f) << 2) | ((o.w > 0.f) << 3));
            }
        }
    });
}

// The backward merge of one channel slice: records [parts][C][1 + NB] -> tab [NB][3][CS] = c1, c2, c3 of every side, and (where
// `write_grads`) dgamma / dbeta.  One body for the fused launch's prologue and the finalize-only launch: the same sums in the
// same order, so the two give the same bits.  The caller synchronises before it reads tab.
template <int NB>
__device__ __forceinline__ void bn_bwd_merge_slice(const float* __restrict__ partial, int parts, int C, int CS, int slice, double count,
                                                   int training, const BnBwdSides<NB>& sd, double* red, float* tab, bool write_grads) {
    constexpr int NR = 1 + NB;
    const int tid = threadIdx.x;
    const int cl = tid % CS, ch = slice * CS + cl;
    float gam[NB], inv[NB], mu[NB];
#pragma unroll
    for (int s = 0; s < NB; ++s) { gam[s] = sd.s[s].gamma[ch]; inv[s] = sd.s[s].invstd[ch]; mu[s] = sd.s[s].mean[ch]; }
    double acc[NR];
    fa_slice_sums<NR, NR>(partial, parts, C, ch, CS, red, acc, [](const float (&r)[NR], double (&v)[NR]) {
#pragma unroll
        for (int k = 0; k < NR; ++k) v[k] = (double)r[k];
    });
    if (tid < CS) {
#pragma unroll
        for (int s = 0; s < NB; ++s) {
            const double s1 = acc[0], s2 = acc[1 + s];
            const double g = (double)gam[s] * inv[s];
            double c2 = 0, c3 = 0;
            if (training) { c2 = -g * inv[s] * s2 / count; c3 = -g * s1 / count - c2 * mu[s]; }
            float* t = tab + 3 * s * CS;
            t[cl] = (float)g; t[CS + cl] = (float)c2; t[2 * CS + cl] = (float)c3;
            if (write_grads) { sd.s[s].dbeta[ch] = (float)s1; sd.s[s].dgamma[ch] = (float)s2; }
        }
    }
}

// Finalize only: one workgroup per channel slice runs the fused launch's merge and leaves coef [3][C] = c1, c2, c3 for a consumer
// that applies dx = c1 dz + c2 x + c3 itself (the strip kernel's row loaders, dam_conv_strip.hip: BNF).
__global__ __launch_bounds__(FA_THREADS) void bn_bwd_fin_only_kernel(const float* __restrict__ partial, int parts, int C, int CS,
                                                                      double count, int training, const BnBwdSides<1> sd,
                                                                      float* __restrict__ coef) {
    __shared__ double red[FA_THREADS * 2];
    __shared__ __attribute__((aligned(16))) float tab[3 * 32];
    bn_bwd_merge_slice<1>(partial, parts, C, CS, blockIdx.x, count, training, sd, red, tab, true);
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < 3 * CS) coef[(tid / CS) * C + blockIdx.x * CS + tid % CS] = tab[tid];
}

// Backward: records [parts][C][1 + NB] = (sum dz, sum dz * xhat of every side) -> dgamma / dbeta (range 0 writes them) and
// dx = c1 dz + c2 x + c3 per side.
template <int MASK, int NB>
__global__ __launch_bounds__(FA_THREADS) void bn_bwd_fin_apply_kernel(const float* __restrict__ partial, int parts, int C, int CS,
                                                                       double count, int training, const BnBwdSides<NB> sd,
                                                                       const float* __restrict__ dy, const float* __restrict__ y_mask,
                                                                       int64_t P, int64_t ppr, const float* __restrict__ mscale,
                                                                       const float* __restrict__ mshift) {
    constexpr int NR = 1 + NB;
    __shared__ double red[FA_THREADS * NR];
    __shared__ __attribute__((aligned(16))) float tab[3 * NB * 32];       // [NB][3][CS]: c1, c2, c3 of every side
    const int tid = threadIdx.x, slice = blockIdx.y, q = CS / 4, tq = tid % q, tp = tid / q, ppi = FA_THREADS / q;
    const int Q = C / 4, cq = slice * q + tq;
    const int64_t lo = blockIdx.x * ppr, hi = (lo + ppr < P) ? lo + ppr : P;
    constexpr int UB = NB == 1 ? 3 : 2;         // 2 + NB streams: three (one BatchNorm) or two (a pair) pieces each per register set
    const int64_t step = (int64_t)ppi * UB;
    float4 gv[2][UB], xv[NB][2][UB], mv[2][UB];
    auto load = [&](auto set, int64_t p0) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int64_t p = p0 + (int64_t)u * ppi;
            const bool ok = p < hi;
            gv[S][u] = ok ? reinterpret_cast<const float4*>(dy)[p * Q + cq] : zero4();
#pragma unroll
            for (int s = 0; s < NB; ++s) xv[s][S][u] = ok ? reinterpret_cast<const float4*>(sd.s[s].x)[p * Q + cq] : zero4();
            if (MASK == 1) mv[S][u] = ok ? reinterpret_cast<const float4*>(y_mask)[p * Q + cq] : zero4();
            if (MASK == 3) mv[S][u] = sign_quad(ok ? reinterpret_cast<const unsigned char*>(y_mask)[p * Q + cq] : 0);
        }
    };
    load(FaSet<0>{}, lo + tp);
    float4 msc = zero4(), msh = zero4();
    if (MASK == 2) { msc = reinterpret_cast<const float4*>(mscale)[cq]; msh = reinterpret_cast<const float4*>(mshift)[cq]; }
    bn_bwd_merge_slice<NB>(partial, parts, C, CS, slice, count, training, sd, red, tab, blockIdx.x == 0);
    __syncthreads();
    float4 k[NB][3];
#pragma unroll
    for (int i = 0; i < 3 * NB; ++i) k[i / 3][i % 3] = *reinterpret_cast<const float4*>(tab + i * CS + tq * 4);
    fa_stream(lo + tp, hi, step, load, [&](auto set, int64_t p0) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int64_t p = p0 + (int64_t)u * ppi;
            if (p < hi) {
                float4 g = gv[S][u];
                if (MASK != 0) {
                    float4 m = mv[S][u];
                    if (MASK == 2) {
                        const float4 v = xv[0][S][u];
                        m = make_float4(fmaf(v.x, msc.x, msh.x), fmaf(v.y, msc.y, msh.y), fmaf(v.z, msc.z, msh.z), fmaf(v.w, msc.w, msh.w));
                    }
                    g.x = m.x > 0.f ? g.x : 0.f; g.y = m.y > 0.f ? g.y : 0.f; g.z = m.z > 0.f ? g.z : 0.f; g.w = m.w > 0.f ? g.w : 0.f;
                }
                float4 o[NB];
#pragma unroll
                for (int s = 0; s < NB; ++s) {
                    const float4 v = xv[s][S][u], c1 = k[s][0], c2 = k[s][1], c3 = k[s][2];
                    o[s].x = fmaf(c1.x, g.x, fmaf(c2.x, v.x, c3.x)); o[s].y = fmaf(c1.y, g.y, fmaf(c2.y, v.y, c3.y));
                    o[s].z = fmaf(c1.z, g.z, fmaf(c2.z, v.z, c3.z)); o[s].w = fmaf(c1.w, g.w, fmaf(c2.w, v.w, c3.w));
                }
#pragma unroll
                for (int s = 0; s < NB; ++s) reinterpret_cast<float4*>(sd.s[s].dx)[p * Q + cq] = o[s];
            }
        }
    });
}

inline int elt_blocks(int64_t n) {
    int64_t b = cdiv(n, 256);
    return (int)(b < 4096 ? (b < 1 ? 1 : b) : 4096);
}

// records a partial pass may leave for a fused consumer: a workgroup's slice table stays <= FA_PARTS_KB KB
constexpr int FA_PARTS_KB = 64;
inline int fa_max_parts(int C, int rec_floats) {
    int m = FA_PARTS_KB * 1024 / (fa_cs(C) * rec_floats * 4);
    if (m > BN_MAX_PARTS) m = BN_MAX_PARTS;
    return m < 64 ? 64 : m;
}

// dam_bn_fin (include/dam_hip.h) -> the kernels' BnFinArgs; false where the struct or one of its required pointers is missing
inline bool fin_args(const dam_bn_fin* f, BnFinArgs* a) {
    if (!f || !f->gamma || !f->beta || !f->save_mean || !f->save_invstd || !f->scale || !f->shift) return false;
    *a = BnFinArgs{f->gamma, f->beta, f->running_mean, f->running_var, (long long*)f->num_batches_tracked, f->momentum,
                   f->eps, f->save_mean, f->save_invstd, f->scale, f->shift};
    return true;
}

// The run-time mask mode as a template argument: calls f(std::integral_constant<int, M>) for the M of MASKS... that equals mask;
// false (and no call) where none does.
template <int... MASKS, typename F>
inline bool with_mask(int mask, F f) {
    return ((mask == MASKS ? (f(std::integral_constant<int, MASKS>{}), true) : false) || ...);
}

// The backward launches of NB BatchNorms in the mask modes MASKS...: the partial pass (unless the records are given) and, where
// `fused`, the finalize inside the apply launch.  Given records that are not fused launch nothing here: the caller
// (dam_bn_backward_f32) then runs the finalize and apply launches of its own.
template <int NB, int... MASKS>
inline int bn_bwd_launch(const BnLaunch& l, bool given, bool fused, int mask, const BnBwdSides<NB>& sd, const float* dy,
                         const float* y_mask, int64_t P, int C, int training, const float* mask_scale, const float* mask_shift,
                         float* workspace, hipStream_t st) {
    if (!given) {
        const bool known = with_mask<MASKS...>(mask, [&](auto m) {
            hipLaunchKernelGGL((bn_bwd_partial_kernel<decltype(m)::value, NB>), dim3(l.parts), dim3(l.threads),
                               (size_t)l.r * C * (1 + NB) * sizeof(float), st, dy, y_mask, sd, P, C, l.q, l.r, l.ppb, mask_scale,
                               mask_shift, workspace);
        });
        if (!known) return DAM_ERR_BAD_ARG;
        DAM_CHECK_LAUNCH();
    }
    if (fused) {
        const FaPlan f = fa_plan(P, C);
        const bool known = with_mask<MASKS...>(mask, [&](auto m) {
            hipLaunchKernelGGL((bn_bwd_fin_apply_kernel<decltype(m)::value, NB>), dim3(f.nranges, f.nslices), dim3(FA_THREADS), 0, st,
                               (const float*)workspace, l.parts, C, f.cs, (double)P, training, sd, dy, y_mask, P, f.ppr, mask_scale,
                               mask_shift);
        });
        if (!known) return DAM_ERR_BAD_ARG;
        DAM_CHECK_LAUNCH();
    }
    return DAM_OK;
}

}  // namespace
}  // namespace dam

using namespace dam;

extern "C" int64_t dam_bn_workspace_floats(int C) { return (int64_t)BN_RECORDS_MAX * C * 3; }

// First half of dam_bn_stats_f32 on its own: the partial records [*parts_host][C][3], sized for a fused consumer
// (dam_bn_finalize_apply_f32) -- or for dam_bn_finalize_f32.
extern "C" int dam_bn_stats_partial_f32(const float* x, int64_t n_pixels, int C, float* workspace, int* parts_host, void* stream) {
    if (!x || !workspace || !parts_host || n_pixels <= 0) return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    const BnLaunch l = bn_plan(n_pixels, C, fa_max_parts(C, 3));
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(l.parts), dim3(l.threads), (size_t)l.r * C * 3 * sizeof(float), (hipStream_t)stream,
                       x, n_pixels, C, l.q, l.r, l.ppb, workspace, (const float*)nullptr, (float*)nullptr);
    DAM_CHECK_LAUNCH();
    *parts_host = l.parts;
    return DAM_OK;
}

// Finalize + apply in one launch: merges `parts` records [parts][C][3] (a convolution epilogue's, dam_bn_stats_partial_f32's)
// exactly as dam_bn_finalize_f32 does -- fin's outputs and running statistics are written -- and applies
// y = relu?(x * scale + shift [+ res [* res_scale + res_shift]]) [+ sign bytes] as dam_bn_apply_f32 does.
extern "C" int dam_bn_finalize_apply_f32(const float* partial, int parts, int C, const dam_bn_fin* fin, const float* x,
                                         int64_t n_pixels, const float* res, const float* res_scale, const float* res_shift,
                                         int relu, float* y, uint8_t* sign_bits, void* stream) {
    BnFinArgs a;
    if (!partial || parts <= 0 || !fin_args(fin, &a) || !x || !y || n_pixels <= 0) return DAM_ERR_BAD_ARG;
    if (res_scale && (!res || !res_shift)) return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (!fa_fwd_table_ok(C, parts)) {
        int rc = dam_bn_finalize_f32(partial, parts, C, fin->gamma, fin->beta, fin->running_mean, fin->running_var,
                                     fin->num_batches_tracked, fin->momentum, fin->eps, fin->save_mean, fin->save_invstd, fin->scale,
                                     fin->shift, stream);
        if (rc != DAM_OK) return rc;
        return dam_bn_apply_f32(x, n_pixels, C, fin->scale, fin->shift, res, res_scale, res_shift, relu, y, sign_bits, stream);
    }
    const FaPlan f = fa_plan(n_pixels, C);
    hipLaunchKernelGGL(bn_fin_apply_kernel, dim3(f.nranges, f.nslices), dim3(FA_THREADS), 0, st, partial, parts, C, f.cs, a, x,
                       n_pixels, f.ppr, res, res_scale, res_shift, relu, y, sign_bits);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_stats_f32(const float* x, int64_t n_pixels, int C, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float momentum, float eps, float* save_mean, float* save_invstd, float* scale,
                                float* shift, float* workspace, void* stream) {
    if (!x || !gamma || !beta || !save_mean || !save_invstd || !scale || !shift || !workspace || n_pixels <= 0)
        return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    const BnLaunch l = bn_plan(n_pixels, C);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(l.parts), dim3(l.threads), (size_t)l.r * C * 3 * sizeof(float), st,
                       x, n_pixels, C, l.q, l.r, l.ppb, workspace, (const float*)nullptr, (float*)nullptr);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, st, workspace, l.parts, C,
                       gamma, beta, running_mean, running_var, (long long*)num_batches_tracked, momentum, eps,
                       save_mean, save_invstd, scale, shift, BnFinArgs{}, (const float*)nullptr);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// Training-mode statistics of TWO tensors of one shape (a block's conv1 output and its shortcut convolution's output: two
// independent BatchNorms that become ready together) in one partial + one finalize launch.
extern "C" int dam_bn_stats_pair_f32(const float* x_a, const float* x_b, int64_t n_pixels, int C, const dam_bn_fin* a,
                                     const dam_bn_fin* b, float* workspace, void* stream) {
    BnFinArgs fa, fb;
    if (!x_a || !x_b || !fin_args(a, &fa) || !fin_args(b, &fb) || !workspace || n_pixels <= 0) return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    const BnLaunch l = bn_plan(n_pixels, C);
    hipStream_t st = (hipStream_t)stream;
    float* ws_b = workspace + (size_t)BN_RECORDS_MAX * C * 3;
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(l.parts, 2), dim3(l.threads), (size_t)l.r * C * 3 * sizeof(float), st, x_a,
                       n_pixels, C, l.q, l.r, l.ppb, workspace, x_b, ws_b);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C, 2), dim3(64), 0, st, workspace, l.parts, C, fa.gamma, fa.beta,
                       fa.running_mean, fa.running_var, fa.num_batches, fa.momentum, fa.eps, fa.save_mean, fa.save_invstd, fa.scale,
                       fa.shift, fb, (const float*)ws_b);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_finalize_f32(const float* partial, int parts, int C, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                   float momentum, float eps, float* save_mean, float* save_invstd, float* scale,
                                   float* shift, void* stream) {
    if (!partial || parts <= 0 || C <= 0 || !gamma || !beta || !save_mean || !save_invstd || !scale || !shift)
        return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, partial, parts, C, gamma, beta,
                       running_mean, running_var, (long long*)num_batches_tracked, momentum, eps, save_mean, save_invstd,
                       scale, shift, BnFinArgs{}, (const float*)nullptr);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_finalize_pair_f32(const float* partial_a, const float* partial_b, int parts, int C, const dam_bn_fin* a,
                                        const dam_bn_fin* b, void* stream) {
    BnFinArgs fa, fb;
    if (!partial_a || !partial_b || parts <= 0 || C <= 0 || !fin_args(a, &fa) || !fin_args(b, &fb)) return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C, 2), dim3(64), 0, (hipStream_t)stream, partial_a, parts, C, fa.gamma, fa.beta,
                       fa.running_mean, fa.running_var, fa.num_batches, fa.momentum, fa.eps, fa.save_mean, fa.save_invstd, fa.scale,
                       fa.shift, fb, partial_b);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_eval_affine_f32(int C, const float* gamma, const float* beta, const float* running_mean,
                                      const float* running_var, float eps, float* save_mean, float* save_invstd,
                                      float* scale, float* shift, void* stream) {
    if (!gamma || !beta || !running_mean || !running_var || !save_mean || !save_invstd || !scale || !shift || C <= 0)
        return DAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, C, gamma, beta,
                       running_mean, running_var, eps, save_mean, save_invstd, scale, shift);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_apply_f32(const float* x, int64_t n_pixels, int C, const float* scale, const float* shift,
                                const float* res, const float* res_scale, const float* res_shift, int relu, float* y,
                                uint8_t* sign_bits, void* stream) {
    if (!x || !scale || !shift || !y || n_pixels <= 0) return DAM_ERR_BAD_ARG;
    if (C % 16) return DAM_ERR_UNSUPPORTED;
    if (res_scale && (!res || !res_shift)) return DAM_ERR_BAD_ARG;
    const int64_t nq = n_pixels * (C / 4);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(elt_blocks(nq)), dim3(256), 0, (hipStream_t)stream, x, nq, C / 4, scale, shift,
                       res, res_scale, res_shift, relu, y, sign_bits);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int dam_bn_backward_f32(const float* dy, const float* y_mask, const float* x, int64_t n_pixels, int C,
                                   const float* gamma, const float* save_mean, const float* save_invstd, int training,
                                   const float* mask_scale, const float* mask_shift, const uint8_t* mask_bits, float* dx,
                                   float* dgamma, float* dbeta, float* workspace, int partials_given, void* stream) {
    if (!dy || !x || !gamma || !save_mean || !save_invstd || !dx || !dgamma || !dbeta || !workspace || n_pixels <= 0)
        return DAM_ERR_BAD_ARG;
    if ((mask_scale != nullptr) != (mask_shift != nullptr) || (y_mask && mask_scale) || (mask_bits && (y_mask || mask_scale)))
        return DAM_ERR_BAD_ARG;
    if (mask_bits) y_mask = reinterpret_cast<const float*>(mask_bits);       // MASK == 3 reads it as bytes
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    BnLaunch l = bn_plan(n_pixels, C, fa_max_parts(C, 2));
    if (partials_given < 0 || partials_given > BN_MAX_PARTS) return DAM_ERR_BAD_ARG;
    if (partials_given) l.parts = partials_given;       // records from a data-gradient epilogue
    // ... which may be more than a fused consumer's table takes: then the finalize and the apply launch of their own
    const bool fused = fa_table_ok(C, l.parts, 2);
    hipStream_t st = (hipStream_t)stream;
    const int mask = mask_bits ? 3 : (y_mask ? 1 : (mask_scale ? 2 : 0));
    const BnBwdSides<1> sd{{{x, gamma, save_mean, save_invstd, dx, dgamma, dbeta}}};
    const int rc = bn_bwd_launch<1, 0, 1, 2, 3>(l, partials_given != 0, fused, mask, sd, dy, y_mask, n_pixels, C, training,
                                                mask_scale, mask_shift, workspace, st);
    if (rc != DAM_OK || fused) return rc;
    float* coef = workspace + (size_t)BN_MAX_PARTS * C * 2;    // workspace holds [parts][C][2] then [3][C]
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, st, workspace, l.parts, C,
                       (double)n_pixels, gamma, save_mean, save_invstd, training, dgamma, dbeta, coef);
    DAM_CHECK_LAUNCH();
    const int64_t nq = n_pixels * (C / 4);
    const bool known = with_mask<0, 1, 2, 3>(mask, [&](auto m) {
        hipLaunchKernelGGL(bn_bwd_apply_kernel<decltype(m)::value>, dim3(elt_blocks(nq)), dim3(256), 0, st, dy, y_mask, x, nq, C / 4,
                           C, (const float*)coef, mask_scale, mask_shift, dx);
    });
    if (!known) return DAM_ERR_BAD_ARG;
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// The finalize of dam_bn_backward_f32(partials_given = parts) without its apply: the same merge (inside the fused launch's table
// limit that launch's own, beyond it bn_bwd_finalize_kernel as there), the coefficients to `coef`.
extern "C" int dam_bn_backward_finalize_f32(const float* partial, int parts, int64_t n_pixels, int C, const float* gamma,
                                            const float* save_mean, const float* save_invstd, int training, float* dgamma,
                                            float* dbeta, float* coef, void* stream) {
    if (!partial || !gamma || !save_mean || !save_invstd || !dgamma || !dbeta || !coef || n_pixels <= 0) return DAM_ERR_BAD_ARG;
    if (parts <= 0 || parts > BN_MAX_PARTS) return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (fa_table_ok(C, parts, 2)) {
        const FaPlan f = fa_plan(n_pixels, C);
        const BnBwdSides<1> sd{{{nullptr, gamma, save_mean, save_invstd, nullptr, dgamma, dbeta}}};
        hipLaunchKernelGGL(bn_bwd_fin_only_kernel, dim3(f.nslices), dim3(FA_THREADS), 0, st, partial, parts, C, f.cs, (double)n_pixels,
                           training, sd, coef);
    } else {
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, st, partial, parts, C, (double)n_pixels, gamma, save_mean,
                           save_invstd, training, dgamma, dbeta, coef);
    }
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

extern "C" int64_t dam_bn_pair_workspace_floats(int C) { return (int64_t)BN_MAX_PARTS * C * 3 + 6 * (int64_t)C; }

extern "C" int dam_bn_backward_pair_f32(const float* dy, const float* y_mask, const uint8_t* mask_bits, int64_t n_pixels, int C,
                                        int training,
                                        const float* x_a, const float* gamma_a, const float* mean_a, const float* invstd_a,
                                        float* dx_a, float* dgamma_a, float* dbeta_a,
                                        const float* x_b, const float* gamma_b, const float* mean_b, const float* invstd_b,
                                        float* dx_b, float* dgamma_b, float* dbeta_b, float* workspace, void* stream) {
    if ((y_mask != nullptr) == (mask_bits != nullptr)) return DAM_ERR_BAD_ARG;      // exactly one form of the mask
    const bool bits = mask_bits != nullptr;
    if (bits) y_mask = reinterpret_cast<const float*>(mask_bits);
    if (!dy || !y_mask || !x_a || !gamma_a || !mean_a || !invstd_a || !dx_a || !dgamma_a || !dbeta_a || !x_b || !gamma_b ||
        !mean_b || !invstd_b || !dx_b || !dgamma_b || !dbeta_b || !workspace || n_pixels <= 0)
        return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    // at most fa_max_parts records, so the fused consumer's table (<= FA_PARTS_KB) is always within FA_TABLE_BYTES_MAX
    const BnLaunch l = bn_plan(n_pixels, C, fa_max_parts(C, 3));
    if ((size_t)l.r * C * 3 * sizeof(float) > 64 * 1024) return DAM_ERR_UNSUPPORTED;
    const BnBwdSides<2> sd{{{x_a, gamma_a, mean_a, invstd_a, dx_a, dgamma_a, dbeta_a},
                            {x_b, gamma_b, mean_b, invstd_b, dx_b, dgamma_b, dbeta_b}}};
    return bn_bwd_launch<2, 1, 3>(l, false, true, bits ? 3 : 1, sd, dy, y_mask, n_pixels, C, training, nullptr, nullptr, workspace,
                                  (hipStream_t)stream);
}

extern "C" int dam_channel_sum_f32(const float* x, int64_t n_pixels, int C, int n_real, float* out, float* workspace,
                                   void* stream) {
    if (!x || !out || !workspace || n_pixels <= 0 || n_real <= 0 || n_real > C) return DAM_ERR_BAD_ARG;
    if (C % 16 || C > 1024) return DAM_ERR_UNSUPPORTED;
    const BnLaunch l = bn_plan(n_pixels, C);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(channel_sum_partial_kernel, dim3(l.parts), dim3(l.threads), (size_t)l.r * C * sizeof(float), st, x,
                       n_pixels, C, l.q, l.r, l.ppb, workspace);
    DAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(channel_sum_finalize_kernel, dim3(n_real), dim3(64), 0, st, workspace, l.parts, C,
                       n_real, out);
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}
