// dam_wgrad.hip -- convolution weight gradient on the gfx950 fp32 matrix cores.
//
// Replaces the autograd weight-gradient of every nn.Conv2d on the path (models/model_resnet.py:11-21,64;
// models/model_scalar_1s.py:167-172; models/model_scalar_2s.py:25-30), reached from loss.backward() at
// model_trainer.py:36.
//
//   dW[n][k][kh][kw] = sum_{b, oh, ow} dY[b, oh, ow, n] * f(X[b, oh*s + kh*d - pad, ow*s + kw*d - pad, k])
//
// GEMM view per tap: D[n][k] += A[n][pix] * B[pix][k] with the PIXEL index as the MFMA reduction
// dimension (v_mfma_f32_16x16x4_f32, 4 pixels per step).  NHWC makes both operands plain ds_read_b32:
// lanes 0-15 read 16 consecutive channels of one pixel, the 4 lane groups read 4 consecutive pixels.
//   * a workgroup owns an output tile (16*TNB out-channels x 16*TKB in-channels x TA x TB taps) and walks a
//     strided subset of 256-pixel tiles (split-K over pixels); per tile it stages the dY pixels and the
//     input rows they touch (same patch layout as the forward kernel, optional fused BN-apply+ReLU);
//   * each of the 4 waves reduces its own quarter of the tile's pixels into the full output tile held in
//     registers; waves are combined through LDS once at the end, the workgroup writes ONE partial slab;
//   * a second kernel sums the slabs in a fixed order (deterministic, no float atomics) and writes
//     torch's [O][I][KH][KW] layout.
#include <string.h>
#include <type_traits>
#include "dam_common.h"
#include "dam_conv_stage.h"
#include "dam_wgrad_plan.h"

namespace dam {

// Weight gradients of ONE geometry batched into one launch of the tile kernel (blockIdx.z = job): the three equal convolutions of
// a deep ResNet stage (models/model_resnet.py:14-21 at 256 / 128 channels) are 20-28 us launches of which ~13 us are launch and
// pipeline fill; one launch of three jobs pays that once and needs a third of the pixel splits (slabs) to fill the chip.
constexpr int WG_MAX_JOBS = 4;
struct WgradJobs {
    const float* X[WG_MAX_JOBS];
    const float* dY[WG_MAX_JOBS];
    const float* sc[WG_MAX_JOBS];
    const float* sh[WG_MAX_JOBS];
    float* partial[WG_MAX_JOBS];
    int relu_in[WG_MAX_JOBS];             // per job (with sc): a block's conv2 reads relu(bn1(c1)), its conv1 the plain block input
};

// Jobs of a batched launch of the direct kernel (see wgrad_direct_batch_kernel; DirectJob: dam_wgrad_plan.h).
constexpr int WD_MAX_JOBS = 8;
struct DirectJobs { DirectJob job[WD_MAX_JOBS]; int njobs; };

namespace {

// What the last dam_conv2d_wgrad_f32 call of this thread committed to (dam_wgrad_last_launch, include/dam_hip.h): a host variable
// written from the plan where a launcher has passed its last refusal, read by tests that must know which instantiation they exercised.
thread_local WgradLaunchNote wgrad_last_launch{};

typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));

// A workgroup stages and computes in turn and relies on a second co-resident workgroup to fill the gaps (its matrix pipe was 58 %
// busy on the scalar models' 9x9 layer).  Loader waves staging the next tile beside the MFMAs measured slower still: C2 5.28 ->
// 5.52 ms, C1 3.71 -> 3.86 ms (profiles/r05_wgrad_loader_waves_ab.txt).
template <int TNB, int TKB, int TA, int TB>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradGeo g, const WgradJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const float* __restrict__ X = jobs.X[blockIdx.z];
    const float* __restrict__ dY = jobs.dY[blockIdx.z];
    const float* __restrict__ in_scale = jobs.sc[blockIdx.z];
    const float* __restrict__ in_shift = jobs.sh[blockIdx.z];
    float* __restrict__ partial = jobs.partial[blockIdx.z];
    constexpr int NBLK = TNB * TKB * TA * TB;
    const int tid = threadIdx.x & 255, lane = tid & 63;          // (the masks are no-ops at 256 threads; they steer register allocation)
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) & 3;
    const int j = lane & 15, kq = lane >> 4;
    int xt = blockIdx.x;
    const int tg = xt % g.tap_groups; xt /= g.tap_groups;
    const int tk = xt % g.tiles_k;
    const int tn = xt / g.tiles_k;
    const int a0 = tg * TA;
    const int HoWo = g.Ho * g.Wo;
    const int chunk_bytes = g.PR * g.PWT * 64;
    const int TMW = g.TMW, WP = g.TMW >> 2;   // pixels per wave

    PatchGeo pg;
    pg.H = g.H; pg.W = g.W; pg.C = g.C; pg.s = g.s; pg.c0 = g.c0; pg.PR = g.PR; pg.PWin = g.PWin; pg.PWs = g.PWs;
    pg.PWT = g.PWT; pg.in_nchw = g.in_nchw; pg.relu_in = jobs.relu_in[blockIdx.z];

    const size_t img_elems = (size_t)g.H * g.W * g.C;
    // stage tile `tile` into the LDS image at `smem` (all 256 threads)
    auto stage_tile = [&](int tile, unsigned char* smem) {
        unsigned char* dy_s = smem + TKB * chunk_bytes;
        const int img = tile / g.tiles_m;
        const int p0 = (tile - img * g.tiles_m) * TMW;
        const int oh_first = p0 / g.Wo;
        // only the input rows the TA kernel rows of this tap group touch (a 1 x KW group needs no vertical halo at all)
        stage_patch(smem, chunk_bytes, X + (size_t)img * img_elems, pg, oh_first * g.s + g.off_h + a0 * g.step_h, tk * TKB, TKB,
                    in_scale, in_shift, tid);
        {   // dY pixels p0 .. p0+TMW-1, channels of this n tile; zero beyond the image / channel count
            constexpr int QPP = TNB * 4;
            const float* dyb = dY + ((size_t)img * HoWo) * g.N + tn * TNB * 16;
            constexpr int U = 4;
            for (int base = tid; base < TMW * QPP; base += 256 * U) {
                float4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = base + 256 * u, pl = e / QPP, cq = e % QPP;
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (e < TMW * QPP && p0 + pl < HoWo && tn * TNB * 16 + cq * 4 < g.N)
                        v[u] = *reinterpret_cast<const float4*>(dyb + (size_t)(p0 + pl) * g.N + cq * 4);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = base + 256 * u, pl = e / QPP, cq = e % QPP;
                    if (e < TMW * QPP)
                        *reinterpret_cast<float4*>(dy_s + (((cq >> 2) * TMW + pl) * 16 + (cq & 3) * 4) * 4) = v[u];
                }
            }
        }
    };
    v4f acc[NBLK];
#pragma unroll
    for (int i = 0; i < NBLK; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};

    int toffs[TA * TB];                      // LDS byte offset of tap (ta, tb) relative to the lane's pixel of the staged patch
#pragma unroll
    for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) {
            const int coff = g.off_w + tb * g.step_w - g.c0;
            const int slotoff = g.s == 1 ? coff : (coff & 1) * g.PWs + (coff >> 1);
            toffs[ta * TB + tb] = (ta * g.step_h * g.PWT + slotoff) * 64;
        }
    // the MFMAs of tile `tile` from the LDS image at `smem` (the four compute waves)
    auto compute_tile = [&](int tile, const unsigned char* smem) {
        const unsigned char* dy_s = smem + TKB * chunk_bytes;
        const int img = tile / g.tiles_m;
        const int p0 = (tile - img * g.tiles_m) * TMW;
        const int oh_first = p0 / g.Wo;
        (void)img;
        // this wave's WP pixels, 4 per MFMA step; lane group kq owns pixel 4*t + kq.  Two operand sets: the TNB + TA*TB*TKB
        // ds_read_b32 of step t + 1 are requested before the MFMAs of step t (one wave per SIMD here -- 80-odd KB of LDS per
        // workgroup -- so nothing else hides the LDS latency: the single-set loop ran the 9x9 / 64 -> 128 layer of the scalar
        // models at 0.41 of the matrix peak)
        int p = p0 + wave * WP + kq;
        int pc = p < HoWo ? p : HoWo - 1;
        int oh = pc / g.Wo, ow = pc - oh * g.Wo;
        const int nsteps = WP >> 2;
        float av[2][TNB], bv[2][TA * TB * TKB];
#define DAM_WG_LOAD(BUF_, T_)                                                                                               \
    do {                                                                                                                  \
        const int pl_ = wave * WP + 4 * (T_) + kq;                                                                        \
        _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                                \
            av[BUF_][nb] = *reinterpret_cast<const float*>(dy_s + ((nb * TMW + pl_) * 16 + j) * 4);                       \
        const int base_ = (((oh - oh_first) * g.s) * g.PWT + ow) * 64 + j * 4;                                            \
        _Pragma("unroll") for (int ta = 0; ta < TA; ++ta)                                                                 \
            _Pragma("unroll") for (int tb = 0; tb < TB; ++tb)                                                             \
                _Pragma("unroll") for (int kb = 0; kb < TKB; ++kb)                                                        \
                    bv[BUF_][(ta * TB + tb) * TKB + kb] =                                                                 \
                        *reinterpret_cast<const float*>(smem + kb * chunk_bytes + base_ + toffs[ta * TB + tb]);           \
        p += 4;                                       /* this lane's pixel of the NEXT step (past the image: dY == 0) */  \
        if (p < HoWo) {                                                                                                   \
            ow += 4;                                                                                                      \
            while (ow >= g.Wo) { ow -= g.Wo; ++oh; }                                                                      \
        }                                                                                                                 \
    } while (0)
#define DAM_WG_MFMA(BUF_)                                                                                                   \
    do {                                                                                                                  \
        _Pragma("unroll") for (int ta = 0; ta < TA; ++ta)                                                                 \
            _Pragma("unroll") for (int tb = 0; tb < TB; ++tb)                                                             \
                _Pragma("unroll") for (int kb = 0; kb < TKB; ++kb)                                                        \
                    _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb) {                                                  \
                        const int idx = ((nb * TKB + kb) * TA + ta) * TB + tb;                                            \
                        acc[idx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[BUF_][nb], bv[BUF_][(ta * TB + tb) * TKB + kb], acc[idx], 0, 0, 0); \
                    }                                                                                                     \
    } while (0)
        DAM_WG_LOAD(0, 0);
        int t = 0;
        for (; t + 2 <= nsteps; t += 2) {
            DAM_WG_LOAD(1, t + 1);
            __builtin_amdgcn_sched_barrier(0);
            DAM_WG_MFMA(0);
            __builtin_amdgcn_sched_barrier(0);
            if (t + 2 < nsteps) DAM_WG_LOAD(0, t + 2);
            __builtin_amdgcn_sched_barrier(0);
            DAM_WG_MFMA(1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t < nsteps) DAM_WG_MFMA(0);
#undef DAM_WG_LOAD
#undef DAM_WG_MFMA
    };
    for (int tile = blockIdx.y; tile < g.total_tiles; tile += g.nsplit) {
        __syncthreads();
        stage_tile(tile, smem_all);
        __syncthreads();
        compute_tile(tile, smem_all);
    }

    // combine the 4 waves through LDS (sequential adds: fixed order), then one slab per workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem_all);
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NBLK; ++i) {
                float4* dst = reinterpret_cast<float4*>(red + (i * 64 + lane) * 4);
                if (w == 0) {
                    *dst = make_float4(acc[i].x, acc[i].y, acc[i].z, acc[i].w);
                } else {
                    float4 o = *dst;
                    o.x += acc[i].x; o.y += acc[i].y; o.z += acc[i].z; o.w += acc[i].w;
                    *dst = o;
                }
            }
        }
        __syncthreads();
    }
    float4* out = reinterpret_cast<float4*>(partial) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NBLK * 64;
    for (int e = tid; e < NBLK * 64; e += 256) out[e] = reinterpret_cast<const float4*>(red)[e];
}

// dW[n][k][kh][kw] = sum over splits of the slabs, for a BATCH of weight gradients in one launch: a reduction is 5-10 us of
// mostly launch latency, a ResNet18 step has 20 of them and nothing but the optimizer waits for any (dam_wgrad_queue_*).
// Block = EL elements x SL split lanes (256 x 1 for few big slabs, 32 x 8 for few small ones, 8 x 32 for many): a thread adds
// a strided subset of the splits (4 independent chains, all loads in flight), the SL subtotals are combined by a fixed tree
// (deterministic).
struct ReduceJob {
    const float* partial;
    float* dw;
    int nsplit, nx, TNB, TKB, TA, TB, n_real, k_real, KH, KW, tap_groups, tiles_k;
    int sl;                  // split lanes: 32, 8 or 1
    int blocks;              // workgroups of the launch that work on this job
};
constexpr int REDUCE_MAX_JOBS = 40;       // one flush per ResNet18 backward (30 weight gradients); 40 x 72 B of kernel arguments
struct ReduceBatch {
    ReduceJob job[REDUCE_MAX_JOBS];
    int njobs;
};

__global__ __launch_bounds__(256) void wgrad_reduce_batch_kernel(const ReduceBatch batch) {
    __shared__ float4 sub[256];
    int ji = 0, b0 = blockIdx.x;
    while (ji + 1 < batch.njobs && b0 >= batch.job[ji].blocks) { b0 -= batch.job[ji].blocks; ++ji; }
    const ReduceJob& j = batch.job[ji];
    const int SL = j.sl, EL = 256 / SL;
    const int nblk_tile = j.TNB * j.TKB * j.TA * j.TB;
    const int64_t per_split4 = (int64_t)j.nx * nblk_tile * 64;       // float4 per slab
    const float4* p4 = reinterpret_cast<const float4*>(j.partial);
    const int el = threadIdx.x % EL, ys = threadIdx.x / EL;
    for (int64_t e0 = (int64_t)b0 * EL; e0 < per_split4; e0 += (int64_t)j.blocks * EL) {
        const int64_t e = e0 + el;
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
        if (e < per_split4) {
            int y = ys;
            for (; y + 3 * SL < j.nsplit; y += 4 * SL) {
                const float4 a = p4[y * per_split4 + e], b = p4[(y + SL) * per_split4 + e];
                const float4 c = p4[(y + 2 * SL) * per_split4 + e], d = p4[(y + 3 * SL) * per_split4 + e];
                s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
                s2.x += c.x; s2.y += c.y; s2.z += c.z; s2.w += c.w; s3.x += d.x; s3.y += d.y; s3.z += d.z; s3.w += d.w;
            }
            for (; y < j.nsplit; y += SL) { const float4 a = p4[y * per_split4 + e]; s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; }
        }
        sub[ys * EL + el] = make_float4((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y), (s0.z + s1.z) + (s2.z + s3.z),
                                        (s0.w + s1.w) + (s2.w + s3.w));
        __syncthreads();
        for (int stride = SL / 2; stride >= 1; stride >>= 1) {
            if (ys < stride) {
                float4 a = sub[ys * EL + el];
                const float4 b = sub[(ys + stride) * EL + el];
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                sub[ys * EL + el] = a;
            }
            __syncthreads();
        }
        if (ys == 0 && e < per_split4) {
            const float4 s = sub[el];
            const float sv[4] = {s.x, s.y, s.z, s.w};
            const int lane = e & 63;
            int64_t q = e >> 6;
            const int blk = q % nblk_tile;
            int xt = q / nblk_tile;
            const int tb = blk % j.TB, ta = (blk / j.TB) % j.TA, kb = (blk / (j.TB * j.TA)) % j.TKB, nb = blk / (j.TB * j.TA * j.TKB);
            const int tg = xt % j.tap_groups; xt /= j.tap_groups;
            const int tk = xt % j.tiles_k, tn = xt / j.tiles_k;
            const int k = (tk * j.TKB + kb) * 16 + (lane & 15);
            const int kh = tg * j.TA + ta;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = (tn * j.TNB + nb) * 16 + (lane >> 4) * 4 + r;
                if (n < j.n_real && k < j.k_real && kh < j.KH) j.dw[(((size_t)n * j.k_real + k) * j.KH + kh) * j.KW + tb] = sv[r];
            }
        }
        __syncthreads();
    }
}

// Host side of a caller-owned queue of deferred reductions (include/dam_hip.h: dam_wgrad_queue_*).
// tile-kernel launches of one geometry recorded, not yet launched (dam_wgrad_queue_set_batching)
struct PendingTile {
    int njobs;                               // 0: nothing pending
    WgradLaunchNote note;                    // the instantiation (as planned for every job)
    WgradGeo g;                              // shared geometry, nsplit = 0 (decided at launch from the number of jobs)
    WgradJobs jobs;
    float* dw[WG_MAX_JOBS];
    int64_t ws_floats[WG_MAX_JOBS];
    WgradReduce red[WG_MAX_JOBS];
};
// direct-kernel launches of one instantiation recorded, not yet launched (any geometry: every job carries its own)
struct PendingDirect {
    WgradLaunchNote note;                    // the instantiation
    DirectJobs jobs;                         // jobs.njobs == 0: nothing pending
    float* dw[WD_MAX_JOBS];
    WgradReduce red[WD_MAX_JOBS];
};
// stride-1 row-kernel launches of one instantiation, geometry and grid recorded, not yet launched (batching mode 2)
struct PendingRows {
    WgradPlan plan;                          // as planned for every job: instantiation, RowsGeo, grid, LDS bytes
    RowsJobs jobs;                           // jobs.njobs == 0: nothing pending
    float* dw[ROWS_MAX_JOBS];
    WgradReduce red[ROWS_MAX_JOBS];
};
struct WgradQueue {
    unsigned magic;
    int batching;                            // 1: tile launches of one geometry and direct launches wait for each other until the flush;
                                             // 2: so do the row kernel's launches of the next call
    ReduceBatch batch;
    PendingTile pend;
    PendingDirect pend_direct;
    PendingRows pend_rows;
};
constexpr unsigned WGRAD_QUEUE_MAGIC = 0x57475251u;     // "WGRQ"

int reduce_flush(ReduceBatch& b, hipStream_t st) {
    if (b.njobs <= 0) return DAM_OK;
    int blocks = 0;
    for (int i = 0; i < b.njobs; ++i) blocks += b.job[i].blocks;
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3(blocks), dim3(256), 0, st, b);
    b.njobs = 0;
    DAM_CHECK_LAUNCH();
    return DAM_OK;
}

// The slab reduction of one weight gradient: launched now (queue == nullptr) or appended to the caller's queue (its slabs
// must then stay untouched until dam_wgrad_queue_flush).
int reduce_submit(void* queue, const float* partial, float* dw, int nsplit, int nx, const WgradReduce& r, hipStream_t st) {
    ReduceJob j;
    j.partial = partial; j.dw = dw; j.nsplit = nsplit; j.nx = nx; j.TNB = r.TNB; j.TKB = r.TKB; j.TA = r.TA; j.TB = r.TB;
    j.n_real = r.n_real; j.k_real = r.k_real; j.KH = r.KH; j.KW = r.KW; j.tap_groups = r.tap_groups; j.tiles_k = r.tiles_k;
    const int64_t per_split4 = (int64_t)nx * r.TNB * r.TKB * r.TA * r.TB * 64;
    if (nsplit >= 64) {
        j.sl = 32;
        j.blocks = (int)(cdiv(per_split4, 8) < 4096 ? cdiv(per_split4, 8) : 4096);
    } else if (per_split4 >= 8192) {
        // few big slabs (the thick stages): one element per thread, the splits added in order by that thread (4 chains, all
        // loads in flight) -- no LDS step at all; the 32 x 8 shape spent its time in one-load-then-barrier rounds
        j.sl = 1;
        j.blocks = (int)(cdiv(per_split4, 256) < 4096 ? cdiv(per_split4, 256) : 4096);
    } else {
        j.sl = 8;
        j.blocks = (int)(cdiv(per_split4, 32) < 2048 ? cdiv(per_split4, 32) : 2048);
    }
    if (!queue) {
        ReduceBatch one;
        one.job[0] = j; one.njobs = 1;
        return reduce_flush(one, st);
    }
    WgradQueue* q = static_cast<WgradQueue*>(queue);
    if (q->magic != WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    if (q->batch.njobs == REDUCE_MAX_JOBS) {
        const int rc = reduce_flush(q->batch, st);
        if (rc != DAM_OK) return rc;
    }
    q->batch.job[q->batch.njobs++] = j;
    return DAM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Row-streaming variant for the 3x3 / stride 1 / pad 1 layers with equal channel counts on both sides (every BasicBlock
// convolution except the strided ones): same partial-slab output and reduce kernel as above, different data movement.
//
//   * A workgroup (4 compute waves + 8 loader waves, one per CU) owns one (out-channel tile, in-channel tile) and a
//     strip of output rows of one image.  X rows and dY rows stream through two LDS rings of whole rows; row pitch P4
//     cells of 16 channels, cell e holds pixel column e-1, the cells outside the image stay zero.  With that pitch the
//     pixel index is linear inside a row for all three column taps: the X cell of tap b is (dY cell) + b - 1.
//   * Slot = 4 output rows, one per compute wave.  A wave's operand addresses for a row are 3*TKB + TNB registers
//     (row bases, scalar ring arithmetic) + immediates: the MFMA stream carries no address arithmetic at all
//     (a streaming MFMA wave owns the SIMD's vector issue port, see dam_conv_strip.hip).
//   * Loader waves: scalar plane arithmetic, buffer_load with per-lane column offsets computed once, ds_write with the
//     column mask in EXEC.  Two slots ahead in two register sets (a slot is ~4 us of MFMAs, about the HBM latency under load).
// Diagnostic build only (-DDAM_WGR_STAMPS, tools/wgr_stamps_probe.py; results are wrong): instead of its slab a workgroup leaves
// s_memtime stamps of compute wave 0 and loader wave 0, [role][32] of (tag << 56 | time): 1 start, 2 first rows staged,
// 5 end of a slot's MFMAs / commits, 7 behind the slot's barrier, 8 end.
#ifdef DAM_WGR_STAMPS
#define DAM_WSTAMP(tag)                                                                                                \
    do {                                                                                                              \
        if (lane == 0 && (wave == 0 || wave == 4) && stamp_n < 32)                                                    \
            stamp_v[stamp_n++] = ((unsigned long long)(tag) << 56) | ((unsigned long long)__builtin_readcyclecounter() & ((1ull << 56) - 1)); \
    } while (0)
#else
#define DAM_WSTAMP(tag) do { } while (0)
#endif
// v % d for the two ring sizes (scalar multiply-shift, v < 30000)
template <int D> __device__ __forceinline__ int rw_mod(int v) { return D == 10 ? v - ((v * 52429) >> 19) * 10 : v - ((v * 43691) >> 18) * 6; }

// HV: 1 = a compute wave takes a whole output row per slot (4 rows per slot), 2 = half a row (2 rows per slot, for rows too
// wide for ten-row rings: the reference's native 216-frame spectrograms); STEPS = MFMA steps per wave and row (part)
// NL: loader waves, 8 or 4.  The hardware starts a workgroup's waves one after the other (the 12th wave of a 768-thread workgroup
// begins ~7 k clocks after the first when all CUs start at once); the narrow stages' few planes per slot do not need eight loaders,
// and at eight waves per workgroup two workgroups really are co-resident on a CU (107 registers x 16 waves).
template <int TNB, int TKB, int STEPS, int KP, int GPP, int HV, int NL>
__global__ __launch_bounds__(256 + 64 * NL) void wgrad_rows_kernel(const RowsGeo g, const RowsJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NBLK = TNB * TKB * 9;
    constexpr int RPS = 4 / HV, RW_NRX = 2 * RPS + 2, RW_NRD = 2 * RPS;     // rows per slot; ring rows (in use + being written)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    // XCD-aware placement: workgroups go to the 8 XCDs round-robin in dispatch order (x fastest), so the nx workgroups that
    // stream the SAME rows (one per (out tile, in tile)) would sit on nx different L2s and every row would be fetched from the
    // fabric nx times (measured: 6 x the algorithmic bytes on the 96-channel stage).  Re-index so that they share an XCD:
    // position r inside XCD c -> (tile r % nx, strip (r / nx) * 8 + c); the strips beyond a multiple of 8 keep their place.
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int nxg = gridDim.x, L = blockIdx.y * nxg + blockIdx.x, full = (gridDim.y >> 3) << 3;
        if (L < full * nxg) { const int c = L & 7, r = L >> 3; bx = r % nxg; by = (r / nxg) * 8 + c; }
    }
    const int tn = bx / g.tiles_k, tk = bx - tn * g.tiles_k;
    // strips: the image's rows in spi nearly equal parts (the feature maps are 2^k + 1 rows high: with strips of whole slots
    // 1025 rows on 32 strips took 9 slots of 4 rows per workgroup for 8.01 slots of work); a last slot of one row is split
    // over all four compute waves by MFMA steps (the waves' sums are added at the end whatever produced them)
    const int img = by / g.spi, sidx = by - img * g.spi;
    const int r_begin = (int)(((long long)sidx * g.H) / g.spi), r_end = (int)(((long long)(sidx + 1) * g.H) / g.spi);
    const int n_slots = (r_end - r_begin + RPS - 1) / RPS;
    const int n_slots2 = n_slots > 0 ? (n_slots + 1) & ~1 : 2;       // (>= 2: the loaders' last pair of slots stands outside their loop)
    const int ROWB = g.P4 * 64;
    const int XPLANE = RW_NRX * ROWB, DPLANE = RW_NRD * ROWB;
    const int XBASE = RW_GUARD, DBASE = XBASE + TKB * XPLANE;
    const int lds_bytes = DBASE + TNB * DPLANE + RW_TAIL;

    // The cells the loaders never write must read as zero for the lifetime of the workgroup: per ring row the padding cells
    // (cell 0 = column -1, cells W + 1 .. P4 - 1), the guard in front of the first row and the tail behind the last.  Only
    // those are cleared (one pass; clearing the whole 150 KB image took the 12 waves 5.5 k clocks of a 27 k-clock prologue) and
    // they are disjoint from what a commit writes, so the clearing needs no barrier of its own.
#define DAM_RW_ZERO()                                                                                                      \
    do {                                                                                                                   \
        const int npad_ = g.P4 - g.W, nrow_ = TKB * RW_NRX + TNB * RW_NRD;                                                 \
        for (int e = tid; e < nrow_ * npad_ * 4; e += (256 + 64 * NL)) {                                                        \
            const int q_ = e & 3, c_ = (e >> 2) % npad_, r_ = (e >> 2) / npad_;                                            \
            const int cell_ = c_ == 0 ? 0 : g.W + c_;                                                                      \
            *reinterpret_cast<float4*>(smem + XBASE + r_ * ROWB + cell_ * 64 + q_ * 16) = make_float4(0.f, 0.f, 0.f, 0.f); \
        }                                                                                                                  \
        for (int e = tid * 16; e < RW_GUARD; e += (256 + 64 * NL) * 16)                                                         \
            *reinterpret_cast<float4*>(smem + e) = make_float4(0.f, 0.f, 0.f, 0.f);                                        \
        for (int e = tid * 16; e < RW_TAIL; e += (256 + 64 * NL) * 16)                                                          \
            *reinterpret_cast<float4*>(smem + lds_bytes - RW_TAIL + e) = make_float4(0.f, 0.f, 0.f, 0.f);                  \
    } while (0)

    // Jobs: the weight gradients of one launch (one geometry, one grid: jobs.njobs of them, see launch_pending_rows).  The workgroup
    // keeps its (tile, strip) and walks them in order: waves started, lane offsets and column masks computed once; per job the
    // accumulators start at zero and the combine below leaves one slab in the job's buffer -- arithmetic, strips and slot order of
    // a job are those of a launch of its own, so its slabs are bitwise the same.  A job boundary costs the slab write-out, not a
    // launch, a wave start and a cold ring: the loaders ask for the next job's first rows (registers only) during the current
    // job's last two slots and commit them once the combine's scratch -- it aliases the ring base -- has been read out.  The
    // scratch runs over padding cells and the front guard, so DAM_RW_ZERO runs per job (a few hundred 16-byte stores).  Both roles
    // carry the job loop themselves (and the combine's barriers): the loaders' register sets must not be live in the MFMA stream.
    const int njobs = jobs.njobs;
    const size_t img_off = (size_t)img * g.H * g.W * g.C;
#define DAM_RW_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
    // one slab per workgroup and job out of the combine's scratch; MORE_: another job follows -- its first rows go where the
    // scratch is, so every wave's reads of it must have returned (the stores may still be on their way)
#ifdef DAM_WGR_STAMPS
#define DAM_RW_WRITEOUT(PARTIAL_, MORE_)                                                                                   \
    do {                                                                                                                   \
        float4* out_ = reinterpret_cast<float4*>(PARTIAL_) + ((size_t)by * gridDim.x + bx) * NBLK * 64;                    \
        DAM_WSTAMP(8);                                                                                                     \
        if (lane == 0 && (wave == 0 || wave == 4)) {                                                                       \
            unsigned long long* sp = reinterpret_cast<unsigned long long*>(out_) + (wave >> 2) * 32;                       \
            for (int i = 0; i < 32; ++i) sp[i] = stamp_v[i];                                                               \
        }                                                                                                                  \
        if (MORE_) DAM_RW_BARRIER();                                                                                       \
    } while (0)
#else
#define DAM_RW_WRITEOUT(PARTIAL_, MORE_)                                                                                   \
    do {                                                                                                                   \
        float4* out_ = reinterpret_cast<float4*>(PARTIAL_) + ((size_t)by * gridDim.x + bx) * NBLK * 64;                    \
        for (int e = tid; e < NBLK * 64; e += (256 + 64 * NL)) out_[e] = reinterpret_cast<const float4*>(smem)[e];         \
        if (MORE_) DAM_RW_BARRIER();                                                                                       \
    } while (0)
#endif
#ifdef DAM_WGR_STAMPS
    unsigned long long stamp_v[32];
    int stamp_n = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) stamp_v[i] = 0;
#endif
    DAM_WSTAMP(1);

    if (wave >= 4) {
        // ================================ loader waves ================================
        const int cwl = wave - 4;
        int loffb[GPP];
        unsigned long long cmask[GPP];
#pragma unroll
        for (int gi = 0; gi < GPP; ++gi) {
            const int L = gi * 64 + lane, e = L >> 2, quad = L & 3, col = e - 1;
            const bool ok = gi < g.gpp && e < g.P4 && col >= 0 && col < g.W;
            const int colc = col < 0 ? 0 : (col >= g.W ? g.W - 1 : col);
            loffb[gi] = (colc * g.C + quad * 4) * 4;
            cmask[gi] = __ballot(ok);
        }
        const int img_bytes = g.H * g.W * g.C * 4;
        const int lane16 = lane * 16;
        const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
        v4f lv[KP][GPP];
        int dst[KP];               // scalar: LDS byte offset of the plane | 1 << 30 (row outside the image: zeros), -1 = none
        int aff[KP], aff2[KP];     // scalar: chunk index kb of an X plane that gets the input affine, -1 other X, -2 dY
        const int rowstride = g.W * g.C * 4;
        // X rows xr0 .. xr0+nx-1 (in-channel chunks of this tile) then dY rows dr0 .. dr0+nd-1 (out-channel blocks), one
        // plane = one (row, 16 channels); loader wave cwl takes planes cwl, cwl+4, ...  Loads are unconditional (clamped).
        // XP_ / DP_: this image of the job's X / dY; HA_: that job has an input affine.
#define DAM_RW_REQUEST(XP_, DP_, HA_, XR0_, NX_, DR0_, ND_, LV_, DST_, KP_, AFF_)                                         \
    do {                                                                                                                   \
        const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(XP_), 0, img_bytes, 0x00020000); \
        const __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(DP_), 0, img_bytes, 0x00020000); \
        _Pragma("unroll") for (int k = 0; k < KP_; ++k) {                                                                  \
            const int pl_ = cwl + NL * k;                                                                          \
            const int nxp_ = (NX_) * TKB;                                                                                  \
            const bool isx_ = pl_ < nxp_;                                                                                  \
            const int q_ = isx_ ? pl_ : pl_ - nxp_;                                                                        \
            const int i_ = isx_ ? q_ / TKB : q_ / TNB, c_ = isx_ ? q_ - i_ * TKB : q_ - i_ * TNB;                          \
            const int row_ = (isx_ ? (XR0_) : (DR0_)) + i_;                                                                \
            const bool need_ = isx_ ? row_ <= r_end : (i_ < (ND_) && row_ < r_end);                                        \
            const bool inimg_ = need_ && row_ >= 0 && row_ < g.H;                                                          \
            const int rel_ = row_ - r_begin + 1;                               /* >= 0 for every needed row */             \
            const int xi_ = rw_mod<RW_NRX>(rel_);                                                                          \
            const int di_ = (row_ - r_begin) & (RW_NRD - 1);                                                               \
            const int ldsoff_ = isx_ ? XBASE + c_ * XPLANE + xi_ * ROWB : DBASE + c_ * DPLANE + di_ * ROWB;                \
            const int chan_ = isx_ ? (tk * TKB + c_) * 64 : (tn * TNB + c_) * 64;                                          \
            const int soff_ = (inimg_ ? row_ : 0) * rowstride + chan_;                                                     \
            if (isx_) {                                                                                                    \
                _Pragma("unroll") for (int gi = 0; gi < GPP; ++gi)                                                         \
                    LV_[k][gi] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, loffb[gi], soff_, 0)); \
            } else {                                                                                                       \
                _Pragma("unroll") for (int gi = 0; gi < GPP; ++gi)                                                         \
                    LV_[k][gi] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(drsrc, loffb[gi], soff_, 0)); \
            }                                                                                                              \
            DST_[k] = need_ ? (ldsoff_ | (inimg_ ? 0 : 1 << 30)) : -1;                                                     \
            AFF_[k] = (isx_ && (HA_)) ? c_ : (isx_ ? -1 : -2);                                                             \
        }                                                                                                                  \
    } while (0)
#define DAM_RW_WRITE(ADDR_, DATA_, GI_)                                                                                    \
    asm volatile("s_mov_b64 exec, %2\n\tds_write_b128 %0, %1 offset:%3\n\ts_mov_b64 exec, -1"                              \
                 : : "v"(ADDR_), "v"(DATA_), "s"(cmask[GI_]), "n"((GI_) * 1024) : "memory")
#define DAM_RW_COMMIT(LV_, DST_, KP_, AFF_)                                                                         \
    do {                                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < KP_; ++k) {                                                                  \
            if (DST_[k] >= 0) {                                                                                            \
                const int va_ = lane16 + (DST_[k] & 0x3fffffff);                                                           \
                if (DST_[k] >> 30) {                                                                                       \
                    _Pragma("unroll") for (int gi = 0; gi < GPP; ++gi) DAM_RW_WRITE(va_, zero4, gi);                       \
                } else if (AFF_[k] >= 0) {                                                                                 \
                    const v4f sc_ = (TKB > 1 && AFF_[k] > 0) ? scq[TKB - 1] : scq[0];                                      \
                    const v4f sh_ = (TKB > 1 && AFF_[k] > 0) ? shq[TKB - 1] : shq[0];                                      \
                    _Pragma("unroll") for (int gi = 0; gi < GPP; ++gi) {                                                   \
                        v4f v_ = __builtin_elementwise_fma(LV_[k][gi], sc_, sh_);                                          \
                        v_ = __builtin_elementwise_max(v_, relu_lo4);       /* -inf without ReLU: no selects */             \
                        DAM_RW_WRITE(va_, v_, gi);                                                                         \
                    }                                                                                                      \
                } else {                                                                                                   \
                    _Pragma("unroll") for (int gi = 0; gi < GPP; ++gi) DAM_RW_WRITE(va_, LV_[k][gi], gi);                  \
                }                                                                                                          \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)
        constexpr int KPB = (2 * TKB + NL - 1) / NL;
        static_assert(KPB <= KP, "the second round of slot 0 fits a register set");
        v4f lv2[KP][GPP];
        int dst2[KP];
        DAM_WSTAMP(9);                                                         // setup done
        // rows of slot 0 of a job: X rows r_begin-1 .. r_begin+RPS, dY rows r_begin .. r_begin+RPS-1, both rounds up front: the
        // first RPS X rows and the dY rows in set lv, the other two X rows in the first KPB planes of set lv2
#define DAM_RW_SLOT0_A(XP_, DP_, HA_) DAM_RW_REQUEST(XP_, DP_, HA_, r_begin - 1, RPS, r_begin, RPS, lv, dst, KP, aff)
#define DAM_RW_SLOT0_B(XP_, DP_, HA_) DAM_RW_REQUEST(XP_, DP_, HA_, r_begin + RPS - 1, 2, r_begin, 0, lv2, dst2, KPB, aff2)
        // the first job's (a later job's are requested inside the job in front of it)
        DAM_RW_SLOT0_A(jobs.job[0].X + img_off, jobs.job[0].dY + img_off, jobs.job[0].in_scale != nullptr);
        DAM_RW_SLOT0_B(jobs.job[0].X + img_off, jobs.job[0].dY + img_off, jobs.job[0].in_scale != nullptr);
        DAM_WSTAMP(10);                                                        // first rows requested
        for (int job = 0; job < njobs; ++job) {
            const RowsJob& J = jobs.job[job];
            const bool more = job + 1 < njobs;
            const float* const Xc = J.X + img_off;
            const float* const Dc = J.dY + img_off;
            const float relu_lo = J.relu_in ? 0.f : -__builtin_inff();
            const v4f relu_lo4 = {relu_lo, relu_lo, relu_lo, relu_lo};
            // fused input affine on the X planes (the producer's BatchNorm + ReLU): a lane holds channel quad (lane & 3) of a cell
            const bool has_aff = J.in_scale != nullptr;
            v4f scq[TKB], shq[TKB];
#pragma unroll
            for (int kb = 0; kb < TKB; ++kb) {
                const int ch = (tk * TKB + kb) * 16 + (lane & 3) * 4;
                scq[kb] = has_aff ? *reinterpret_cast<const v4f*>(J.in_scale + ch) : (v4f){1.f, 1.f, 1.f, 1.f};
                shq[kb] = has_aff ? *reinterpret_cast<const v4f*>(J.in_shift + ch) : (v4f){0.f, 0.f, 0.f, 0.f};
            }
            DAM_RW_ZERO();
            DAM_WSTAMP(11);                                                    // padding cells cleared
            DAM_RW_COMMIT(lv, dst, KP, aff);
            DAM_RW_COMMIT(lv2, dst2, KPB, aff2);
            DAM_WSTAMP(12);                                                    // first rows written (their loads have landed)
            // the compute waves start slot 0 HERE; the requests for slots 1 and 2 follow (in front of this barrier they held the
            // first MFMA back by 5-8 k clocks: with three slots of rows wanted by 256 CUs at once the request queue backs up)
            DAM_RW_BARRIER();
            // steady state, two slots ahead (HBM latency under this load is about one slot): slot s writes the rows slot s+1
            // adds (X rows r_begin+RPS(s+1)+1 .. +RPS, dY rows r_begin+RPS(s+1) .. +RPS-1; requested during slot s-1) and
            // requests those of slot s+3.  Two register sets alternate; slots come in pairs so that no steady-state load sits
            // inside a conditional.  The last pair stands apart: it has nothing left to ask for of its own job, so each set, once
            // committed, takes its round of the NEXT job's slot 0 where there is one (registers only: the ring is the current
            // job's until the combine is over).
#define DAM_RW_SLOT(T_, LV_, DST_, AFF_) \
    DAM_RW_REQUEST(Xc, Dc, has_aff, r_begin + RPS * (T_) + 1, RPS, r_begin + RPS * (T_), RPS, LV_, DST_, KP, AFF_)
            DAM_WSTAMP(2);
            DAM_RW_SLOT(1, lv, dst, aff);
            DAM_RW_SLOT(2, lv2, dst2, aff2);
            for (int s = 0; s + 2 < n_slots2; s += 2) {
                DAM_RW_COMMIT(lv, dst, KP, aff);
                DAM_RW_SLOT(s + 3, lv, dst, aff);
                DAM_WSTAMP(5);
                DAM_RW_BARRIER();
                DAM_WSTAMP(7);
                DAM_RW_COMMIT(lv2, dst2, KP, aff2);
                DAM_RW_SLOT(s + 4, lv2, dst2, aff2);
                DAM_WSTAMP(5);
                DAM_RW_BARRIER();
                DAM_WSTAMP(7);
            }
            const RowsJob& Jn = jobs.job[more ? job + 1 : job];
            DAM_RW_COMMIT(lv, dst, KP, aff);
            if (more) DAM_RW_SLOT0_A(Jn.X + img_off, Jn.dY + img_off, Jn.in_scale != nullptr);
            DAM_WSTAMP(5);
            DAM_RW_BARRIER();
            DAM_WSTAMP(7);
            DAM_RW_COMMIT(lv2, dst2, KP, aff2);
            if (more) DAM_RW_SLOT0_B(Jn.X + img_off, Jn.dY + img_off, Jn.in_scale != nullptr);
            DAM_WSTAMP(5);
            DAM_RW_BARRIER();
            DAM_WSTAMP(7);
#undef DAM_RW_SLOT
            // the combine of the compute waves (below): its barriers, then this wave's share of the slab
#pragma unroll
            for (int w = 0; w < 4; ++w) DAM_RW_BARRIER();
            DAM_RW_WRITEOUT(J.partial, more);
        }
#undef DAM_RW_SLOT0_A
#undef DAM_RW_SLOT0_B
#undef DAM_RW_REQUEST
#undef DAM_RW_WRITE
#undef DAM_RW_COMMIT
    } else {
        // ================================ compute waves ================================
        const int cw = wave;
        const int lane_b = kq * 64 + j * 4;       // lane group kq owns cell 4t + kq of step t, lane j channel j of the cell
        // operand reads of step t + 1 against the MFMAs of step t: one read behind each of the first MFMAs (as a burst in front
        // of them the launch is 1.3-1.6 us slower: the pipe drains while seven reads issue).  MFMAs between two operand reads:
        // 2 measured -1.1 us on the four-loader 129x17 kernel, +0.5 us on the others
#define DAM_RW_SCHED()                                                                                                     \
    do {                                                                                                                   \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) {                                                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, NL == 4 ? 2 : 1, 0);                                               \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                             \
        }                                                                                                                  \
        __builtin_amdgcn_sched_group_barrier(0x008, 9 * TNB * TKB, 0);                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
    } while (0)
        // one (row, first cell, step stride) assignment of this wave for the slot: F = 1 a whole row part (the steady state),
        // F = 4 / 2 every fourth / second MFMA step of the one / two rows of a strip's last slot
#define DAM_RW_LOAD(T_, BUF_)                                                                                              \
    do {                                                                                                                   \
        _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                                 \
            av[BUF_][nb] = *reinterpret_cast<const float*>(smem + vd[nb] + (T_) * 256);                                    \
        _Pragma("unroll") for (int kb = 0; kb < TKB; ++kb)                                                                 \
            _Pragma("unroll") for (int a = 0; a < 3; ++a)                                                                  \
                _Pragma("unroll") for (int b = 0; b < 3; ++b)                                                              \
                    bv[BUF_][kb][a * 3 + b] = *reinterpret_cast<const float*>(smem + vx[kb][a] + ((T_) * 256 + b * 64));   \
    } while (0)
#define DAM_RW_ROW(F_, RW_, PART_, SUB_)                      /* steps SUB_, SUB_ + F_, ... of row RW_ of the slot */ \
    do {                                                                                                                   \
        int vx[TKB][3], vd[TNB];                                                                                           \
        _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                                    \
            const int xi = rw_mod<RW_NRX>(RPS * s + (RW_) + a);               /* row r - 1 + a relative to r_begin - 1 */  \
            _Pragma("unroll") for (int kb = 0; kb < TKB; ++kb) vx[kb][a] = lane_b + (XBASE - 64 + kb * XPLANE + xi * ROWB + (PART_)); \
        }                                                                                                                  \
        _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                                 \
            vd[nb] = lane_b + (DBASE + nb * DPLANE + ((RPS * s + (RW_)) & (RW_NRD - 1)) * ROWB + (PART_));                 \
        float av[2][TNB], bv[2][TKB][9];                                                                                   \
        constexpr int NS_ = (STEPS + (F_) - 1) / (F_);                                                                     \
        DAM_RW_LOAD(0, 0);                                                                                                 \
        _Pragma("unroll") for (int t = 0; t < NS_; ++t) {                                                                  \
            if ((F_) > 1 && (SUB_) + (F_) * t >= STEPS) break;                /* (scalar; last step of the split form only) */ \
            if (t + 1 < NS_) DAM_RW_LOAD((F_) * (t + 1), (t + 1) & 1);                                                     \
            _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                             \
                _Pragma("unroll") for (int kb = 0; kb < TKB; ++kb)                                                         \
                    _Pragma("unroll") for (int tap = 0; tap < 9; ++tap) {                                                  \
                        const int idx = (nb * TKB + kb) * 9 + tap;                                                         \
                        acc[idx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t & 1][nb], bv[t & 1][kb][tap], acc[idx], 0, 0, 0); \
                    }                                                                                                      \
            DAM_RW_SCHED();                                                                                                \
        }                                                                                                                  \
    } while (0)
        for (int job = 0; job < njobs; ++job) {
            v4f acc[NBLK];
#pragma unroll
            for (int i = 0; i < NBLK; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
            DAM_RW_ZERO();
            DAM_RW_BARRIER();                                                     // rows of slot 0 are in LDS, padding cleared
            DAM_WSTAMP(2);
            for (int s = 0; s < n_slots2; ++s) {
                const int rows_here = r_end - (r_begin + RPS * s);                // rows of this slot (<= 0: none)
                // a strip's last row: every fourth step per wave.  Only for the one-block tile: with 18 accumulator blocks a second
                // copy of the MFMA stream -- unrolled, rolled, or the same copy with an early exit (which halves its speed) -- makes
                // the register allocator spill (168 registers at three waves per SIMD)
                if (HV == 1 && TNB * TKB == 1 && rows_here == 1) {
                    DAM_RW_ROW(4, 0, cw * 256, cw);
                } else {
                    const int rw = cw / HV, half = cw - rw * HV;                  // row of the slot, part of the row
                    if (rw < rows_here) DAM_RW_ROW(1, rw, half * STEPS * 256, 0);
                }
                DAM_WSTAMP(5);
                DAM_RW_BARRIER();
                DAM_WSTAMP(7);
            }
            // combine the 4 compute waves through LDS (sequential adds: fixed order), one slab per workgroup and job; the last
            // slot's barrier is behind every wave's ring reads
            float* red = reinterpret_cast<float*>(smem);
            for (int w = 0; w < 4; ++w) {
                if (cw == w) {
#pragma unroll
                    for (int i = 0; i < NBLK; ++i) {
                        float4* d4 = reinterpret_cast<float4*>(red + (i * 64 + lane) * 4);
                        if (w == 0) {
                            *d4 = make_float4(acc[i].x, acc[i].y, acc[i].z, acc[i].w);
                        } else {
                            float4 o = *d4;
                            o.x += acc[i].x; o.y += acc[i].y; o.z += acc[i].z; o.w += acc[i].w;
                            *d4 = o;
                        }
                    }
                }
                DAM_RW_BARRIER();
            }
            DAM_RW_WRITEOUT(jobs.job[job].partial, job + 1 < njobs);
        }
    }
#undef DAM_RW_ROW
#undef DAM_RW_LOAD
#undef DAM_RW_SCHED
#undef DAM_RW_WRITEOUT
#undef DAM_RW_BARRIER
}

#undef DAM_RW_ZERO

// ---------------------------------------------------------------------------------------------------------------------
// Row-streaming variant for 3x3 / stride 2 / pad 1 (the first convolution of a down-sampling block,
// models/model_resnet.py:18-21 of the reference): the same workgroup shape, rings, slabs and reduce kernel as
// wgrad_rows_kernel, with the X rows kept as two column-parity planes so that all three column taps stay "dY cell + constant":
//
//   * X ring row = [odd plane | even plane], P4 cells of 16 channels each: odd cell e holds input column 2e-1 (cell 0 = the
//     left padding column), even cell e holds column 2e.  Output column ow reads tap 0 at odd cell ow, tap 1 at even cell ow
//     and tap 2 at odd cell ow+1; the dY ring row holds output column e in cell e (pitch P4 as well).
//   * Output row r reads X rows 2r-1, 2r, 2r+1.  A slot of RPS output rows brings in the 2*RPS rows 2r, 2r+1 of its output
//     rows (row 2*r_begin-1 comes with slot 0), so the X ring holds 2*RPS+1 rows in use + 2*RPS being written.
//   * one 16-channel chunk of X per workgroup (TKB = 1): the ring of two chunks does not fit beside the dY ring.
template <> __device__ __forceinline__ int rw_mod<18>(int v) { return v - ((v * 58255) >> 20) * 18; }     // v < 36000

// HV as in wgrad_rows_kernel; GPPX / GPPD: 1 KB pieces per X row plane (both parities) / dY row plane; KP planes per loader wave
template <int TNB, int STEPS, int KP, int GPPX, int GPPD, int HV>
__global__ __launch_bounds__(RW_THREADS) void wgrad_rows_s2_kernel(const RowsS2Geo g, const float* __restrict__ X,
                                                                   const float* __restrict__ dY, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NBLK = TNB * 9;
    constexpr int RPS = 4 / HV, NRX = 4 * RPS + 2, NRD = 2 * RPS;
    constexpr int P4 = STEPS * 4 * HV;
    constexpr int XROWB = 2 * P4 * 64, DROWB = P4 * 64;
    constexpr int XPLANE = NRX * XROWB, DPLANE = NRD * DROWB;
    constexpr int XBASE = RW_GUARD, DBASE = XBASE + XPLANE;
    constexpr int lds_bytes = DBASE + TNB * DPLANE + RW_TAIL;
    constexpr int NXP = 2 * RPS;                      // X planes a slot brings in
    constexpr int GPP = GPPX > GPPD ? GPPX : GPPD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, kq = lane >> 4;
    // XCD-aware placement as in wgrad_rows_kernel: the nx workgroups of a strip share an L2
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int nxg = gridDim.x, L = blockIdx.y * nxg + blockIdx.x, full = (gridDim.y >> 3) << 3;
        if (L < full * nxg) { const int c = L & 7, r = L >> 3; bx = r % nxg; by = (r / nxg) * 8 + c; }
    }
    const int tn = bx / g.tiles_k, tk = bx - tn * g.tiles_k;
    const int img = by / g.spi, sidx = by - img * g.spi;             // strips and their last slot as in wgrad_rows_kernel
    const int r_begin = (int)(((long long)sidx * g.Ho) / g.spi), r_end = (int)(((long long)(sidx + 1) * g.Ho) / g.spi);
    const int n_slots = (r_end - r_begin + RPS - 1) / RPS;
    const int n_slots2 = (n_slots + 1) & ~1;

#define DAM_RW_ZERO()                                                                                                      \
    do {                                                                                                                   \
        for (int e = tid * 16; e < lds_bytes; e += RW_THREADS * 16)                                                        \
            *reinterpret_cast<float4*>(smem + e) = make_float4(0.f, 0.f, 0.f, 0.f);                                        \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                                                    \
    } while (0)

    v4f acc[NBLK];
#pragma unroll
    for (int i = 0; i < NBLK; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};

    if (wave >= 4) {
        // ================================ loader waves ================================
        // plane cwl + 8k of a slot: the first NXP are X rows, the rest dY (row, out-channel block) planes -- which kind a
        // (wave, k) pair carries never changes, so the per-lane column offsets and write masks are set up once per k
        const int cwl = wave - 4;
        int loffb[KP][GPP];
        unsigned long long cmask[KP][GPP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const bool isx = cwl + RW_LOADERS * k < NXP;
#pragma unroll
            for (int gi = 0; gi < GPP; ++gi) {
                const int L = gi * 64 + lane, e = L >> 2, quad = L & 3;
                const int col = isx ? (e < P4 ? 2 * e - 1 : 2 * (e - P4)) : e;
                const int lim = isx ? g.W : g.Wo, cells = isx ? 2 * P4 : P4;
                const bool ok = e < cells && col >= 0 && col < lim;
                const int colc = col < 0 ? 0 : (col >= lim ? lim - 1 : col);
                loffb[k][gi] = (colc * (isx ? g.C : g.N) + quad * 4) * 4;
                cmask[k][gi] = __ballot(ok);
            }
        }
        const int ximg_bytes = g.H * g.W * g.C * 4, dimg_bytes = g.Ho * g.Wo * g.N * 4;
        const __amdgpu_buffer_rsrc_t xrsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X) + (size_t)img * g.H * g.W * g.C, 0, ximg_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t drsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dY) + (size_t)img * g.Ho * g.Wo * g.N, 0, dimg_bytes, 0x00020000);
        const int lane16 = lane * 16;
        const v4f zero4 = {0.f, 0.f, 0.f, 0.f};
        const int xrowstride = g.W * g.C * 4, drowstride = g.Wo * g.N * 4;
        const int x_first = 2 * r_begin - 1, x_last = 2 * r_end - 1;            // X rows this strip reads
        v4f lv[KP][GPP], lv2[KP][GPP], lvb[GPPX];
        int dst[KP], dst2[KP], dstb;   // scalar: LDS byte offset of the plane | 1 << 30 (row outside the image: zeros), -1 = none
        // X rows XR0_ .. XR0_+NXP-1, then dY rows DR0_ .. DR0_+RPS-1 (TNB planes each).  Loads are unconditional (clamped).
#define DAM_RW2_REQUEST(XR0_, DR0_, LV_, DST_)                                                                             \
    do {                                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < KP; ++k) {                                                                   \
            const int pl_ = cwl + RW_LOADERS * k;                                                                          \
            const bool isx_ = pl_ < NXP;                                                                                   \
            const int q_ = isx_ ? pl_ : pl_ - NXP;                                                                         \
            const int i_ = isx_ ? q_ : q_ / TNB, c_ = isx_ ? 0 : q_ - i_ * TNB;                                            \
            const int row_ = (isx_ ? (XR0_) : (DR0_)) + i_;                                                                \
            const bool need_ = isx_ ? row_ <= x_last : (i_ < RPS && row_ < r_end);                                         \
            const bool inimg_ = need_ && row_ >= 0 && row_ < (isx_ ? g.H : g.Ho);                                          \
            const int xi_ = rw_mod<NRX>(isx_ ? row_ - x_first : 0);                                                        \
            const int di_ = (row_ - r_begin) & (NRD - 1);                                                                  \
            const int ldsoff_ = isx_ ? XBASE + xi_ * XROWB : DBASE + c_ * DPLANE + di_ * DROWB;                            \
            const int soff_ = (inimg_ ? row_ : 0) * (isx_ ? xrowstride : drowstride) + (isx_ ? tk * 64 : (tn * TNB + c_) * 64); \
            if (isx_) {                                                                                                    \
                _Pragma("unroll") for (int gi = 0; gi < GPPX; ++gi)                                                        \
                    LV_[k][gi] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, loffb[k][gi], soff_, 0)); \
            } else {                                                                                                       \
                _Pragma("unroll") for (int gi = 0; gi < GPPD; ++gi)                                                        \
                    LV_[k][gi] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(drsrc, loffb[k][gi], soff_, 0)); \
            }                                                                                                              \
            DST_[k] = need_ ? (ldsoff_ | (inimg_ ? 0 : 1 << 30) | (isx_ ? 1 << 29 : 0)) : -1;                              \
        }                                                                                                                  \
    } while (0)
#define DAM_RW2_WRITE(ADDR_, DATA_, MASK_, GI_)                                                                            \
    asm volatile("s_mov_b64 exec, %2\n\tds_write_b128 %0, %1 offset:%3\n\ts_mov_b64 exec, -1"                              \
                 : : "v"(ADDR_), "v"(DATA_), "s"(MASK_), "n"((GI_) * 1024) : "memory")
#define DAM_RW2_COMMIT(LV_, DST_)                                                                                          \
    do {                                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < KP; ++k) {                                                                   \
            if (DST_[k] >= 0) {                                                                                            \
                const int va_ = lane16 + (DST_[k] & 0x1fffffff);                                                           \
                const bool zero_ = (DST_[k] >> 30) & 1;                                                                    \
                if ((DST_[k] >> 29) & 1) {                                                                                 \
                    _Pragma("unroll") for (int gi = 0; gi < GPPX; ++gi) {                                                  \
                        const v4f v_ = zero_ ? zero4 : LV_[k][gi];                                                         \
                        DAM_RW2_WRITE(va_, v_, cmask[k][gi], gi);                                                          \
                    }                                                                                                      \
                } else {                                                                                                   \
                    _Pragma("unroll") for (int gi = 0; gi < GPPD; ++gi) {                                                  \
                        const v4f v_ = zero_ ? zero4 : LV_[k][gi];                                                         \
                        DAM_RW2_WRITE(va_, v_, cmask[k][gi], gi);                                                          \
                    }                                                                                                      \
                }                                                                                                          \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)
        // slot 0: X rows 2*r_begin .. +NXP-1 and dY rows r_begin .. +RPS-1 like every slot, plus X row 2*r_begin-1 (loader
        // wave 0, whose k = 0 plane is an X plane: its offsets and masks apply)
        DAM_RW2_REQUEST(2 * r_begin, r_begin, lv, dst);
        {
            const bool inimg = x_first >= 0;
            const int soff = (inimg ? x_first : 0) * xrowstride + tk * 64;
#pragma unroll
            for (int gi = 0; gi < GPPX; ++gi)
                lvb[gi] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, loffb[0][gi], soff, 0));
            dstb = cwl == 0 ? (XBASE | (inimg ? 0 : 1 << 30)) : -1;
        }
        DAM_RW_ZERO();
        DAM_RW2_COMMIT(lv, dst);
        if (dstb >= 0) {
            const int va = lane16 + (dstb & 0x1fffffff);
#pragma unroll
            for (int gi = 0; gi < GPPX; ++gi) {
                const v4f v = (dstb >> 30) & 1 ? zero4 : lvb[gi];
                DAM_RW2_WRITE(va, v, cmask[0][gi], gi);
            }
        }
        // steady state as in wgrad_rows_kernel: slot s writes the rows of slot s+1 and requests those of slot s+3
#define DAM_RW2_SLOT(T_, LV_, DST_) DAM_RW2_REQUEST(2 * (r_begin + RPS * (T_)), r_begin + RPS * (T_), LV_, DST_)
        DAM_RW2_SLOT(1, lv, dst);
        DAM_RW2_SLOT(2, lv2, dst2);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        for (int s = 0; s < n_slots2; s += 2) {
            DAM_RW2_COMMIT(lv, dst);
            DAM_RW2_SLOT(s + 3, lv, dst);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            DAM_RW2_COMMIT(lv2, dst2);
            DAM_RW2_SLOT(s + 4, lv2, dst2);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
#undef DAM_RW2_SLOT
#undef DAM_RW2_REQUEST
#undef DAM_RW2_WRITE
#undef DAM_RW2_COMMIT
    } else {
        // ================================ compute waves ================================
        const int cw = wave;
        const int lane_b = kq * 64 + j * 4;       // lane group kq owns cell 4t + kq of step t, lane j channel j of the cell
        DAM_RW_ZERO();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // rows of slot 0 are in LDS
        // (the operand reads interleaved with the MFMAs as in wgrad_rows_kernel measured SLOWER here: 42.0 -> 43.6, 40.3 -> 42.2,
        // 46.2 -> 47.0 us)
        // column taps: odd-plane cell ow, even-plane cell ow, odd-plane cell ow + 1
#define DAM_RW2_LOAD(T_, BUF_)                                                                                             \
    do {                                                                                                                   \
        _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                                 \
            av[BUF_][nb] = *reinterpret_cast<const float*>(smem + vd[nb] + (T_) * 256);                                    \
        _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                                    \
            bv[BUF_][a * 3 + 0] = *reinterpret_cast<const float*>(smem + vx[a] + (T_) * 256);                              \
            bv[BUF_][a * 3 + 1] = *reinterpret_cast<const float*>(smem + vx[a] + ((T_) * 256 + P4 * 64));                  \
            bv[BUF_][a * 3 + 2] = *reinterpret_cast<const float*>(smem + vx[a] + ((T_) * 256 + 64));                       \
        }                                                                                                                  \
    } while (0)
#define DAM_RW2_ROW(F_, RW_, PART_, SUB_)                     /* as DAM_RW_ROW of wgrad_rows_kernel */                      \
    do {                                                                                                                   \
        int vx[3], vd[TNB];                                                                                                \
        _Pragma("unroll") for (int a = 0; a < 3; ++a)                         /* X row 2r - 1 + a, relative to 2*r_begin - 1 */ \
            vx[a] = lane_b + (XBASE + rw_mod<NRX>(2 * (RPS * s + (RW_)) + a) * XROWB + (PART_));                           \
        _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                                 \
            vd[nb] = lane_b + (DBASE + nb * DPLANE + ((RPS * s + (RW_)) & (NRD - 1)) * DROWB + (PART_));                   \
        float av[2][TNB], bv[2][9];                                                                                        \
        constexpr int NS_ = (STEPS + (F_) - 1) / (F_);                                                                     \
        DAM_RW2_LOAD(0, 0);                                                                                                \
        _Pragma("unroll") for (int t = 0; t < NS_; ++t) {                                                                  \
            if ((F_) > 1 && (SUB_) + (F_) * t >= STEPS) break;                                                             \
            if (t + 1 < NS_) DAM_RW2_LOAD((F_) * (t + 1), (t + 1) & 1);                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
            _Pragma("unroll") for (int nb = 0; nb < TNB; ++nb)                                                             \
                _Pragma("unroll") for (int tap = 0; tap < 9; ++tap)                                                        \
                    acc[nb * 9 + tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t & 1][nb], bv[t & 1][tap], acc[nb * 9 + tap], 0, 0, 0); \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
        }                                                                                                                  \
    } while (0)
        for (int s = 0; s < n_slots2; ++s) {
            const int rows_here = r_end - (r_begin + RPS * s);                // rows of this slot (<= 0: none)
            if (HV == 1 && TNB == 1 && rows_here == 1) {
                DAM_RW2_ROW(4, 0, cw * 256, cw);
            } else {
                const int rw = cw / HV, half = cw - rw * HV;                  // row of the slot, part of the row
                if (rw < rows_here) DAM_RW2_ROW(1, rw, half * STEPS * 256, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    }
#undef DAM_RW2_ROW
#undef DAM_RW2_LOAD
#undef DAM_RW_ZERO

    // combine the 4 compute waves through LDS (sequential adds: fixed order), one slab per workgroup
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NBLK; ++i) {
                float4* d4 = reinterpret_cast<float4*>(red + (i * 64 + lane) * 4);
                if (w == 0) {
                    *d4 = make_float4(acc[i].x, acc[i].y, acc[i].z, acc[i].w);
                } else {
                    float4 o = *d4;
                    o.x += acc[i].x; o.y += acc[i].y; o.z += acc[i].z; o.w += acc[i].w;
                    *d4 = o;
                }
            }
        }
        __syncthreads();
    }
    float4* out = reinterpret_cast<float4*>(partial) + ((size_t)by * gridDim.x + bx) * NBLK * 64;
    for (int e = tid; e < NBLK * 64; e += RW_THREADS) out[e] = reinterpret_cast<const float4*>(red)[e];
}

// ---------------------------------------------------------------------------------------------------------------------
// Direct variant: nothing goes through LDS.  dW[n][k][a][b] = sum over output pixels of dY[p][n] * X[s*p + tap][k]; a
// wave walks whole output rows, lane = (pixel 4t + kq, channel j), both MFMA operands are buffer loads (dword per lane,
// 64-byte segments) straight from HBM / L2 -- every X element is wanted by at most KH*KW/s^2 taps and those re-reads are
// L2 hits.  Addresses are linear in t; lanes past the row end or on a padding column get an out-of-range offset and read
// 0; a tap row outside the image is skipped (scalar branch).  U steps of loads are in flight per wave.
//   1x1: the strided shortcut of a down-sampling block (models/model_resnet.py:18-21) -- a skinny memory-bound GEMM;
//   3x3: the strided first convolution of those blocks (a staged patch would hold both column parities of every row).
// Output: the same partial slabs + reduce kernel as the other variants.
// (bx, by) of a (gx, gy) grid: the launch's own block indices, or a job's share of a batched launch
template <int TNB, int TKB, int KH, int KW>
__device__ __forceinline__ void wgrad_direct_body(const float* __restrict__ X, const float* __restrict__ dY, int rows, int Ho, int Wo,
                                                  int H, int W, int C, int N, int s, int pad, int dil, int tiles_k,
                                                  float* __restrict__ partial, int bx, int by, int gx, int gy) {
    constexpr int NBLK = TNB * TKB * KH * KW, U = KH * KW == 1 ? 8 : 4;
    __shared__ float4 red[NBLK * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const int tn = bx / tiles_k, tk = bx - tn * tiles_k;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dY), 0, 0x7fffffff, 0x00020000);
    v4f acc[NBLK];
#pragma unroll
    for (int i = 0; i < NBLK; ++i) acc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
    const int steps = (Wo + 3) >> 2;
    const int lane_x = (kq * s * C + tk * TKB * 16 + j) * 4, lane_d = (kq * N + tn * TNB * 16 + j) * 4;   // bytes
    const int step_x = 4 * s * C * 4, step_d = 4 * N * 4;
    for (int row = by * 4 + wave; row < rows; row += gy * 4) {        // row = (image, output row)
        const int img = row / Ho, oh = row - img * Ho;
        const int ds = (int)(((int64_t)row * Wo) * N * 4);                           // scalar byte offsets (< 2^31: host check)
        for (int t0 = 0; t0 < steps; t0 += U) {
            float av[U][TNB];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u;
                const int vd = (t < steps && 4 * t + kq < Wo) ? lane_d + t * step_d : 0x7fffffff;
#pragma unroll
                for (int nb = 0; nb < TNB; ++nb)
                    av[u][nb] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dr, vd + nb * 64, ds, 0));
            }
#pragma unroll
            for (int a = 0; a < KH; ++a) {
                const int ih = oh * s + a * dil - pad;
                if (ih < 0 || ih >= H) continue;                                     // wave-uniform
                const int xs = (int)(((int64_t)(img * H + ih) * W) * C * 4);
                float bv[U][KW][TKB];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = t0 + u;
#pragma unroll
                    for (int b = 0; b < KW; ++b) {
                        const int iw = (4 * t + kq) * s + b * dil - pad;
                        const int vx = (t < steps && 4 * t + kq < Wo && iw >= 0 && iw < W) ? lane_x + t * step_x + (b * dil - pad) * C * 4
                                                                                         : 0x7fffffff;
#pragma unroll
                        for (int kb = 0; kb < TKB; ++kb)
                            bv[u][b][kb] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, vx + kb * 64, xs, 0));
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int nb = 0; nb < TNB; ++nb)
#pragma unroll
                        for (int kb = 0; kb < TKB; ++kb)
#pragma unroll
                            for (int b = 0; b < KW; ++b) {
                                const int idx = ((nb * TKB + kb) * KH + a) * KW + b;
                                acc[idx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][nb], bv[u][b][kb], acc[idx], 0, 0, 0);
                            }
            }
        }
    }
    for (int w = 0; w < 4; ++w) {            // combine the 4 waves in fixed order
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NBLK; ++i) {
                float4 o = w == 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : red[i * 64 + lane];
                o.x += acc[i].x; o.y += acc[i].y; o.z += acc[i].z; o.w += acc[i].w;
                red[i * 64 + lane] = o;
            }
        }
        __syncthreads();
    }
    float4* out = reinterpret_cast<float4*>(partial) + ((size_t)by * gx + bx) * NBLK * 64;
    for (int e = tid; e < NBLK * 64; e += 256) out[e] = red[e];
}

template <int TNB, int TKB, int KH, int KW>
__global__ __launch_bounds__(256) void wgrad_direct_kernel(const float* __restrict__ X, const float* __restrict__ dY, int rows,
                                                           int Ho, int Wo, int H, int W, int C, int N, int s, int pad, int dil,
                                                           int tiles_k, float* __restrict__ partial) {
    wgrad_direct_body<TNB, TKB, KH, KW>(X, dY, rows, Ho, Wo, H, W, C, N, s, pad, dil, tiles_k, partial, blockIdx.x, blockIdx.y,
                                        gridDim.x, gridDim.y);
}

// Direct launches of ONE instantiation and DIFFERENT geometries in one launch (round 5): the 1x1 shortcut convolutions of the
// four 32 -> 256-channel down-sampling blocks (models/model_resnet.py:18-21) are 11-16 us launches of a memory- and latency-bound
// kernel, leaves of the backward pass; recorded in a batching queue they run as one flat grid at the flush (a workgroup finds its
// job by the prefix sums `wg0`), the jobs sharing the chip's workgroup slots (launch_pending_direct).
template <int TNB, int TKB, int KH, int KW>
__global__ __launch_bounds__(256) void wgrad_direct_batch_kernel(const DirectJobs jobs) {
    int ji = 0;
    while (ji + 1 < jobs.njobs && (int)blockIdx.x >= jobs.job[ji + 1].wg0) ++ji;
    const DirectJob& j = jobs.job[ji];
    const int li = (int)blockIdx.x - j.wg0;
    wgrad_direct_body<TNB, TKB, KH, KW>(j.X, j.dY, j.rows, j.Ho, j.Wo, j.H, j.W, j.C, j.N, j.s, j.pad, j.dil, j.tiles_k, j.partial,
                                        li % j.nx, li / j.nx, j.nx, j.nsplit);
}

// ---------------------------------------------------------------------------------------------------------------------
// Launch from the plan (dam_wgrad_plan.h).  Nothing is decided here: a launcher holds the table from the note's template parameters
// to the instantiation -- generated from the plan header's instantiation lists, so a kernel exists exactly for the rows of those
// lists --, the LDS limit, the queue logic, the launch and the slab reduction.

// f(integral_constant<int, I>) for the row I of an N-row instantiation list that `match` picks; DAM_ERR_LAUNCH: the note names none
template <int N, int I = 0, class Match, class F>
int with_inst(Match match, F f) {
    if constexpr (I == N) return DAM_ERR_LAUNCH;
    else return match(I) ? f(std::integral_constant<int, I>()) : with_inst<N, I + 1>(match, f);
}
bool same_inst(const WgradLaunchNote& a, const WgradLaunchNote& b) { return a.TNB == b.TNB && a.TKB == b.TKB && a.TA == b.TA && a.TB == b.TB; }

// The one write of the record: where a launcher has passed its last refusal, before it launches (or records the launch).
void commit(const WgradPlan& p) { wgrad_last_launch = p.note; }

bool rows_inst_is(const WgradLaunchNote& n, int i) {
    const RowsInst& t = ROWS_INST[i];
    return n.TNB == t.TNB && n.TKB == t.TKB && n.STEPS == t.STEPS && n.KP == t.KP && n.GPP == t.GPP && n.HV == t.HV && n.NL == t.NL;
}
// The LDS limit of the note's row instantiation, raised.
int rows_lds_ready(const WgradLaunchNote& n) {
    return with_inst<ROWS_INST_N>([&](int i) { return rows_inst_is(n, i); }, [&](auto I) -> int {
        constexpr RowsInst t = ROWS_INST[I];
        return raise_lds_limit<&wgrad_rows_kernel<t.TNB, t.TKB, t.STEPS, t.KP, t.GPP, t.HV, t.NL>>(160 * 1024) ? DAM_OK : DAM_ERR_LAUNCH;
    });
}
// One launch of the row kernel for the jobs of the table (plan p: instantiation, geometry and grid of every one).
int launch_rows_jobs(const WgradPlan& p, const RowsJobs& jobs, hipStream_t st) {
    return with_inst<ROWS_INST_N>([&](int i) { return rows_inst_is(p.note, i); }, [&](auto I) -> int {
        constexpr RowsInst t = ROWS_INST[I];
        hipLaunchKernelGGL((wgrad_rows_kernel<t.TNB, t.TKB, t.STEPS, t.KP, t.GPP, t.HV, t.NL>), dim3(p.nx, p.nsplit), dim3(256 + 64 * t.NL),
                           p.lds, st, p.rows, jobs);
        DAM_CHECK_LAUNCH();
        return DAM_OK;
    });
}

// The recorded row launches of a queue, as one launch (and nothing pending afterwards, whatever the outcome), then their reductions.
int launch_pending_rows(WgradQueue* q, hipStream_t st) {
    PendingRows& p = q->pend_rows;
    const int n = p.jobs.njobs;
    p.jobs.njobs = 0;
    if (n <= 0) return DAM_OK;
    RowsJobs jobs = p.jobs;
    jobs.njobs = n;
    int rc = launch_rows_jobs(p.plan, jobs, st);
    for (int i = 0; i < n && rc == DAM_OK; ++i) rc = reduce_submit(q, jobs.job[i].partial, p.dw[i], p.plan.nsplit, p.plan.nx, p.red[i], st);
    return rc;
}

int launch_rows(const WgradPlan& p, const WgradOperands& a, void* queue, hipStream_t st) {
    WgradQueue* q = static_cast<WgradQueue*>(queue);
    if (q && q->magic != WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    const int rc = rows_lds_ready(p.note);
    if (rc != DAM_OK) return rc;
    const RowsJob j{a.x, a.dy, a.in_scale, a.in_shift, a.workspace, p.relu_in, 0};
    if (p.note.issued == WGRAD_LAUNCH_RECORDED) {
        // record instead of launching: jobs of one instantiation, geometry and grid wait for each other until the queue is flushed,
        // another kind arrives or the table is full; the caller keeps X, dY, the affine and the slabs valid until then
        PendingRows& pr = q->pend_rows;
        const WgradLaunchNote& o = pr.plan.note;
        const bool same = o.TNB == p.note.TNB && o.TKB == p.note.TKB && o.STEPS == p.note.STEPS && o.KP == p.note.KP && o.GPP == p.note.GPP &&
                          o.HV == p.note.HV && o.NL == p.note.NL && memcmp(&pr.plan.rows, &p.rows, sizeof(RowsGeo)) == 0 &&
                          pr.plan.nx == p.nx && pr.plan.nsplit == p.nsplit && pr.plan.lds == p.lds;
        if (pr.jobs.njobs > 0 && (pr.jobs.njobs == ROWS_MAX_JOBS || !same)) {
            const int rc2 = launch_pending_rows(q, st);
            if (rc2 != DAM_OK) return rc2;
        }
        const int i = pr.jobs.njobs++;
        pr.plan = p; pr.jobs.job[i] = j; pr.dw[i] = a.dw; pr.red[i] = p.red;
        commit(p);
        return DAM_OK;
    }
    commit(p);
    RowsJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    jobs.job[0] = j; jobs.njobs = 1;
    const int rc1 = launch_rows_jobs(p, jobs, st);
    return rc1 != DAM_OK ? rc1 : reduce_submit(queue, a.workspace, a.dw, p.nsplit, p.nx, p.red, st);
}

int launch_rows_s2(const WgradPlan& p, const WgradOperands& a, void* queue, hipStream_t st) {
    const WgradLaunchNote& n = p.note;
    auto match = [&](int i) {
        const RowsS2Inst& t = ROWS_S2_INST[i];
        return n.TNB == t.TNB && n.STEPS == t.STEPS && n.KP == t.KP && n.GPP == t.GPPX && n.GPPD == t.GPPD && n.HV == t.HV;
    };
    return with_inst<ROWS_S2_INST_N>(match, [&](auto I) -> int {
        constexpr RowsS2Inst t = ROWS_S2_INST[I];
        constexpr int RPS = 4 / t.HV, NRX = 4 * RPS + 2, P4 = t.STEPS * 4 * t.HV;
        static_assert(NRX == 18 || NRX == 10, "ring sizes with a multiply-shift modulo");
        static_assert((2 * RPS + RPS * t.TNB + RW_LOADERS - 1) / RW_LOADERS <= t.KP, "planes per loader wave");
        static_assert(2 * P4 * 64 <= t.GPPX * 1024 && P4 * 64 <= t.GPPD * 1024, "pieces per plane");
        if (!raise_lds_limit<&wgrad_rows_s2_kernel<t.TNB, t.STEPS, t.KP, t.GPPX, t.GPPD, t.HV>>(160 * 1024)) return DAM_ERR_LAUNCH;
        commit(p);
        hipLaunchKernelGGL((wgrad_rows_s2_kernel<t.TNB, t.STEPS, t.KP, t.GPPX, t.GPPD, t.HV>), dim3(p.nx, p.nsplit), dim3(RW_THREADS), p.lds,
                           st, p.rows_s2, a.x, a.dy, a.workspace);
        DAM_CHECK_LAUNCH();
        return reduce_submit(queue, a.workspace, a.dw, p.nsplit, p.nx, p.red, st);
    });
}

// The direct kernel of the note's instantiation: job j alone on its own (nx, nsplit) grid, or (batch given) the batch's flat grid.
int launch_direct_kernel(const WgradLaunchNote& n, const DirectJob& j, const DirectJobs* batch, int total, hipStream_t st) {
    auto match = [&](int i) { return n.TNB == DIRECT_INST[i].TNB && n.TKB == DIRECT_INST[i].TKB && n.TA == DIRECT_INST[i].K && n.TB == n.TA; };
    return with_inst<DIRECT_INST_N>(match, [&](auto I) -> int {
        constexpr DirectInst t = DIRECT_INST[I];
        if (batch) {
            hipLaunchKernelGGL((wgrad_direct_batch_kernel<t.TNB, t.TKB, t.K, t.K>), dim3(total), dim3(256), 0, st, *batch);
        } else {
            hipLaunchKernelGGL((wgrad_direct_kernel<t.TNB, t.TKB, t.K, t.K>), dim3(j.nx, j.nsplit), dim3(256), 0, st, j.X, j.dY, j.rows, j.Ho,
                               j.Wo, j.H, j.W, j.C, j.N, j.s, j.pad, j.dil, j.tiles_k, j.partial);
        }
        DAM_CHECK_LAUNCH();
        return DAM_OK;
    });
}

// The recorded direct launches of a queue, as one launch (and nothing pending afterwards, whatever the outcome).
int launch_pending_direct(WgradQueue* q, hipStream_t st) {
    PendingDirect& p = q->pend_direct;
    const int n = p.jobs.njobs;
    p.jobs.njobs = 0;
    if (n <= 0) return DAM_OK;
    // Pixel splits: alone, a launch wants 3-4 workgroups per CU (`nsplit` as recorded); n jobs in one launch fill the chip
    // together, so each takes its share -- a quarter of the slabs to write and to reduce, four times the rows per wave (the
    // 129 x 17 shortcut had ONE 17-pixel row per wave: 40 us for the four jobs, 8.4 MB of slabs for a 32 KB gradient).  A batch of
    // one keeps the split of the plain launch (bitwise the same slabs).
    int total = 0;
    for (int i = 0; i < n; ++i) {
        DirectJob& j = p.jobs.job[i];
        if (n > 1) {
            const int share = (int)cdiv(1536, (int64_t)n * j.nx);
            if (share < j.nsplit) j.nsplit = share < 1 ? 1 : share;
        }
        j.wg0 = total;
        total += j.nx * j.nsplit;
    }
    DirectJobs jobs = p.jobs;
    jobs.njobs = n;
    int rc = launch_direct_kernel(p.note, jobs.job[0], &jobs, total, st);
    for (int i = 0; i < n && rc == DAM_OK; ++i) {
        const DirectJob& j = jobs.job[i];
        rc = reduce_submit(q, j.partial, p.dw[i], j.nsplit, j.nx, p.red[i], st);
    }
    return rc;
}

int launch_direct(const WgradPlan& p, const WgradOperands& a, void* queue, hipStream_t st) {
    WgradQueue* q = static_cast<WgradQueue*>(queue);
    if (q && q->magic != WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    DirectJob j = p.direct;
    j.X = a.x; j.dY = a.dy; j.partial = a.workspace;
    if (p.note.issued == WGRAD_LAUNCH_RECORDED) {
        // record instead of launching: launches of this instantiation wait for each other until the queue is flushed (the caller
        // keeps X, dY and the slabs valid until then: the batching contract of include/dam_hip.h)
        PendingDirect& pd = q->pend_direct;
        if (pd.jobs.njobs > 0 && (!same_inst(pd.note, p.note) || pd.jobs.njobs == WD_MAX_JOBS)) {
            const int rc = launch_pending_direct(q, st);
            if (rc != DAM_OK) return rc;
        }
        const int i = pd.jobs.njobs++;
        pd.note = p.note; pd.jobs.job[i] = j; pd.dw[i] = a.dw; pd.red[i] = p.red;
        commit(p);
        return DAM_OK;
    }
    commit(p);
    const int rc = launch_direct_kernel(p.note, j, nullptr, 0, st);
    return rc != DAM_OK ? rc : reduce_submit(queue, a.workspace, a.dw, p.nsplit, p.nx, p.red, st);
}

bool tile_inst_is(const WgradLaunchNote& n, int i) {
    return n.TNB == TILE_INST[i].TNB && n.TKB == TILE_INST[i].TKB && n.TA == TILE_INST[i].TA && n.TB == TILE_INST[i].TB;
}
// The LDS limit of the note's instantiation, raised where the launch needs more than the default.
int tile_lds_ready(const WgradLaunchNote& n, size_t lds) {
    return with_inst<TILE_INST_N>([&](int i) { return tile_inst_is(n, i); }, [&](auto I) -> int {
        constexpr TileInst t = TILE_INST[I];
        return lds <= 64 * 1024 || raise_lds_limit<&wgrad_kernel<t.TNB, t.TKB, t.TA, t.TB>>(160 * 1024) ? DAM_OK : DAM_ERR_LAUNCH;
    });
}
// One launch of the tile kernel for `njobs` weight gradients of geometry g (blockIdx.z = job), then their slab reductions.
int launch_tile_jobs(const WgradLaunchNote& n, const WgradGeo& g, size_t lds, const WgradJobs& jobs, int njobs, float* const* dw,
                     const WgradReduce* red, void* queue, hipStream_t st) {
    const int nx = g.tiles_n * g.tiles_k * g.tap_groups;
    int rc = with_inst<TILE_INST_N>([&](int i) { return tile_inst_is(n, i); }, [&](auto I) -> int {
        constexpr TileInst t = TILE_INST[I];
        hipLaunchKernelGGL((wgrad_kernel<t.TNB, t.TKB, t.TA, t.TB>), dim3(nx, g.nsplit, njobs), dim3(256), lds, st, g, jobs);
        DAM_CHECK_LAUNCH();
        return DAM_OK;
    });
    for (int i = 0; i < njobs && rc == DAM_OK; ++i) rc = reduce_submit(queue, jobs.partial[i], dw[i], g.nsplit, nx, red[i], st);
    return rc;
}

// The recorded tile launches of a queue, as one launch (and nothing pending afterwards, whatever the outcome): the refusals a
// recorded call had ahead of it -- pixel split for this number of jobs in the smallest workspace, LDS size, LDS limit -- are met here.
int launch_pending_tile(WgradQueue* q, hipStream_t st) {
    PendingTile& p = q->pend;
    const int n = p.njobs;
    p.njobs = 0;
    if (n <= 0) return DAM_OK;
    int64_t ws = p.ws_floats[0];
    for (int i = 1; i < n; ++i) ws = p.ws_floats[i] < ws ? p.ws_floats[i] : ws;
    const int NBLK = p.note.TNB * p.note.TKB * p.note.TA * p.note.TB;
    size_t lds = tile_lds(p.g, p.note.TNB, p.note.TKB);
    if (lds < (size_t)NBLK * 1024) lds = (size_t)NBLK * 1024;
    WgradGeo g = p.g;
    g.nsplit = plan_tile_split(g, NBLK, lds, n, ws);
    if (!g.nsplit) return DAM_ERR_WORKSPACE;
    if (lds > 160 * 1024) return DAM_ERR_UNSUPPORTED;
    const int rc = tile_lds_ready(p.note, lds);
    return rc != DAM_OK ? rc : launch_tile_jobs(p.note, g, lds, p.jobs, n, p.dw, p.red, q, st);
}

int launch_tile(const WgradPlan& p, const WgradOperands& a, void* queue, hipStream_t st) {
    WgradQueue* q = static_cast<WgradQueue*>(queue);
    if (q && q->magic != WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    if (p.note.issued == WGRAD_LAUNCH_RECORDED) {
        // record instead of launching: jobs of the same instantiation and geometry wait for each other until the queue is
        // flushed (or another geometry arrives); the caller keeps X, dY, the affine and the slabs valid until then
        PendingTile& pt = q->pend;
        if (pt.njobs > 0 && (!same_inst(pt.note, p.note) || memcmp(&pt.g, &p.tile, sizeof(WgradGeo)) != 0 || pt.njobs == WG_MAX_JOBS)) {
            const int rc = launch_pending_tile(q, st);
            if (rc != DAM_OK) return rc;
        }
        const int i = pt.njobs++;
        pt.note = p.note; pt.g = p.tile;
        pt.jobs.X[i] = a.x; pt.jobs.dY[i] = a.dy; pt.jobs.sc[i] = a.in_scale; pt.jobs.sh[i] = a.in_shift; pt.jobs.partial[i] = a.workspace;
        pt.jobs.relu_in[i] = p.relu_in;
        pt.dw[i] = a.dw; pt.ws_floats[i] = p.workspace_floats; pt.red[i] = p.red;
        commit(p);
        return DAM_OK;
    }
    const int rc = tile_lds_ready(p.note, p.lds);
    if (rc != DAM_OK) return rc;
    commit(p);
    WgradJobs jobs;
    memset(&jobs, 0, sizeof(jobs));
    jobs.X[0] = a.x; jobs.dY[0] = a.dy; jobs.sc[0] = a.in_scale; jobs.sh[0] = a.in_shift; jobs.partial[0] = a.workspace;
    jobs.relu_in[0] = p.relu_in;
    return launch_tile_jobs(p.note, p.tile, p.lds, jobs, 1, &a.dw, &p.red, queue, st);
}

void note_to_ints(const WgradLaunchNote& n, int* out16) {
    const int v[16] = {n.family, n.TNB, n.TKB, n.STEPS, n.KP, n.GPP, n.GPPD, n.HV, n.NL, n.TA, n.TB, n.nx, n.nsplit, n.spi_tmw, n.rps,
                       n.issued};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
}

}  // namespace
}  // namespace dam

extern "C" int64_t dam_wgrad_queue_bytes(void) { return (int64_t)sizeof(dam::WgradQueue); }

extern "C" int dam_wgrad_queue_init(void* queue) {
    if (!queue) return DAM_ERR_BAD_ARG;
    dam::WgradQueue* q = static_cast<dam::WgradQueue*>(queue);
    const int batching = q->magic == dam::WGRAD_QUEUE_MAGIC ? q->batching : 0;      // re-initialising keeps the mode
    memset(q, 0, sizeof(*q));
    q->magic = dam::WGRAD_QUEUE_MAGIC;
    q->batching = batching;
    return DAM_OK;
}

extern "C" int dam_wgrad_queue_set_batching(void* queue, int on) {
    dam::WgradQueue* q = static_cast<dam::WgradQueue*>(queue);
    if (!q || q->magic != dam::WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    if (on < 0 || on > 2) return DAM_ERR_BAD_ARG;
    // between the two batching modes the queue may hold recorded launches (the mode says what becomes of the NEXT call; what is
    // recorded runs at the flush either way); switching batching off or on needs an empty queue
    const bool pending = q->pend.njobs > 0 || q->pend_direct.jobs.njobs > 0 || q->pend_rows.jobs.njobs > 0;
    if (pending && (on == 0 || q->batching == 0)) return DAM_ERR_BAD_ARG;                      // flush first
    q->batching = on;
    return DAM_OK;
}

extern "C" int dam_wgrad_queue_pending(const void* queue) {
    const dam::WgradQueue* q = static_cast<const dam::WgradQueue*>(queue);
    return q && q->magic == dam::WGRAD_QUEUE_MAGIC ? q->batch.njobs + q->pend.njobs + q->pend_direct.jobs.njobs + q->pend_rows.jobs.njobs
                                                   : -1;
}

extern "C" int dam_wgrad_queue_flush(void* queue, void* stream) {
    dam::WgradQueue* q = static_cast<dam::WgradQueue*>(queue);
    if (!q || q->magic != dam::WGRAD_QUEUE_MAGIC) return DAM_ERR_BAD_ARG;
    int rc = dam::launch_pending_rows(q, (hipStream_t)stream);
    if (rc == DAM_OK) rc = dam::launch_pending_tile(q, (hipStream_t)stream);
    if (rc == DAM_OK) rc = dam::launch_pending_direct(q, (hipStream_t)stream);
    return rc != DAM_OK ? rc : dam::reduce_flush(q->batch, (hipStream_t)stream);
}

extern "C" int dam_wgrad_last_launch(int* out16_host) {
    if (!out16_host) return DAM_ERR_BAD_ARG;
    dam::note_to_ints(dam::wgrad_last_launch, out16_host);
    return DAM_OK;
}

extern "C" int64_t dam_conv2d_wgrad_workspace_floats(int n_out, int c_in, int kh, int kw) {
    if (n_out <= 0 || c_in <= 0 || kh <= 0 || kw <= 0) return 0;
    // enough for ~512 workgroup slabs of the largest tile, and at least 4 splits of the whole gradient
    const int64_t whole = dam::cdiv(n_out, 32) * dam::cdiv(c_in, 32) * 4 * 256 * (int64_t)kh * kw;
    const int64_t a = 512LL * 36 * 256 + 4 * whole;
    return a;
}

extern "C" int dam_conv2d_wgrad_plan(int B, int H, int W, int C, int in_nchw, int relu_in, int Ho, int Wo, int n_chan, int n_out, int kh,
                                     int kw, int stride, int pad, int dil, int c_real, int has_affine, int has_shift, int queue_mode,
                                     int64_t workspace_floats, int* out16_host) {
    using namespace dam;
    if (!out16_host) return DAM_ERR_BAD_ARG;
    WgradPlan plan{};
    const WgradRequest rq{B, H, W, C, in_nchw, relu_in, Ho, Wo, n_chan, n_out, kh, kw, stride, pad, dil, c_real, has_affine != 0,
                          has_shift != 0, workspace_floats, queue_mode};
    const int rc = !wgrad_queue_mode_ok(queue_mode) ? DAM_ERR_BAD_ARG : plan_wgrad(rq, plan);
    note_to_ints(plan.note, out16_host);     // (all zero on any refusal)
    return rc;
}

extern "C" int dam_conv2d_wgrad_f32(const float* x, int B, int H, int W, int C, int in_nchw, const float* in_scale,
                                    const float* in_shift, int relu_in, const float* dy, int Ho, int Wo, int n_chan,
                                    int n_out, int kh, int kw, int stride, int pad, int dil, float* dw, int c_real,
                                    float* workspace, int64_t workspace_floats, void* reduce_queue, void* stream) {
    using namespace dam;
    wgrad_last_launch = WgradLaunchNote{};
    if (!x || !dy || !dw || !workspace) return DAM_ERR_BAD_ARG;
    // (a queue that is none -- wrong magic -- plans as one without batching and is refused by the launcher)
    const WgradQueue* q = static_cast<const WgradQueue*>(reduce_queue);
    const WgradRequest rq{B, H, W, C, in_nchw, relu_in, Ho, Wo, n_chan, n_out, kh, kw, stride, pad, dil, c_real, in_scale != nullptr,
                          in_shift != nullptr, workspace_floats,
                          !q ? 0 : q->magic != WGRAD_QUEUE_MAGIC || !q->batching ? 1 : q->batching == 2 ? 4 : 2};
    WgradPlan plan;
    const int rc = plan_wgrad(rq, plan);
    if (rc != DAM_OK) return rc;
    const WgradOperands a{x, dy, in_scale, in_shift, workspace, dw};
    hipStream_t st = (hipStream_t)stream;
    switch (plan.note.family) {
        case WGRAD_FAM_ROWS: return launch_rows(plan, a, reduce_queue, st);
        case WGRAD_FAM_ROWS_S2: return launch_rows_s2(plan, a, reduce_queue, st);
        case WGRAD_FAM_DIRECT: return launch_direct(plan, a, reduce_queue, st);
        default: return launch_tile(plan, a, reduce_queue, st);
    }
}
