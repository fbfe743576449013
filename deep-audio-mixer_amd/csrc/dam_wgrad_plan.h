// Dispatch of dam_conv2d_wgrad_f32 as a value: which kernel family and instantiation a call gets, with the geometry that kernel
// receives, its grid and the parameters of its slab reduction.  Planning is host arithmetic only -- no HIP call, no device pointer,
// no queue -- so dam_conv2d_wgrad_plan answers "which kernel does this layer get" on a machine without a GPU; the launch functions
// of dam_wgrad.hip take a plan and hold the table from instantiation to kernel, the LDS limit, the launch and the reduction.
#pragma once
#include <string.h>
#include "dam_common.h"

namespace dam {

// Everything the decision depends on: the scalar arguments of dam_conv2d_wgrad_f32, which optional operands are present, and what
// the caller's queue does with the launch (0 no queue, 1 queue without batching, 2 batching queue, 4 batching queue that records
// the stride-1 row kernel's launches too; 3 is no mode).
struct WgradRequest {
    int B, H, W, C, in_nchw, relu_in, Ho, Wo, n_chan, n_out, kh, kw, stride, pad, dil, c_real;
    bool affine, shift;      // in_scale / in_shift given
    int64_t workspace_floats;
    int queue_mode;
};

// What a dam_conv2d_wgrad_f32 call committed to (dam_wgrad_last_launch, include/dam_hip.h).
enum WgradFamily { WGRAD_FAM_NONE = 0, WGRAD_FAM_ROWS = 1, WGRAD_FAM_ROWS_S2 = 2, WGRAD_FAM_DIRECT = 3, WGRAD_FAM_TILE = 4 };
enum WgradIssue { WGRAD_REDUCED_NOW = 0, WGRAD_REDUCTION_QUEUED = 1, WGRAD_LAUNCH_RECORDED = 2 };
struct WgradLaunchNote {
    int family, TNB, TKB, STEPS, KP, GPP, GPPD, HV, NL, TA, TB, nx, nsplit, spi_tmw, rps, issued;
};

// ------------------------------------------------------------------------------------------- geometry, as the kernels receive it
struct WgradGeo {            // tile kernel (wgrad_kernel)
    int B, H, W, C;          // input tensor
    int Ho, Wo, N;           // dY tensor [B][Ho][Wo][N]
    int s;                   // conv stride (1 or 2)
    int KH, KW;              // full kernel
    int off_h, step_h, off_w, step_w;   // tap (kh,kw) reads input (oh*s + off_h + kh*step_h, ...)
    int r0, c0;
    int PR, PWin, PWs, PWT;
    int nchunks;             // ceil(C/16) (1 if in_nchw)
    int nblk;                // N/16
    int tiles_n, tiles_k, tap_groups;
    int tiles_m, total_tiles, nsplit;
    int in_nchw, relu_in;
    int TMW;                 // pixels per tile (a multiple of 16, <= 256): 4 waves x TMW/4 pixels
};
struct RowsGeo {             // stride-1 row kernel (wgrad_rows_kernel)
    int B, H, W, C;          // C channels per pixel in X and in dY
    int P4;                  // ring row pitch in cells: roundup4(W + 2)
    int rps, spi;            // output rows per strip (multiple of 4), strips per image
    int tiles_k;             // in-channel tiles
    int gpp;                 // 1 KB pieces per row plane
};
struct RowsS2Geo {           // stride-2 row kernel (wgrad_rows_s2_kernel)
    int B, H, W, C;          // X
    int Ho, Wo, N;           // dY
    int rps, spi;            // output rows per strip (multiple of the slot's rows), strips per image
    int tiles_k;             // in-channel tiles (= chunks)
};
// Direct kernel: its scalars, and as such one job of a batched launch (see wgrad_direct_batch_kernel): each with its own geometry
// and grid share.  A plan leaves the pointers null.
struct DirectJob {
    const float* X; const float* dY; float* partial;
    int rows, Ho, Wo, H, W, C, N, s, pad, dil, tiles_k;
    int nx, nsplit, wg0;                     // the job's (nx, nsplit) grid and its first workgroup in the flat launch
};
// Stride-1 row kernel: the operands of one weight gradient, and the job table of one launch (a kernel argument).  All jobs of a
// launch share one RowsGeo and one grid; a workgroup keeps its (tile, strip) and walks the jobs in order.
struct RowsJob {
    const float *X, *dY, *in_scale, *in_shift;
    float* partial;
    int relu_in, pad_;
};
constexpr int ROWS_MAX_JOBS = 8;             // stem + layer1 of a ResNet18 are five of one geometry; 8 x 48 B of kernel arguments
struct RowsJobs {
    RowsJob job[ROWS_MAX_JOBS];
    int njobs;
};
constexpr int RW_LOADERS = 8;                 // loader waves (waves 4..11)
constexpr int RW_THREADS = 256 + 64 * RW_LOADERS, RW_GUARD = 64, RW_TAIL = 1280;   // (tail: the step-split last slot prefetches up to 1 KB past a row)

// What wgrad_reduce_batch_kernel needs to know of the slabs it sums (reduce_submit).
struct WgradReduce { int TNB, TKB, TA, TB, n_real, k_real, KH, KW, tap_groups, tiles_k; };

struct WgradPlan {
    WgradLaunchNote note;    // family and template parameters, grid, how it is issued
    RowsGeo rows;            // the note's family says which of the four is filled
    RowsS2Geo rows_s2;
    DirectJob direct;
    WgradGeo tile;           // nsplit = 0 in a recorded plan: decided at the flush from the number of jobs (plan_tile_split)
    int nx, nsplit;
    size_t lds;              // dynamic LDS bytes
    int relu_in;             // travels beside the geometry (row kernel: a kernel argument; tile kernel: per job)
    int64_t workspace_floats;   // as requested (a recorded tile launch is split at the flush, in the smallest workspace of its batch)
    WgradReduce red;
};

// -------------------------------------------------------------------------------------------------- the instantiation tables
// The single lists of instantiations: the planners take a row, the launch tables of dam_wgrad.hip are generated from them.
// stride-1 row kernel <TN, TK, steps, planes per loader wave, pieces per plane, row parts, loader waves>: the shapes of the ResNet
// stages at 130 frames (3 s clips) and at the reference's native 216 frames
// (the last parameter, loader waves: four measured 53.7 -> 48.5 us on the 129x17 stage, where two workgroups then share a
// CU; no difference on the three wide stages -- 56.6 / 57.5 / 59.5 against 57.0 / 57.0 / 59.2 us -- and 31.8 -> 32.7 on 65x9)
struct RowsInst { int TNB, TKB, STEPS, KP, GPP, HV, NL; };
enum { R33, R28H2, R14H2, R17, R14, R9, R5, R3, ROWS_INST_N };
constexpr RowsInst ROWS_INST[ROWS_INST_N] = {
    {1, 1, 33, 1, 9, 1, 8}, {1, 1, 28, 1, 14, 2, 8},                             // 16 channels
    {2, 1, 14, 1, 7, 2, 8},
    {2, 1, 17, 2, 5, 1, 8}, {2, 1, 14, 2, 4, 1, 8},
    {2, 1, 9, 2, 3, 1, 8},
    {2, 1, 5, 3, 2, 1, 4},   // 17-pixel rows (129x17 stage), four loader waves
    {2, 1, 3, 2, 1, 1, 8},   // 9-pixel rows (65x9 stage): 40.8 -> 32.1 us; narrower: tile kernel
};
// The instantiations whose launches a queue in mode 4 records and runs as one launch of up to ROWS_MAX_JOBS jobs (launch_pending_rows):
// those whose one batched launch measured shorter than its launches alone (DESIGN.md section 4.3 has the ladder).
constexpr bool ROWS_BATCHED[ROWS_INST_N] = {true, false, false, true, false, true, true, true};
inline bool rows_batched(const RowsInst& t) {
    for (int i = 0; i < ROWS_INST_N; ++i) {
        const RowsInst& u = ROWS_INST[i];
        if (u.TNB == t.TNB && u.TKB == t.TKB && u.STEPS == t.STEPS && u.KP == t.KP && u.GPP == t.GPP && u.HV == t.HV && u.NL == t.NL)
            return ROWS_BATCHED[i];
    }
    return false;
}
// stride-2 row kernel <TN, steps, planes per loader wave, pieces per X plane, per dY plane, row parts>: the down-sampling
// convolutions of the ResNet stages at 130 frames (65-, 33- and 17-pixel output rows) and at the reference's native 216 (54, 27)
struct RowsS2Inst { int TNB, STEPS, KP, GPPX, GPPD, HV; };
enum { S9H2, S7H2, S9, S7, S5, ROWS_S2_INST_N };
constexpr RowsS2Inst ROWS_S2_INST[ROWS_S2_INST_N] = {{2, 9, 1, 9, 5, 2}, {2, 7, 1, 7, 4, 2}, {2, 9, 2, 5, 3, 1}, {2, 7, 2, 4, 2, 1},
                                                     {2, 5, 2, 3, 2, 1}};
// direct kernel <TN, TK, K, K> (alone and batched), tile kernel <TN, TK, TA, TB>
struct DirectInst { int TNB, TKB, K; };
constexpr int DIRECT_INST_N = 5;
constexpr DirectInst DIRECT_INST[DIRECT_INST_N] = {{2, 2, 1}, {2, 1, 1}, {1, 1, 1}, {2, 1, 3}, {1, 1, 3}};
struct TileInst { int TNB, TKB, TA, TB; };
constexpr int TILE_INST_N = 11;
constexpr TileInst TILE_INST[TILE_INST_N] = {{1, 1, 3, 3}, {2, 2, 3, 3}, {1, 1, 1, 1}, {2, 2, 1, 1}, {1, 1, 1, 5}, {3, 2, 1, 5},
                                             {2, 2, 1, 5}, {1, 1, 1, 7}, {2, 2, 1, 7}, {1, 1, 1, 9}, {2, 2, 1, 9}};

// ------------------------------------------------------------------------------------------------------------------ planners
// One per family: DAM_OK and the plan, DAM_ERR_UNSUPPORTED (the layer does not fit the family) or DAM_ERR_WORKSPACE.
inline int wgrad_issue(const WgradRequest& rq, bool recordable) {
    return recordable && rq.queue_mode >= 2 ? WGRAD_LAUNCH_RECORDED : rq.queue_mode ? WGRAD_REDUCTION_QUEUED : WGRAD_REDUCED_NOW;
}
inline bool wgrad_queue_mode_ok(int m) { return m == 0 || m == 1 || m == 2 || m == 4; }

// Strips of the two row kernels: `rows` output rows per image in spi nearly equal parts; false: the workspace holds not even one.
inline bool plan_strips(int B, int rows, int RPS, int nx, int NBLK, size_t lds, int64_t ws_floats, int& spi_out, int& rps_out) {
    // Strips: as many workgroups as the chip holds at once and no more (a strip that has to wait for a CU doubles the
    // launch: 96 channels on 8 images gave 288 workgroups on 256 CUs, 63 us).  One workgroup per CU when whole strips per
    // image fill >= 80 % of the CUs that way; otherwise size for two co-resident workgroups per CU (the register file
    // holds two of these 8-wave workgroups, the narrow stages' rings leave the LDS for both): 432 workgroups, 50 us.
    // Measured both ways: where one per CU already fills the chip, two cost 15 % (more slabs, shared pipe).
    auto strips = [&](int per_cu) { const int w = (int)(256 * per_cu / ((int64_t)nx * B)); return w > 0 ? w : 1; };
    int spi = strips(1);
    if ((int64_t)nx * B * spi < 205 && lds * 2 <= 160 * 1024) spi = strips(2);
    if (spi > (int)cdiv(rows, RPS)) spi = (int)cdiv(rows, RPS);
    if (spi > rows) spi = rows;
    for (;; --spi)                                // (rows in spi nearly equal parts, see the kernel)
        if ((int64_t)B * spi * nx * NBLK * 256 <= ws_floats || spi == 1) break;
    spi_out = spi;
    rps_out = (int)cdiv(rows, spi);
    return (int64_t)B * spi * nx * NBLK * 256 <= ws_floats;
}

inline int plan_rows(const WgradRequest& rq, const RowsInst& t, WgradPlan& p) {
    const int NBLK = t.TNB * t.TKB * 9;
    RowsGeo g;
    g.B = rq.B; g.H = rq.H; g.W = rq.W; g.C = rq.C;
    const int RPS = 4 / t.HV, NRX = 2 * RPS + 2, NRD = 2 * RPS;
    g.P4 = ((rq.W + 2 + 4 * t.HV - 1) / (4 * t.HV)) * (4 * t.HV);
    if (g.P4 != t.STEPS * 4 * t.HV) return DAM_ERR_UNSUPPORTED;
    g.gpp = (g.P4 * 64 + 1023) / 1024;
    if (g.gpp > t.GPP || (RPS * (t.TKB + t.TNB) + t.NL - 1) / t.NL > t.KP) return DAM_ERR_UNSUPPORTED;
    const int nblk = rq.C / 16;
    if (nblk % t.TNB || nblk % t.TKB || rq.H >= 8000) return DAM_ERR_UNSUPPORTED;
    g.tiles_k = nblk / t.TKB;
    const int nx = (nblk / t.TNB) * g.tiles_k;
    const size_t rowb = (size_t)g.P4 * 64;
    size_t lds = RW_GUARD + (size_t)t.TKB * NRX * rowb + (size_t)t.TNB * NRD * rowb + RW_TAIL;
    if (lds < (size_t)NBLK * 1024) lds = (size_t)NBLK * 1024;
    if (lds > 160 * 1024) return DAM_ERR_UNSUPPORTED;
    if (!plan_strips(rq.B, rq.H, RPS, nx, NBLK, lds, rq.workspace_floats, g.spi, g.rps)) return DAM_ERR_WORKSPACE;
    p.rows = g; p.nx = nx; p.nsplit = rq.B * g.spi; p.lds = lds;
    p.note = WgradLaunchNote{WGRAD_FAM_ROWS, t.TNB, t.TKB, t.STEPS, t.KP, t.GPP, 0, t.HV, t.NL, 0, 0, nx, p.nsplit, g.spi, g.rps,
                             wgrad_issue(rq, rq.queue_mode == 4 && rows_batched(t))};
    p.red = WgradReduce{t.TNB, t.TKB, 3, 3, rq.n_out, 0, 3, 3, 1, g.tiles_k};
    return DAM_OK;
}

inline int plan_rows_s2(const WgradRequest& rq, const RowsS2Inst& t, WgradPlan& p) {
    const int H = rq.H, W = rq.W, C = rq.C, Ho = rq.Ho, Wo = rq.Wo, N = rq.n_chan;
    const int NBLK = t.TNB * 9;
    const int RPS = 4 / t.HV, NRX = 4 * RPS + 2, NRD = 2 * RPS, P4 = t.STEPS * 4 * t.HV;
    if (Ho != (H - 1) / 2 + 1 || Wo != (W - 1) / 2 + 1) return DAM_ERR_UNSUPPORTED;
    if (((Wo + 1 + 4 * t.HV - 1) / (4 * t.HV)) * (4 * t.HV) != P4) return DAM_ERR_UNSUPPORTED;
    const int nblk = N / 16;
    if (nblk % t.TNB || C % 16 || H >= 8000) return DAM_ERR_UNSUPPORTED;
    if ((int64_t)H * W * C * 4 >= (1ll << 31) || (int64_t)Ho * Wo * N * 4 >= (1ll << 31)) return DAM_ERR_UNSUPPORTED;
    RowsS2Geo g;
    g.B = rq.B; g.H = H; g.W = W; g.C = C; g.Ho = Ho; g.Wo = Wo; g.N = N;
    g.tiles_k = C / 16;
    const int nx = (nblk / t.TNB) * g.tiles_k;
    size_t lds = RW_GUARD + (size_t)NRX * 2 * P4 * 64 + (size_t)t.TNB * NRD * P4 * 64 + RW_TAIL;
    if (lds < (size_t)NBLK * 1024) lds = (size_t)NBLK * 1024;
    if (lds > 160 * 1024) return DAM_ERR_UNSUPPORTED;
    // strips as for the stride-1 kernel: fill the chip once
    if (!plan_strips(rq.B, Ho, RPS, nx, NBLK, lds, rq.workspace_floats, g.spi, g.rps)) return DAM_ERR_WORKSPACE;
    p.rows_s2 = g; p.nx = nx; p.nsplit = rq.B * g.spi; p.lds = lds;
    p.note = WgradLaunchNote{WGRAD_FAM_ROWS_S2, t.TNB, 1, t.STEPS, t.KP, t.GPPX, t.GPPD, t.HV, RW_LOADERS, 0, 0, nx, p.nsplit, g.spi,
                             g.rps, wgrad_issue(rq, false)};
    p.red = WgradReduce{t.TNB, 1, 3, 3, rq.n_out, 0, 3, 3, 1, g.tiles_k};
    return DAM_OK;
}

inline int plan_direct(const WgradRequest& rq, const DirectInst& t, WgradPlan& p) {
    const int KH = rq.kh, KW = rq.kw, N = rq.n_chan;
    const int NBLK = t.TNB * t.TKB * KH * KW;
    const int nblk = N / 16, nch = rq.C / 16;
    if (KH != t.K || KW != t.K || nblk % t.TNB || nch % t.TKB) return DAM_ERR_UNSUPPORTED;
    if ((int64_t)rq.B * rq.H * rq.W * rq.C * 4 >= (1ll << 31) || (int64_t)rq.B * rq.Ho * rq.Wo * N * 4 >= (1ll << 31))
        return DAM_ERR_UNSUPPORTED;
    const int tiles_k = nch / t.TKB, nx = (nblk / t.TNB) * tiles_k;
    const int rows = rq.B * rq.Ho;
    int nsplit = (int)cdiv(KH * KW == 1 ? 1024 : 768, nx);      // 3-4 workgroups per CU: the kernel lives on loads in flight
    if (nsplit > (int)cdiv(rows, 4)) nsplit = (int)cdiv(rows, 4);
    while (nsplit > 1 && (int64_t)nsplit * nx * NBLK * 256 > rq.workspace_floats) --nsplit;
    if ((int64_t)nsplit * nx * NBLK * 256 > rq.workspace_floats) return DAM_ERR_WORKSPACE;
    DirectJob& j = p.direct;
    j.rows = rows; j.Ho = rq.Ho; j.Wo = rq.Wo; j.H = rq.H; j.W = rq.W; j.C = rq.C; j.N = N; j.s = rq.stride;
    j.pad = rq.pad; j.dil = rq.dil; j.tiles_k = tiles_k; j.nx = nx; j.nsplit = nsplit; j.wg0 = 0;
    p.nx = nx; p.nsplit = nsplit; p.lds = 0;
    // (a recorded launch: nsplit is the upper bound, its share of a batch is decided at the flush)
    p.note = WgradLaunchNote{WGRAD_FAM_DIRECT, t.TNB, t.TKB, 0, 0, 0, 0, 0, 0, KH, KW, nx, nsplit, 0, 0, wgrad_issue(rq, true)};
    p.red = WgradReduce{t.TNB, t.TKB, KH, KW, rq.n_out, 0, KH, KW, 1, tiles_k};
    return DAM_OK;
}

inline size_t tile_lds(const WgradGeo& g, int tnb, int tkb) { return (size_t)tkb * g.PR * g.PWT * 64 + (size_t)tnb * g.TMW * 64; }

// Pixel splits of a tile-kernel launch of `njobs` jobs of geometry g (lds: with the NBLK KB floor); 0: the workspace holds not even
// one slab set.  Apart from plan_tile, a batched flush asks: it knows the number of jobs only then.
inline int plan_tile_split(const WgradGeo& g, int NBLK, size_t lds, int njobs, int64_t ws_floats) {
    const int nx = g.tiles_n * g.tiles_k * g.tap_groups;
    auto split_for = [&](int64_t slots, double fixed) {
        // Pixel split by MAKESPAN: every CU works through ceil(workgroups / slots) workgroups of ceil(total_tiles / nsplit) tiles
        // each (co-resident workgroups share the matrix pipe, so it is the count per CU that matters).  The first rule -- at least
        // 512 workgroups -- gave the 9x9 / 64 -> 128 layer of the scalar models 72 x 8 = 576 workgroups of 40 tiles: a third round
        // for a quarter of the chip (1.64 ms); 72 x 7 = 504 of 46 tiles is two rounds.  Batched jobs multiply the workgroups, not the
        // tiles of one: three jobs need a third of the splits -- and slabs.
        int ns_best = 1;
        double best = 1e300;
        // (up to 512 splits: a layer with ONE channel tile -- the scalar models' 4 -> 16 first convolution -- had 63 workgroups on
        // 256 CUs under the former cap of 64: 170 us for 0.15 GFLOP)
        const int hi = g.total_tiles < 512 ? g.total_tiles : 512;
        for (int ns = 1; ns <= hi; ++ns) {
            const int64_t wgs = (int64_t)nx * ns * njobs;
            if ((int64_t)nx * ns * NBLK * 256 > ws_floats && ns > 1) break;
            const double cost = (double)cdiv(wgs, slots) * ((double)cdiv(g.total_tiles, ns) + fixed);   // + fixed: per-workgroup part
            if (cost < best * 0.999) { best = cost; ns_best = ns; }
        }
        return ns_best;
    };
    // slots: two workgroups per CU where the LDS holds two (the small-patch layers: their staging phases overlap each
    // other -- 256 workgroups of two tiles measured slower than 512 of one on the 33 x 5 stage), one otherwise
    int nsplit = split_for(lds * 2 <= 160 * 1024 ? 512 : 256, 1.0);
    while (nsplit > 1 && (int64_t)nsplit * nx * NBLK * 256 > ws_floats) --nsplit;
    return (int64_t)nsplit * nx * NBLK * 256 > ws_floats ? 0 : nsplit;
}

inline int plan_tile(const WgradRequest& rq, WgradPlan& p) {
    const int kh = rq.kh, kw = rq.kw, Ho = rq.Ho, Wo = rq.Wo, stride = rq.stride, pad = rq.pad, dil = rq.dil;
    WgradGeo& g = p.tile;
    memset(&g, 0, sizeof(g));               // (compared bytewise when launches of one geometry are batched)
    g.B = rq.B; g.H = rq.H; g.W = rq.W; g.C = rq.C; g.Ho = Ho; g.Wo = Wo; g.N = rq.n_chan; g.s = stride; g.KH = kh; g.KW = kw;
    g.off_h = -pad; g.step_h = dil; g.off_w = -pad; g.step_w = dil;
    g.r0 = -pad; g.c0 = -pad;
    g.PWin = (Wo - 1) * stride + (kw - 1) * dil + 1;
    g.PWs = (int)cdiv(g.PWin, stride);
    g.PWT = g.PWs * stride;
    const int ta_rows = (kh == 3 && kw == 3) ? 3 : 1;               // TA of the instantiations below
    auto set_tile = [&](int tmw_max) {
        // pixels per tile: the image in equal parts of at most tmw_max pixels, rounded up to the 16 a step of the four waves takes
        // (165 pixels of the 33 x 5 stage in a 256-pixel tile were 16 MFMA steps per wave for 10.3 of work: 176 -> 11)
        const int64_t npix_ = (int64_t)Ho * Wo, parts_ = cdiv(npix_, tmw_max);
        const int tmw = (int)(cdiv(cdiv(npix_, parts_), 16) * 16);
        int rows_out = (tmw + Wo - 2) / Wo + 1;
        if (rows_out > Ho) rows_out = Ho;
        g.TMW = tmw;
        g.PR = (rows_out - 1) * stride + (ta_rows - 1) * dil + 1;        // rows one tap group (TA kernel rows) touches
        g.tiles_m = (int)cdiv((int64_t)Ho * Wo, tmw);
        g.total_tiles = g.tiles_m * rq.B;
    };
    g.nchunks = rq.in_nchw ? 1 : rq.C / 16;
    g.nblk = rq.n_chan / 16;
    g.in_nchw = rq.in_nchw;                  // (relu_in travels per job, not in the shared geometry)
    // tile choice: 2x2 channel blocks when both sides have them and LDS allows two workgroups per CU.  48 OUTPUT channels (three blocks:
    // the scalar models' 5x5 / 32 -> 48 layer) take a three-block tile on that side instead of two tiles of two with the fourth block
    // empty (a quarter of the MFMAs on zeros): 167 -> 115 us.  The same on the INPUT side (7x7 / 48 -> 64
    // as a 1x3 tile) measured 476 us against 463: 22 LDS reads per 21 MFMAs; a 2x3 tile needs 273 VGPRs.  Not instantiated.
    int tnb = 2, tkb = 2;
    if (kh == 5 && kw == 5 && g.nblk == 3 && g.nchunks % 2 == 0) { tnb = 3; tkb = 2; }
    bool small = g.nchunks == 1 || g.nblk == 1;
    set_tile(256);
    if (!small && tile_lds(g, tnb, tkb) > 72 * 1024) {
        set_tile(128);
        if (tile_lds(g, tnb, tkb) > 72 * 1024) {
            if (tnb == 2 && tkb == 2) small = true;
            else { tnb = tkb = 2; set_tile(256); if (tile_lds(g, 2, 2) > 72 * 1024) { set_tile(128); if (tile_lds(g, 2, 2) > 72 * 1024) small = true; } }
        }
    }
    if (small) {
        tnb = tkb = 1;
        set_tile(256);
        if (tile_lds(g, 1, 1) > 72 * 1024) set_tile(128);
    }
    int TA, TB;                              // 3x3 and 1x1 whole; a kernel row of 5, 7 or 9 taps per tap group, whatever kh
    if (kw == 3 && kh == 3) TA = TB = 3;
    else if (kw == 1 && kh == 1) TA = TB = 1;
    else if (kw == 5 || kw == 7 || kw == 9) { TA = 1; TB = kw; }
    else return DAM_ERR_UNSUPPORTED;
    const int NBLK = tnb * tkb * TA * TB;
    g.tiles_n = (int)cdiv(g.nblk, tnb);
    g.tiles_k = (int)cdiv(g.nchunks, tkb);
    g.tap_groups = (int)cdiv(g.KH, TA);
    p.nx = g.tiles_n * g.tiles_k * g.tap_groups;
    p.lds = tile_lds(g, tnb, tkb);
    if (p.lds < (size_t)NBLK * 1024) p.lds = (size_t)NBLK * 1024;
    const int issued = wgrad_issue(rq, true);
    if (issued != WGRAD_LAUNCH_RECORDED) {   // (a recorded launch has these refusals ahead of it, at the flush)
        p.nsplit = g.nsplit = plan_tile_split(g, NBLK, p.lds, 1, rq.workspace_floats);
        if (!p.nsplit) return DAM_ERR_WORKSPACE;
        if (p.lds > 160 * 1024) return DAM_ERR_UNSUPPORTED;
    }
    p.note = WgradLaunchNote{WGRAD_FAM_TILE, tnb, tkb, 0, 0, 0, 0, 0, 0, TA, TB, p.nx, p.nsplit, g.TMW, 0, issued};
    p.red = WgradReduce{tnb, tkb, TA, TB, rq.n_out, 0, g.KH, g.KW, g.tap_groups, g.tiles_k};
    return DAM_OK;
}

// The argument checks that depend on no pointer, and the fall-through order of the families (the only place that holds it).  A
// status other than DAM_ERR_UNSUPPORTED from a family ends the search.
inline int plan_wgrad(const WgradRequest& rq, WgradPlan& p) {
    p = WgradPlan{};
    if (rq.B <= 0 || rq.H <= 0 || rq.W <= 0 || rq.C <= 0 || rq.Ho <= 0 || rq.Wo <= 0) return DAM_ERR_BAD_ARG;
    if (rq.c_real < 0 || rq.c_real > rq.C) return DAM_ERR_BAD_ARG;
    if (rq.n_chan % 16 || rq.n_out > rq.n_chan || (rq.stride != 1 && rq.stride != 2)) return DAM_ERR_UNSUPPORTED;
    if (rq.in_nchw ? rq.C > 16 : rq.C % 16) return DAM_ERR_UNSUPPORTED;
    if (rq.affine && !rq.shift) return DAM_ERR_BAD_ARG;
    if (rq.in_nchw && rq.affine) return DAM_ERR_UNSUPPORTED;        // the NCHW loader (stage_patch) applies no affine: the first layer reads raw features
    const int kh = rq.kh, kw = rq.kw, W = rq.W, Wo = rq.Wo;
    const bool k33 = kh == 3 && kw == 3 && !rq.in_nchw;
    int rc = DAM_ERR_UNSUPPORTED;
    if (k33 && rq.stride == 1 && rq.pad == 1 && rq.dil == 1 && rq.Ho == rq.H && Wo == W && rq.C == rq.n_chan) {
        // row-streaming kernel for the shapes of the ResNet stages; anything else takes the tile kernel below
        auto rows = [&](int i) { return plan_rows(rq, ROWS_INST[i], p); };
        if (rq.C == 16) { rc = rows(R33); if (rc == DAM_ERR_UNSUPPORTED) rc = rows(R28H2); }
        else if (W > 80) rc = rows(R14H2);
        else if (W > 48) { rc = rows(R17); if (rc == DAM_ERR_UNSUPPORTED) rc = rows(R14); }
        else if (W > 20) rc = rows(R9);
        else if (W > 12) rc = rows(R5);
        else if (W > 6) rc = rows(R3);
    }
    if (rc == DAM_ERR_UNSUPPORTED && kh == 1 && kw == 1 && rq.pad == 0 && !rq.in_nchw && !rq.affine)
        for (int i = 0; i < 3 && rc == DAM_ERR_UNSUPPORTED; ++i) rc = plan_direct(rq, DIRECT_INST[i], p);
    // strided 3x3 (the first convolution of a down-sampling block): measured 61/62/58 us against 80/78/67 us for the tile
    // kernel; for stride-1 narrow rows (17 pixels, 96 channels) it is slower (117 vs 60 us: nine L2 reads per element)
    if (rc == DAM_ERR_UNSUPPORTED && k33 && !rq.affine && rq.stride == 2 && rq.pad == 1 && rq.dil == 1) {
        auto rows_s2 = [&](int i) { return plan_rows_s2(rq, ROWS_S2_INST[i], p); };
        if (Wo > 56) rc = rows_s2(S9H2);
        else if (Wo > 34) rc = rows_s2(S7H2);
        else if (Wo > 28) rc = rows_s2(S9);
        else if (Wo > 18) rc = rows_s2(S7);
        else if (Wo > 14) rc = rows_s2(S5);
        // narrower rows stay on the tile kernel: slots of 3 / 2 MFMA steps are all barrier (measured 38.5 vs 38.9 us on the
        // 65x9 stage, 31.6 vs 29.5 us on 33x5)
    }
    if (rc == DAM_ERR_UNSUPPORTED && k33 && !rq.affine && Wo >= 16 && rq.stride == 2)
        for (int i = 3; i < DIRECT_INST_N && rc == DAM_ERR_UNSUPPORTED; ++i) rc = plan_direct(rq, DIRECT_INST[i], p);
    if (rc == DAM_ERR_UNSUPPORTED) rc = plan_tile(rq, p);
    if (rc != DAM_OK) { p = WgradPlan{}; return rc; }
    p.red.k_real = rq.c_real ? rq.c_real : rq.C;       // dw rows kept: the real input channels (the stem's zero-padded planes drop out)
    p.relu_in = rq.relu_in;
    p.workspace_floats = rq.workspace_floats;
    return DAM_OK;
}

// Device pointers of one call, as dam_conv2d_wgrad_f32 got them.
struct WgradOperands {
    const float *x, *dy, *in_scale, *in_shift;
    float *workspace, *dw;
};

}  // namespace dam
