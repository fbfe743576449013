// Dispatch of the three entry points of a down-sampling block (dam_conv_s2_pair_fwd_f32, dam_dgrad_s2_3x3_f32,
// dam_conv1x1_pair_f32) as a value: which kernel family and instantiation a call gets, its grid, its dynamic LDS and the scalar
// arguments the kernel receives.  Planning is host arithmetic only -- no HIP call, no device pointer -- on the scalar arguments,
// the operand flags and the two facts the decision takes from the device (S2Device), which the planners are GIVEN: so
// dam_conv_s2_pair_fwd_plan / dam_dgrad_s2_3x3_plan / dam_conv1x1_pair_plan answer "which kernel does this layer get" on a machine
// without a GPU.  The launch functions of dam_conv_s2.hip, dam_dgrad_s2.hip and dam_conv.hip take a plan and hold the table from
// instantiation to kernel, the LDS limit, the occupancy question and the launch.
#pragma once
#include "dam_common.h"

namespace dam {

// What a call of one of the three entry points committed to (dam_s2_last_launch, include/dam_hip.h): the plan's note, copied into a
// host variable of the calling thread once the launch is made (cleared at the top of each of the three), read by tests that must
// know which instantiation they exercised.
enum S2Entry { S2_ENTRY_NONE = 0, S2_ENTRY_PAIR_FWD = 1, S2_ENTRY_DGRAD = 2, S2_ENTRY_PAIR_1X1 = 3 };
enum S2Family { S2_FAM_NONE = 0, S2_FAM_RESIDENT = 1, S2_FAM_STREAM_LDS = 2, S2_FAM_STREAM = 3, S2_FAM_PAIR_1X1 = 4 };
struct S2LaunchNote {
    int entry, family, NB, NCH, MB, WAVES, pair, sums, workgroups, units, rounds, n_xcd, records;
};
extern thread_local S2LaunchNote s2_last_launch;       // (defined in dam_conv_s2.hip)
inline void s2_note_to_ints(const S2LaunchNote& n, int* out16) {
    const int v[16] = {n.entry, n.family, n.NB, n.NCH, n.MB, n.WAVES, n.pair, n.sums, n.workgroups, n.units, n.rounds, n.n_xcd, n.records,
                       0, 0, 0};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
}

// The only two things the decision takes from the device: its CU count, and how many workgroups of the persistent instantiation
// the channel counts name one CU holds (registers and LDS: the runtime's occupancy answer; 1 where no persistent kernel is named).
struct S2Device { int cus, resident_per_cu; };

struct S2Plan {
    S2LaunchNote note;       // entry, family and template parameters, grid, units, records
    size_t lds;              // dynamic LDS bytes
    int threads;             // per workgroup
    unsigned grid_x, grid_y;
    int64_t px, units;       // pixels (forward, data gradient: of the half-size tensor) and wave units, as the kernel receives them
    int64_t xb;              // forward: bytes of x (the range of its checked loads)
    int64_t groups;          // streaming forward: groups of 64 pixels (one statistics record each)
    int segs;                // 1x1 pair: 16-pixel segments per row
};

// The unit walk of the two persistent kernels (conv_s2_pair_kernel, dgrad_s2_kernel) in host arithmetic: every XCD takes one
// contiguous share `per_xcd` of the units, its wave w of workgroup g starts at unit w * wg_per_xcd + g of the share and steps by
// wg_per_xcd * WAVES.  -> the largest number of units any wave takes (the first wave of XCD 0, whose share is never cut short).
inline int s2_resident_rounds(int64_t units, int64_t wgs, int waves, int* n_xcd_out) {
    const int n_xcd = (wgs & 7) == 0 ? 8 : 1;
    const int64_t wg_per_xcd = wgs / n_xcd, per_xcd = (units + n_xcd - 1) / n_xcd;
    const int64_t share = per_xcd < units ? per_xcd : units, ustride = wg_per_xcd * waves;
    if (n_xcd_out) *n_xcd_out = n_xcd;
    return ustride > 0 ? (int)cdiv(share, ustride) : 0;
}

// One record per workgroup of a persistent kernel, at most `record_limit` of them (0: the launch writes none).  The forward LOWERS
// the workgroups per CU until the full grid fits (and refuses a device with more CUs than records, statistics or not); the data
// gradient sizes its grid without the limit and REFUSES the launch when the grid it got exceeds it.
enum S2RecordPolicy { S2_RECORDS_LOWER, S2_RECORDS_REFUSE };

// The grid of a persistent kernel, by makespan: n resident workgroups per CU put n waves on every SIMD, which share its MFMA pipe, so
// a SIMD's time is (units per wave) * n unit times; more waves hide the operand latency better, which decides while the costs are
// within ~15 %.  At most 3 per CU, 1 for the 8-wave kernels (two waves per SIMD already), never more than the CU holds (a grid beyond
// that would run a second, partial round) and never more workgroups than cdiv(units, waves).  -> workgroups; 0: refused.
inline int64_t s2_resident_grid(int64_t units, int waves, const S2Device& dev, int record_limit, S2RecordPolicy policy) {
    int max_per_cu = dev.resident_per_cu;
    if (max_per_cu > 3) max_per_cu = 3;
    if (waves == 8) max_per_cu = 1;
    if (max_per_cu < 1) max_per_cu = 1;
    if (record_limit && policy == S2_RECORDS_LOWER) {
        while (max_per_cu > 1 && (int64_t)dev.cus * max_per_cu > record_limit) --max_per_cu;
        if (dev.cus > record_limit) return 0;
    }
    int per_cu = 1;
    int64_t best = 0;
    for (int n = 1; n <= max_per_cu; ++n) {
        const int64_t cost = cdiv(units, (int64_t)waves * dev.cus * n) * n * 100;
        if (n == 1 || cost * 100 <= best * 115) { best = n == 1 ? cost : (cost < best ? cost : best); per_cu = n; }
    }
    int64_t wgs = (int64_t)dev.cus * per_cu;
    if (wgs > cdiv(units, waves)) wgs = cdiv(units, waves);
    if (record_limit && policy == S2_RECORDS_REFUSE && wgs > record_limit) return 0;
    return wgs;
}

// The persistent instantiations, by channel counts: conv_s2_pair_kernel <NB, NCH, STATS, WAVES> and dgrad_s2_kernel <NB, NCH, MB,
// PAIR, WAVES, SUMS> with both weight images resident in LDS (20 / 80 KB).  Fills the note's instantiation fields; false: the
// channel counts name none.  (Apart from the planners, the entry points ask: the occupancy question needs the instantiation.)
inline bool s2_pair_fwd_resident(int Ci, int Co, bool stats, S2LaunchNote& n) {
    if (Ci == 16 && Co == 32) n = S2LaunchNote{S2_ENTRY_PAIR_FWD, S2_FAM_RESIDENT, 2, 1, 1, 4, 1, stats ? 1 : 0};
    else if (Ci == 32 && Co == 64) n = S2LaunchNote{S2_ENTRY_PAIR_FWD, S2_FAM_RESIDENT, 4, 2, 1, 8, 1, stats ? 1 : 0};
    else return false;
    return true;
}
inline bool s2_dgrad_resident(int Co, int Ci, bool pair, bool sums, S2LaunchNote& n) {
    if (Co == 32 && Ci == 16) n = S2LaunchNote{S2_ENTRY_DGRAD, S2_FAM_RESIDENT, 1, 2, 2, 4, pair ? 1 : 0, sums ? 1 : 0};
    else if (Co == 64 && Ci == 32) n = S2LaunchNote{S2_ENTRY_DGRAD, S2_FAM_RESIDENT, 2, 4, 1, 8, pair ? 1 : 0, sums ? 1 : 0};
    else return false;
    return true;
}
// Dynamic LDS of a persistent instantiation: the packed weight images, [9 taps + the shortcut's][NCH][NB] blocks of 1 KB (the data
// gradient without a pair term keeps nine).
inline size_t s2_resident_lds(const S2LaunchNote& n) {
    return (size_t)(n.entry == S2_ENTRY_PAIR_FWD || n.pair ? 10 : 9) * n.NCH * n.NB * 1024;
}
// Grid, walk and records of a persistent launch into the plan (whose note names the instantiation); false: refused.
inline bool plan_s2_resident(S2Plan& p, int record_limit, S2RecordPolicy policy, const S2Device& dev) {
    S2LaunchNote& n = p.note;
    const int64_t wgs = s2_resident_grid(p.units, n.WAVES, dev, record_limit, policy);
    if (!wgs) return false;
    p.lds = s2_resident_lds(n);
    p.threads = 64 * n.WAVES;
    p.grid_x = (unsigned)wgs; p.grid_y = 1;
    n.workgroups = (int)wgs;
    n.units = (int)p.units;
    n.rounds = s2_resident_rounds(p.units, wgs, n.WAVES, &n.n_xcd);
    n.records = n.sums ? (int)wgs : 0;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ planners
// One per entry point: its scalar argument checks, the family choice with its fall-through order and every refusal -- the status
// the entry point returns (DAM_OK and the plan, DAM_ERR_BAD_ARG, DAM_ERR_UNSUPPORTED: not a layer these kernels take; the plan is
// all zero then).

// dam_conv_s2_pair_fwd_f32.  stats: partial / partial_sc given.
inline int plan_s2_pair_fwd(int B, int H, int W, int Ci, int Co, bool stats, const S2Device& dev, S2Plan& out) {
    out = S2Plan{};
    if (B <= 0 || H <= 0 || W <= 0) return DAM_ERR_BAD_ARG;
    S2Plan p{};
    const int Hd = (H + 1) / 2, Wd = (W + 1) / 2;
    p.px = (int64_t)B * Hd * Wd;
    p.xb = (int64_t)B * H * W * Ci * 4;
    if (s2_pair_fwd_resident(Ci, Co, stats, p.note)) {
        if (p.px >= (1ll << 26) || p.xb >= (1ll << 31)) return DAM_ERR_UNSUPPORTED;      // byte offsets of the range-checked loads
        p.units = cdiv(p.px, 16);
        // one statistics record per workgroup, <= BN_RECORDS_MAX
        if (!plan_s2_resident(p, BN_RECORDS_MAX, S2_RECORDS_LOWER, dev)) return DAM_ERR_UNSUPPORTED;
    } else if (Ci > 0 && Co > 0 && Ci % 32 == 0 && Co % 16 == 0) {
        // the wide blocks: weight fragments streamed from L2 (an even chunk count: the two register sets alternate); a wave takes
        // exactly one (16 pixels, 16 channels) unit, group g of 64 pixels runs on XCD g % 8 and fills one record
        const int NCH = Ci / 16, NB = Co / 16;
        p.groups = cdiv(p.px, 64);
        if (p.px >= (1ll << 26) || p.xb >= (1ll << 31) || p.groups * NB >= (1ll << 31) || (int64_t)9 * Ci * Co * 4 >= (1ll << 31))
            return DAM_ERR_UNSUPPORTED;
        if (stats && p.groups > BN_RECORDS_MAX) return DAM_ERR_UNSUPPORTED;
        p.units = cdiv(p.px, 16) * NB;
        p.threads = 256;
        p.grid_x = (unsigned)(cdiv(p.groups, 8) * 8 * NB); p.grid_y = 1;       // whole rounds of eight groups (one per XCD)
        p.note = S2LaunchNote{S2_ENTRY_PAIR_FWD, S2_FAM_STREAM_LDS, NB, NCH, 1, 4, 1, stats ? 1 : 0, (int)p.grid_x, (int)p.units, 1, 8,
                              stats ? (int)p.groups : 0};
    } else {
        return DAM_ERR_UNSUPPORTED;
    }
    out = p;
    return DAM_OK;
}

// dam_dgrad_s2_3x3_f32.  pair: dy_pair given; sums: the upstream BatchNorm's backward sums asked for (taken by the persistent
// kernels; a streaming layer plans without them: sums = 0, records = 0 -- "not produced").
inline int plan_dgrad_s2(int B, int Hd, int Wd, int Co, int Ci, int H, int W, bool pair, bool sums, const S2Device& dev, S2Plan& out) {
    out = S2Plan{};
    if (B <= 0 || Hd <= 0 || Wd <= 0 || H <= 0 || W <= 0) return DAM_ERR_BAD_ARG;
    if (Hd != (H + 1) / 2 || Wd != (W + 1) / 2) return DAM_ERR_BAD_ARG;             // 3x3 / stride 2 / pad 1 geometry
    if ((int64_t)B * Hd * Wd * Co * 4 >= (1ll << 31)) return DAM_ERR_UNSUPPORTED;   // byte offsets of the range-checked loads
    S2Plan p{};
    // Units are 16 * MB pixels of the FLATTENED [B * Hd * Wd] index space (a unit per row segment left the last segment of every row
    // nearly empty: Wd = 33 -> half the MFMAs on padding), each lane finds its row / column by division.
    p.px = (int64_t)B * Hd * Wd;
    if (s2_dgrad_resident(Co, Ci, pair, sums, p.note)) {
        if (p.px >= (1ll << 30)) return DAM_ERR_UNSUPPORTED;
        p.units = cdiv(p.px, 16 * p.note.MB);
        // one record of sums per workgroup, <= BN_BWD_RECORDS_MAX
        if (!plan_s2_resident(p, sums ? BN_BWD_RECORDS_MAX : 0, S2_RECORDS_REFUSE, dev)) return DAM_ERR_UNSUPPORTED;
    } else if (Co > 0 && Ci > 0 && Co % 32 == 0 && Ci % 16 == 0 && (int64_t)9 * Co * Ci * 4 < (1ll << 31)) {
        // wider layers: the weight image streams from L2 (even chunk count: the two register sets alternate); a wave takes exactly
        // one (16 * MB pixels, 16 channels) unit
        const int NCH = Co / 16, NB = Ci / 16;
        const int MB = cdiv(p.px, 16) * NB >= 8 * 1024 ? 2 : 1;                     // two pixel blocks per wave once the chip is full
        p.units = cdiv(p.px, 16 * MB) * NB;
        if (p.px >= (1ll << 26) || p.units >= (1ll << 30)) return DAM_ERR_UNSUPPORTED;
        p.threads = 256;
        p.grid_y = 1;
        if (MB == 1) {      // fragments staged in LDS per workgroup: whole rounds of eight groups of 64 pixels (group g on XCD g % 8)
            p.grid_x = (unsigned)(cdiv(cdiv(p.px, 64), 8) * 8 * NB);
            p.note = S2LaunchNote{S2_ENTRY_DGRAD, S2_FAM_STREAM_LDS, NB, NCH, 1, 4, pair ? 1 : 0, 0, (int)p.grid_x, (int)p.units, 1, 8, 0};
        } else {
            p.grid_x = (unsigned)cdiv(p.units, 4);
            p.note = S2LaunchNote{S2_ENTRY_DGRAD, S2_FAM_STREAM, NB, NCH, 2, 4, pair ? 1 : 0, 0, (int)p.grid_x, (int)p.units, 1, 1, 0};
        }
    } else {
        return DAM_ERR_UNSUPPORTED;
    }
    out = p;
    return DAM_OK;
}

// dam_conv1x1_pair_f32: conv1x1_pair_kernel <NB, R, BOTH> (the note carries R as WAVES, BOTH as pair); a wave takes exactly one
// (image, row, 16-pixel segment) unit of NB channel blocks.
inline int plan_pair_1x1(int B, int H, int W, int C, int n_out, int OHt, int OWt, int out_stride, int out_off_h, int out_off_w,
                         S2Plan& out) {
    out = S2Plan{};
    if (B <= 0 || H <= 0 || W <= 0 || out_stride < 1) return DAM_ERR_BAD_ARG;
    if (C % 16 || n_out % 16 || C <= 0 || n_out <= 0) return DAM_ERR_UNSUPPORTED;
    if ((H - 1) * out_stride + out_off_h >= OHt || (W - 1) * out_stride + out_off_w >= OWt || out_off_h < 0 || out_off_w < 0)
        return DAM_ERR_BAD_ARG;
    if ((int64_t)B * H * W * C * 4 >= (1ll << 31)) return DAM_ERR_UNSUPPORTED;
    S2Plan p{};
    p.segs = (int)cdiv(W, 16);
    p.px = (int64_t)B * H * W;
    p.units = (int64_t)B * H * p.segs;
    if (p.units >= (1ll << 30)) return DAM_ERR_UNSUPPORTED;
    const int nblk = n_out / 16, nch = C / 16;
    const int NB = nblk % 2 == 0 ? 2 : 1;
    const int R = nch <= 2 ? 2 : nch <= 4 ? 4 : NB == 2 ? 4 : 8;      // chunk slots per operand and round
    const int BOTH = nch <= 4 ? 1 : 0;                                // all chunks of both operands in one round
    p.threads = 256;
    p.grid_x = (unsigned)cdiv(p.units, 4); p.grid_y = (unsigned)(nblk / NB);
    p.note = S2LaunchNote{S2_ENTRY_PAIR_1X1, S2_FAM_PAIR_1X1, NB, nch, 0, R, BOTH, 0, (int)(cdiv(p.units, 4) * (nblk / NB)), (int)p.units,
                          1, 1, 0};
    out = p;
    return DAM_OK;
}

}  // namespace dam
