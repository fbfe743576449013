// Dispatch of dam_conv2d_tapgrid_f32 as a value: which kernel family and instantiation a call gets, with the geometry that kernel
// receives.  Planning is host arithmetic only -- no HIP call, no device pointer -- so dam_conv2d_tapgrid_plan answers "which kernel
// does this layer get" on a machine without a GPU; the launch functions take a plan and hold the instantiation tables, nothing else.
#pragma once
#include "dam_conv_geo.h"

namespace dam {

// Everything the decision depends on: the scalar arguments of dam_conv2d_tapgrid_f32 and which optional operands are present.
struct ConvRequest {
    int B, H, W, C, in_nchw, k_chunks, n_out, relu_in, relu_out, OHt, OWt, Ho, Wo, out_stride, out_off_h, out_off_w, in_stride,
        nA, nB, off_h, step_h, off_w, step_w, wt_base, wt_sa, wt_sb;
    bool bias, in_scale, in_shift, res, res_mask, bn_partial, workspace, batch;
    bool bn_bwd, bwd_mask_bits, bwd_res_mask_bits, bwd_mask_scale;      // dam_bn_bwd_sums: x, mask_bits, res_mask_bits, mask_scale given
    bool bn_in, bn_in_bits;                                             // dam_bn_bwd_in: given, its mask as sign bytes
    int64_t workspace_floats;
};

// One kernel launch.  stats: what the kernel is asked to leave in bn_partial -- 0 nothing, 1 forward statistics records,
// 2 BatchNorm-backward sums (BnBwdEpi).
struct ConvLaunchPlan {
    ConvLaunchNote note;     // family and template parameters (dam_conv_last_launch)
    ConvGeo g;               // as the kernel receives it
    StripGeo sg;             // strip family only
    size_t lds;              // dynamic LDS bytes
    int stats;
};

constexpr int CONV_RANGES_MAX = 4;
struct ConvPlan : ConvLaunchPlan {
    int bn_records;          // what the caller gets in *bn_parts_host
    // pipe kernel on column ranges: `ranges` launches of `range_w` output columns (the last one narrower); the base part is a copy
    // of the last range's launch with the family renamed
    int ranges, range_w;
    ConvLaunchPlan range[CONV_RANGES_MAX];
};

// The geometry every family starts from (patch columns, tap-grid origin; PR / CG / tiles_m / split-K unset).
ConvGeo conv_base_geo(const ConvRequest& rq);
inline int tap_span(int n, int step) { return (n - 1) * (step < 0 ? -step : step); }    // max - min tap offset along one axis

// One planner per family: DAM_OK and the plan, or DAM_ERR_UNSUPPORTED (the layer does not fit the family).
int plan_1x1(const ConvGeo& g, ConvLaunchPlan& p);                                            // dam_conv.hip
int plan_strip(const ConvRequest& rq, const ConvGeo& g, int stats, ConvLaunchPlan& p, int* records);     // dam_conv_strip.hip
int plan_pipe(const ConvGeo& g, bool in_scale, int stats, ConvLaunchPlan& p, int* records);  // dam_conv_pipe.hip
int plan_tile(const ConvRequest& rq, const ConvGeo& g, ConvLaunchPlan& p);                    // dam_conv.hip
// Argument checks and the fall-through order of the families (the only place that holds it).
int plan_conv(const ConvRequest& rq, ConvPlan& plan);                                         // dam_conv.hip

// Device pointers of one call, as dam_conv2d_tapgrid_f32 got them.
struct ConvOperands {
    const float *x, *w_packed, *bias, *in_scale, *in_shift, *res, *res_mask;
    float *y, *bn_partial, *workspace;
    BnBwdEpi bwd;
    BnBwdIn bin;
};

// Launch what the plan says: the table from template parameters to instantiation; DAM_OK or DAM_ERR_LAUNCH.
int launch_strip(const ConvLaunchPlan& p, const ConvOperands& a, hipStream_t st);             // dam_conv_strip.hip
int launch_pipe(const ConvLaunchPlan& p, const ConvOperands& a, hipStream_t st);              // dam_conv_pipe.hip

}  // namespace dam
