"""GPU: the TRAINING and DATA-GRADIENT write-outs of every convolution kernel behind dam_conv2d_tapgrid_f32 against float64:
BatchNorm partial statistics (conv2d_fwd(bn_partial=)), the masked residual res * (res_mask > 0) (conv2d_dgrad(res=, res_mask=))
and the BatchNorm-backward sums (conv2d_dgrad(bn_bwd=)), plus the silent retreats to a launch without records.

The entry point falls back from kernel family to kernel family silently and the strip kernel spells its write-out once per
template instantiation, so every case NAMES the launch it means and asserts it through ops.conv_last_launch() before it looks
at a number; test_coverage asserts that the union of the records seen covers REQUIRED.  tests/test_conv_epilogue_gpu.py does
the same for the inference write-outs and tests/test_wgrad_kernels_gpu.py for the weight gradient.

Forms per case (reference: the CPU in float64; every result is written through out= into the middle of a buffer with
4096-float guard bands that must keep their fill pattern bit for bit):
  stats / stats_affine / stats_bias   conv2d_fwd(bn_partial=), plain, with in_scale / in_shift / relu_in (conv2 of a block), and with
      a bias (the strip's self-overlapped statistics write-out takes no bias: the ping-pong form with statistics runs).  Input
      x * 3 + 7 (a sum-of-squares shortcut fails).  y within 2e-5 of max|y|; the test merges the `parts` records (n, mean, M2) itself
      in float64 with Chan's formula: counts sum exactly to B * Ho * Wo, M2 >= 0, merged mean within 1e-5 of max|mean|, merged
      1 / sqrt(var + eps) within 2e-5 relative; records of zero-padded channels have mean 0 and M2 0; bn_partial sits between
      guard bands and nothing behind record `parts` changes; y is bitwise the y of the call without bn_partial when both records
      agree on family and tile, else within 2e-6 of the scale (two summation orders).
  plain / mask   conv2d_dgrad without and with res= / res_mask=: within 2e-5 of the max-abs of conv2d_input [+ res * (mask > 0)] in
      float64; where the mask is <= 0 the masked result is bitwise the plain one (2e-6 of the scale if the two records differ in
      family or tile).  |mask| >= 0.1, 25-75 % set, max|res| >= 0.1 of the scale, weights random (not symmetric: the strip kernel
      re-indexes the taps of the mirrored column walk).
  sums / res_sums / res_bits   conv2d_dgrad(bn_bwd=) with the affine mask, with residual + res_mask_bits + affine mask, and with the
      upstream mask as sign bytes: dx bitwise the call without bn_bwd; the two sums per channel against float64 sums formed from
      the FLOAT64 REFERENCE dx (not from the kernel's output) within 2e-5 of that channel's float64 sum |term|, no absolute
      allowance.  A mask bit that differed between fp32 and float64 would move a sum by a whole |dx|, so x is edited on the CPU
      until every |x * msc + msh| >= 1e-3 (asserted); the sign bytes come from the same float64 sign.

Which launches the table must reach (REQUIRED, read off conv_strip_try, conv_pipe_try and the entry point):
  strip SO 2 (statistics), SO 5 (masked residual), EPI 1 SO 1 at 16 and 32 channels; EPI 2 / 3 SO 1 at 16 channels;
  strip EPI 1 with the wide-row loader at 16 and 32 channels, EPI 2 / 3 with it at 16 channels;
  the ping-pong strip with statistics and with the masked residual: all six tiles of the compile-time grid, all eight of the
      run-time grid (strided forward, dilated), the four wide-row instantiations (run-time grid there: one or two rows) -- and
      <4, 1, 1> / <2, 2, 2> with the compile-time grid, which only a statistics launch that also carries a bias / ReLU / residual
      reaches (statistics only: the masked residual never has a bias, so SO 5 takes those shapes);
  conv_pipe_kernel STATS 1, STATS 2 and the masked residual on all eleven launch_pipe<MB, NB, PU, KS>: the five tiles with loader
      depth 5 and 8 (DAM_TILE forces the tiles the rule does not pick at B = 3) and the K split <1, 1, 3, 2>;
  conv_igemm_kernel (one pass and split-K: splitk_reduce_kernel applies the mask) and conv1x1_direct_kernel <NB, chunk slots>
      with the masked residual.

Unreachable from conv2d_fwd / conv2d_dgrad (named here instead of being dropped):
  * strip EPI 1 / 2 / 3 in the PING-PONG form without the wide-row loader (launch_strip<4, 1, 1, true, false, E> and
    <2, 2, 2, true, false, 1> with SO = 0): the loaders' rule rows_new * nchunks <= STRIP_LOADERS * kp admits at most 4 (16 channels)
    / 6 (32) output rows per tile, which always satisfies the self-overlapped form's ring-row bound rows_tile * nchunks <= 8 / 16;
    every such shape takes the SO = 1 instantiation.
  * strip EPI 2 / 3 at 32 channels: not instantiated (`if (bwd.x && res) { if (c16) ...`, `nchunks != 1 -> UNSUPPORTED`): the entry
    point's second conv_strip_try runs SO 5 / the ping-pong write-out with the FLOAT mask and reports no records (test_retreat_backward_sums).
  * strip statistics with more than one channel workgroup (cdiv(nblk, NB) != 1) and with more than 1024 records: retreats, below.
  * strided data gradients (parity classes, dam_dgrad_s2_3x3_f32) and dam_conv_s2_pair_fwd_f32: other entry points, with a launch
    record and a table of their own in tests/test_s2_kernels_gpu.py;
    so the run-time tap grid of the strip is reached by the masked residual through dilated layers only.
  * pipe STATS 1 / 2 on column ranges: the entry point runs ranges only without bn_partial (`!bn_partial`): a statistics call on
    such a shape takes conv_igemm_kernel and reports parts == 0 (test_retreat_statistics_on_column_ranges).
  * tile_batch: only the parity classes of strided data gradients pass a batch.
  * the sums at 32 channels on rows of 16 pixels: such a layer is the ping-pong <4, 2, 2> (MB = 4 fits whenever Ho <= 6, and taller
    images fit no tile), EPI 1 exists for <2, 2, 2> only (`if (g.nchunks == 2 && MB == 2 && NB == 2)`): test_retreat_backward_sums.

The retreats (test_retreat_*): parts == 0 / partials None, bn_partial untouched, a correct result and the record of the kernel
that did run -- statistics with two channel workgroups (16 -> 64), 1025 strip records (and 1024: still produced), statistics on a
shape that needs column ranges, residual + sums at 32 channels (SO 5 / ping-pong wide-row with the float mask), bn_bwd on
layers no sums kernel takes (dilated, two output blocks, 5x5); conv_pipe_kernel behind 2048 statistics records.

Findings on dispatch, settled with the launch record (every case launched what its row names on the first run):
  * conv2d_fwd(bias=, bn_partial=) on a self-overlapped shape reaches launch_strip<4, 1, 1, true> and <2, 2, 2, true> in the
    PING-PONG form (the SO 2 write-out takes neither bias nor ReLU nor residual) -- instantiations the inference table of
    tests/test_conv_epilogue_gpu.py lists as unreachable from its call form.  Its y is bitwise the SO 3 launch's.
  * Statistics on a shape that runs column ranges do not fall to a ranges launch without records: the tile kernel answers
    (a different summation order: y agrees with the ranges launch to 2e-6 of the scale, not bitwise).
  * conv_pipe_kernel also drops its statistics silently -- behind 2048 records (B * tiles * waves), its sums behind 1024:
    test_retreat_statistics_2048_pipe_records; tests/test_conv_gpu.py has the sums' case (8, 64, 65, 33).
  * Rows too narrow or too wide for the strip (W = 23 at 16 channels, W = 111 at 32) take conv_pipe_kernel <1, 1> with STATS 1 / 2
    at 16 and 32 channels, although its comment says 16-channel stride-1 layers never get there.
  * tests/test_conv_gpu.py, checked with the record: test_dgrad_bn_backward_sums_epilogue reaches strip EPI 1 SO 1 at 16 and 32
    channels, EPI 1 with the wide-row loader at (1, 16, 9, 216) and (1, 32, 7, 108), and pipe STATS 2 on <1, 1, 5>, <1, 1, 3, KS 2>
    and <2, 1, 5> -- four of the eight strip and three of the eleven pipe instantiations, as its docstring's two families say;
    test_dgrad_identity_shortcut_with_upstream_sums reaches EPI 2 / 3 in the SO form and, at (1, 16, 9, 216), with the wide-row
    loader; its 32- and 64-channel cases run SO 5 and pipe with the float mask.  test_loader_wave_tile_kernel says "every tile of
    its rule": at (2, 96, 11, 17) DAM_TILE=1x4 does not divide the six blocks and conv_igemm_kernel <1, 3> (split-K) answers; the
    1x4 tile is reached by its 64-, 128- and 256-channel shapes.  test_conv_fwd_dgrad's first case (2, 16, 16, 37, 23) is
    conv_pipe_kernel <1, 1, 5>, not the strip.  No case had to gain a shape.
  * No kernel bug was found: the ragged last tile (SO_LAST and the ping-pong `j < nvalid`), the record index and the record
    count at exactly 1024 (strip) / 2048 (pipe) records are right.

Worst error seen, relative to its scale (bound), per family and write-out:
  y (2e-5): strip SO 8.2e-7, strip ping-pong 8.2e-7, strip wide-row 8.8e-7, pipe 2.4e-6
  dx (2e-5): strip SO 6.8e-7, ping-pong 7.2e-7, wide-row 6.7e-7, pipe 2.1e-6, tile 1.0e-6, 1x1 5.0e-7
  merged mean (1e-5): strip SO 5.4e-8, ping-pong 5.4e-8, wide-row 3.8e-8, pipe 1.6e-7
  merged invstd (2e-5): strip SO 1.3e-7, ping-pong 1.4e-7, wide-row 2.5e-7, pipe 7.9e-7
  sums, of the channel's sum |term| (2e-5): strip SO 8.4e-8, wide-row 4.0e-8, pipe 6.6e-7
  Nothing comes within a factor of four of its bound (closest: y of the 256-channel pipe cases, a factor of eight).

Mutations, each compiled into a scratch copy of the library and run against this file as it stands (not committed):
  * `(mask > 0)` dropped for one component in the SO 5 write-out and in the ping-pong write-out: all 32 strip cases with the
    masked residual failed, and the three 32-channel residual + sums retreats; nothing else.
  * the sums of the SO and ping-pong write-outs also take the lanes past HoWo of the last tile (the store stays predicated):
    13 of the 14 strip cases with sums failed.  dg_so16_w16 passes, and must: 3 x 16 pixels are three WHOLE 16-pixel blocks,
    blocks past the image are skipped as blocks, so no written block has a lane past the image and the mutated code computes
    the same there.  That run is why the table has the condition "Ho * Wo is no multiple of 16 unless Wo = 16" and the W = 17
    cases beside the W = 16 ones (dg_so16_w17 fails under the mutation).
  * statistics / sums record index shifted by one workgroup (strip) or one tile (pipe): all 147 strip and pipe cases with records
    failed (the counts no longer sum to B * Ho * Wo; record 0 keeps the fill pattern), and the 1024- and 2048-record cases.

NaN propagation through the write-outs is not decided here."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

TOL = 2e-5                          # the project's forward / data-gradient tolerance (tests/test_conv_gpu.py)
TOL_ORDER = 2e-6                    # two float32 summation orders (test_loader_wave_kernel_k_split_matches_unsplit)
TOL_MEAN, TOL_INVSTD = 1e-5, 2e-5   # test_loader_wave_kernel_statistics_epilogue
TOL_SUMS = 2e-5                     # of the channel's float64 sum |term| (test_strided_dgrad_takes_the_upstream_batchnorm_sums)
EPS = 1e-5
MARGIN = 1e-3                       # |x * msc + msh| >= MARGIN: the fp32 and float64 mask bits cannot differ
GUARD = 4096
FILL = 0x5EADBEEF                   # guard-band pattern (as float32: 7.8e18, so an unwritten element fails too)

FWD_FORMS = ('stats', 'stats_affine', 'stats_bias')
DGRAD_FORMS = ('mask', 'sums', 'res_sums', 'res_bits')

Case = collections.namedtuple('Case', 'id op B Ci Co H W k s p d env forms expect')


def Fw(id, Ci, Co, H, W, forms=('stats', 'stats_affine'), k=3, s=1, p=1, d=1, B=3, env=None, **expect):
    """Forward convolution Ci -> Co (Co real channels) of a [B, H, W] input."""
    return Case(id, 'fwd', B, Ci, Co, H, W, k, s, p, d, env or {}, tuple(forms), expect)


def Dg(id, K, N, H, W, forms=('mask',), k=3, p=1, d=1, B=3, env=None, **expect):
    """Stride-1 data gradient as the kernel sees it: dy has K channels, dx [B, H, W] has N (the convolution is N -> K)."""
    return Case(id, 'dgrad', B, N, K, H, W, k, 1, p, d, env or {}, tuple(forms), expect)


def _strip(MB, NB, NCH, T33=1, LW=0, so=False):
    """so: the shape takes the self-overlapped form (write-out variant by the form, see expected())."""
    return dict(family='strip', MB=MB, NB=NB, NCH=NCH, T33=T33, LW=LW, so=so)


def _pipe(MB, NB, PU, KS=1):
    return dict(family='pipe', MB=MB, NB=NB, PU=PU, KS=KS)


def _tile(MB, NB, split):
    return dict(family='tile', MB=MB, NB=NB, split=split)


def expected(c, form):
    """The launch record `form` of case `c` must leave (form 'plain': the call without records / residual)."""
    e = dict(c.expect)
    if e['family'] == 'strip':
        so = e.pop('so')
        e['EPI'] = {'sums': 1, 'res_sums': 2, 'res_bits': 3}.get(form, 0)
        e['SO'] = {'plain': 1, 'stats': 2, 'stats_affine': 2, 'stats_bias': 0, 'mask': 5}.get(form, 1) if so else 0
    elif e['family'] == 'pipe':
        e['STATS'] = 1 if form.startswith('stats') else (2 if form == 'sums' else 0)
    e.pop('split', None)
    return e


def _tile_px(c):
    """Output pixels of one tile of the expected launch."""
    e = c.expect
    return 64 * e.get('MB', 1) // e.get('KS', 1)


def _out_hw(c):
    if c.op == 'dgrad':
        return c.H, c.W
    return ((c.H + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1, (c.W + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1)


def _n16(n):
    return (n + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------- the table
CASES = [
    # ---- strip, self-overlapped form: SO 2 (statistics); SO 5 / EPI 1-3 in the data-gradient cases below
    Fw('st_so16_w130', 16, 16, 9, 130, forms=FWD_FORMS, **_strip(4, 1, 1, so=True)),
    Fw('st_so16_w142', 16, 16, 7, 142, **_strip(4, 1, 1, so=True)),               # last width before the wide-row loader
    Fw('st_so16_w16', 16, 16, 3, 16, **_strip(4, 1, 1, so=True)),                 # narrowest row the strip decodes (Wo >= 16)
    Fw('st_so16_w17', 16, 16, 3, 17, **_strip(4, 1, 1, so=True)),                 # (at W = 16 every pixel block is whole)
    Fw('st_so16to4_w129', 16, 4, 9, 129, **_strip(4, 1, 1, so=True)),             # 12 zero-padded output channels
    Fw('st_so32_w65', 32, 32, 11, 65, forms=FWD_FORMS, **_strip(2, 2, 2, so=True)),
    Fw('st_so32_w78', 32, 32, 7, 78, **_strip(2, 2, 2, so=True)),                 # last width before the wide-row loader
    Fw('st_so32to20_w26', 32, 20, 7, 26, **_strip(2, 2, 2, so=True)),             # 12 zero-padded output channels
    # ---- strip, ping-pong form with statistics: compile-time grid
    Fw('st_pp16to32_w130', 16, 32, 9, 130, **_strip(4, 2, 1)),
    Fw('st_pp16_w50', 16, 16, 21, 50, **_strip(2, 1, 1)),
    Fw('st_pp16to32_w50', 16, 32, 21, 50, **_strip(2, 2, 1)),
    Fw('st_pp32_w53', 32, 32, 13, 53, **_strip(4, 2, 2)),
    Fw('st_pp32_w16', 32, 32, 5, 16, **_strip(4, 2, 2)),                          # Wo = 16 at 32 channels
    Fw('st_pp32to16_w53', 32, 16, 13, 53, **_strip(4, 1, 2)),
    Fw('st_pp32to4_w65', 32, 4, 11, 65, **_strip(2, 1, 2)),                       # 12 zero-padded output channels
    # ---- run-time tap grid (T33 = 0): strided forward where one tile spans <= 2 output rows, dilated 3x3
    Fw('st_s2_16to32_h3_w130', 16, 32, 3, 130, s=2, **_strip(4, 2, 1, T33=0)),
    Fw('st_s2_32_h5_w49', 32, 32, 5, 49, s=2, **_strip(4, 2, 2, T33=0)),
    Fw('st_d2_16_w130', 16, 16, 9, 130, p=2, d=2, **_strip(4, 1, 1, T33=0)),
    Fw('st_d2_16to32_w130', 16, 32, 9, 130, p=2, d=2, **_strip(2, 2, 1, T33=0)),
    Fw('st_d2_16_w46', 16, 16, 5, 46, p=2, d=2, **_strip(2, 1, 1, T33=0)),
    Fw('st_d2_32_w40', 32, 32, 7, 40, p=2, d=2, **_strip(2, 2, 2, T33=0)),
    Fw('st_d2_32to16_w51', 32, 16, 7, 51, p=2, d=2, **_strip(4, 1, 2, T33=0)),
    Fw('st_d2_32to16_w40', 32, 16, 7, 40, p=2, d=2, **_strip(2, 1, 2, T33=0)),
    # ---- wide-row loader, both edges of its window (16 channels: W = 143 .. 222, 32 channels: 79 .. 110)
    Fw('st_lw16_w143', 16, 16, 7, 143, **_strip(4, 1, 1, LW=1)),
    Fw('st_lw16_w222', 16, 16, 7, 222, **_strip(4, 1, 1, LW=1)),
    Fw('st_lw16to4_w216', 16, 4, 9, 216, **_strip(4, 1, 1, LW=1)),
    Fw('st_lw32_w79', 32, 32, 7, 79, **_strip(2, 2, 2, LW=1)),
    Fw('st_lw32_w110', 32, 32, 7, 110, **_strip(2, 2, 2, LW=1)),
    Fw('st_lw_s2_16_h2_w216', 16, 16, 2, 216, s=2, **_strip(4, 1, 1, T33=0, LW=1)),
    Fw('st_lw_s2_32_h2_w108', 32, 32, 2, 108, s=2, **_strip(2, 2, 2, T33=0, LW=1)),

    # ---- data gradient at 16 channels: SO 1 plain, SO 5 masked, EPI 1 / 2 / 3 sums (SO form, then the wide-row loader)
    Dg('dg_so16_w130', 16, 16, 9, 130, forms=DGRAD_FORMS, **_strip(4, 1, 1, so=True)),
    Dg('dg_so16_w142', 16, 16, 7, 142, forms=DGRAD_FORMS, **_strip(4, 1, 1, so=True)),
    Dg('dg_so16_w16', 16, 16, 3, 16, forms=DGRAD_FORMS, **_strip(4, 1, 1, so=True)),
    Dg('dg_so16_w17', 16, 16, 3, 17, forms=DGRAD_FORMS, **_strip(4, 1, 1, so=True)),
    Dg('dg_so16_w127', 16, 16, 23, 127, forms=DGRAD_FORMS, **_strip(4, 1, 1, so=True)),
    Dg('dg_lw16_w143', 16, 16, 7, 143, forms=DGRAD_FORMS, **_strip(4, 1, 1, LW=1)),
    Dg('dg_lw16_w222', 16, 16, 7, 222, forms=DGRAD_FORMS, **_strip(4, 1, 1, LW=1)),
    Dg('dg_lw16_w216', 16, 16, 9, 216, forms=DGRAD_FORMS, **_strip(4, 1, 1, LW=1)),
    # ---- at 32 channels: SO 5 and EPI 1 (residual + sums: the retreats)
    Dg('dg_so32_w65', 32, 32, 11, 65, forms=('mask', 'sums'), **_strip(2, 2, 2, so=True)),
    Dg('dg_so32_w78', 32, 32, 7, 78, forms=('mask', 'sums'), **_strip(2, 2, 2, so=True)),
    Dg('dg_so32_w26', 32, 32, 7, 26, forms=('mask', 'sums'), **_strip(2, 2, 2, so=True)),
    Dg('dg_so32to64_w65', 32, 64, 11, 65, **_strip(2, 2, 2, so=True)),                # two workgroups per strip in dx
    Dg('dg_lw32_w79', 32, 32, 7, 79, forms=('mask', 'sums'), **_strip(2, 2, 2, LW=1)),
    Dg('dg_lw32_w110', 32, 32, 7, 110, forms=('mask', 'sums'), **_strip(2, 2, 2, LW=1)),
    Dg('dg_lw32_w108', 32, 32, 9, 108, forms=('mask', 'sums'), **_strip(2, 2, 2, LW=1)),
    # ---- ping-pong form with the masked residual (compile-time grid; dilated: run-time grid)
    Dg('dg_pp16to32_w130', 16, 32, 9, 130, **_strip(4, 2, 1)),
    Dg('dg_pp16_w50', 16, 16, 21, 50, **_strip(2, 1, 1)),
    Dg('dg_pp16to32_w50', 16, 32, 21, 50, **_strip(2, 2, 1)),
    Dg('dg_pp32_w53', 32, 32, 13, 53, **_strip(4, 2, 2)),
    Dg('dg_pp32to16_w53', 32, 16, 13, 53, **_strip(4, 1, 2)),
    Dg('dg_pp32to16_w65', 32, 16, 11, 65, **_strip(2, 1, 2)),
    Dg('dg_d2_16_w130', 16, 16, 9, 130, p=2, d=2, **_strip(4, 1, 1, T33=0)),
    Dg('dg_d2_16to32_w130', 16, 32, 9, 130, p=2, d=2, **_strip(2, 2, 1, T33=0)),
    Dg('dg_d2_16to32_w100', 16, 32, 9, 100, p=2, d=2, **_strip(4, 2, 1, T33=0)),
    Dg('dg_d2_16_w46', 16, 16, 5, 46, p=2, d=2, **_strip(2, 1, 1, T33=0)),
    Dg('dg_d2_32_w40', 32, 32, 7, 40, p=2, d=2, **_strip(2, 2, 2, T33=0)),
    Dg('dg_d2_32_w51', 32, 32, 7, 51, p=2, d=2, **_strip(4, 2, 2, T33=0)),
    Dg('dg_d2_32to16_w51', 32, 16, 7, 51, p=2, d=2, **_strip(4, 1, 2, T33=0)),
    Dg('dg_d2_32to16_w40', 32, 16, 7, 40, p=2, d=2, **_strip(2, 1, 2, T33=0)),
    # run-time grid with the wide-row loader: dilated, two rows (the ring holds eight rows there, as in the strided forward cases)
    Dg('dg_lw_d2_16_h2_w215', 16, 16, 2, 215, p=2, d=2, **_strip(4, 1, 1, T33=0, LW=1)),
    Dg('dg_lw_d2_32_h2_w107', 32, 32, 2, 107, p=2, d=2, **_strip(2, 2, 2, T33=0, LW=1)),
    Dg('dg_pp32_w16', 32, 32, 5, 16, **_strip(4, 2, 2)),                              # Wo = 16 at 32 channels
    # ---- rows too narrow / too wide for the strip: conv_pipe_kernel at 16 and 32 channels
    Fw('st_narrow16_w23', 16, 16, 21, 23, **_pipe(1, 1, 5)),
    Fw('st_edge32_w111', 32, 32, 7, 111, **_pipe(1, 1, 8)),
    Dg('dg_narrow16_w23', 16, 16, 21, 23, forms=('mask', 'sums'), **_pipe(1, 1, 5)),
    Dg('dg_edge32_w111', 32, 32, 7, 111, forms=('mask', 'sums'), **_pipe(1, 1, 8)),
]

# conv_pipe_kernel: the shapes of tests/test_conv_epilogue_gpu.py, the tile of the rule and every other tile that fits, few
# persistent workgroups (each walks many units: the records cross unit and image boundaries); STATS 1 forward, STATS 2 and the
# masked residual in the stride-1 data gradient
PIPE_SHAPES = [('64_w33', 64, 20, 33, 1), ('96_w17', 96, 11, 17, 1), ('128_w9', 128, 13, 9, 1), ('256_w5', 256, 7, 5, 1),
               ('64_w12_s2', 64, 12, 12, 2), ('64_w54', 64, 9, 54, 1), ('128_h17_w9', 128, 17, 9, 1)]
# per shape: (MB, NB, PU, KS) of the rule's own tile, PU of the 2-row tiles (2x2, 2x1), KS of the forced 1x1 tile
PIPE_RULE = {'64_w33': ((1, 1, 5, 1), 5, 1), '96_w17': ((1, 1, 3, 2), 5, 2), '128_w9': ((1, 1, 3, 2), 5, 2),
             '256_w5': ((2, 1, 5, 1), 5, 2), '64_w12_s2': ((2, 1, 5, 1), 5, 1), '64_w54': ((1, 1, 5, 1), 8, 1),
             '128_h17_w9': ((1, 1, 3, 2), 5, 2)}


def _pipe_cases(name, ch, h, w, st, cid, env, rec):
    out = [Fw('st_pipe_' + cid, ch, ch - 12 if name == '64_w33' else ch, h, w, s=st, env=env, **rec)]
    if st == 1:
        out.append(Dg('dg_pipe_' + cid, ch, ch, h, w, forms=('mask', 'sums'), env=env, **rec))
    return out


for name, ch, h, w, st in PIPE_SHAPES:
    rule, pu2, ks1 = PIPE_RULE[name]
    CASES += _pipe_cases(name, ch, h, w, st, name, None, _pipe(*rule))
    CASES += _pipe_cases(name, ch, h, w, st, name + '_wgs3', {'DAM_PIPE_WGS': '3'}, _pipe(*rule))
    for (mb, nb), wgs in (((1, 4), 5), ((2, 2), 2), ((1, 2), 3), ((2, 1), 5), ((1, 1), 7)):
        if (ch // 16) % nb:
            continue                            # the tile must divide the block count (96 channels: no 1x4)
        ks = ks1 if (mb, nb) == (1, 1) else 1
        pu = 3 if ks == 2 else (pu2 if mb == 2 else 5)
        CASES += _pipe_cases(name, ch, h, w, st, '%s_%dx%d' % (name, mb, nb),
                             {'DAM_TILE': '%dx%d' % (mb, nb), 'DAM_PIPE_WGS': str(wgs)}, _pipe(mb, nb, pu, ks))
    if rule[3] == 2:                            # the K split switched off: the plain one-block tile
        CASES += _pipe_cases(name, ch, h, w, st, name + '_ks1', {'DAM_PIPE_KS': '1', 'DAM_PIPE_WGS': '4'}, _pipe(1, 1, 5, 1))

# the deep loader (PU 8) under the 1x4 and 1x2 tiles: 102 patch columns x 4 rows (the other three tiles: 64_w54 and edge32_w111)
for mb, nb, wgs in ((1, 4, 5), (1, 2, 3)):
    CASES += _pipe_cases('64_w100', 64, 7, 100, 1, '64_w100_%dx%d' % (mb, nb), {'DAM_TILE': '%dx%d' % (mb, nb), 'DAM_PIPE_WGS': str(wgs)},
                         _pipe(mb, nb, 8))

CASES += [
    # ---- conv_igemm_kernel with the masked residual, pipe kernel switched off (split-K: splitk_reduce_kernel applies the mask)
    Dg('dg_nopipe64_w33', 64, 64, 20, 33, env={'DAM_NO_PIPE': '1'}, **_tile(4, 4, True)),
    Dg('dg_nopipe256_w5', 256, 256, 7, 5, env={'DAM_NO_PIPE': '1'}, **_tile(1, 4, True)),
    Dg('dg_nopipe16_w23', 16, 16, 21, 23, env={'DAM_NO_PIPE': '1'}, **_tile(1, 1, False)),
    # ---- conv1x1_direct_kernel <NB, chunk slots> with the masked residual: 1x1 / stride-1 data gradients
    Dg('dg_1x1_32to32', 32, 32, 11, 65, k=1, p=0, family='1x1', NB=2, NCH=2),
    Dg('dg_1x1_32to48', 32, 48, 11, 65, k=1, p=0, family='1x1', NB=1, NCH=2),
    Dg('dg_1x1_64to32', 64, 32, 13, 33, k=1, p=0, family='1x1', NB=2, NCH=4),
    Dg('dg_1x1_64to48', 64, 48, 13, 33, k=1, p=0, family='1x1', NB=1, NCH=4),
    Dg('dg_1x1_128to32', 128, 32, 9, 17, k=1, p=0, family='1x1', NB=2, NCH=8),
    Dg('dg_1x1_96to48', 96, 48, 9, 17, k=1, p=0, family='1x1', NB=1, NCH=8),
]
# the twelve <MB, NB> instantiations: 5x5 data gradients 64 -> 16 / 32 / 48 / 64 at three sizes (MB by least padding, NB by block count)
for co, nb in ((16, 1), (32, 2), (48, 3), (64, 4)):
    for (h, w), mb, split in (((22, 17), 2, True), ((13, 17), 4, True), ((7, 5), 1, False)):
        CASES.append(Dg('dg_tile_k5_64to%d_%dx%d' % (co, h, w), 64, co, h, w, k=5, p=0, **_tile(mb, nb, split)))
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def _variant(rec, stats=False):
    """The part of a launch record that names a kernel instantiation / write-out path.  `stats`: the launch left statistics
    records (the strip's ping-pong form takes them at run time: the record alone does not say so)."""
    if rec.family == 'strip':
        return ('strip', rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.EPI, rec.SO) + (('stats',) if stats and rec.SO == 0 else ())
    if rec.family == 'pipe':
        return ('pipe', rec.MB, rec.NB, rec.PU, rec.STATS, rec.KS)
    if rec.family == 'pipe_ranges':
        return ('pipe_ranges', rec.ranges)
    if rec.family == 'tile':
        return ('tile', rec.MB, rec.NB, 'split-K' if rec.ksplit > 1 else 'one pass')
    if rec.family == '1x1':
        return ('1x1', rec.NB, rec.NCH)
    return (rec.family,)


def _tile_of(rec):
    """Family and tile: two launches that agree here sum in the same order."""
    return (rec.family, rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.PU, rec.KS, rec.ksplit, rec.ranges)


_PP = [(4, 2, 1, 1, 0), (2, 1, 1, 1, 0), (2, 2, 1, 1, 0), (4, 2, 2, 1, 0), (4, 1, 2, 1, 0), (2, 1, 2, 1, 0),
       (4, 2, 1, 0, 0), (4, 2, 2, 0, 0), (4, 1, 1, 0, 0), (2, 2, 1, 0, 0), (2, 1, 1, 0, 0), (2, 2, 2, 0, 0), (4, 1, 2, 0, 0), (2, 1, 2, 0, 0),
       (4, 1, 1, 1, 1), (2, 2, 2, 1, 1), (4, 1, 1, 0, 1), (2, 2, 2, 0, 1)]
# all eleven launch_pipe<MB, NB, PU, KS>: five tiles x loader depth 5 / 8, the K split
_PIPE_TILES = [(mb, nb, pu, 1) for mb, nb in ((1, 4), (2, 2), (1, 2), (2, 1), (1, 1)) for pu in (5, 8)] + [(1, 1, 3, 2)]
REQUIRED = {
    # form group -> variants (as _variant() names them) some case of the group must launch
    'stats': (
        [('strip', 4, 1, 1, 1, 0, 0, 2), ('strip', 2, 2, 2, 1, 0, 0, 2)] +
        # the ping-pong form with statistics; <4, 1, 1> / <2, 2, 2> with the compile-time grid: statistics + bias only
        [('strip',) + t + (0, 0, 'stats') for t in _PP] +
        [('strip', 4, 1, 1, 1, 0, 0, 0, 'stats'), ('strip', 2, 2, 2, 1, 0, 0, 0, 'stats')] +
        [('pipe', mb, nb, pu, 1, ks) for mb, nb, pu, ks in _PIPE_TILES]),
    'mask': (
        [('strip', 4, 1, 1, 1, 0, 0, 5), ('strip', 2, 2, 2, 1, 0, 0, 5)] +
        # (strided layers reach the data gradient through other entry points: the run-time grid by dilation only)
        [('strip',) + t + (0, 0) for t in _PP] +
        [('pipe', mb, nb, pu, 0, ks) for mb, nb, pu, ks in _PIPE_TILES] +
        [('tile', mb, nb, 'split-K') for mb in (4, 2) for nb in (1, 2, 3, 4)] + [('tile', 1, nb, 'one pass') for nb in (1, 2, 3, 4)] +
        [('tile', 1, 4, 'split-K')] +
        [('1x1', nb, nch) for nb in (2, 1) for nch in (2, 4, 8)]),
    'sums': (
        [('strip', 4, 1, 1, 1, 0, epi, 1) for epi in (1, 2, 3)] + [('strip', 2, 2, 2, 1, 0, 1, 1)] +
        [('strip', 4, 1, 1, 1, 1, epi, 0) for epi in (1, 2, 3)] + [('strip', 2, 2, 2, 1, 1, 1, 0)] +
        [('pipe', mb, nb, pu, 2, ks) for mb, nb, pu, ks in _PIPE_TILES]),
}
GROUP = {'stats': 'stats', 'stats_affine': 'stats', 'stats_bias': 'stats', 'mask': 'mask', 'sums': 'sums', 'res_sums': 'sums',
         'res_bits': 'sums'}


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(c, salt=0):
    return torch.Generator().manual_seed(5000 + 10 * list(BY_ID).index(c.id) + salt)


def _signed_mask(shape, g):
    """i.i.d., |m| >= 0.1: `> 0` is unambiguous."""
    m = torch.randn(shape, generator=g)
    return torch.where(m >= 0, m + 0.1, m - 0.1)


def _sign_bytes(positive):
    """[B, H, W, C] bool -> the sign bytes of bn_apply: bit i of byte [b, h, w, q] is channel 4 * q + i."""
    B, H, W, C = positive.shape
    weights = torch.tensor([1, 2, 4, 8], dtype=torch.int32)
    return (positive.view(B, H, W, C // 4, 4).to(torch.int32) * weights).sum(-1).to(torch.uint8).contiguous()


@functools.lru_cache(maxsize=4)
def fwd_inputs(cid):
    """x [B, Ci, H, W] = randn * 3 + 7, w, in_scale / in_shift, bias [n16] (zero in the padded channels) and the float64
    convolutions [B, Ho, Wo, Co] of the three forms."""
    c = BY_ID[cid]
    g = _gen(c)
    x = torch.randn(c.B, c.Ci, c.H, c.W, generator=g) * 3 + 7
    w = torch.randn(c.Co, c.Ci, c.k, c.k, generator=g) / (c.Ci * c.k * c.k) ** 0.5
    sc, sh = torch.rand(c.Ci, generator=g) + 0.5, torch.randn(c.Ci, generator=g)
    bias = torch.zeros(_n16(c.Co))
    bias[:c.Co] = torch.randn(c.Co, generator=g)
    a = torch.relu(x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
    want = {'stats': F.conv2d(x.double(), w.double(), None, c.s, c.p, c.d).permute(0, 2, 3, 1),
            'stats_affine': F.conv2d(a, w.double(), None, c.s, c.p, c.d).permute(0, 2, 3, 1)}
    want['stats_bias'] = want['stats'] + bias[:c.Co].double()
    return dict(x=x, w=w, sc=sc, sh=sh, bias=bias, want=want)


@functools.lru_cache(maxsize=4)
def dgrad_inputs(cid):
    """dy [B, Ho, Wo, K], w [K, N, k, k], the float64 data gradient [B, H, W, N]; res / res_mask [B, H, W, n16] i.i.d. (zero in
    the padded channels); the upstream BatchNorm's x (edited so that the mask has its margin), statistics and mask maps; an
    upstream mask of its own for the sign-byte form."""
    c = BY_ID[cid]
    g = _gen(c)
    n16 = _n16(c.Ci)
    Ho, Wo = c.H + 2 * c.p - c.d * (c.k - 1), c.W + 2 * c.p - c.d * (c.k - 1)
    dy = torch.randn(c.B, Ho, Wo, c.Co, generator=g)
    w = torch.randn(c.Co, c.Ci, c.k, c.k, generator=g) / (c.Co * c.k * c.k) ** 0.5
    want = torch.nn.grad.conv2d_input((c.B, c.Ci, c.H, c.W), w.double(), dy.permute(0, 3, 1, 2).double(), 1, c.p, c.d).permute(0, 2, 3, 1)
    res, mask = torch.zeros(c.B, c.H, c.W, n16), torch.ones(c.B, c.H, c.W, n16)
    res[..., :c.Ci] = torch.randn(c.B, c.H, c.W, c.Ci, generator=g)
    mask[..., :c.Ci] = _signed_mask((c.B, c.H, c.W, c.Ci), g)
    d = dict(dy=dy, w=w, want=want.contiguous(), res=res, mask=mask)
    if set(c.forms) & {'sums', 'res_sums', 'res_bits'}:
        assert n16 == c.Ci
        x = torch.randn(c.B, c.H, c.W, n16, generator=g) * 1.5 + 0.3
        gamma, beta = torch.rand(n16, generator=g) + 0.5, 0.3 * torch.randn(n16, generator=g)
        mean = x.double().mean((0, 1, 2)).float()
        invstd = (1.0 / torch.sqrt(x.double().var((0, 1, 2), unbiased=False) + EPS)).float()
        msc = gamma * invstd
        msh = beta - mean * msc
        t = x.double() * msc.double() + msh.double()
        near = t.abs() < MARGIN
        moved = (torch.where(t >= 0, 2 * MARGIN, -2 * MARGIN) - msh.double()) / msc.double()
        x = torch.where(near, moved, x.double()).float()
        t = x.double() * msc.double() + msh.double()
        um = _signed_mask((c.B, c.H, c.W, n16), g)
        d.update(x=x, mean=mean, invstd=invstd, msc=msc, msh=msh, t=t, um=um,
                 xhat=(x.double() - mean.double()) * invstd.double())
    return d


# ------------------------------------------------------------------------------------------- conditions, without a GPU
def test_table_conditions():
    """B >= 2 everywhere and B = 3 at least once per required variant (here: everywhere); the last tile of every launch is
    ragged (tiles straddle rows and images); H within 3 .. 23 (2 where the run-time grid meets wide rows); both edges of every
    width window in every form group."""
    for c in CASES:
        Ho, Wo = _out_hw(c)
        assert c.B == 3 and (2 if c.expect.get('LW') and not c.expect.get('T33') else 3) <= c.H <= 23, c.id   # (run-time grid on wide rows: <= 2 rows)
        assert (Ho * Wo) % _tile_px(c) != 0, '%s: %d output pixels, tile of %d' % (c.id, Ho * Wo, _tile_px(c))
        # ... and so is its last 16-pixel block: lanes past the image inside a block that is written (whole blocks past the image
        # are skipped as blocks).  Impossible at Wo = 16, the narrowest row -- the W = 17 cases stand beside those.
        assert (Ho * Wo) % 16 != 0 or Wo == 16, c.id
        assert c.forms and set(c.forms) <= set(FWD_FORMS if c.op == 'fwd' else DGRAD_FORMS), c.id
        if c.expect['family'] == 'strip':
            assert Wo >= 16, c.id
    for group, forms in (('stats', FWD_FORMS), ('mask', ('mask',)), ('sums', ('sums',))):
        strips = [c for c in CASES if c.expect['family'] == 'strip' and set(c.forms) & set(forms) and c.s == 1 and c.d == 1]
        k16 = {_out_hw(c)[1] for c in strips if (c.Ci if c.op == 'fwd' else c.Co) == 16}
        k32 = {_out_hw(c)[1] for c in strips if (c.Ci if c.op == 'fwd' else c.Co) == 32}
        assert {16, 142, 143, 222} <= k16, (group, sorted(k16))
        # (Wo = 16 at 32 channels is the ping-pong <4, 2, 2>, which has no sums epilogue: test_retreat_backward_sums[rt_sums_32_w16])
        assert {78, 79, 110} | ({16} if group != 'sums' else set()) <= k32, (group, sorted(k32))
    # 12 zero-padded output channels in at least one statistics case per family
    for fam in ('strip', 'pipe'):
        assert any(c.op == 'fwd' and c.expect['family'] == fam and _n16(c.Co) - c.Co == 12 for c in CASES), fam
    # every required variant is named by some case of its group
    for group, variants in REQUIRED.items():
        named = set()
        for c in CASES:
            for form in c.forms:
                if GROUP[form] == group:
                    named.add(_variant(ops_record(expected(c, form), c.expect.get('split')), stats=group == 'stats'))
        assert not [v for v in variants if v not in named], (group, [v for v in variants if v not in named])


def ops_record(e, split=False):
    """An expected-record dict as a full launch record (fields a family does not use are 0)."""
    fields = 'family MB NB NCH T33 LW EPI SO PU STATS KS ksplit ranges'.split()
    return collections.namedtuple('Rec', fields)(*[e.get(f, 0) for f in fields])._replace(ksplit=2 if split else 1)


@pytest.mark.parametrize('cid', [c.id for c in CASES if c.op == 'dgrad'])
def test_input_conditions(cid):
    """What keeps a broken write-out from passing, on the CPU: 25-75 % of the mask bits set (both kinds of mask), |mask| >= 0.1,
    max|res| >= 0.1 of the scale, the margin of the affine mask, res and the masks differ from element to element."""
    c = BY_ID[cid]
    d = dgrad_inputs(cid)
    _check_dgrad_inputs(c, d)


def _check_dgrad_inputs(c, d):
    scale = d['want'].abs().max().item()
    live = d['mask'][..., :c.Ci]
    assert 0.25 <= (live > 0).double().mean().item() <= 0.75 and live.abs().min().item() >= 0.1
    assert d['res'].abs().max().item() >= 0.1 * scale
    r = d['res'][..., :c.Ci].reshape(-1)
    assert torch.unique(r).numel() >= 0.99 * r.numel()              # i.i.d. per element: no value repeats along any axis
    if 'x' in d:
        assert d['t'].abs().min().item() >= MARGIN
        for m in (d['t'], d['um']):
            assert 0.25 <= (m > 0).double().mean().item() <= 0.75
        assert d['um'].abs().min().item() >= 0.1


# ------------------------------------------------------------------------------------------------------------ the device
@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


SEEN = {}           # (case id, form) -> (ConvLaunch, statistics records left?)
WORST = {}          # (family, quantity) -> (relative error / share of the bound, case id, form)


def _note(rec, what, value, cid, form):
    key = (rec.family + ('' if rec.family != 'strip' else (' SO' if rec.SO else (' LW' if rec.LW else ' PP'))), what)
    if value > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (value, cid, form)


def _guarded(shape):
    numel = 1
    for n in shape:
        numel *= n
    buf = torch.full((2 * GUARD + numel,), FILL, dtype=torch.int32, device='cuda')
    return buf, buf.view(torch.float32)[GUARD:GUARD + numel].view(shape)


def _result(buf, shape, what):
    """Guard bands intact -> the result as float32 on the host."""
    host = buf.cpu()
    assert bool((host[:GUARD] == FILL).all()) and bool((host[-GUARD:] == FILL).all()), '%s: guard band written' % what
    return host.view(torch.float32)[GUARD:-GUARD].view(shape)


def _assert_record(c, form, rec, parts_left=False):
    SEEN[(c.id, form)] = (rec, parts_left)
    want = expected(c, form)
    got = {k: getattr(rec, k) for k in want}
    assert got == want, '%s %s: launched %s' % (c.id, form, rec)
    if 'split' in c.expect:
        assert (rec.ksplit > 1) == c.expect['split'], '%s %s: launched %s' % (c.id, form, rec)


class _Env:
    def __init__(self, monkeypatch, env):
        self.ctx = monkeypatch.context()
        self.env = env

    def __enter__(self):
        mp = self.ctx.__enter__()
        for k, v in self.env.items():
            mp.setenv(k, v)

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


def _fwd_call(ops, c, form, dev, with_stats, check=True):
    """One conv2d_fwd of `form` into guarded buffers -> (y buffer, statistics buffer or None, parts, record)."""
    Ho, Wo = _out_hw(c)
    n16 = _n16(c.Co)
    ybuf, out = _guarded((c.B, Ho, Wo, n16))
    kw = {}
    if form == 'stats_affine':
        kw.update(in_scale=dev['sc'], in_shift=dev['sh'], relu_in=True)
    if form == 'stats_bias':
        kw.update(bias=dev['bias'])
    sbuf, parts = None, 0
    if with_stats:
        from deep_audio_mixer_amd import _lib
        sbuf, part_view = _guarded((int(_lib.lib().dam_bn_workspace_floats(n16)),))
        y, parts = ops.conv2d_fwd(dev['x'], dev['wp'], c.Co, c.k, c.k, c.s, c.p, c.d, bn_partial=part_view, out=out, **kw)
    else:
        y = ops.conv2d_fwd(dev['x'], dev['wp'], c.Co, c.k, c.k, c.s, c.p, c.d, out=out, **kw)
    rec = ops.conv_last_launch()
    plan = ops.conv2d_fwd_plan(dev['x'].shape, c.Co, c.k, c.k, c.s, c.p, c.d, bn_partial=with_stats, parts=True, **kw)
    assert plan == (rec, parts), '%s %s: launched %s with %d records, planned %s' % (c.id, form, rec, parts, plan)
    assert y is out
    if with_stats and check:
        _assert_record(c, form, rec, parts > 0)
    return ybuf, sbuf, parts, rec


def merge_records(rec):
    """[parts, C, 3] float64 records (n, mean, M2) -> (n, mean, M2) per channel, record by record with Chan's formula."""
    C = rec.shape[1]
    n, mean, m2 = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for r in rec:
        nb = r[:, 0]
        nn = n + nb
        f = torch.where(nn > 0, nb / nn.clamp(min=1), torch.zeros_like(nn))
        dlt = r[:, 1] - mean
        mean = mean + dlt * f
        m2 = m2 + r[:, 2] + dlt * dlt * n * f
        n = nn
    return n, mean, m2


def test_merge_records_matches_two_pass():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(7, 50, 4, generator=g, dtype=torch.float64) * 2 + 5
    rec = torch.stack([torch.full((7, 4), 50.0, dtype=torch.float64), v.mean(1), ((v - v.mean(1, keepdim=True)) ** 2).sum(1)], -1)
    rec[3] = 0                                                          # an empty record
    v = torch.cat([v[:3], v[4:]]).reshape(-1, 4)
    n, mean, m2 = merge_records(rec)
    assert bool((n == 300).all()) and torch.allclose(mean, v.mean(0), rtol=1e-13) and torch.allclose(m2 / n, v.var(0, unbiased=False), rtol=1e-12)


def check_statistics(c, form, host_stats, parts, want, rec):
    """The records of one launch against the float64 convolution `want` [B, Ho, Wo, Co]."""
    n16 = _n16(c.Co)
    used = parts * n16 * 3
    assert 0 < parts <= 2048
    assert bool((host_stats.view(torch.int32)[used:] == FILL).all()), '%s %s: written behind record %d' % (c.id, form, parts)
    r = host_stats[:used].view(parts, n16, 3).double()
    count = r[..., 0]
    assert bool((count >= 0).all()) and bool((count == count.round()).all()), '%s %s: counts' % (c.id, form)
    npx = want.shape[0] * want.shape[1] * want.shape[2]
    assert bool((count.sum(0)[:c.Co] == npx).all()), '%s %s: counts sum to %s, %d pixels' % (c.id, form, count.sum(0)[:c.Co].tolist(), npx)
    assert bool((r[..., 2] >= 0).all()), '%s %s: negative M2' % (c.id, form)
    if c.Co < n16:
        assert torch.count_nonzero(r[:, c.Co:, 1:]) == 0, '%s %s: padded channels with mean / M2' % (c.id, form)
    n, mean, m2 = merge_records(r[:, :c.Co])
    wm, wv = want.mean((0, 1, 2)), want.var((0, 1, 2), unbiased=False)
    e_mean = ((mean - wm).abs().max() / wm.abs().max()).item()
    e_inv = ((1 / (m2 / n + EPS).sqrt() - 1 / (wv + EPS).sqrt()).abs() * (wv + EPS).sqrt()).max().item()
    print('%s %s: %d records; mean err %.2e of max|mean|, invstd err %.2e relative' % (c.id, form, parts, e_mean, e_inv))
    _note(rec, 'mean', e_mean, c.id, form), _note(rec, 'invstd', e_inv, c.id, form)
    assert e_mean <= TOL_MEAN, '%s %s: mean err %.3g' % (c.id, form, e_mean)
    assert e_inv <= TOL_INVSTD, '%s %s: invstd err %.3g' % (c.id, form, e_inv)


def check_values(c, form, got, want, rec, what):
    """got [.., n16] float32 against want [.., n real] float64: 2e-5 of the max-abs, padded channels exactly zero."""
    n = want.shape[-1]
    if n < got.shape[-1]:
        assert torch.count_nonzero(got[..., n:]) == 0, '%s %s: padded channels not zero' % (c.id, form)
    scale = want.abs().max().item()
    err = (got[..., :n].double() - want).abs()
    worst = err.max().item()
    where = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
    print('%s %s: %s  %s err %.2e of scale %.3g at %s' % (c.id, form, rec, what, worst / scale, scale, where))
    _note(rec, what, worst / scale, c.id, form)
    assert worst <= TOL * scale, '%s %s: %s err %.3g > %.3g at %s (%d elements over)' % (
        c.id, form, what, worst, TOL * scale, where, int((err > TOL * scale).sum()))
    return scale


def check_same(c, form, a, rec_a, b, rec_b, scale, where=None):
    """a is bitwise b (where `where`) if the two launches agree on family and tile, else within 2e-6 of the scale."""
    if where is not None:
        a, b = a[where], b[where]
    if _tile_of(rec_a) == _tile_of(rec_b):
        assert torch.equal(a, b), '%s %s: not bitwise the other call (%d elements differ; %s / %s)' % (
            c.id, form, int((a != b).sum()), rec_a, rec_b)
    else:
        worst = (a.double() - b.double()).abs().max().item()
        assert worst <= TOL_ORDER * scale, '%s %s: %.3g apart from the other call (%s / %s)' % (c.id, form, worst, rec_a, rec_b)


def _fwd_device(ops, c, d):
    return dict(x=d['x'].permute(0, 2, 3, 1).contiguous().cuda(), wp=ops.pack_weights(d['w'].cuda()), sc=d['sc'].cuda(),
                sh=d['sh'].cuda(), bias=d['bias'].cuda())


def run_fwd_case(ops, c, monkeypatch, check=True):
    d = fwd_inputs(c.id)
    dev = _fwd_device(ops, c, d)
    Ho, Wo = _out_hw(c)
    shape = (c.B, Ho, Wo, _n16(c.Co))
    for form in c.forms:
        with _Env(monkeypatch, c.env):
            ybuf, sbuf, parts, rec = _fwd_call(ops, c, form, dev, True, check)
            ybuf0, _, _, rec0 = _fwd_call(ops, c, form, dev, False)
        if not check:
            SEEN.setdefault((c.id, form), (rec, parts > 0))
            continue
        torch.cuda.synchronize()
        assert parts > 0, '%s %s: no statistics from %s' % (c.id, form, rec)
        y, y0 = _result(ybuf, shape, c.id + ' y'), _result(ybuf0, shape, c.id + ' y without bn_partial')
        stats = _result(sbuf, (sbuf.numel() - 2 * GUARD,), c.id + ' bn_partial')
        want = d['want'][form]
        scale = check_values(c, form, y, want, rec, 'y')
        check_same(c, form, y, rec, y0, rec0, scale)
        check_statistics(c, form, stats, parts, want, rec)


def _dgrad_device(ops, c, d):
    dev = dict(dy=d['dy'].cuda(), wpt=ops.pack_weights(d['w'].cuda(), transpose=True), res=d['res'].cuda(), mask=d['mask'].cuda())
    if 'x' in d:
        dev.update(bits=_sign_bytes(d['mask'] > 0).cuda(), ubits=_sign_bytes(d['um'] > 0).cuda(),
                   **{k: d[k].cuda() for k in ('x', 'mean', 'invstd', 'msc', 'msh')})
    return dev


def _dgrad_call(ops, c, form, dev):
    """One conv2d_dgrad of `form` into a guarded buffer -> (buffer, partials, record)."""
    buf, out = _guarded((c.B, c.H, c.W, _n16(c.Ci)))
    kw = {}
    if form in ('mask', 'res_sums', 'res_bits'):
        kw.update(res=dev['res'], res_mask=dev['mask'])
    if form == 'sums':
        kw.update(bn_bwd=(dev['x'], dev['mean'], dev['invstd'], dev['msc'], dev['msh']))
    if form == 'res_sums':
        kw.update(res_mask_bits=dev['bits'], bn_bwd=(dev['x'], dev['mean'], dev['invstd'], dev['msc'], dev['msh']))
    if form == 'res_bits':
        kw.update(res_mask_bits=dev['bits'], bn_bwd=(dev['x'], dev['mean'], dev['invstd'], None, None, dev['ubits']))
    got = ops.conv2d_dgrad(dev['dy'], dev['wpt'], c.Ci, c.H, c.W, c.k, c.k, 1, c.p, c.d, out=out, **kw)
    rec = ops.conv_last_launch()
    dx, partials = got if isinstance(got, tuple) else (got, None)
    plan = ops.conv2d_dgrad_plan(dev['dy'].shape, c.Ci, c.H, c.W, c.k, c.k, 1, c.p, c.d, parts=True, **kw)
    assert plan == (rec, partials[1] if partials else 0), '%s %s: launched %s with %s, planned %s' % (c.id, form, rec, partials and partials[1], plan)
    assert dx is out
    return buf, partials, rec


def check_sums(c, form, partials, want_dx, upstream_positive, xhat, rec):
    """The two sums per channel against float64 sums over the float64 reference dx."""
    records, parts = partials
    C = want_dx.shape[-1]
    assert 0 < parts <= 1024
    sums = records[:parts * C * 2].view(parts, C, 2).double().sum(0).cpu()
    dz = want_dx * upstream_positive
    for col, term, name in ((0, dz, 'sum dz'), (1, dz * xhat, 'sum dz*xhat')):
        bound = term.abs().sum((0, 1, 2))
        share = ((sums[:, col] - term.sum((0, 1, 2))).abs() / bound).max().item()
        print('%s %s: %d records; %s err %.2e of sum |term|' % (c.id, form, parts, name, share))
        _note(rec, name, share, c.id, form)
        assert share <= TOL_SUMS, '%s %s: %s err %.3g of sum |term|' % (c.id, form, name, share)


def run_dgrad_case(ops, c, monkeypatch, check=True):
    d = dgrad_inputs(c.id)
    dev = _dgrad_device(ops, c, d)
    shape = (c.B, c.H, c.W, _n16(c.Ci))
    if check:
        _check_dgrad_inputs(c, d)
    with _Env(monkeypatch, c.env):
        calls = {}
        for form in c.forms:
            calls[form] = _dgrad_call(ops, c, form, dev)
            if form in ('mask', 'sums'):                     # each is followed by the plain call on the same dy and weights
                calls['plain after ' + form] = _dgrad_call(ops, c, 'plain', dev)
    for form in c.forms:
        SEEN.setdefault((c.id, form), (calls[form][2], calls[form][1] is not None))
    if not check:
        return
    torch.cuda.synchronize()
    want = d['want']
    want_res = want.clone()
    want_res += (d['res'] * (d['mask'] > 0))[..., :c.Ci].double()
    host = {k: _result(v[0], shape, '%s %s' % (c.id, k)) for k, v in calls.items()}
    for form in c.forms:
        buf, partials, rec = calls[form]
        _assert_record(c, form, rec, partials is not None)
        if form == 'mask':
            plain, rec_p = host['plain after mask'], calls['plain after mask'][2]
            _assert_record(c, 'plain', rec_p)
            scale = check_values(c, 'plain', plain, want, rec_p, 'dx')
            check_values(c, form, host[form], want_res, rec, 'dx')
            check_same(c, form, host[form], rec, plain, rec_p, scale, where=d['mask'] <= 0)
            continue
        assert partials is not None, '%s %s: no sums from %s' % (c.id, form, rec)
        if form == 'sums':
            base, rec_b, ref = host['plain after sums'], calls['plain after sums'][2], want
        else:
            base, rec_b, ref = host['mask'], calls['mask'][2], want_res
        check_values(c, form, host[form], ref, rec, 'dx')
        assert torch.equal(host[form], base), '%s %s: dx is not bitwise the call without bn_bwd (%s / %s)' % (c.id, form, rec, rec_b)
        check_sums(c, form, partials, ref, (d['um'] > 0) if form == 'res_bits' else (d['t'] > 0), d['xhat'], rec)


def run_case(ops, c, monkeypatch, check=True):
    (run_fwd_case if c.op == 'fwd' else run_dgrad_case)(ops, c, monkeypatch, check)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_training_epilogue(ops, case, monkeypatch):
    run_case(ops, case, monkeypatch)


@pytest.mark.gpu
def test_coverage(ops, monkeypatch):
    """The union of the launches the table made covers REQUIRED.  (Cases that did not run in this process -- a -k selection --
    are launched here without their oracle, so the test stands on its own.)"""
    for c in CASES:
        if any((c.id, f) not in SEEN for f in c.forms):
            run_case(ops, c, monkeypatch, check=False)
    torch.cuda.synchronize()
    for key in sorted(WORST):
        print('worst %s, %s: %.2e (%s, %s)' % (key + WORST[key]))
    for group, variants in REQUIRED.items():
        seen = {_variant(rec, stats=left and group == 'stats') for (cid, form), (rec, left) in SEEN.items() if GROUP.get(form) == group}
        print('%s: variants seen: %s' % (group, sorted(seen, key=str)))
        lacking = [v for v in variants if v not in seen]
        assert not lacking, '%s: kernel variants no case reached: %s' % (group, lacking)


# ----------------------------------------------------------------------------------------------------------- the retreats
def _retreat_fwd(ops, Ci, Co, H, W, B, s=1, p=1, d=1, seed=0):
    """conv2d_fwd(bn_partial=) -> (y, parts, record, statistics buffer untouched?, float64 reference, y without bn_partial, its record)"""
    from deep_audio_mixer_amd import _lib
    g = torch.Generator().manual_seed(9000 + seed)
    x = torch.randn(B, Ci, H, W, generator=g) * 3 + 7
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
    want = F.conv2d(x.double(), w.double(), None, s, p, d).permute(0, 2, 3, 1)
    xd, wp = x.permute(0, 2, 3, 1).contiguous().cuda(), ops.pack_weights(w.cuda())
    ybuf, out = _guarded(tuple(want.shape))
    sbuf, part_view = _guarded((int(_lib.lib().dam_bn_workspace_floats(Co)),))
    _, parts = ops.conv2d_fwd(xd, wp, Co, 3, 3, s, p, d, bn_partial=part_view, out=out)
    rec = ops.conv_last_launch()
    y0 = ops.conv2d_fwd(xd, wp, Co, 3, 3, s, p, d)
    rec0 = ops.conv_last_launch()
    torch.cuda.synchronize()
    y = _result(ybuf, tuple(want.shape), 'y')
    stats = _result(sbuf, (sbuf.numel() - 2 * GUARD,), 'bn_partial')
    return y, parts, rec, stats, want, y0.cpu(), rec0


def _assert_close(got, want, what):
    scale = want.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print('%s: err %.2e of scale %.3g' % (what, err / scale, scale))
    assert err <= TOL * scale, (what, err, scale)
    return scale


@pytest.mark.gpu
def test_retreat_statistics_two_channel_workgroups(ops):
    """16 -> 64: the strip needs two workgroups per strip for the 64 output channels -> no statistics, the plain strip launch."""
    y, parts, rec, stats, want, y0, rec0 = _retreat_fwd(ops, 16, 64, 9, 130, 3, seed=1)
    assert parts == 0 and bool((stats.view(torch.int32) == FILL).all())
    assert (rec.family, rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.EPI, rec.SO) == ('strip', 4, 2, 1, 1, 0, 0, 0), rec
    _assert_close(y, want, 'y')
    assert rec0 == rec and torch.equal(y, y0)


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1024, 1025])
def test_retreat_statistics_1024_strip_records(ops, B):
    """One strip per 3 x 16 image: 1024 images still leave their 1024 records, 1025 leave none (the same launch without)."""
    y, parts, rec, stats, want, y0, rec0 = _retreat_fwd(ops, 16, 16, 3, 16, B, seed=2)
    _assert_close(y, want, 'y')
    assert torch.equal(y, y0)
    assert (rec.family, rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.EPI) == ('strip', 4, 1, 1, 1, 0, 0), rec
    if B > 1024:
        assert parts == 0 and rec.SO == 1 and bool((stats.view(torch.int32) == FILL).all())
        return
    assert parts == 1024 and rec.SO == 2
    c = Fw('records_1024', 16, 16, 3, 16, B=B, **_strip(4, 1, 1, so=True))
    check_statistics(c, 'stats', stats, parts, want, rec)


@pytest.mark.gpu
def test_retreat_statistics_on_column_ranges(ops):
    """16 -> 32 / stride 2 at W = 130 runs conv_pipe_kernel on two column ranges -- but not with bn_partial (ranges leave no
    records): conv_igemm_kernel answers, parts == 0."""
    y, parts, rec, stats, want, y0, rec0 = _retreat_fwd(ops, 16, 32, 12, 130, 3, s=2, seed=3)
    assert parts == 0 and bool((stats.view(torch.int32) == FILL).all())
    assert rec.family == 'tile' and (rec0.family, rec0.ranges) == ('pipe_ranges', 2), (rec, rec0)
    scale = _assert_close(y, want, 'y')
    assert (y.double() - y0.double()).abs().max().item() <= TOL_ORDER * scale


@pytest.mark.gpu
@pytest.mark.parametrize('B', [256, 257])
def test_retreat_statistics_2048_pipe_records(ops, B):
    """conv_pipe_kernel leaves one record per image tile and wave: 256 images of 5 x 17 pixels (two 64-pixel tiles) fill the
    2048 records of the workspace, 257 leave none -- the same kernel without the epilogue."""
    y, parts, rec, stats, want, y0, rec0 = _retreat_fwd(ops, 64, 64, 5, 17, B, seed=4)
    _assert_close(y, want, 'y')
    assert (rec.family, rec.MB, rec.NB, rec.KS) == ('pipe', 1, 4, 1) and rec0 == rec._replace(STATS=0) and torch.equal(y, y0), (rec, rec0)
    if B > 256:
        assert parts == 0 and rec.STATS == 0 and bool((stats.view(torch.int32) == FILL).all())
        return
    assert parts == 2048 and rec.STATS == 1
    check_statistics(Fw('records_2048', 64, 64, 5, 17, B=B, **_pipe(1, 4, 5)), 'stats', stats, parts, want, rec)


def _retreat_dgrad(ops, c, form, monkeypatch):
    """-> (dx of `form`, partials, record, dx of the float-mask / plain call, its record, float64 reference)"""
    d = dgrad_inputs(c.id)
    dev = _dgrad_device(ops, c, d)
    base_form = 'mask' if form.startswith('res') else 'plain'
    buf, partials, rec = _dgrad_call(ops, c, form, dev)
    buf0, _, rec0 = _dgrad_call(ops, c, base_form, dev)
    torch.cuda.synchronize()
    shape = (c.B, c.H, c.W, _n16(c.Ci))
    want = d['want'] + ((d['res'] * (d['mask'] > 0))[..., :c.Ci].double() if form.startswith('res') else 0)
    return _result(buf, shape, 'dx'), partials, rec, _result(buf0, shape, 'dx'), rec0, want


RETREATS = [
    # residual + sums at 32 channels: no EPI 2 / 3 instantiation -> the float mask: SO 5, ping-pong wide-row
    (Dg('rt_res_sums_32_w65', 32, 32, 11, 65, forms=DGRAD_FORMS), 'res_sums', ('strip', 2, 2, 2, 1, 0, 0, 5)),
    (Dg('rt_res_bits_32_w65', 32, 32, 11, 65, forms=DGRAD_FORMS), 'res_bits', ('strip', 2, 2, 2, 1, 0, 0, 5)),
    (Dg('rt_res_sums_32_w108', 32, 32, 9, 108, forms=DGRAD_FORMS), 'res_sums', ('strip', 2, 2, 2, 1, 1, 0, 0)),
    # bn_bwd on layers no sums kernel takes: run-time tap grid, two output blocks per workgroup, 5x5
    (Dg('rt_sums_d2_16_w130', 16, 16, 9, 130, p=2, d=2, forms=DGRAD_FORMS), 'sums', ('strip', 4, 1, 1, 0, 0, 0, 0)),
    (Dg('rt_sums_16to32_w130', 16, 32, 9, 130, forms=DGRAD_FORMS), 'sums', ('strip', 4, 2, 1, 1, 0, 0, 0)),
    (Dg('rt_sums_k5_16', 16, 16, 21, 31, k=5, p=0, forms=DGRAD_FORMS), 'sums', ('tile', 1, 1, 0, 0, 0, 0, 0)),
    # the narrowest row at 32 channels: the ping-pong <4, 2, 2> (EPI 1 exists for <2, 2, 2> only)
    (Dg('rt_sums_32_w16', 32, 32, 5, 16, forms=DGRAD_FORMS), 'sums', ('strip', 4, 2, 2, 1, 0, 0, 0)),
]
BY_ID.update({r[0].id: r[0] for r in RETREATS})


@pytest.mark.gpu
@pytest.mark.parametrize('case,form,want_rec', RETREATS, ids=[r[0].id for r in RETREATS])
def test_retreat_backward_sums(ops, case, form, want_rec, monkeypatch):
    dx, partials, rec, dx0, rec0, want = _retreat_dgrad(ops, case, form, monkeypatch)
    assert partials is None
    assert (rec.family, rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.EPI, rec.SO) == want_rec, rec
    assert rec0 == rec and torch.equal(dx, dx0)
    _assert_close(dx, want, 'dx')


@pytest.mark.gpu
def test_dgrad_out_argument(ops):
    """conv2d_dgrad(out=) refuses a result tensor of the wrong type, layout or shape; without it nothing changes."""
    dy, w = torch.randn(1, 5, 20, 16).cuda(), torch.randn(16, 16, 3, 3).cuda()
    wpt = ops.pack_weights(w, transpose=True)
    dx = ops.conv2d_dgrad(dy, wpt, 16, 5, 20, 3, 3, 1, 1, 1)
    out = torch.empty_like(dx)
    assert ops.conv2d_dgrad(dy, wpt, 16, 5, 20, 3, 3, 1, 1, 1, out=out) is out and torch.equal(out, dx)
    for bad in (torch.empty(1, 5, 20, 32, device='cuda'), torch.empty(1, 5, 20, 16, device='cuda', dtype=torch.float64),
                torch.empty(1, 5, 16, 20, device='cuda').transpose(2, 3), torch.empty(1, 5, 20, 16)):
        with pytest.raises(ValueError):
            ops.conv2d_dgrad(dy, wpt, 16, 5, 20, 3, 3, 1, 1, 1, out=bad)
    with pytest.raises(ValueError):
        ops.conv2d_dgrad(dy, wpt, 16, 5, 20, 3, 3, 1, 1, 1, out=out, accumulate_into=dx)
    # stride 2: the one-launch kernel (pad 1), with the upstream BatchNorm's sums, and the parity-class launches (pad 0)
    w2 = torch.randn(32, 16, 3, 3).cuda()
    wpt2 = ops.pack_weights(w2, transpose=True)
    u, mean, invstd = torch.randn(2, 9, 21, 16).cuda(), torch.zeros(16).cuda(), torch.ones(16).cuda()
    _, bits = ops.bn_apply(torch.randn(2, 9, 21, 16).cuda(), torch.ones(16).cuda(), torch.zeros(16).cuda(), relu=True, sign_bits=True)
    for pad, kw in ((1, {}), (1, dict(bn_bwd=(u, mean, invstd, None, None, bits))), (0, {})):
        dy2 = torch.randn(2, (9 + 2 * pad - 3) // 2 + 1, (21 + 2 * pad - 3) // 2 + 1, 32).cuda()
        want = ops.conv2d_dgrad(dy2, wpt2, 16, 9, 21, 3, 3, 2, pad, 1, **kw)
        out2 = torch.full((2, 9, 21, 16), float('nan'), device='cuda')
        got = ops.conv2d_dgrad(dy2, wpt2, 16, 9, 21, 3, 3, 2, pad, 1, out=out2, **kw)
        if kw:
            assert got[0] is out2 and torch.equal(out2, want[0]) and (got[1] is None) == (want[1] is None)
        else:
            assert got is out2 and torch.equal(out2, want)
