"""GPU: every instantiation of the convolution weight gradient (dam_wgrad.hip) against torch.nn.grad.conv2d_weight on the CPU in
float64, each case asserting through ops.wgrad_last_launch() the kernel it names and that
the record equals the plan of the same call (ops.conv2d_wgrad_plan; tests/test_wgrad_plan_cpu.py plans the whole table on the CPU).

dam_conv2d_wgrad_f32 picks between four kernel families -- wgrad_rows_kernel (3x3 / stride 1 / pad 1, equal channel counts),
wgrad_rows_s2_kernel (3x3 / stride 2 / pad 1), wgrad_direct_kernel (1x1, and strided 3x3 outside the stride-2 row windows) and the
tile kernel wgrad_kernel -- and a row instantiation is taken only when the row width lands in a window of 4 or 8 widths
(stride 1: roundup(W + 2, 4 HV) == STEPS 4 HV; stride 2: roundup(Wo + 1, 4 HV) == STEPS 4 HV); everything else falls through to
the tile kernel without telling.  So every case of the table NAMES family and instantiation, the helper asserts the record
before it looks at a number, and the closing test asserts that the union of records covers REQUIRED.

Reference and tolerance: conv2d_weight in float64; with an affine the input is x * scale + shift (clamped at 0 with relu_in)
formed in float64.  5e-5 of the max-abs of the float64 gradient (tests/test_conv_gpu.py's weight-gradient bound).
Forms per case: plain; affine with relu_in; affine without; out= into the middle of a buffer with 4096-float guard bands of a
fixed bit pattern on both sides, checked bit for bit (and the result bitwise equal to the plain one); defer=True + wgrad_flush()
bitwise equal to the immediate result; n_out 12 short of the channel count (the channels of dy past n_out hold i.i.d. values: their
rows must not be written).  The stride-2 row kernel and the direct kernel refuse an affine: those forms must be RECORDED as the
tile kernel instantiation AFFINE_TILE names, and are checked against float64 like the others.  NCHW input with an affine is
refused by the entry point: asserted as an error.
Conditions that keep a broken kernel from passing, asserted: |in_shift| >= 0.1 of the activation scale on every channel and
positive on at least half of them (an affine applied to a padding cell gives relu(shift) > 0 there); with relu_in 25-75 % of the
pre-activations negative; x and dy i.i.d. per element; B >= 2 in at least one case per instantiation (strips cross images);
Ho * Wo no multiple of 64 for tile-kernel cases; the window arithmetic of every row case, both edges of every window present
(test_table_conditions and test_input_conditions: no GPU needed).

Worst error seen per family, relative to the scale (MI355X): rows 4.2e-7 (r33_w130_stem8, affine), rows_s2 2.1e-7
(s9_wo32_w63_h2_64to96, n_out), direct 2.7e-7 (d33_wo63, plain), tile 2.3e-7 (t_k5_16to32, n_out).

What the affine conditions buy, tried once: a library whose row kernel wrote relu(shift) instead of zero into the ring rows
above and below the image, and whose tile kernel ran the affine over the out-of-image cells of its patch, failed the first affine
form of all 89 cases with padding (every row and padded tile case; the stride-2 and direct-3x3 cases on the tile kernel their
affine forms take) and passed the 11 without padding (1x1, pad 0); the two NCHW cases ran no affine form then.

Findings on dispatch, settled with the launch record:
  * tests/test_conv_gpu.py::test_wgrad_row_streaming_shapes (1, 16, 3, 213): W = 213 is in neither 16-channel window (127..130,
    215..222): tile kernel <1,1,3,3>.  The short-strip case it was meant to be is r28h2_w215_h3 / r33_w127_h3 here and
    (1, 16, 3, 215) there.  (2, 256, 33, 5): tile <2,2,3,3>, as its docstring says.
  * test_wgrad_strided_row_streaming_shapes: Wo = 9 and 5 (W = 17, 18, 9, 10) run the tile kernel -- the dispatcher keeps rows
    under 15 pixels off the stride-2 row kernel -- <2,2,3,3>, except (2,96,128,65,17), which the 72 KB LDS rule puts on
    <1,1,3,3> with a 160-pixel tile (48 workgroup columns); the other eleven cases take the five row instantiations.
  * test_wgrad_direct_kernel_shapes: only four of its eight shapes ran the direct kernel.  (2,16,32,41,65) and (1,32,64,33,34)
    3x3 / stride 2 have Wo = 33 and 17: stride-2 ROW kernel <2,9,2,5,3,1> / <2,5,2,3,2,1>; (2,96,96,9,17) stride 1: row kernel
    <2,1,5,3,2,1,4>; (1,48,48,20,30) stride 1 with three channel blocks: tile <2,2,3,3>.  (1,64,96,21,33) 1x1 has 4 and 6 channel
    blocks, none odd: direct <2,2,1,1>.  The direct 3x3 kernel is reached at Wo = 108 and 20 (outside every window).
  * test_fused_bn_relu_prologue (2,32,33,29): W = 29 is in no window -- the only relu_in weight gradient at kernel level ran the
    tile kernel.
  * A stride-2 or 1x1 layer WITH an affine lands on the tile kernel: <2,2,...>, or <1,1,...> with one channel block on a side
    and, for stride-2 shapes with more than a few wide rows, through the 72 KB LDS rule (128-pixel tiles where 256 do not fit).
    AFFINE_TILE pins the instantiation and the tile size of every such case.
  * in_nchw with in_scale: the tile kernel's NCHW loader applies no affine (dam_conv_stage.h), and the entry point used to
    return DAM_OK with the gradient of the RAW input.  No layer asks for the combination (the stem reads raw features), so
    dam_conv2d_wgrad_f32 now refuses it with DAM_ERR_UNSUPPORTED; the affine forms of the two NCHW cases assert the error,
    a record of "none" and an untouched result buffer.

Unreachable from ops.conv2d_wgrad (named here instead of being dropped):
  * issue mode 1 (launched, reduction queued) of the direct and the tile kernel: ops switches batching on for every queue
    (ops.WGRAD_BATCH is a constant), so a deferred call of these two families is recorded (mode 2), never launched at once.
  * nothing else: every instantiation dam_conv2d_wgrad_f32 names is in REQUIRED, the batched form of every direct instantiation
    (wgrad_direct_batch_kernel, reached by defer=True) included."""
import collections

import pytest
import torch

GUARD = 4096
FILL = 0x5EADBEEF                   # guard-band pattern (as float32: 7.8e18, so an unwritten gradient element fails too)
TOL = 5e-5
WD_MAX_JOBS = 8                     # dam_wgrad.hip: jobs of one batched launch of the direct kernel

FORMS = ('plain', 'relu', 'affine', 'out', 'defer', 'nout')

Case = collections.namedtuple('Case', 'id B Ci Co H W k s p d nchw c_real expect')


def _rows(TNB, TKB, STEPS, KP, GPP, HV=1, NL=8):
    return dict(family='rows', TNB=TNB, TKB=TKB, STEPS=STEPS, KP=KP, GPP=GPP, GPPD=0, HV=HV, NL=NL, TA=0, TB=0)


def _rows_s2(STEPS, KP, GPPX, GPPD, HV):
    return dict(family='rows_s2', TNB=2, TKB=1, STEPS=STEPS, KP=KP, GPP=GPPX, GPPD=GPPD, HV=HV, NL=8, TA=0, TB=0)


def _direct(TNB, TKB, K):
    return dict(family='direct', TNB=TNB, TKB=TKB, STEPS=0, KP=0, GPP=0, GPPD=0, HV=0, NL=0, TA=K, TB=K)


def _tile(TNB, TKB, TA, TB, **more):
    return dict(family='tile', TNB=TNB, TKB=TKB, STEPS=0, KP=0, GPP=0, GPPD=0, HV=0, NL=0, TA=TA, TB=TB, **more)


def C(id, B, Ci, Co, H, W, expect, k=3, s=1, p=1, d=1, nchw=False, c_real=None):
    return Case(id, B, Ci, Co, H, W, k, s, p, d, nchw, c_real, expect)


# ---------------------------------------------------------------------------------------------------------------- the table
# stride-1 row kernel: instantiation -> (channel rule, first and last width of its window)
ROWS = collections.OrderedDict([
    ('r33', (_rows(1, 1, 33, 1, 9), 16, 127, 130)),
    ('r28h2', (_rows(1, 1, 28, 1, 14, 2), 16, 215, 222)),
    ('r3', (_rows(2, 1, 3, 2, 1), 32, 7, 10)),
    ('r5', (_rows(2, 1, 5, 3, 2, 1, 4), 32, 15, 18)),
    ('r9', (_rows(2, 1, 9, 2, 3), 32, 31, 34)),
    ('r14', (_rows(2, 1, 14, 2, 4), 32, 51, 54)),
    ('r17', (_rows(2, 1, 17, 2, 5), 32, 63, 66)),
    ('r14h2', (_rows(2, 1, 14, 1, 7, 2), 32, 103, 110)),
])
# per instantiation: (B, C, H, W) at the bottom edge, an interior width, the top edge (+ extras); H in {1, 3, 5, ragged}
ROWS_SHAPES = {
    'r33': [(2, 16, 3, 127), (2, 16, 5, 128), (1, 16, 22, 130), (3, 16, 1, 129)],
    'r28h2': [(2, 16, 3, 215), (2, 16, 1, 218), (1, 16, 11, 222), (2, 16, 5, 216)],
    'r3': [(2, 32, 1, 7), (2, 256, 5, 9), (1, 64, 22, 10), (3, 32, 3, 8)],             # 256 channels: 16 x 8 tiles
    'r5': [(1, 32, 11, 15), (2, 96, 3, 17), (2, 64, 5, 18), (2, 32, 1, 16)],           # 96 channels: three tiles per side
    'r9': [(2, 64, 1, 31), (2, 32, 3, 33), (1, 32, 22, 34), (2, 64, 5, 32)],
    'r14': [(2, 32, 5, 51), (2, 32, 3, 52), (1, 64, 11, 54), (2, 32, 1, 53)],
    'r17': [(2, 32, 3, 63), (2, 64, 5, 65), (1, 32, 22, 66), (2, 32, 1, 64)],
    'r14h2': [(2, 32, 1, 103), (2, 32, 5, 108), (1, 32, 11, 110), (2, 64, 3, 104)],
}
CASES = []
for name, shapes in ROWS_SHAPES.items():
    for B, ch, H, W in shapes:
        CASES.append(C('%s_w%d_h%d' % (name, W, H), B, ch, ch, H, W, ROWS[name][0]))
# the stem through the NHWC-16 relayout (8 real input channels: the gradient keeps 8 columns) at a row-kernel width
CASES.append(C('r33_w130_stem8', 2, 16, 16, 5, 130, ROWS['r33'][0], c_real=8))

# stride-2 row kernel: instantiation -> first and last OUTPUT width of its window
ROWS_S2 = collections.OrderedDict([
    ('s5', (_rows_s2(5, 2, 3, 2, 1), 16, 18)),
    ('s7', (_rows_s2(7, 2, 4, 2, 1), 24, 27)),
    ('s9', (_rows_s2(9, 2, 5, 3, 1), 32, 34)),
    ('s7h2', (_rows_s2(7, 1, 7, 4, 2), 48, 55)),
    ('s9h2', (_rows_s2(9, 1, 9, 5, 2), 64, 71)),
])
S2_PAIRS = [(16, 32), (32, 64), (64, 96)]
# both edges x both parities of W; per instantiation the heights cover odd, even and Ho = 1 (H = 1 or 2), B = 2 on two of the four
S2_BH = [[(2, 7), (1, 2), (1, 12), (2, 1)], [(1, 1), (2, 10), (2, 23), (1, 4)], [(2, 2), (1, 9), (1, 1), (2, 6)],
         [(1, 5), (2, 1), (2, 2), (1, 8)], [(2, 4), (1, 11), (1, 2), (2, 3)]]
for i, (name, (exp, lo, hi)) in enumerate(ROWS_S2.items()):
    for j, (wo, W) in enumerate(((lo, 2 * lo - 1), (lo, 2 * lo), (hi, 2 * hi - 1), (hi, 2 * hi))):
        B, H = S2_BH[i][j]
        ci, co = S2_PAIRS[(i + j) % 3]
        CASES.append(C('%s_wo%d_w%d_h%d_%dto%d' % (name, wo, W, H, ci, co), B, ci, co, H, W, exp, s=2))

CASES += [
    # direct kernel, 1x1 / stride 2: <2,2> needs even block counts on both sides, <2,1> an even output count, <1,1> the rest
    C('d11_32to64', 2, 32, 64, 9, 21, _direct(2, 2, 1), k=1, s=2, p=0),
    C('d11_64to96', 2, 64, 96, 12, 33, _direct(2, 2, 1), k=1, s=2, p=0),
    C('d11_48to32', 2, 48, 32, 9, 21, _direct(2, 1, 1), k=1, s=2, p=0),
    C('d11_16to32', 3, 16, 32, 7, 130, _direct(2, 1, 1), k=1, s=2, p=0),
    C('d11_32to48', 2, 32, 48, 9, 21, _direct(1, 1, 1), k=1, s=2, p=0),
    C('d11_48to48_s1', 1, 48, 48, 5, 13, _direct(1, 1, 1), k=1, s=1, p=0),
    # direct kernel, 3x3 / stride 2 just outside the row windows
    C('d33_wo19', 2, 16, 32, 7, 37, _direct(2, 1, 3), s=2),
    C('d33_wo23', 1, 32, 64, 10, 46, _direct(2, 1, 3), s=2),
    C('d33_wo28', 2, 64, 96, 5, 55, _direct(2, 1, 3), s=2),
    C('d33_wo35', 2, 16, 32, 2, 70, _direct(2, 1, 3), s=2),
    C('d33_wo47', 1, 32, 64, 9, 93, _direct(2, 1, 3), s=2),
    C('d33_wo56', 2, 16, 32, 4, 112, _direct(2, 1, 3), s=2),
    C('d33_wo63', 2, 32, 64, 1, 125, _direct(2, 1, 3), s=2),
    C('d33_wo72', 1, 16, 32, 11, 144, _direct(2, 1, 3), s=2),
    # ... with an odd output block count (inside a row window too: the row kernel's two-block tile refuses it)
    C('d33_wo19_32to48', 2, 32, 48, 7, 38, _direct(1, 1, 3), s=2),
    C('d33_wo17_32to48', 2, 32, 48, 6, 33, _direct(1, 1, 3), s=2),
    C('d33_wo20_16to16', 2, 16, 16, 9, 40, _direct(1, 1, 3), s=2),
    # tile kernel, 3x3 / stride 1 at widths between the windows
    C('t16_w11', 2, 16, 16, 7, 11, _tile(1, 1, 3, 3)),
    C('t16_w20', 2, 16, 16, 5, 20, _tile(1, 1, 3, 3)),
    C('t16_w40', 2, 16, 16, 9, 40, _tile(1, 1, 3, 3)),
    C('t16_w90', 2, 16, 16, 3, 90, _tile(1, 1, 3, 3)),
    C('t16_w131', 2, 16, 16, 5, 131, _tile(1, 1, 3, 3)),
    C('t16_w214', 1, 16, 16, 3, 214, _tile(1, 1, 3, 3)),
    C('t16_w45_stem8', 2, 16, 16, 7, 45, _tile(1, 1, 3, 3), c_real=8),
    C('t256_w5', 2, 256, 256, 7, 5, _tile(2, 2, 3, 3)),
    C('t64_w12', 2, 64, 64, 9, 12, _tile(2, 2, 3, 3)),
    C('t32_w29', 2, 32, 32, 11, 29, _tile(2, 2, 3, 3)),
    C('t32_w67', 2, 32, 32, 5, 67, _tile(2, 2, 3, 3)),
    C('t48_w30', 2, 48, 48, 7, 30, _tile(2, 2, 3, 3)),                       # three channel blocks: the second tile half empty
    # 3x3 / stride 2 with Wo < 16
    C('t_s2_wo9', 2, 96, 128, 11, 17, _tile(2, 2, 3, 3), s=2),
    C('t_s2_wo14', 2, 16, 32, 9, 28, _tile(1, 1, 3, 3), s=2),
    C('t_s2_wo5', 3, 128, 256, 4, 10, _tile(2, 2, 3, 3), s=2),
    # unequal channel counts at stride 1; one channel block on either side
    C('t32to64_w33', 2, 32, 64, 7, 33, _tile(2, 2, 3, 3)),
    C('t64to32_w17', 2, 64, 32, 5, 17, _tile(2, 2, 3, 3)),
    C('t16to32_w130', 2, 16, 32, 3, 130, _tile(1, 1, 3, 3)),
    C('t32to16_w65', 2, 32, 16, 5, 65, _tile(1, 1, 3, 3)),
    # the NCHW stem of the scalar models (4 planes, stride 2, dilation 2), dilation 2 on NHWC
    C('t_nchw4_d2', 2, 4, 16, 21, 45, _tile(1, 1, 3, 3), s=2, p=0, d=2, nchw=True),
    C('t_nchw8', 2, 8, 16, 7, 45, _tile(1, 1, 3, 3), nchw=True),
    C('t32_d2', 2, 32, 32, 9, 21, _tile(2, 2, 3, 3), p=2, d=2),
    # 5x5 (three output blocks: <3,2,1,5>), 7x7, 9x9
    C('t_k5_32to48', 2, 32, 48, 13, 19, _tile(3, 2, 1, 5), k=5, p=0),
    C('t_k5_32to64', 2, 32, 64, 13, 19, _tile(2, 2, 1, 5), k=5, p=0),
    C('t_k5_48to48', 2, 48, 48, 11, 17, _tile(2, 2, 1, 5), k=5, p=2),        # three INPUT blocks as well: no three-block tile
    C('t_k5_16to32', 2, 16, 32, 13, 19, _tile(1, 1, 1, 5), k=5, p=0),
    C('t_k7_48to64', 2, 48, 64, 13, 17, _tile(2, 2, 1, 7), k=7, p=0),
    C('t_k7_16to16', 2, 16, 16, 9, 15, _tile(1, 1, 1, 7), k=7, p=3),
    C('t_k9_64to128', 2, 64, 128, 13, 15, _tile(2, 2, 1, 9), k=9, p=0),
    C('t_k9_32to16', 2, 32, 16, 11, 13, _tile(1, 1, 1, 9), k=9, p=4),
    # the 72 KB LDS rule: a patch that forces the 128-pixel tile, one that forces the one-block tile
    C('t_lds_tmw128', 2, 32, 64, 5, 70, _tile(2, 2, 3, 3, TMW=128)),
    C('t_lds_small', 2, 32, 64, 5, 90, _tile(1, 1, 3, 3)),
]
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}

# The tile-kernel instantiation an affine sends the cases of the refusing families to.  1x1: two blocks a side unless a side has one.
AFFINE_TILE = {'d11_32to64': _tile(2, 2, 1, 1), 'd11_64to96': _tile(2, 2, 1, 1), 'd11_48to32': _tile(2, 2, 1, 1),
               'd11_16to32': _tile(1, 1, 1, 1), 'd11_32to48': _tile(2, 2, 1, 1), 'd11_48to48_s1': _tile(2, 2, 1, 1)}
# 3x3 / stride 2: id -> (channel blocks a side, pixels per tile).  One block with 16 input channels, and wherever the patch
# of a two-block tile (both column parities of 2 * rows + 1 input rows) is past the tile kernel's 72 KB rule at 256 and at 128
# pixels per tile -- most shapes with more than a few wide rows; the one-block tile then takes 128 pixels where 256 do not fit.
AFFINE_TILE_S2 = {
    's5_wo16_w31_h7_16to32': (1, 64), 's5_wo16_w32_h2_32to64': (2, 16), 's5_wo18_w35_h12_64to96': (1, 112),
    's5_wo18_w36_h1_16to32': (1, 32), 's7_wo24_w47_h1_32to64': (2, 32), 's7_wo24_w48_h10_64to96': (1, 128),
    's7_wo27_w53_h23_16to32': (1, 176), 's7_wo27_w54_h4_32to64': (2, 64), 's9_wo32_w63_h2_64to96': (2, 32),
    's9_wo32_w64_h9_16to32': (1, 160), 's9_wo34_w67_h1_32to64': (2, 48), 's9_wo34_w68_h6_64to96': (1, 112),
    's7h2_wo48_w95_h5_16to32': (1, 144), 's7h2_wo48_w96_h1_32to64': (2, 48), 's7h2_wo55_w109_h2_64to96': (2, 64),
    's7h2_wo55_w110_h8_16to32': (1, 112), 's9h2_wo64_w127_h4_32to64': (1, 128), 's9h2_wo64_w128_h11_64to96': (1, 128),
    's9h2_wo71_w141_h2_16to32': (1, 80), 's9h2_wo71_w142_h3_32to64': (1, 144),
    'd33_wo19': (1, 80), 'd33_wo23': (1, 128), 'd33_wo28': (2, 96), 'd33_wo35': (1, 48), 'd33_wo47': (1, 128), 'd33_wo56': (1, 112),
    'd33_wo63': (2, 64), 'd33_wo72': (1, 112), 'd33_wo19_32to48': (2, 80), 'd33_wo17_32to48': (2, 64), 'd33_wo20_16to16': (1, 112)}
for _id, (_nb, _tmw) in AFFINE_TILE_S2.items():
    AFFINE_TILE[_id] = _tile(_nb, _nb, 3, 3, TMW=_tmw)
assert set(AFFINE_TILE) == {c.id for c in CASES if c.expect['family'] in ('rows_s2', 'direct')}


def _variant(rec):
    """The part of a launch record that names a kernel."""
    if rec.family == 'rows':
        return ('rows', rec.TNB, rec.TKB, rec.STEPS, rec.KP, rec.GPP, rec.HV, rec.NL)
    if rec.family == 'rows_s2':
        return ('rows_s2', rec.TNB, rec.STEPS, rec.KP, rec.GPP, rec.GPPD, rec.HV)
    if rec.family == 'direct':
        return ('direct', rec.TNB, rec.TKB, rec.TA, rec.TB, 'batched' if rec.issued == 2 else 'alone')
    return (rec.family, rec.TNB, rec.TKB, rec.TA, rec.TB)


REQUIRED = (
    # wgrad_rows_kernel <TNB, TKB, STEPS, KP, GPP, HV, NL>
    [('rows', 1, 1, 33, 1, 9, 1, 8), ('rows', 1, 1, 28, 1, 14, 2, 8), ('rows', 2, 1, 3, 2, 1, 1, 8), ('rows', 2, 1, 5, 3, 2, 1, 4),
     ('rows', 2, 1, 9, 2, 3, 1, 8), ('rows', 2, 1, 14, 2, 4, 1, 8), ('rows', 2, 1, 17, 2, 5, 1, 8), ('rows', 2, 1, 14, 1, 7, 2, 8)] +
    # wgrad_rows_s2_kernel <TNB, STEPS, KP, GPPX, GPPD, HV>
    [('rows_s2', 2, 5, 2, 3, 2, 1), ('rows_s2', 2, 7, 2, 4, 2, 1), ('rows_s2', 2, 9, 2, 5, 3, 1), ('rows_s2', 2, 7, 1, 7, 4, 2),
     ('rows_s2', 2, 9, 1, 9, 5, 2)] +
    # wgrad_direct_kernel and wgrad_direct_batch_kernel <TNB, TKB, KH, KW>
    [('direct', tn, tk, k, k, how) for tn, tk, k in ((2, 2, 1), (2, 1, 1), (1, 1, 1), (2, 1, 3), (1, 1, 3)) for how in ('alone', 'batched')] +
    # wgrad_kernel <TNB, TKB, TA, TB>
    [('tile', 1, 1, 3, 3), ('tile', 2, 2, 3, 3), ('tile', 1, 1, 1, 1), ('tile', 2, 2, 1, 1), ('tile', 1, 1, 1, 5), ('tile', 3, 2, 1, 5),
     ('tile', 2, 2, 1, 5), ('tile', 1, 1, 1, 7), ('tile', 2, 2, 1, 7), ('tile', 1, 1, 1, 9), ('tile', 2, 2, 1, 9)])


def _roundup(v, m):
    return (v + m - 1) // m * m


def _out_hw(c):
    return ((c.H + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1, (c.W + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1)


def _in_s2_window(wo):
    return any(lo <= wo <= hi for _, lo, hi in ROWS_S2.values())


def test_table_conditions():
    """The arithmetic behind the table, on the CPU: every row case sits in the window of the instantiation it names and both
    edges of every window are present; every direct 3x3 case is outside the stride-2 windows; tile cases have ragged last
    tiles; every named instantiation has a case with B >= 2; the heights cover 1, 3, 5 and a ragged one."""
    for name, (exp, cmin, lo, hi) in ROWS.items():
        q = 4 * exp['HV']
        # (at 16 channels the dispatcher offers every width to both instantiations; from 32 on W 7..12 / 13..20 / 21..48 / 49..80 /
        #  81.. to r3 / r5 / r9 / r17 then r14 / r14h2)
        route = {'r3': (7, 12), 'r5': (13, 20), 'r9': (21, 48), 'r14': (49, 80), 'r17': (49, 80), 'r14h2': (81, 399)}.get(name, (1, 399))
        assert [w for w in range(route[0], route[1] + 1) if _roundup(w + 2, q) == exp['STEPS'] * q] == list(range(lo, hi + 1)), name
        mine = [c for c in CASES if c.expect is exp]
        assert {lo, hi} <= {c.W for c in mine} and any(lo < c.W < hi for c in mine), name
        for c in mine:
            assert c.k == 3 and c.s == 1 and c.p == 1 and c.d == 1 and c.Ci == c.Co and not c.nchw, c.id
            assert (c.Ci == 16) if cmin == 16 else (c.Ci >= 32 and c.Ci // 16 % 2 == 0), c.id
            assert c.B <= 3 and c.H <= 23, c.id
    assert {1, 3, 5, 11, 22} <= {c.H for c in CASES if c.expect['family'] == 'rows'}
    assert any(c.Ci == 96 for c in CASES if c.expect is ROWS['r5'][0]) and any(c.Ci == 256 for c in CASES if c.expect is ROWS['r3'][0])
    for name, (exp, lo, hi) in ROWS_S2.items():
        q = 4 * exp['HV']
        # (the dispatcher offers Wo 15..18 / 19..28 / 29..34 / 35..56 / 57.. to the five instantiations; each takes its window)
        route = {'s5': (15, 18), 's7': (19, 28), 's9': (29, 34), 's7h2': (35, 56), 's9h2': (57, 399)}[name]
        assert [w for w in range(route[0], route[1] + 1) if _roundup(w + 1, q) == exp['STEPS'] * q] == list(range(lo, hi + 1)), name
        mine = [c for c in CASES if c.expect is exp]
        assert {(lo, 2 * lo - 1), (lo, 2 * lo), (hi, 2 * hi - 1), (hi, 2 * hi)} == {(_out_hw(c)[1], c.W) for c in mine}, name
        assert any(c.H % 2 for c in mine) and any(c.H % 2 == 0 for c in mine) and any(_out_hw(c)[0] == 1 for c in mine), name
        for c in mine:
            assert c.k == 3 and c.s == 2 and c.p == 1 and c.d == 1 and (c.Co // 16) % 2 == 0 and c.B <= 3 and c.H <= 23, c.id
    assert {(c.Ci, c.Co) for c in CASES if c.expect['family'] == 'rows_s2'} == set(S2_PAIRS)
    for c in CASES:
        Ho, Wo = _out_hw(c)
        assert c.B <= 3 and c.H <= 23, c.id
        if c.expect['family'] == 'direct' and c.k == 3:
            assert c.s == 2 and Wo >= 16 and (not _in_s2_window(Wo) or (c.Co // 16) % 2), c.id
        if c.expect['family'] == 'tile':
            assert (Ho * Wo) % 64 != 0, c.id
            if c.k == 3 and c.s == 1 and c.p == 1 and c.d == 1 and c.Ci == c.Co and not c.nchw and (c.Ci == 16 or c.Ci // 16 % 2 == 0):
                assert not any(lo <= c.W <= hi for _, cmin, lo, hi in ROWS.values() if (cmin == 16) == (c.Ci == 16)), c.id
            if c.k == 3 and c.s == 2 and c.p == 1 and c.d == 1 and not c.nchw:
                assert Wo < 16, c.id
    assert {19, 23, 28, 35, 47, 56, 63, 72} <= {_out_hw(c)[1] for c in CASES if c.expect['family'] == 'direct' and c.k == 3}
    named = {}
    for c in CASES:
        named.setdefault(tuple(sorted((k, v) for k, v in c.expect.items() if k != 'TMW')), []).append(c)
    for key, cs in named.items():
        assert any(c.B >= 2 for c in cs), key


# --------------------------------------------------------------------------------------------------------- inputs, oracle
@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _inputs(c):
    """x [B, Ci, H, W], dy [B, Co, Ho, Wo], scale and shift [C]: all i.i.d.; |shift| in 0.2 .. 1.0 against activations of
    standard deviation 0.5 .. 1.5, positive on half the channels (rounded up)."""
    g = torch.Generator().manual_seed(3000 + [k.id for k in CASES].index(c.id))
    Ho, Wo = _out_hw(c)
    x = torch.randn(c.B, c.Ci, c.H, c.W, generator=g)
    if c.c_real:
        x[:, c.c_real:] = 0                     # the zero planes of the re-laid stem input
    dy = torch.randn(c.B, c.Co, Ho, Wo, generator=g)
    sc = torch.rand(c.Ci, generator=g) + 0.5
    sign = torch.ones(c.Ci)
    sign[(c.Ci + 1) // 2:] = -1
    sh = (0.2 + 0.8 * torch.rand(c.Ci, generator=g)) * sign[torch.randperm(c.Ci, generator=g)]
    return x, dy, sc, sh


def _pre_activation(c, x, sc, sh):
    """x * scale + shift in float64; asserts the conditions that make a wrongly applied affine visible."""
    kr = c.c_real or c.Ci
    x64 = x.double()
    pre = x64 * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    act_scale = (x64[:, :kr] * sc.double()[:kr].view(1, -1, 1, 1)).std().item()
    assert sh.abs().min().item() >= 0.1 * act_scale and (sh > 0).sum().item() * 2 >= c.Ci, c.id
    neg = (pre[:, :kr] < 0).double().mean().item()
    assert 0.25 <= neg <= 0.75, (c.id, neg)
    return pre


def test_input_conditions():
    """The conditions on the generated affine (shift size and sign share, share of negative pre-activations) for every case of
    the table, on the CPU: a case that stops meeting them fails here as well as in its GPU test."""
    for c in CASES:
        x, _, sc, sh = _inputs(c)
        _pre_activation(c, x, sc, sh)


def _oracle(c, x, dy, sc, sh):
    """form -> float64 gradient [Co, c_real or Ci, k, k] (plain, relu, affine); asserts the conditions on the affine."""
    kr = c.c_real or c.Ci
    x64, dy64 = x.double(), dy.double()
    pre = _pre_activation(c, x, sc, sh)
    want = {}
    for form, a in (('plain', x64), ('relu', pre.clamp(min=0)), ('affine', pre)):
        want[form] = torch.nn.grad.conv2d_weight(a, (c.Co, c.Ci, c.k, c.k), dy64, c.s, c.p, c.d)[:, :kr].contiguous()
    return want


def _device_inputs(c, x, dy, sc, sh):
    xd = (x if c.nchw else x.permute(0, 2, 3, 1).contiguous()).cuda()
    return xd, dy.permute(0, 2, 3, 1).contiguous().cuda(), sc.cuda(), sh.cuda()


def _forms(c):
    return list(FORMS)


def _refused(c, form):
    """The NCHW loader applies no affine: the entry point refuses the combination (DAM_ERR_UNSUPPORTED)."""
    return c.nchw and form in ('relu', 'affine')


def _expected(c, form):
    if _refused(c, form):
        return dict(family='none', TNB=0, TKB=0, TA=0, TB=0, nx=0, nsplit=0, issued=0)
    e = dict(c.expect)
    if form in ('relu', 'affine') and e['family'] in ('rows_s2', 'direct'):
        e = dict(AFFINE_TILE[c.id])             # the family refuses an affine: tile kernel
    if form == 'defer':
        e['issued'] = 1 if e['family'] in ('rows', 'rows_s2') else 2
    else:
        e['issued'] = 0
    return e


def planned(ops, x, dy, n_out, k, s, p, d, defer=False, **kw):
    """ops.conv2d_wgrad_plan of the conv2d_wgrad call just made on x and dy (before any flush), in the workspace that call was
    given: ops' slab buffers only grow, so a call can be handed more floats than it asks for, and a pixel split may use them."""
    dev = x.device
    key = (dev.type, dev.index) + (('wgrad slabs', ops._wgrad_queue(dev)[1] - 1) if defer else ())
    return ops.conv2d_wgrad_plan(tuple(x.shape), tuple(dy.shape), n_out, k, k, s, p, d, defer=defer,
                                 workspace_floats=ops._workspaces[key].numel(), **kw)


SEEN = {}           # (case id, form) -> WgradLaunch
WORST = {}          # family -> (relative error, case id, form)


def _launch(ops, c, form, xd, dyd, scd, shd):
    """One conv2d_wgrad of the form -> (guarded buffer as int32 or None, result); asserts the dispatch."""
    n_out = c.Co - 12 if form == 'nout' else c.Co
    kr = c.c_real or c.Ci
    kw = dict(in_nchw=c.nchw)
    if c.c_real:
        kw['c_real'] = c.c_real
    if form in ('relu', 'affine'):
        kw.update(in_scale=scd, in_shift=shd, relu_in=form == 'relu')
    buf = None
    if form != 'plain':
        numel = n_out * kr * c.k * c.k
        buf = torch.full((2 * GUARD + numel,), FILL, dtype=torch.int32, device='cuda')
        kw['out'] = buf.view(torch.float32)[GUARD:GUARD + numel].view(n_out, kr, c.k, c.k)
    if _refused(c, form):
        with pytest.raises(RuntimeError, match='DAM_ERR_UNSUPPORTED'):
            ops.conv2d_wgrad(xd, dyd, n_out, c.k, c.k, c.s, c.p, c.d, **kw)
        rec = SEEN[(c.id, form)] = ops.wgrad_last_launch()
        with pytest.raises(RuntimeError, match='DAM_ERR_UNSUPPORTED'):      # the plan of the same call: the same refusal
            ops.conv2d_wgrad_plan(tuple(xd.shape), tuple(dyd.shape), n_out, c.k, c.k, c.s, c.p, c.d, affine=True, relu_in=form == 'relu',
                                  in_nchw=True)
        want = _expected(c, form)
        assert {k: getattr(rec, k) for k in want} == want, '%s %s: recorded %s' % (c.id, form, rec)
        torch.cuda.synchronize()
        assert bool((buf == FILL).all()), '%s %s: a refused call wrote its result' % (c.id, form)
        return None, None
    got = ops.conv2d_wgrad(xd, dyd, n_out, c.k, c.k, c.s, c.p, c.d, defer=form == 'defer', **kw)
    rec = ops.wgrad_last_launch()
    plan = planned(ops, xd, dyd, n_out, c.k, c.s, c.p, c.d, defer=form == 'defer', affine=form in ('relu', 'affine'),
                   relu_in=form == 'relu', in_nchw=c.nchw, c_real=c.c_real)
    assert rec == plan, '%s %s: launched %s, planned %s' % (c.id, form, rec, plan)      # (defer: the recorded form)
    if form == 'defer':
        torch.cuda.synchronize()
        assert bool((buf == FILL).all()), '%s: written before the flush' % c.id
        ops.wgrad_flush()
        assert ops.wgrad_last_launch() == rec, 'the flush changed the record of the last call'
    SEEN[(c.id, form)] = rec
    want = _expected(c, form)
    assert {k: getattr(rec, k) for k in want} == want, '%s %s: launched %s' % (c.id, form, rec)
    assert rec.nx >= 1 and (rec.nsplit >= 1 or (rec.family == 'tile' and rec.issued == 2)), rec
    if rec.family in ('rows', 'rows_s2'):
        rows = c.H if rec.family == 'rows' else _out_hw(c)[0]
        assert rec.nsplit == c.B * rec.spi and rec.spi >= 1 and rec.spi * rec.rps >= rows and rec.TMW == 0, rec
    else:
        assert rec.spi == 0 and rec.rps == 0 and (rec.TMW > 0) == (rec.family == 'tile'), rec
    assert tuple(got.shape) == (n_out, kr, c.k, c.k)
    return buf, got


def _check_case(ops, c):
    x, dy, sc, sh = _inputs(c)
    want = _oracle(c, x, dy, sc, sh)
    dev = _device_inputs(c, x, dy, sc, sh)
    plain = None
    for form in _forms(c):
        buf, got = _launch(ops, c, form, *dev)
        if got is None:
            continue                            # refused, as asserted
        torch.cuda.synchronize()
        if buf is not None:
            host = buf.cpu()
            assert bool((host[:GUARD] == FILL).all()) and bool((host[-GUARD:] == FILL).all()), '%s %s: guard band written' % (c.id, form)
        got = got.cpu()
        if form == 'plain':
            plain = got
        elif form in ('out', 'defer'):
            assert torch.equal(got, plain), '%s %s: not bitwise the plain result' % (c.id, form)
        w = want.get(form, want['plain'])[:got.shape[0]]
        scale = w.abs().max().item()
        err = (got.double() - w).abs()
        worst = err.max().item()
        where = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        fam = SEEN[(c.id, form)].family
        if worst / scale > WORST.get(fam, (-1.0,))[0]:
            WORST[fam] = (worst / scale, c.id, form)
        print('%s %s: %s  err %.2e of scale %.3g at [n, k, kh, kw] = %s' % (c.id, form, SEEN[(c.id, form)], worst / scale, scale, where))
        assert worst <= TOL * scale, '%s %s: err %.3g > %.3g at [n, k, kh, kw] = %s (%d elements over)' % (
            c.id, form, worst, TOL * scale, where, int((err > TOL * scale).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_wgrad_kernel(ops, case):
    _check_case(ops, case)


@pytest.mark.gpu
def test_direct_batched_jobs(ops):
    """The batched launch of the direct kernel (wgrad_direct_batch_kernel): deferred 1x1 / stride-2 shortcut gradients of one
    instantiation and DIFFERENT geometries wait for each other and share one flat grid, each with its share of the pixel splits.
    Two <2,2,1,1> jobs, a <2,1,1,1> job in between (it launches what is pending), then WD_MAX_JOBS + 1 jobs of <2,2,1,1>: the
    ninth launches the full batch of eight and is left for the flush.  Every gradient against float64."""
    assert ops.WGRAD_BATCH
    g = torch.Generator().manual_seed(4100)
    A, Bj = _direct(2, 2, 1), _direct(2, 1, 1)
    plan = [(A, 2, 32, 64, 9, 21), (A, 1, 64, 64, 4, 35), (Bj, 2, 16, 32, 7, 66)]
    plan += [(A, 1 + i % 3, (32, 64, 96)[i % 3], (64, 32, 128)[(i // 3) % 3], 3 + 2 * i, 9 + 7 * i) for i in range(WD_MAX_JOBS + 1)]
    jobs = []
    for exp, B, ci, co, H, W in plan:
        x, dy = torch.randn(B, ci, H, W, generator=g), torch.randn(B, co, (H + 1) // 2, (W + 1) // 2, generator=g)
        want = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 1, 1), dy.double(), 2, 0, 1)
        out = torch.full((co, ci, 1, 1), float('nan'), device='cuda')
        jobs.append((x.permute(0, 2, 3, 1).contiguous().cuda(), dy.permute(0, 2, 3, 1).contiguous().cuda(), out, want))
        ops.conv2d_wgrad(jobs[-1][0], jobs[-1][1], co, 1, 1, 2, 0, 1, out=out, defer=True)
        rec = ops.wgrad_last_launch()
        assert {k: getattr(rec, k) for k in exp} == exp and rec.issued == 2, rec
        assert rec == planned(ops, jobs[-1][0], jobs[-1][1], co, 1, 2, 0, 1, defer=True), rec
    ops.wgrad_flush()
    torch.cuda.synchronize()
    for i, (_, _, out, want) in enumerate(jobs):
        err, scale = (out.cpu().double() - want).abs().max().item(), want.abs().max().item()
        print('direct job %d %s: err %.2e of scale %.3g' % (i, plan[i][1:], err / scale, scale))
        assert err <= TOL * scale, (i, plan[i], err, scale)


@pytest.mark.gpu
def test_coverage(ops):
    """The union of the launches the table made covers REQUIRED.  (Cases that did not run in this process -- a -k selection --
    are launched here without their oracle, so the test stands on its own.)"""
    for c in CASES:
        missing = [f for f in _forms(c) if (c.id, f) not in SEEN]
        if missing:
            dev = _device_inputs(c, *_inputs(c))
            for f in missing:
                _launch(ops, c, f, *dev)
    torch.cuda.synchronize()
    seen = {_variant(r) for r in SEEN.values()}
    for fam in sorted(WORST):
        print('worst error, %s: %.2e of the scale (%s, %s)' % ((fam,) + WORST[fam]))
    print('variants seen: %s' % sorted(seen))
    lacking = [v for v in REQUIRED if v not in seen]
    assert not lacking, 'kernel variants no case reached: %s' % lacking
    # the refusal order: no stride-2 row or direct launch ever carried an affine
    for (cid, form), r in SEEN.items():
        if form in ('relu', 'affine'):
            assert r.family == 'none' if BY_ID[cid].nchw else r.family in ('rows', 'tile'), (cid, form, r)
