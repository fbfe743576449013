"""GPU: the fused INFERENCE epilogue (bias, residual add, ReLU) of every forward convolution kernel against float64, at the
tensor level, and the folded conv -> BatchNorm(eval) modules built on it against the float64 modules.

Every eval-mode product reaches the network through layers.FoldedConvBn.fwd -> ops.conv2d_fwd(bias=, res=, relu_out=), and the
write-out is spelled separately in each kernel family.  dam_conv2d_tapgrid_f32 falls back from family to family silently, so
every case NAMES the kernel it means to exercise and asserts it through ops.conv_last_launch(); the closing test asserts that
the union of launches seen covers REQUIRED below.

Kernel level (test_epilogue): for every case the four epilogues of a residual block -- bias + ReLU (conv1, stem), bias only
(shortcut), bias + res + ReLU (conv2), res only -- against F.conv2d on the CPU in float64 + float64 bias + float64 res, ReLU
last.  Tolerance: 2e-5 of the max-abs of the float64 pre-activation (test_conv_gpu.py's forward tolerance: fp32 MFMA is an exact
fp32 fma chain).  Exact checks: y >= 0, y == 0 where the float64 pre-activation is below -tol, y > 0 where it is above +tol,
padded channels exactly zero, and the 4096-float guard bands on both sides of the result keep their fill pattern bit for bit
(the result is written through conv2d_fwd(out=) into the middle of a larger buffer).  Conditions that keep a broken epilogue
from passing are asserted: 25-75 % negative pre-activations, max|bias| and max|res| >= 0.1 of the scale, res i.i.d. per element,
Ho * Wo no multiple of 64, B = 2 (tiles straddle rows and images, the last tile is ragged).
Worst error seen per family, relative to the scale: strip 5.7e-7, pipe 1.3e-6, pipe on ranges 6.9e-7, tile 1.5e-6, 1x1 3.3e-7.

Which cases guard which write-out.  Deleting the bias add, the residual add or the ReLU there fails them (bias is i.i.d.
per channel and res i.i.d. per element, each >= 0.1 of the scale against a tolerance of 2e-5; the ReLU checks are exact on the
half of the elements that is negative) -- tried once with the three deletions compiled into every write-out below: every case
of the table failed each time.  Shifting either add by one pixel block or one channel block replaces an i.i.d. value of
order 1 by another one at every element of the block, an error of order 1 against 2e-5 of a scale of about 5; a residual
read or a store at the wrong pixel of the ragged last tile is the same error on fewer elements, and the max-abs check
sees a single element.
  strip, self-overlapped write-out (SO_UNIT), SO 3 / SO 4 ..... so16_*, so32_*; test_folded_stem, test_basic_block
  strip, ping-pong write-out, compile-time 3x3 grid .......... pp*
  strip, ping-pong write-out, run-time tap grid (T33 = 0) .... s2_*_h*, d2_*
  strip, wide-row loader (LW) ................................ lw*, edge16_w143, edge16_w222, edge32_w79, edge32_w110
  conv_pipe_kernel ........................................... pipe_* (every tile that fits, both loader depths PU, KS = 1
                                                               and 2), narrow*, s2_16to32_w65, s2_32to64_w66, edge32_w111
  conv_pipe_kernel on column ranges .......................... ranges*, edge16_w223 (y and res offsets of every range)
  conv_igemm_kernel (one pass) ............................... tile_k5_*, tile_k7_*, tile_stem_*, nopipe16/32/64*, *_7x5
  splitk_reduce_kernel ....................................... *_splitk, tile_k5_64to*_22x17 / _13x17
  conv1x1_direct_kernel ...................................... sc_*

Findings on dispatch, settled with the launch record:
  * test_conv_gpu.py CASES[12] (2,16,32,21,130 stride 2, "two column ranges") IS the pipe kernel on two column ranges; the
    strip kernel does not take it.  conv_strip_try refuses a strided layer unless one tile spans at most two output rows
    (rows_new * nchunks <= STRIP_LOADERS * kp), so the run-time tap grid (T33 = 0) of the strip kernel is reached by strided
    layers only for Ho <= 2 at 16 channels and for short narrow images at 32, and by dilated 3x3 / stride-1 layers; the
    down-sampling convolutions of real inputs run the pipe kernel, in one launch (W = 65, 66) or on ranges (W = 108 .. 216).
  * CASES[13] (1,16,32,9,216 stride 2) said "three" ranges: the record says four.
  * 32 -> 64 3x3 / stride 1 at W = 65 takes the self-overlapped form like 32 -> 32 (the rule looks at chunk count and tile,
    not at Cout); the ping-pong form at 32 input channels needs the 4 x 2 tile (W = 53) or one output block (32 -> 16).
  * 16 -> 32 stride 2 at W = 216 cannot take the wide-row loader (instantiated for NB = 1 at 16 channels only): column ranges.
  * Past the strip's widest rows: 16 channels at W = 223 -> pipe on two ranges; 32 channels at W = 111 -> pipe, one launch.
  * Rows too narrow for the strip (W = 23 at 16 channels, W = 14 at 32) -> pipe <1, 1>, not the tile kernel.

Unreachable from conv2d_fwd's inference call form (named here instead of being dropped):
  * strip <4,1,1> and <2,2,2> with the compile-time grid in the PING-PONG form without LW: every such shape fits the
    self-overlapped form's ring-row bound (rows_out <= 6 follows from the loaders' rows_new rule), so it goes there.
  * strip SO 1 / 2 / 5 and EPI 1-3: statistics, BatchNorm-backward and masked-residual write-outs (bn_partial, bn_bwd or
    res_mask given: training and data gradient).  pipe STATS 1 / 2: the same.
  * tile_batch: only with a caller-owned batch (the parity classes of conv2d_dgrad); conv2d_fwd passes none.
  * strip LW with 16 -> 32 (above), strip with more than 32 input channels (weights no longer resident).

Block level (test_basic_block, test_folded_stem, test_conv_block2d): layers.BasicBlock / the folded stem / ConvBlock2d in
.eval() under no_grad against the float64 oracle modules on the WHOLE output tensor, max-abs error relative to the max-abs of
the oracle output.  Folding rounds weight * scale and the shift to float32 before the convolution; that effect is measured on
the oracle alone (float64 convolutions with float32-folded weights and bias against the unfolded float64 module) and the test
allows max(2e-5, 4 x measured).  Measured folding effect over the cases below: 3e-8 .. 1.2e-7 of max|out| (worst: the
32 -> 32 block at 17x65), so 2e-5 is the bound everywhere; the device's error on the same cases is 2.5e-7 .. 1.0e-6.  What the kernels
receive (FoldedConvBn.get(): packed weights unpacked, bias) is compared with a float64 fold of the same parameters.

NaN propagation through fmaxf in the ReLU write-outs is not decided here."""
import collections

import pytest
import torch
import torch.nn.functional as F

from _randomize import _randomize
from oracle import models_ref

pytestmark = pytest.mark.gpu
TOL = 2e-5
GUARD = 4096
FILL = 0x5EADBEEF                   # guard-band pattern (as float32: 7.8e18, so an unwritten result element fails too)

# name -> (bias, res, relu)
EPILOGUES = collections.OrderedDict([('bias_relu', (True, False, True)), ('bias', (True, False, False)),
                                     ('bias_res_relu', (True, True, True)), ('res', (False, True, False))])

Case = collections.namedtuple('Case', 'id B Ci Co H W k s p d nchw env expect')


def C(id, Ci, Co, H, W, k=3, s=1, p=1, d=1, nchw=False, env=None, **expect):
    return Case(id, 2, Ci, Co, H, W, k, s, p, d, nchw, env or {}, expect)


def _strip(MB, NB, NCH, T33, LW, SO):
    """SO='so': the self-overlapped form, write-out variant 3 (bias / ReLU) or 4 (residual) by epilogue."""
    return dict(family='strip', MB=MB, NB=NB, NCH=NCH, T33=T33, LW=LW, EPI=0, SO=SO)


def _pipe(MB, NB, PU, KS=1):
    return dict(family='pipe', MB=MB, NB=NB, PU=PU, STATS=0, KS=KS)


def _tile(MB, NB, split):
    return dict(family='tile', MB=MB, NB=NB, split=split)


CASES = []          # filled below


def expected(case, res):
    e = dict(case.expect)
    if e.get('SO') == 'so':
        e['SO'] = 4 if res else 3
    e.pop('split', None)
    return e


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _out_hw(c):
    return ((c.H + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1, (c.W + 2 * c.p - c.d * (c.k - 1) - 1) // c.s + 1)


def _inputs(c):
    """x (NCHW), w, bias [n16] (zero in the padded channels), res [B,Ho,Wo,n16] i.i.d. (zero in the padded channels)."""
    g = torch.Generator().manual_seed(1000 + [k.id for k in CASES].index(c.id))
    n16 = (c.Co + 15) // 16 * 16
    Ho, Wo = _out_hw(c)
    x = torch.randn(c.B, c.Ci, c.H, c.W, generator=g)
    w = torch.randn(c.Co, c.Ci, c.k, c.k, generator=g) / (c.Ci * c.k * c.k) ** 0.5
    bias, res = torch.zeros(n16), torch.zeros(c.B, Ho, Wo, n16)
    bias[:c.Co] = torch.randn(c.Co, generator=g)
    res[..., :c.Co] = torch.randn(c.B, Ho, Wo, c.Co, generator=g)
    return x, w, bias, res


SEEN = {}           # (case id, epilogue) -> ConvLaunch
WORST = {}          # family -> (relative error, case id, epilogue)


def _launch(ops, c, epi, xd, wp, bias_d, res_d, monkeypatch):
    """One conv2d_fwd into the middle of a guarded buffer -> (buffer as int32, result view); asserts the dispatch."""
    use_bias, use_res, relu = EPILOGUES[epi]
    Ho, Wo = _out_hw(c)
    n16 = (c.Co + 15) // 16 * 16
    numel = c.B * Ho * Wo * n16
    buf = torch.full((2 * GUARD + numel,), FILL, dtype=torch.int32, device='cuda')
    out = buf.view(torch.float32)[GUARD:GUARD + numel].view(c.B, Ho, Wo, n16)
    with monkeypatch.context() as mp:
        for k, v in c.env.items():
            mp.setenv(k, v)
        y = ops.conv2d_fwd(xd, wp, c.Co, c.k, c.k, c.s, c.p, c.d, bias=bias_d if use_bias else None, in_nchw=c.nchw,
                           res=res_d if use_res else None, relu_out=relu, out=out)
        rec = ops.conv_last_launch()
        plan = ops.conv2d_fwd_plan(xd.shape, c.Co, c.k, c.k, c.s, c.p, c.d, bias=bias_d if use_bias else None, in_nchw=c.nchw,
                                   res=res_d if use_res else None, relu_out=relu, parts=True)
    assert y is out
    assert plan == (rec, 0), '%s %s: launched %s, planned %s' % (c.id, epi, rec, plan)
    SEEN[(c.id, epi)] = rec
    want = expected(c, use_res)
    got = {k: getattr(rec, k) for k in want}
    assert got == want, '%s %s: launched %s' % (c.id, epi, rec)
    if 'split' in c.expect:
        assert (rec.ksplit > 1) == c.expect['split'], '%s %s: launched %s' % (c.id, epi, rec)
    return buf, out


def _device_inputs(ops, c, x, w, bias, res):
    xd = (x if c.nchw else x.permute(0, 2, 3, 1).contiguous()).cuda()
    return xd, ops.pack_weights(w.cuda()), bias.cuda(), res.cuda()


def _check_case(ops, c, monkeypatch):
    x, w, bias, res = _inputs(c)
    Ho, Wo = _out_hw(c)
    assert c.B == 2 and (Ho * Wo) % 64 != 0, 'ragged last tile wanted: Ho * Wo = %d' % (Ho * Wo)
    conv = F.conv2d(x.double(), w.double(), None, c.s, c.p, c.d).permute(0, 2, 3, 1)         # [B, Ho, Wo, Co]
    assert conv.shape == (c.B, Ho, Wo, c.Co)
    dev = _device_inputs(ops, c, x, w, bias, res)
    n16 = bias.numel()
    errs = {}
    for epi, (use_bias, use_res, relu) in EPILOGUES.items():
        pre = conv.clone()
        if use_bias:
            pre += bias[:c.Co].double()
        if use_res:
            pre += res[..., :c.Co].double()
        scale = pre.abs().max().item()
        # the inputs make a broken epilogue visible
        neg = (pre < 0).double().mean().item()
        assert 0.25 <= neg <= 0.75, (c.id, epi, neg)
        assert not use_bias or bias.abs().max().item() >= 0.1 * scale
        assert not use_res or res.abs().max().item() >= 0.1 * scale
        buf, out = _launch(ops, c, epi, *dev, monkeypatch)
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:GUARD] == FILL).all()) and bool((host[-GUARD:] == FILL).all()), '%s %s: guard band written' % (c.id, epi)
        y = host.view(torch.float32)[GUARD:-GUARD].view(c.B, Ho, Wo, n16).double()
        if c.Co < n16:
            assert torch.count_nonzero(y[..., c.Co:]) == 0, '%s %s: padded channels not zero' % (c.id, epi)
        y = y[..., :c.Co]
        want = pre.clamp(min=0) if relu else pre
        err = (y - want).abs()
        worst = err.max().item()
        where = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        errs[epi] = worst / scale
        fam = SEEN[(c.id, epi)].family
        if errs[epi] > WORST.get(fam, (-1.0,))[0]:
            WORST[fam] = (errs[epi], c.id, epi)
        print('%s %s: %s  err %.2e of scale %.3g at [b, oh, ow, ch] = %s' % (c.id, epi, SEEN[(c.id, epi)], errs[epi], scale, where))
        assert worst <= TOL * scale, '%s %s: err %.3g > %.3g at [b, oh, ow, ch] = %s (%d elements over)' % (
            c.id, epi, worst, TOL * scale, where, int((err > TOL * scale).sum()))
        if relu:
            assert bool((y >= 0).all()), '%s %s: negative output behind the ReLU' % (c.id, epi)
            assert bool((y[pre < -TOL * scale] == 0).all()), '%s %s: ReLU missing somewhere' % (c.id, epi)
            assert bool((y[pre > TOL * scale] > 0).all()), '%s %s: positive pre-activation zeroed' % (c.id, epi)
    return errs


# ------------------------------------------------------------------------------------------------------------- the table
# (B = 2 everywhere.)  C(id, Cin, Cout, H, W, k=3, s=1, p=1, d=1, ...)
CASES += [
    # strip, self-overlapped form (SO 3 with bias / ReLU, SO 4 with the residual)
    C('so16_w130', 16, 16, 9, 130, **_strip(4, 1, 1, 1, 0, 'so')),
    C('so16_w142', 16, 16, 7, 142, **_strip(4, 1, 1, 1, 0, 'so')),           # last width before the wide-row loader
    C('so32_w65', 32, 32, 11, 65, **_strip(2, 2, 2, 1, 0, 'so')),
    C('so32to64_w65', 32, 64, 11, 65, **_strip(2, 2, 2, 1, 0, 'so')),        # two workgroups per strip in y
    C('so32_w78', 32, 32, 7, 78, **_strip(2, 2, 2, 1, 0, 'so')),             # last width before the wide-row loader
    # strip, ping-pong form, 3x3 / stride 1
    C('pp16to32_w130', 16, 32, 9, 130, **_strip(4, 2, 1, 1, 0, 0)),
    C('pp16_w50', 16, 16, 21, 50, **_strip(2, 1, 1, 1, 0, 0)),               # 9 ring rows per tile: too many for the SO form
    C('pp32_w53', 32, 32, 13, 53, **_strip(4, 2, 2, 1, 0, 0)),
    C('pp16to32_w50', 16, 32, 21, 50, **_strip(2, 2, 1, 1, 0, 0)),
    C('pp32to16_w53', 32, 16, 13, 53, **_strip(4, 1, 2, 1, 0, 0)),
    C('pp32to16_w65', 32, 16, 11, 65, **_strip(2, 1, 2, 1, 0, 0)),
    # strip, run-time tap grid (T33 = 0).  Strided: only where one tile spans <= 2 output rows (the loaders' rows_new rule in
    # conv_strip_try), i.e. Ho <= 2 at 16 channels and short narrow images at 32 -- the down-sampling convolutions of real
    # inputs take the pipe kernel (below).  Dilated 3x3 / stride 1 reaches the same write-out at ordinary heights.
    C('s2_16to32_h3_w130', 16, 32, 3, 130, s=2, **_strip(4, 2, 1, 0, 0, 0)),
    C('s2_16to32_h4_w129', 16, 32, 4, 129, s=2, **_strip(4, 2, 1, 0, 0, 0)),
    C('s2_16to32_h3_w65', 16, 32, 3, 65, s=2, **_strip(4, 2, 1, 0, 0, 0)),
    C('s2_32to64_h5_w49', 32, 64, 5, 49, s=2, **_strip(4, 2, 2, 0, 0, 0)),
    C('s2_32to64_h4_w46', 32, 64, 4, 46, s=2, **_strip(4, 2, 2, 0, 0, 0)),
    C('d2_16_w130', 16, 16, 9, 130, p=2, d=2, **_strip(4, 1, 1, 0, 0, 0)),
    C('d2_16to32_w130', 16, 32, 9, 130, p=2, d=2, **_strip(2, 2, 1, 0, 0, 0)),
    C('d2_16_w46', 16, 16, 5, 46, p=2, d=2, **_strip(2, 1, 1, 0, 0, 0)),
    C('d2_32_w40', 32, 32, 7, 40, p=2, d=2, **_strip(2, 2, 2, 0, 0, 0)),
    # strip, wide-row loader
    C('lw16_w216', 16, 16, 7, 216, **_strip(4, 1, 1, 1, 1, 0)),
    C('lw16_w213', 16, 16, 9, 213, **_strip(4, 1, 1, 1, 1, 0)),
    C('lw32_w108', 32, 32, 7, 108, **_strip(2, 2, 2, 1, 1, 0)),
    C('lw_s2_16_h2_w216', 16, 16, 2, 216, s=2, **_strip(4, 1, 1, 0, 1, 0)),   # (16 -> 32 needs NB = 2, which the LW form lacks)
    C('lw_s2_32to64_h2_w108', 32, 64, 2, 108, s=2, **_strip(2, 2, 2, 0, 1, 0)),
    # the dispatch boundaries in width (142 and 78: above, with the SO form)
    C('edge16_w143', 16, 16, 7, 143, **_strip(4, 1, 1, 1, 1, 0)),
    C('edge16_w222', 16, 16, 7, 222, **_strip(4, 1, 1, 1, 1, 0)),
    C('edge16_w223', 16, 16, 7, 223, family='pipe_ranges', ranges=2),
    C('edge32_w79', 32, 32, 7, 79, **_strip(2, 2, 2, 1, 1, 0)),
    C('edge32_w110', 32, 32, 7, 110, **_strip(2, 2, 2, 1, 1, 0)),
    C('edge32_w111', 32, 32, 7, 111, **_pipe(1, 1, 8)),
    # rows too narrow for the strip kernel
    C('narrow16_w23', 16, 16, 21, 23, **_pipe(1, 1, 5)),
    C('narrow32_w14', 32, 32, 21, 14, **_pipe(1, 1, 5)),
    # the down-sampling 3x3 / stride-2 convolutions at the stage widths: pipe, or pipe on column ranges
    C('s2_16to32_w65', 16, 32, 11, 65, s=2, **_pipe(1, 1, 8)),
    C('s2_32to64_w66', 32, 64, 10, 66, s=2, **_pipe(1, 1, 8)),
    C('ranges_s2_16to32_w130', 16, 32, 12, 130, s=2, family='pipe_ranges', ranges=2),
    C('ranges_s2_16to32_w129', 16, 32, 21, 129, s=2, family='pipe_ranges', ranges=2),
    C('ranges_s2_16to32_w216', 16, 32, 9, 216, s=2, family='pipe_ranges', ranges=4),
    C('ranges_s2_32to64_w108', 32, 64, 9, 108, s=2, family='pipe_ranges', ranges=2),
    C('ranges64_w216', 64, 64, 5, 216, family='pipe_ranges', ranges=2),
]


# conv_pipe_kernel: the shapes of test_conv_gpu.py::test_loader_wave_tile_kernel (B = 2), the tile of the rule and every other
# tile that fits, few persistent workgroups (each walks many units: the stream crosses unit and image boundaries)
PIPE_SHAPES = [('64_w33', 64, 20, 33, 1), ('96_w17', 96, 11, 17, 1), ('128_w9', 128, 13, 9, 1), ('256_w5', 256, 7, 5, 1),
               ('64_w12_s2', 64, 12, 12, 2), ('64_w54', 64, 9, 54, 1), ('128_h17_w9', 128, 17, 9, 1)]
# per shape: (MB, NB, PU, KS) of the rule's own tile, PU of the 2-row tiles (2x2, 2x1), KS of the forced 1x1 tile
PIPE_RULE = {'64_w33': ((1, 1, 5, 1), 5, 1), '96_w17': ((1, 1, 3, 2), 5, 2), '128_w9': ((1, 1, 3, 2), 5, 2),
             '256_w5': ((2, 1, 5, 1), 5, 2), '64_w12_s2': ((2, 1, 5, 1), 5, 1), '64_w54': ((1, 1, 5, 1), 8, 1),
             '128_h17_w9': ((1, 1, 3, 2), 5, 2)}
for name, ch, h, w, st in PIPE_SHAPES:
    rule, pu2, ks1 = PIPE_RULE[name]
    CASES.append(C('pipe_' + name, ch, ch, h, w, s=st, **_pipe(*rule)))
    CASES.append(C('pipe_%s_wgs3' % name, ch, ch, h, w, s=st, env={'DAM_PIPE_WGS': '3'}, **_pipe(*rule)))
    for (mb, nb), wgs in (((1, 4), 5), ((2, 2), 2), ((1, 2), 3), ((2, 1), 5), ((1, 1), 7)):
        if (ch // 16) % nb:
            continue                            # the tile must divide the block count (96 channels: no 1x4)
        ks = ks1 if (mb, nb) == (1, 1) else 1
        pu = 3 if ks == 2 else (pu2 if mb == 2 else 5)
        CASES.append(C('pipe_%s_%dx%d' % (name, mb, nb), ch, ch, h, w, s=st,
                       env={'DAM_TILE': '%dx%d' % (mb, nb), 'DAM_PIPE_WGS': str(wgs)}, **_pipe(mb, nb, pu, ks)))
    if rule[3] == 2:                            # the K split switched off: the plain one-block tile
        CASES.append(C('pipe_%s_ks1' % name, ch, ch, h, w, s=st, env={'DAM_PIPE_KS': '1', 'DAM_PIPE_WGS': '4'}, **_pipe(1, 1, 5, 1)))

CASES += [
    # tile kernel (conv_igemm_kernel), no split-K: the scalar models' 5x5 / 7x7 kernels, 48 and 24 (padded) output channels, the
    # NCHW stem with dilation, narrow 3x3 rows with the pipe kernel switched off
    C('tile_k5_16to32', 16, 32, 21, 31, k=5, p=0, **_tile(1, 1, False)),
    C('tile_k5_32to48', 32, 48, 21, 31, k=5, p=0, **_tile(1, 1, False)),
    C('tile_k5_32to24', 32, 24, 21, 31, k=5, p=0, **_tile(1, 1, False)),
    C('tile_k7_48to64', 48, 64, 21, 33, k=7, p=0, **_tile(1, 1, False)),
    C('tile_stem_nchw_d2', 4, 16, 21, 45, s=2, p=0, d=2, nchw=True, **_tile(1, 1, False)),
    C('tile_stem_nchw_d1', 8, 16, 21, 45, s=2, p=0, nchw=True, **_tile(1, 1, False)),
    C('nopipe16_w23', 16, 16, 21, 23, env={'DAM_NO_PIPE': '1'}, **_tile(1, 1, False)),
    C('nopipe32_w14', 32, 32, 21, 14, env={'DAM_NO_PIPE': '1'}, **_tile(1, 1, False)),
    C('nopipe64_w12_s2', 64, 64, 12, 12, s=2, env={'DAM_NO_PIPE': '1'}, **_tile(1, 4, False)),
    # ... with split-K: splitk_reduce_kernel writes the result (bias, residual, ReLU there)
    C('tile_k9_splitk', 64, 128, 30, 25, k=9, p=0, **_tile(2, 4, True)),
    C('tile_1x1_256_splitk', 256, 256, 13, 9, k=1, s=2, p=0, **_tile(1, 4, True)),
    C('nopipe256_w5_splitk', 256, 256, 7, 5, env={'DAM_NO_PIPE': '1'}, **_tile(1, 4, True)),
    C('nopipe64_w33_splitk', 64, 64, 20, 33, env={'DAM_NO_PIPE': '1'}, **_tile(4, 4, True)),
    C('nopipe96_w17_splitk', 96, 96, 11, 17, env={'DAM_NO_PIPE': '1'}, **_tile(1, 3, True)),
]
# the twelve <MB, NB> instantiations: 64 -> 16 / 32 / 48 / 64 5x5 at three image sizes (MB by least padding, NB by block count)
for co, nb in ((16, 1), (32, 2), (48, 3), (64, 4)):
    for (ho, wo), mb, split in (((22, 17), 2, True), ((13, 17), 4, True), ((7, 5), 1, False)):
        CASES.append(C('tile_k5_64to%d_%dx%d' % (co, ho, wo), 64, co, ho + 4, wo + 4, k=5, p=0, **_tile(mb, nb, split)))

CASES += [
    # direct 1x1 / stride 2 (the shortcut convolutions): <NB, chunk slots>
    C('sc_16to32', 16, 32, 21, 130, k=1, s=2, p=0, family='1x1', NB=2, NCH=2),
    C('sc_32to64', 32, 64, 11, 65, k=1, s=2, p=0, family='1x1', NB=2, NCH=2),
    C('sc_64to96', 64, 96, 13, 33, k=1, s=2, p=0, family='1x1', NB=2, NCH=4),
    C('sc_96to128', 96, 128, 9, 17, k=1, s=2, p=0, family='1x1', NB=2, NCH=8),
    C('sc_128to256', 128, 256, 9, 9, k=1, s=2, p=0, family='1x1', NB=2, NCH=8),
    C('sc_32to48', 32, 48, 11, 65, k=1, s=2, p=0, family='1x1', NB=1, NCH=2),
    C('sc_64to48', 64, 48, 12, 34, k=1, s=2, p=0, family='1x1', NB=1, NCH=4),
    C('sc_96to48', 96, 48, 9, 18, k=1, s=2, p=0, family='1x1', NB=1, NCH=8),
]
assert len({c.id for c in CASES}) == len(CASES)


def _variant(rec):
    """The part of a launch record that names a kernel instantiation / write-out path."""
    if rec.family == 'strip':
        return ('strip', rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.SO)
    if rec.family == 'pipe':
        return ('pipe', rec.MB, rec.NB, rec.PU, rec.KS)
    if rec.family == 'pipe_ranges':
        return ('pipe_ranges', rec.ranges)
    if rec.family == 'tile':
        return ('tile', rec.MB, rec.NB, 'split-K' if rec.ksplit > 1 else 'one pass')
    if rec.family == '1x1':
        return ('1x1', rec.NB, rec.NCH)
    return (rec.family,)


REQUIRED = (
    # strip <MB, NB, NCH, T33, LW, SO>: self-overlapped write-outs 3 and 4 at 16 and 32 channels
    [('strip', 4, 1, 1, 1, 0, so) for so in (3, 4)] + [('strip', 2, 2, 2, 1, 0, so) for so in (3, 4)] +
    # ping-pong form: compile-time 3x3 grid, run-time tap grid (strided, dilated), wide-row loader with either
    [('strip', 4, 2, 1, 1, 0, 0), ('strip', 2, 1, 1, 1, 0, 0), ('strip', 2, 1, 2, 1, 0, 0), ('strip', 2, 2, 1, 1, 0, 0), ('strip', 4, 2, 2, 1, 0, 0), ('strip', 4, 1, 2, 1, 0, 0),
     ('strip', 4, 2, 1, 0, 0, 0), ('strip', 4, 2, 2, 0, 0, 0), ('strip', 4, 1, 1, 0, 0, 0), ('strip', 2, 2, 1, 0, 0, 0),
     ('strip', 2, 1, 1, 0, 0, 0), ('strip', 2, 2, 2, 0, 0, 0),
     ('strip', 4, 1, 1, 1, 1, 0), ('strip', 2, 2, 2, 1, 1, 0), ('strip', 4, 1, 1, 0, 1, 0), ('strip', 2, 2, 2, 0, 1, 0)] +
    # pipe <MB, NB, PU, KS>: every tile of its rule, both loader depths, the K split
    [('pipe', mb, nb, 5, 1) for mb, nb in ((1, 4), (2, 2), (1, 2), (2, 1), (1, 1))] +
    [('pipe', 2, 2, 8, 1), ('pipe', 2, 1, 8, 1), ('pipe', 1, 1, 8, 1), ('pipe', 1, 1, 3, 2)] +
    [('pipe_ranges', 2), ('pipe_ranges', 4)] +
    # tile <MB, NB>: all twelve instantiations; split-K (splitk_reduce_kernel writes the result) and one pass
    [('tile', mb, nb, 'split-K') for mb in (4, 2) for nb in (1, 2, 3, 4)] + [('tile', 1, nb, 'one pass') for nb in (1, 2, 3, 4)] +
    [('tile', 1, 4, 'split-K'), ('tile', 1, 3, 'split-K')] +
    # direct 1x1 <NB, chunk slots>
    [('1x1', nb, nch) for nb in (2, 1) for nch in (2, 4, 8)])


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_epilogue(ops, case, monkeypatch):
    _check_case(ops, case, monkeypatch)


def test_coverage(ops, monkeypatch):
    """The union of the launches the table made covers REQUIRED.  (Cases that did not run in this process -- a -k selection --
    are launched here without their oracle, so the test stands on its own.)"""
    for c in CASES:
        missing = [e for e in EPILOGUES if (c.id, e) not in SEEN]
        if missing:
            dev = _device_inputs(ops, c, *_inputs(c))
            for e in missing:
                _launch(ops, c, e, *dev, monkeypatch)
    torch.cuda.synchronize()
    seen = {_variant(r) for r in SEEN.values()}
    for fam in sorted(WORST):
        print('worst error, %s: %.2e of the scale (%s, %s)' % ((fam,) + WORST[fam]))
    print('variants seen: %s' % sorted(seen))
    lacking = [v for v in REQUIRED if v not in seen]
    assert not lacking, 'kernel variants no case reached: %s' % lacking
    # every residual epilogue of a column-range launch went through more than one range
    assert all(r.ranges >= 2 for r in SEEN.values() if r.family == 'pipe_ranges')


def test_out_argument(ops):
    """conv2d_fwd(out=) refuses a result tensor of the wrong type, layout or shape; without it nothing changes."""
    x, w = torch.randn(1, 5, 20, 16).cuda(), torch.randn(16, 16, 3, 3).cuda()
    wp = ops.pack_weights(w)
    y = ops.conv2d_fwd(x, wp, 16, 3, 3, 1, 1, 1)
    out = torch.empty_like(y)
    assert ops.conv2d_fwd(x, wp, 16, 3, 3, 1, 1, 1, out=out) is out and torch.equal(out, y)
    for bad in (torch.empty(1, 5, 20, 32, device='cuda'), torch.empty(1, 5, 20, 16, device='cuda', dtype=torch.float64),
                torch.empty(1, 5, 16, 20, device='cuda').transpose(2, 3), torch.empty(1, 5, 20, 16)):
        with pytest.raises(ValueError):
            ops.conv2d_fwd(x, wp, 16, 3, 3, 1, 1, 1, out=bad)


# ------------------------------------------------------------------------------------------------------------ block level
def _fold(conv, bn, dtype):
    """FoldedConvBn.get()'s arithmetic in `dtype` on the CPU -> (weight, bias, magnitude of the bias terms) as float64."""
    cast = lambda t: t.detach().cpu().to(dtype)
    scale = cast(bn.weight) * torch.rsqrt(cast(bn.running_var) + bn.eps)
    shift = cast(bn.bias) - cast(bn.running_mean) * scale
    mag = cast(bn.bias).abs() + (cast(bn.running_mean) * scale).abs()
    if conv.bias is not None:
        shift = shift + cast(conv.bias) * scale
        mag = mag + (cast(conv.bias) * scale).abs()
    return (cast(conv.weight) * scale.view(-1, 1, 1, 1)).double(), shift.double(), mag.double()


def _unpack(wp, n16, k16, kh, kw):
    """Packed forward weights [tap][chunk][block][kq][i][s] (n = block * 16 + i, k = chunk * 16 + kq * 4 + s) -> [n16, k16, kh, kw]."""
    assert wp.numel() == n16 * k16 * kh * kw
    return wp.view(kh * kw, k16 // 16, n16 // 16, 4, 16, 4).permute(2, 4, 1, 3, 5, 0).reshape(n16, k16, kh, kw)


def _check_folded_inputs(f):
    """What the kernels receive against a float64 fold of the same parameters.  Bound: the float32 fold is var + eps, rsqrt
    (<= 2 ulp), * gamma, * weight -- under 6e-7 relative; the shift adds one product and two sums of terms whose magnitudes
    are summed in `mag`.  1e-6 of the value (weights) / of mag (bias)."""
    wp, bias = f.get()
    conv, co, ci, k = f.conv, f.spec.cout, f.conv.in_channels, f.spec.k
    n16, k16 = (co + 15) // 16 * 16, (ci + 15) // 16 * 16
    w64, b64, mag = _fold(conv, f.bn, torch.float64)
    got_w, got_b = _unpack(wp, n16, k16, k, k).double().cpu(), bias.double().cpu()
    assert bool(((got_w[:co, :ci] - w64).abs() <= 1e-6 * w64.abs()).all())
    assert torch.count_nonzero(got_w[co:]) == 0 and torch.count_nonzero(got_w[:, ci:]) == 0
    assert got_b.numel() == n16 and bool(((got_b[:co] - b64).abs() <= 1e-6 * mag).all())
    assert torch.count_nonzero(got_b[co:]) == 0
    assert float(got_b.abs().max()) > 0


def _conv_bn_folded32(conv, bn, x, relu, res=None):
    """float64 convolution with the float32-folded weights and bias: the oracle's view of the folding error alone."""
    w, b, _ = _fold(conv, bn, torch.float32)
    y = F.conv2d(x, w, b, conv.stride, conv.padding, conv.dilation)
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def _rel_max(got, want):
    return float((got - want).abs().max() / want.abs().max())


FOLD_WORST = [0.0]


def _compare(name, got, want, want_folded32):
    fold = _rel_max(want_folded32, want)
    FOLD_WORST[0] = max(FOLD_WORST[0], fold)
    tol = max(TOL, 4 * fold)
    err = _rel_max(got, want)
    live = float((want > 0).double().mean())
    print('%s: err %.2e of max|out| (folding alone: %.2e, allowed %.2e); %.0f %% of the outputs positive' % (name, err, fold, tol, 100 * live))
    assert 0.1 <= live <= 0.9, (name, live)
    assert err <= tol, (name, err, tol)


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double().cpu()


BLOCKS = [(16, 16, 1, (130, 216)), (16, 32, 2, (130, 216)), (32, 32, 1, (65, 108)), (32, 64, 2, (65, 108)), (64, 64, 1, (33, 54)),
          (64, 96, 2, (33, 54)), (96, 128, 2, (17, 27)), (128, 256, 2, (9, 14)), (256, 256, 1, (5, 7))]
BLOCK_CASES = [(ci, co, s, 7 + (5 * i + 9 * j) % 15, w) for i, (ci, co, s, ws) in enumerate(BLOCKS) for j, w in enumerate(ws)]


@pytest.mark.parametrize('cin,cout,stride,H,W', BLOCK_CASES, ids=['%dto%d_s%d_%dx%d' % b for b in BLOCK_CASES])
def test_basic_block(ops, cin, cout, stride, H, W):
    """layers.BasicBlock in eval() under no_grad (three folded launches, two without a shortcut convolution) against
    RefBasicBlock in float64, whole output tensor, at the stage widths of 130- and 216-frame inputs."""
    from deep_audio_mixer_amd import layers
    gen = torch.Generator().manual_seed(7000 + BLOCK_CASES.index((cin, cout, stride, H, W)))
    blk = _randomize(layers.BasicBlock(cin, cout, stride), gen)
    ref = models_ref.RefBasicBlock(cin, cout, stride).double()
    ref.load_state_dict({k: v.double() for k, v in blk.state_dict().items()})
    ref.eval()
    x = torch.relu(torch.randn((2, H, W, cin), generator=gen))
    x64 = x.permute(0, 3, 1, 2).double()
    with torch.no_grad():
        want = ref(x64)
        a1 = _conv_bn_folded32(ref.conv1, ref.bn1, x64, True)
        sc = _conv_bn_folded32(ref.shortcut[0], ref.shortcut[1], x64, False) if len(ref.shortcut) else x64
        want32 = _conv_bn_folded32(ref.conv2, ref.bn2, a1, True, res=sc)
        blk = blk.cuda().eval()
        out = blk(x.cuda())
        assert out.grad_fn is None and tuple(out.shape) == (2, want.shape[2], want.shape[3], cout)
        for f in blk._folded():
            if f is not None:
                _check_folded_inputs(f)
    _compare('block %d->%d s%d %dx%d' % (cin, cout, stride, H, W), _nchw64(out), want, want32)


def _db_input_stats(conv64, bn_modules, x64, gen):
    """Running statistics around where a dB-valued input puts the convolution output (as tests/test_eval_backward_gpu.py)."""
    with torch.no_grad():
        c = conv64(x64).float()
        mean = c.mean((0, 2, 3)) + 0.3 * c.std((0, 2, 3)) * torch.randn(c.shape[1], generator=gen)
        var = c.var((0, 2, 3)) * (0.5 + torch.rand(c.shape[1], generator=gen))
        for bn in bn_modules:
            bn.running_mean.copy_(mean), bn.running_var.copy_(var)


@pytest.mark.parametrize('H,W', [(11, 130), (9, 216)])
def test_folded_stem(ops, H, W):
    """The ResNet stem, ConvSpec(8, 16, 3, 1, 1, in_nchw=True), through FoldedConvBn.fwd: the NCHW planes re-laid as NHWC-16
    and the 16-channel strip kernel with bias + ReLU, against relu(bn(conv(x))) in float64."""
    from deep_audio_mixer_amd import layers
    gen = torch.Generator().manual_seed(7100 + W)
    stem = _randomize(torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)), gen)
    ref = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)).double()
    x = -20.0 + 15.0 * torch.randn((2, 8, H, W), generator=gen)
    ref.load_state_dict({k: v.double() for k, v in stem.state_dict().items()})
    _db_input_stats(ref[0], (stem[1], ref[1]), x.double(), gen)
    ref.eval()
    with torch.no_grad():
        want = torch.relu(ref(x.double()))
        want32 = _conv_bn_folded32(ref[0], ref[1], x.double(), True)
        stem = stem.cuda().eval()
        f = layers.FoldedConvBn(layers.ConvSpec(8, 16, 3, 1, 1, in_nchw=True), stem[0], stem[1])
        assert f.spec.nhwc16 is not None and f.foldable()
        out = f.fwd(x.cuda())
        rec = ops.conv_last_launch()
        _check_folded_inputs(f)
    assert rec.family == 'strip' and rec.NCH == 1 and (rec.SO == 3 if W == 130 else rec.LW == 1), rec
    _compare('stem %dx%d' % (H, W), _nchw64(out), want, want32)


# the five ConvBlock2d geometries of the scalar models (conv bias, eps 1e-3; first layer NCHW, stride 2, dilation 1 or 2)
CONV_BLOCKS = [('b1_1s', 4, 16, 3, 2, 1, 21, 45, True), ('b1_2s', 4, 16, 3, 2, 2, 21, 45, True), ('b2', 16, 32, 5, 1, 1, 21, 31, False),
               ('b3', 32, 48, 5, 1, 1, 21, 31, False), ('b4', 48, 64, 7, 1, 1, 21, 33, False), ('b5', 64, 128, 9, 1, 1, 21, 25, False)]


@pytest.mark.parametrize('name,cin,cout,k,stride,dil,H,W,nchw', CONV_BLOCKS, ids=[b[0] for b in CONV_BLOCKS])
def test_conv_block2d(ops, name, cin, cout, k, stride, dil, H, W, nchw):
    """layers.ConvBlock2d in eval() under no_grad (one folded launch; the convolution's own bias goes into the folded bias)
    against RefConvBlock2d in float64."""
    from deep_audio_mixer_amd import layers
    gen = torch.Generator().manual_seed(7200 + [b[0] for b in CONV_BLOCKS].index(name))
    blk = _randomize(layers.ConvBlock2d(cin, cout, k, stride=stride, dilation=dil, dropout_p=0.2, in_nchw=nchw), gen)
    ref = models_ref.RefConvBlock2d(cin, cout, k, stride, dil, 0.2).double()
    ref.load_state_dict({k_: v.double() for k_, v in blk.state_dict().items()})
    if nchw:
        x = -20.0 + 15.0 * torch.randn((2, cin, H, W), generator=gen)
        x64 = x.double()
        _db_input_stats(ref.conv, (blk.batch_norm, ref.batch_norm), x64, gen)
    else:
        x = torch.relu(torch.randn((2, H, W, cin), generator=gen))
        x64 = x.permute(0, 3, 1, 2).double()
    ref.eval()
    with torch.no_grad():
        want = ref(x64)
        want32 = _conv_bn_folded32(ref.conv, ref.batch_norm, x64, True)
        blk = blk.cuda().eval()
        out = blk(x.cuda())
        assert blk.conv.bias is not None and float(blk.conv.bias.abs().max()) > 0
        _check_folded_inputs(blk._fold)
    n16 = (cout + 15) // 16 * 16
    assert tuple(out.shape) == (2, want.shape[2], want.shape[3], n16) and torch.count_nonzero(out[..., cout:]) == 0
    _compare('ConvBlock2d %s' % name, _nchw64(out[..., :cout]), want, want32)
