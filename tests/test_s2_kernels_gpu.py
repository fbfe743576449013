"""GPU: every kernel and instantiation behind the three entry points that carry the ResNet's down-sampling blocks
(dam_conv_s2_pair_fwd_f32, dam_dgrad_s2_3x3_f32, dam_conv1x1_pair_f32) against F.conv2d / torch.nn.grad.conv2d_input on the CPU in
float64, each case asserting through ops.s2_last_launch() the launch it names.

Each entry point picks its kernel by a plan (csrc/dam_s2_plan.h) -- by channel counts (persistent kernels with the packed weights
resident in LDS for 16 <-> 32 and 32 <-> 64 channels, streaming kernels for the wide layers), by pixel count (two pixel blocks per
wave of the streaming data gradient from cdiv(px, 16) * NB >= 8192), by the CU count, an occupancy answer and a makespan rule (the
grid of a persistent kernel, and with it how often a wave goes round its unit loop and whether the units are dealt to eight XCDs) --
and ops.conv2d_dgrad falls from dam_dgrad_s2_3x3_f32 to the parity classes + dam_conv1x1_pair_f32 when that refuses.  The plan can be
asked without launching (ops.conv_s2_pair_fwd_plan, ops.conv2d_dgrad_s2_plan, ops.conv1x1_pair_plan; tests/test_s2_plan_cpu.py
holds the dispatch table on a machine without a GPU).  Every row of the table NAMES the launch it means, the helper asserts the
whole record (_record: instantiation, grid, units, rounds, n_xcd, records -- host arithmetic from the shape, an independent second
derivation, checked in test_table_conditions) and that the record equals the plan of the same call on this device (_plan) before
it looks at a number, and test_coverage asserts that the union of the records covers REQUIRED.

Reference: F.conv2d / torch.nn.grad.conv2d_input (+ the shortcut term) on the CPU in float64, at most 1.25 GFLOP per case
(the block of test_retreat_block_forward: 1.8 for its two 3x3 convolutions).  Every
result goes through out= / records= into the middle of a buffer with 4096-element guard bands of 0x5EADBEEF, checked bit for bit;
of a record buffer everything behind record `parts` as well.  Bounds (the project's own, the constants below): y and dx 2e-5 of
the max-abs of the float64 result; merged mean 1e-5 of the largest mean, merged 1 / sqrt(var + eps) 2e-5 relative; the two backward
sums 2e-5 of the channel's float64 sum |term| with no absolute allowance (a channel whose pixels are all masked must be exactly
0); dx with bn_bwd bitwise the dx without whenever the two records agree; c1 / cs without statistics bitwise those with.
Forward forms: stats, nostats.  x = 3 z + 7 per element and weights with a small positive mean, so |mean| >= std of the float64
outputs on at least half the channels (asserted): a sum-of-squares shortcut in the shifted one-pass statistics would fail.  The
test merges the records itself with Chan's formula (counts add up to B * Hd * Wd exactly, every M2 >= 0, records with n = 0 legal)
and hands them to bn_finalize_pair once per instantiation.
Data-gradient forms: alone, pair, sums, pair_sums.  Weights random without symmetry, dy and ds i.i.d.; the sign bytes are an
INPUT, built on the CPU from a random float64 y with |y| >= 0.1, 25-75 % set (asserted); the sums reference is formed from the
float64 reference dx, never from the kernel's.  Streaming kernels must report sums None with dx still right.

The table (workgroups and rounds of the loop rows were read from the record on the first run on an MI355X, 256 CUs, and are
pinned: occupancy 2 workgroups per CU for the 4-wave kernels at these sizes, 1 by construction for the 8-wave ones):
  * 8 edge shapes x {16 -> 32, 32 -> 64 resident; 32 -> 48 (NB 3), 64 -> 96 (NB 6) streaming} forward and x {16 <- 32, 32 <- 64
    resident; 48 <- 96 (NB 3), 32 <- 32 streaming} backward: (2, 41 | 40, 27 | 28) -- every H / W parity, Wd = 14, units straddle
    rows and images, px no multiple of 64 -- and (1, 3, 3), (1, 2, 2), (1, 1, 5), (3, 6, 1): fewer pixels than a unit, no odd row
    or column class.  One round, n_xcd 1 (resident) -- the grid is cdiv(units, WAVES) workgroups.
  * *_xcd8: (1, 99, 79) / (1, 121, 63): 125 / 61 units on 32 / 16 workgroups: one round on eight XCDs, XCD 7's share short.
  * f16to32_loop (8, 385, 130): 6273 units, 512 workgroups, rounds 4: 129 waves take 4 units, 1919 take 3 (odd AND even counts
    for the two-units-per-iteration loop of NCH == 1), XCD 7 takes 778 of 785.
    f32to64_loop (8, 129, 130): 2113 units, 256 workgroups of 8 waves, rounds 2, XCD 7 takes 258 of 265.
    d16from32_loop (8, 385, 130): 3137 units of 32 pixels, 512 workgroups, rounds 2 -- all four PAIR x SUMS forms.
    d32from64_loop (8, 129, 130): 2113 units, 256 workgroups of 8 waves, rounds 2 -- all four forms.
  * d48from32_stream (2, 299, 293): 8271 (pixel block, channel block) pairs: the MB = 2 streaming kernel with NB = 3.
  * p*: dam_conv1x1_pair_f32, all six <NB, R, BOTH>: behind shapes dam_dgrad_s2_3x3_f32 refuses by itself (Co = 48, 80, 144:
    record entry pair_1x1, ops.dgrad_s2_launches unchanged; <1, 8, false> with a last round of 5 and of 1 live chunk, <2, 4, false>
    of 1) and behind the model's shapes with ops.DGRAD_S2 off.  Without a shortcut term the refused shapes leave record "none".
  * test_retreat_*: forward streaming statistics at exactly 2048 groups (2048 records) and at 2056 (None, record "none", every
    buffer untouched; without statistics it runs); a BasicBlock forward at such a shape (layers.py takes the separate launches);
    bn_bwd at stride 2 on a refused shape ((dx, None), record buffer untouched).

Worst error seen (MI355X), against its bound:
  forward resident     c1 1.1e-6, cs 3.0e-7 (2e-5); mean 3.8e-7 (1e-5); invstd 4.0e-6 (2e-5); through bn_finalize_pair 7.2e-8, 1.5e-7
  forward stream_lds   c1 1.3e-6, cs 3.9e-7; mean 6.7e-7; invstd 6.4e-6; through bn_finalize_pair 6.7e-8, 2.6e-7
  dgrad resident       dx 7.3e-7 (2e-5); sum dz 3.5e-6, sum dz uhat 3.4e-6 (2e-5; both on (1, 1, 5), three pixels of dy)
  dgrad stream_lds     dx 8.7e-7        dgrad stream (MB 2)  dx 4.5e-7        parity classes + 1x1 pair  dx 5.9e-7
  block forward        2.9e-7 of the norm (2e-5)

Findings on dispatch, settled with the launch record (tests/test_conv_gpu.py):
  * test_strided_dgrad_one_launch: only (8, 16 <- 32, 1025, 130) loops (768 workgroups, rounds 3, no sums).  (2, 32 <- 64, 513, 65)
    is 1061 units on 133 workgroups: one unit per wave, n_xcd 1 -- <2, 4, 1, 8> never went round its loop in a kernel-level
    test.  (2, 64 <- 96, 513, 130) is the only MB = 2 streaming launch, the other wide shapes take stream_lds.
  * test_strided_dgrad_takes_the_upstream_batchnorm_sums: every case is one round on one "XCD" (at most 69 workgroups): the SUMS
    instantiations' accumulation across units and their u / sign-byte prefetch under a unit with a successor ran in whole-model
    tests only.  The sums were compared with sums over the kernel's own dx.
  * test_downsampling_pair_forward_one_launch: (8, 16 -> 32, 1025, 130) loops 9 times on 512 workgroups with statistics and 6
    times on 768 without (the two instantiations differ in occupancy); (8, 32 -> 64, 513, 65) 3 times; everything else one round.
  * None of the three docstrings claimed a loop or a kernel it did not run; they now say what the record shows.
  * A 3x3 / stride-2 convolution of 32 channels with rows of 480 pixels or more is refused by dam_conv2d_tapgrid_f32 itself
    (dam_conv2d_tapgrid_plan says so without a GPU), so a BasicBlock at the issue's (2, 32 -> 16, 513, 512) raises instead of
    retreating; the block test uses (2, 657, 400), 2057 groups.  Loud, not silent: left as it is.
  * No case exposed a wrong number.

Unreachable here (named instead of dropped):
  * the refusals that need a shape no float64 reference can follow or a device this one is not -- the record limits of the two
    persistent kernels, the 2 GiB byte-offset and 2^26 / 2^30 pixel refusals, n_xcd 1 together with rounds >= 2 (a CU count that
    is no multiple of 8) -- are planned in tests/test_s2_plan_cpu.py, where CU count and occupancy are arguments.
  * DAM_ERR_LAUNCH of raise_lds_limit: the runtime grants 160 KB on this device.

Mutations, each compiled into a scratch copy of the library and run once against this file (numbers only: no store address,
no load bound changed):
  * dgrad_s2_kernel rotates in the CURRENT unit's offsets (o** = o**): d16from32_loop and d32from64_loop fail (dx off by the
    scale), the other 87 tests pass.
  * the SUMS write-out counts an odd-column class outside the image with all four bits set: the twelve resident cases with odd W
    fail ((2, 41 | 40, 27), (1, 3, 3), (1, 1, 5), (3, 6, 1), *_xcd8: W = 63, 79), the even-W cases pass.
  * conv_s2_pair_kernel <.., NCH = 1> skips the statistics of the second unit of an iteration: f16to32_loop fails (the counts add
    up to 65 536, not 100 360); the one-round cases and the NCH = 2 kernel pass.
  * conv1x1_pair_kernel <1, 8, false> repeats the last chunk in the dead slots of its last round: p16from80 and p16from144 fail
    (dx off by 1.5 and 2.0 of the scale), everything else passes.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

GUARD = 4096
FILL = 0x5EADBEEF                   # guard-band pattern (as float32: 7.8e18, so an unwritten output element fails too)
# The project's own bounds:
TOL_OUT = 2e-5                      # y, dx: of the max-abs of the float64 result (tests/test_conv_gpu.py: TOL, fp32 accumulation)
TOL_MEAN = 1e-5                     # merged mean: of the max-abs of the float64 means (test_downsampling_pair_forward_one_launch)
TOL_INVSTD = 2e-5                   # merged 1 / sqrt(var + eps): relative, per channel
TOL_SUMS = 2e-5                     # the two backward sums: of that channel's float64 sum |term|, no absolute allowance
                                    # (test_strided_dgrad_takes_the_upstream_batchnorm_sums)
TOL_BLOCK = 2e-5                    # a block's forward: of the norm of the float64 output (tests/test_blocks_gpu.py: TOL)
EPS = 1e-5
CUS = 256                           # MI355X: the workgroup counts of the loop cases below were read on it
BN_RECORDS_MAX = 2048               # dam_common.h

FWD_FORMS = ('stats', 'nostats')
DGRAD_FORMS = ('alone', 'pair', 'sums', 'pair_sums')

# kind 'fwd': x [B, H, W, Ci] -> c1, cs [B, Hd, Wd, Co]; kind 'dgrad': dy, ds [B, Hd, Wd, Co] -> dx [B, H, W, Ci]
# family: resident / stream_lds / stream / pair_1x1; wgs: workgroups of a resident launch where the shape does not decide them
# (the loop cases: read from the record on the first run on the device); rounds, n_xcd: what the row CLAIMS (asserted)
# inst (pair_1x1): <NB, R, BOTH>; patch: reached with ops.DGRAD_S2 off (the model's shapes)
Case = collections.namedtuple('Case', 'id kind B Ci Co H W family wgs rounds n_xcd inst patch')


def _cdiv(a, b):
    return (a + b - 1) // b


def _geo(c):
    Hd, Wd = (c.H + 1) // 2, (c.W + 1) // 2
    return Hd, Wd, c.B * Hd * Wd


def _resident_inst(c):
    """<NB, NCH, MB, WAVES> of the persistent kernel the channel counts pick."""
    if c.kind == 'fwd':
        return {(16, 32): (2, 1, 1, 4), (32, 64): (4, 2, 1, 8)}[(c.Ci, c.Co)]
    return {(16, 32): (1, 2, 2, 4), (32, 64): (2, 4, 1, 8)}[(c.Ci, c.Co)]


def _walk(units, wgs, waves):
    """The unit walk of the persistent kernels (per_xcd / u_lo / unit_end / ustride) -> n_xcd, units per wave (every wave of the
    grid), units per XCD."""
    n_xcd = 8 if wgs % 8 == 0 else 1
    wg_per_xcd, per_xcd = wgs // n_xcd, _cdiv(units, n_xcd)
    ustride = wg_per_xcd * waves
    counts, shares = [], []
    for x in range(n_xcd):
        lo = x * per_xcd
        share = max(0, min(lo + per_xcd, units) - lo)
        shares.append(share)
        for first in range(ustride):
            counts.append(_cdiv(share - first, ustride) if first < share else 0)
    return n_xcd, counts, shares


def _record(c, form):
    """The S2Launch the case's form must leave, from the shape and what the row names."""
    Hd, Wd, px = _geo(c)
    none = dict(entry='none', family='none', NB=0, NCH=0, MB=0, WAVES=0, pair=0, sums=0, workgroups=0, units=0, rounds=0, n_xcd=0,
                records=0)
    pair = 1 if c.kind == 'fwd' or 'pair' in form else 0
    sums = 1 if form in ('stats', 'sums', 'pair_sums') else 0
    entry = 'pair_fwd' if c.kind == 'fwd' else 'dgrad_s2'
    nb_out = (c.Co if c.kind == 'fwd' else c.Ci) // 16
    nch_in = (c.Ci if c.kind == 'fwd' else c.Co) // 16
    if c.family == 'resident':
        NB, NCH, MB, WAVES = _resident_inst(c)
        units = _cdiv(px, 16 * MB)
        wgs = c.wgs if c.wgs else _cdiv(units, WAVES)
        n_xcd, counts, _ = _walk(units, wgs, WAVES)
        return dict(entry=entry, family='resident', NB=NB, NCH=NCH, MB=MB, WAVES=WAVES, pair=pair, sums=sums, workgroups=wgs,
                    units=units, rounds=max(counts), n_xcd=n_xcd, records=wgs if sums else 0)
    if c.family == 'stream_lds':
        groups = _cdiv(px, 64)
        return dict(entry=entry, family='stream_lds', NB=nb_out, NCH=nch_in, MB=1, WAVES=4, pair=pair,
                    sums=sums if c.kind == 'fwd' else 0, workgroups=_cdiv(groups, 8) * 8 * nb_out, units=_cdiv(px, 16) * nb_out,
                    rounds=1, n_xcd=8, records=groups if (sums and c.kind == 'fwd') else 0)
    if c.family == 'stream':
        units = _cdiv(px, 32) * nb_out
        return dict(entry=entry, family='stream', NB=nb_out, NCH=nch_in, MB=2, WAVES=4, pair=pair, sums=0,
                    workgroups=_cdiv(units, 4), units=units, rounds=1, n_xcd=1, records=0)
    assert c.family == 'pair_1x1'
    if not pair:
        return none                                 # no shortcut term: the parity classes alone, none of the three entry points
    NB, R, BOTH = c.inst
    units = c.B * Hd * _cdiv(Wd, 16)
    return dict(entry='pair_1x1', family='pair_1x1', NB=NB, NCH=nch_in, MB=0, WAVES=R, pair=1 if BOTH else 0, sums=0,
                workgroups=_cdiv(units, 4) * (nb_out // NB), units=units, rounds=1, n_xcd=1, records=0)


def C(id, kind, B, Ci, Co, H, W, family, wgs=0, rounds=1, n_xcd=None, inst=None, patch=False):
    return Case(id, kind, B, Ci, Co, H, W, family, wgs, rounds, n_xcd, inst, patch)


# ---------------------------------------------------------------------------------------------------------------- the table
# edge shapes (B, H, W): the four H / W parities with B = 2 and Wd = 14 (units straddle rows and images), then 3x3, 2x2 (one
# pixel), one row, one column of three images -- all of 27 or fewer pixels but the first four
EDGES = [(2, 41, 27), (2, 41, 28), (2, 40, 27), (2, 40, 28), (1, 3, 3), (1, 2, 2), (1, 1, 5), (3, 6, 1)]
FWD_PAIRS = [(16, 32, 'resident'), (32, 64, 'resident'), (32, 48, 'stream_lds'), (64, 96, 'stream_lds')]        # Ci -> Co
DGRAD_PAIRS = [(16, 32, 'resident'), (32, 64, 'resident'), (48, 96, 'stream_lds'), (32, 32, 'stream_lds')]      # Ci <- Co
CASES = []
for _ci, _co, _fam in FWD_PAIRS:
    for _b, _h, _w in EDGES:
        CASES.append(C('f%dto%d_b%d_%dx%d' % (_ci, _co, _b, _h, _w), 'fwd', _b, _ci, _co, _h, _w, _fam,
                       n_xcd=1 if _fam == 'resident' else 8))
for _ci, _co, _fam in DGRAD_PAIRS:
    for _b, _h, _w in EDGES:
        CASES.append(C('d%dfrom%d_b%d_%dx%d' % (_ci, _co, _b, _h, _w), 'dgrad', _b, _ci, _co, _h, _w, _fam,
                       n_xcd=1 if _fam == 'resident' else 8))
CASES += [
    # one round on eight XCDs, the last XCD's share shorter: 125 units -> 16 each, 13 for XCD 7 (61 -> 8 each, 5)
    C('f16to32_xcd8', 'fwd', 1, 16, 32, 99, 79, 'resident', n_xcd=8),
    C('f32to64_xcd8', 'fwd', 1, 32, 64, 99, 79, 'resident', n_xcd=8),
    C('d16from32_xcd8', 'dgrad', 1, 16, 32, 121, 63, 'resident', n_xcd=8),
    C('d32from64_xcd8', 'dgrad', 1, 32, 64, 99, 79, 'resident', n_xcd=8),
    # the unit loop (workgroups as recorded on the first run on an MI355X: two per CU for the 4-wave kernels, one for the 8-wave)
    C('f16to32_loop', 'fwd', 8, 16, 32, 385, 130, 'resident', wgs=512, rounds=4, n_xcd=8),       # 6273 units: waves take 4 or 3
    C('f32to64_loop', 'fwd', 8, 32, 64, 129, 130, 'resident', wgs=256, rounds=2, n_xcd=8),       # 2113 units: waves take 2 or 1
    C('d16from32_loop', 'dgrad', 8, 16, 32, 385, 130, 'resident', wgs=512, rounds=2, n_xcd=8),   # 3137 units of 32 pixels
    C('d32from64_loop', 'dgrad', 8, 32, 64, 129, 130, 'resident', wgs=256, rounds=2, n_xcd=8),   # 2113 units of 16 pixels
    # the streaming data gradient with two pixel blocks per wave (cdiv(px, 16) * NB >= 8192), three channel blocks
    C('d48from32_stream', 'dgrad', 2, 48, 32, 299, 293, 'stream', n_xcd=1),
    # dam_conv1x1_pair_f32 behind shapes the one-launch kernel refuses by itself (Co % 32 != 0) ...
    C('p16from48', 'dgrad', 2, 16, 48, 9, 21, 'pair_1x1', n_xcd=1, inst=(1, 4, True)),
    C('p32from48', 'dgrad', 2, 32, 48, 10, 35, 'pair_1x1', n_xcd=1, inst=(2, 4, True)),
    C('p16from80', 'dgrad', 2, 16, 80, 9, 21, 'pair_1x1', n_xcd=1, inst=(1, 8, False)),          # one round, 5 of 8 chunks live
    C('p16from144', 'dgrad', 2, 16, 144, 7, 12, 'pair_1x1', n_xcd=1, inst=(1, 8, False)),        # last round: 1 of 8 chunks live
    C('p32from80', 'dgrad', 1, 32, 80, 6, 33, 'pair_1x1', n_xcd=1, inst=(2, 4, False)),          # last round: 1 of 4 chunks live
    # ... and behind the model's shapes with the one-launch kernel switched off
    C('p16from32_off', 'dgrad', 2, 16, 32, 9, 21, 'pair_1x1', n_xcd=1, inst=(1, 2, True), patch=True),
    C('p32from32_off', 'dgrad', 2, 32, 32, 9, 21, 'pair_1x1', n_xcd=1, inst=(2, 2, True), patch=True),
    C('p32from64_off', 'dgrad', 2, 32, 64, 10, 35, 'pair_1x1', n_xcd=1, inst=(2, 4, True), patch=True),
    C('p64from96_off', 'dgrad', 2, 64, 96, 7, 12, 'pair_1x1', n_xcd=1, inst=(2, 4, False), patch=True),
]
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}


def _forms(c):
    if c.kind == 'fwd':
        return FWD_FORMS
    if c.family == 'pair_1x1':
        return ('pair',) if c.patch else ('alone', 'pair')
    return DGRAD_FORMS


def _tags(c, form, rec):
    """What a launch contributes to the coverage: (instantiation, property) pairs."""
    if rec['entry'] == 'none':
        return set()
    if rec['family'] == 'pair_1x1':
        inst = ('pair_1x1', rec['NB'], rec['WAVES'], rec['pair'])
        live = rec['NCH'] - (_cdiv(rec['NCH'], rec['WAVES']) - 1) * rec['WAVES']       # live chunks of the last round
        return {(inst, 'ran'), (inst, 'refused' if not c.patch else 'switched_off'), (inst, 'last_round_live_%d' % live)}
    if rec['family'] == 'resident':
        inst = (rec['entry'], 'resident', rec['NB'], rec['NCH'], rec['MB'], rec['WAVES'], rec['pair'], rec['sums'])
        n_xcd, counts, shares = _walk(rec['units'], rec['workgroups'], rec['WAVES'])
        t = {(inst, 'rounds1' if rec['rounds'] == 1 else 'rounds2+'), (inst, 'xcd%d' % rec['n_xcd'])}
        if rec['rounds'] >= 3:
            t.add((inst, 'rounds3+'))
        live = [n for n in counts if n]
        if any(n % 2 for n in live) and any(n % 2 == 0 for n in live):
            t.add((inst, 'odd_and_even'))
        if n_xcd == 8 and min(shares) < max(shares):
            t.add((inst, 'xcd8_short_tail'))
        return t
    inst = (rec['entry'], rec['family'], rec['pair'], rec['sums'])
    _, _, px = _geo(c)
    t = {(inst, 'ran'), (inst, 'nb_odd' if rec['NB'] % 2 else 'nb_even')}
    if px % 64:
        t.add((inst, 'px_not_64'))
    return t


def _required():
    req = []
    for nb, nch, waves in ((2, 1, 4), (4, 2, 8)):                                  # conv_s2_pair_kernel <NB, NCH, STATS, WAVES>
        for stats in (0, 1):
            inst = ('pair_fwd', 'resident', nb, nch, 1, waves, 1, stats)
            req += [(inst, p) for p in ('rounds1', 'rounds2+', 'xcd1', 'xcd8', 'xcd8_short_tail')]
            if nch == 1:
                req += [(inst, 'rounds3+'), (inst, 'odd_and_even')]
    for stats in (0, 1):                                                           # conv_s2_pair_stream_kernel <STATS>
        req += [(('pair_fwd', 'stream_lds', 1, stats), p) for p in ('nb_odd', 'nb_even', 'px_not_64')]
    for nb, nch, mb, waves in ((1, 2, 2, 4), (2, 4, 1, 8)):                        # dgrad_s2_kernel <NB, NCH, MB, PAIR, WAVES, SUMS>
        for pair in (0, 1):
            for sums in (0, 1):
                inst = ('dgrad_s2', 'resident', nb, nch, mb, waves, pair, sums)
                req += [(inst, p) for p in ('rounds1', 'rounds2+', 'xcd1', 'xcd8')]
    for fam in ('stream_lds', 'stream'):                                           # dgrad_s2_stream_lds_kernel / _stream_kernel <PAIR>
        for pair in (0, 1):
            req.append((('dgrad_s2', fam, pair, 0), 'ran'))
    req += [(('dgrad_s2', 'stream_lds', 1, 0), 'nb_odd'), (('dgrad_s2', 'stream', 1, 0), 'nb_odd')]
    for nb in (1, 2):                                                              # conv1x1_pair_kernel <NB, R, BOTH>
        for r, both in ((2, 1), (4, 1), (4 if nb == 2 else 8, 0)):
            req.append((('pair_1x1', nb, r, both), 'ran'))
    req += [(('pair_1x1', 1, 4, 1), 'refused'), (('pair_1x1', 2, 4, 1), 'refused'), (('pair_1x1', 1, 8, 0), 'refused'),
            (('pair_1x1', 1, 8, 0), 'last_round_live_5'), (('pair_1x1', 1, 8, 0), 'last_round_live_1'),
            (('pair_1x1', 1, 2, 1), 'switched_off'), (('pair_1x1', 2, 4, 1), 'switched_off'), (('pair_1x1', 2, 4, 0), 'switched_off')]
    return req


REQUIRED = _required()


def test_table_conditions():
    """The arithmetic behind the table, on the CPU: the record every row's forms must leave covers REQUIRED; every row's rounds
    and n_xcd claim follows from its units and workgroups by the kernels' own unit walk; the loop rows have waves with odd and
    with even unit counts and a short last XCD; the small rows need no more workgroups than the chip has CUs (so the shape alone
    decides their grid); the streaming rows sit on the side of the MB threshold they name; the reference work stays bounded."""
    tags = set()
    for c in CASES:
        Hd, Wd, px = _geo(c)
        for form in _forms(c):
            rec = _record(c, form)
            tags |= _tags(c, form, rec)
            if rec['entry'] == 'none':
                continue
            assert rec['rounds'] == c.rounds and rec['n_xcd'] == c.n_xcd, (c.id, form, rec)
            if c.family == 'resident':
                n_xcd, counts, shares = _walk(rec['units'], rec['workgroups'], rec['WAVES'])
                assert sum(counts) == sum(shares) == rec['units'], c.id          # the walk takes every unit exactly once
                if not c.wgs:
                    assert rec['workgroups'] <= CUS and rec['rounds'] == 1, c.id
                else:
                    assert rec['workgroups'] in (CUS, 2 * CUS, 3 * CUS) and rec['units'] > rec['workgroups'] * rec['WAVES'], c.id
        flop = 2 * px * c.Co * c.Ci * 9
        assert flop <= 1.5e9, (c.id, flop)
        if c.kind == 'dgrad' and c.family in ('stream_lds', 'stream'):
            assert c.Co % 32 == 0 and c.Ci % 16 == 0 and (c.Co, c.Ci) not in ((32, 16), (64, 32)), c.id
            assert (_cdiv(px, 16) * (c.Ci // 16) >= 8192) == (c.family == 'stream'), c.id
        if c.kind == 'fwd' and c.family == 'stream_lds':
            assert c.Ci % 32 == 0 and c.Co % 16 == 0 and (c.Ci, c.Co) != (32, 64) and _cdiv(px, 64) <= BN_RECORDS_MAX, c.id
        if c.family == 'pair_1x1' and not c.patch:
            assert c.Co % 32 != 0 and c.Co % 16 == 0, c.id                         # what dam_dgrad_s2_3x3_f32 refuses
        if c.family == 'pair_1x1':
            nblk, nch = c.Ci // 16, c.Co // 16
            want = ((2, 2, True) if nch <= 2 else (2, 4, True) if nch <= 4 else (2, 4, False)) if nblk % 2 == 0 else \
                   ((1, 2, True) if nch <= 2 else (1, 4, True) if nch <= 4 else (1, 8, False))
            assert c.inst == want, c.id
    lacking = [r for r in REQUIRED if r not in tags]
    assert not lacking, lacking
    # the edge shapes: every H / W parity, B >= 2 with Wd no multiple of 16, fewer pixels than one unit, single rows and columns
    for ci, co, _ in FWD_PAIRS + DGRAD_PAIRS:
        assert {(h % 2, w % 2) for b, h, w in EDGES if b >= 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(((w + 1) // 2) % 16 for b, h, w in EDGES if b >= 2)
    assert {(1, 3, 3), (1, 2, 2), (1, 1, 5), (3, 6, 1)} <= set(EDGES)
    assert any(b * ((h + 1) // 2) * ((w + 1) // 2) < 16 for b, h, w in EDGES)


# --------------------------------------------------------------------------------------------------------- inputs, oracle
@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    torch.set_num_threads(16)
    return ops


def _seed(c):
    return 5000 + [k.id for k in CASES].index(c.id)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _guarded(shape):
    """A result tensor in the middle of a buffer with GUARD elements of FILL on both sides (the result itself FILL too)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((2 * GUARD + numel,), FILL, dtype=torch.int32, device='cuda')
    return buf, buf.view(torch.float32)[GUARD:GUARD + numel].view(shape)


def _bands_intact(buf, what, written=None):
    """Both guard bands bit for bit; with `written`, everything of the payload behind its first `written` elements as well."""
    host = buf.cpu()
    assert bool((host[:GUARD] == FILL).all()) and bool((host[-GUARD:] == FILL).all()), '%s: guard band written' % what
    if written is not None:
        assert bool((host[GUARD + written:] == FILL).all()), '%s: written behind record %d' % (what, written)


SEEN = {}           # (case id, form) -> record as a dict
WORST = {}          # (family, write-out) -> (error relative to its bound's scale, case id, form)
FINALIZED = set()   # instantiations whose records went through bn_finalize_pair


def _note(fam, what, err, c, form):
    if err > WORST.get((fam, what), (-1.0,))[0]:
        WORST[(fam, what)] = (err, c.id, form)


def _plan(ops, c, form, **device):
    """The plan of the launch whose record (c, form) leaves, from the plan entry of the entry point that leaves it.  device:
    cus=, resident= (tests/test_s2_plan_cpu.py: no GPU asked); neither: the current device's, as the launching entry takes them."""
    if c.kind == 'fwd':
        return ops.conv_s2_pair_fwd_plan((c.B, c.H, c.W, c.Ci), c.Co, stats=form == 'stats', **device)
    Hd, Wd, _ = _geo(c)
    dy_shape, pair = (c.B, Hd, Wd, c.Co), 'pair' in form
    if not c.patch:                                     # (patch: dam_dgrad_s2_3x3_f32 is not asked)
        one = ops.conv2d_dgrad_s2_plan(dy_shape, c.Ci, c.H, c.W, pair=pair, sums='sums' in form, **device)
        if c.family != 'pair_1x1':
            return one
        assert one.entry == 'none', '%s %s: dam_dgrad_s2_3x3_f32 would take a row named pair_1x1: %s' % (c.id, form, one)
    # the parity classes: class (0, 0) rides in the 1x1 pair launch where there is a shortcut term, else none of the three entries runs
    return ops.conv1x1_pair_plan(dy_shape, c.Ci, c.H, c.W) if pair else ops.S2Launch('none', 'none', *([0] * 11))


def _assert_record(ops, c, form):
    rec = ops.s2_last_launch()._asdict()
    want = _record(c, form)
    SEEN[(c.id, form)] = rec
    assert rec == want, '%s %s: launched %s, the row names %s' % (c.id, form, rec, want)
    plan = _plan(ops, c, form)._asdict()
    assert rec == plan, '%s %s: launched %s, the plan of the same call is %s' % (c.id, form, rec, plan)
    return rec


def _fwd_inputs(c):
    """x = 3 z + 7 per element (|mean| of an output channel is 7 |sum w| against a deviation of 3 |w|: a sum-of-squares shortcut
    fails), weights random around a small positive mean (so that most channels' sum w is away from zero)."""
    g = torch.Generator().manual_seed(_seed(c))
    x = torch.randn(c.B, c.Ci, c.H, c.W, generator=g) * 3 + 7
    w = (torch.randn(c.Co, c.Ci, 3, 3, generator=g) + 0.5) / (c.Ci * 9) ** 0.5
    wsc = (torch.randn(c.Co, c.Ci, 1, 1, generator=g) + 0.5) / c.Ci ** 0.5
    return x, w, wsc


def _fwd_oracle(x, w, wsc):
    return F.conv2d(x.double(), w.double(), None, 2, 1), F.conv2d(x.double(), wsc.double(), None, 2, 0)


def _merge_records(rec, parts, Co, npx, what):
    """Chan's merge of the records [parts][Co][3] = (n, mean, M2) in float64 -> mean, biased variance; the counts add up to the
    tensor's pixels exactly, no M2 is negative (records with n = 0 -- workgroups or waves without pixels -- are legal)."""
    r = rec[:parts * Co * 3].view(parts, Co, 3).double().cpu()
    n, mean, m2 = torch.zeros(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
    assert bool((r[:, :, 0] >= 0).all()) and bool((r[:, :, 2] >= 0).all()), '%s: a negative count or M2' % what
    for p in range(parts):
        nb, nn = r[p, :, 0], n + r[p, :, 0]
        rr = torch.where(nn > 0, nb / nn.clamp(min=1), torch.zeros_like(nn))
        d = r[p, :, 1] - mean
        mean = mean + d * rr
        m2 = m2 + r[p, :, 2] + d * d * n * rr
        n = nn
    assert torch.equal(n, torch.full((Co,), float(npx), dtype=torch.float64)), '%s: the counts add up to %s, not %d' % (what, n.tolist(), npx)
    return mean, m2 / npx


def _check_stats(mean, var_or_invstd, want, c, form, fam, is_invstd=False):
    var64, mu64 = torch.var_mean(want, dim=(0, 2, 3), unbiased=False)
    e_mean = ((mean.double().cpu() - mu64).abs().max() / mu64.abs().max()).item()
    inv64 = 1.0 / torch.sqrt(var64 + EPS)
    inv = var_or_invstd.double().cpu() if is_invstd else 1.0 / torch.sqrt(var_or_invstd + EPS)
    e_inv = ((inv - inv64).abs() / inv64).max().item()
    _note(fam, 'mean', e_mean, c, form), _note(fam, 'invstd', e_inv, c, form)
    assert e_mean <= TOL_MEAN, '%s %s: merged mean off by %.3g of the scale' % (c.id, form, e_mean)
    assert e_inv <= TOL_INVSTD, '%s %s: merged invstd off by %.3g' % (c.id, form, e_inv)


def _check_out(got, want, c, form, fam, what):
    scale = want.abs().max().item()
    err = (got.double().cpu() - want).abs()
    worst = err.max().item() / scale
    where = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
    _note(fam, what, worst, c, form)
    print('%s %s %s: err %.2e of scale %.3g at [b, c, h, w] = %s' % (c.id, form, what, worst, scale, where))
    assert worst <= TOL_OUT, '%s %s %s: err %.3g of the scale at [b, c, h, w] = %s (%d elements over)' % (
        c.id, form, what, worst, where, int((err > TOL_OUT * scale).sum()))


def _launch_fwd(ops, c, form, xd, wp, wps):
    Hd, Wd, px = _geo(c)
    n_rec = ops._lib.lib().dam_bn_workspace_floats(c.Co)
    bufs = [_guarded((c.B, Hd, Wd, c.Co)), _guarded((c.B, Hd, Wd, c.Co))]
    kw = dict(out=(bufs[0][1], bufs[1][1]))
    if form == 'stats':
        bufs += [_guarded((n_rec,)), _guarded((n_rec,))]
        kw['records'] = (bufs[2][1], bufs[3][1])
    got = ops.conv_s2_pair_fwd(xd, wp, wps, c.Co, stats=form == 'stats', **kw)
    rec = _assert_record(ops, c, form)
    assert got is not None
    torch.cuda.synchronize()
    parts = got[2][2] if form == 'stats' else 0
    assert (got[2] is None) == (form != 'stats') and parts == rec['records']
    for i, (buf, _) in enumerate(bufs):
        _bands_intact(buf, '%s %s buffer %d' % (c.id, form, i), written=parts * c.Co * 3 if i >= 2 else None)
    return got, rec


def _check_fwd(ops, c):
    x, w, wsc = _fwd_inputs(c)
    want1, wants = _fwd_oracle(x, w, wsc)
    Hd, Wd, px = _geo(c)
    for want in (want1, wants):
        var, mu = torch.var_mean(want, dim=(0, 2, 3), unbiased=False)
        assert px == 1 or int((mu.abs() >= var.sqrt()).sum()) * 2 >= c.Co, '%s: |mean| >= std on fewer than half the channels' % c.id
    xd, wp, wps = _nhwc(x).cuda(), ops.pack_weights(w.cuda()), ops.pack_weights(wsc.cuda())
    (c1, cs, (p1, p2, parts)), rec = _launch_fwd(ops, c, 'stats', xd, wp, wps)
    fam = 'fwd ' + rec['family']
    _check_out(c1.permute(0, 3, 1, 2), want1, c, 'stats', fam, 'c1')
    _check_out(cs.permute(0, 3, 1, 2), wants, c, 'stats', fam, 'cs')
    for p, want, name in ((p1, want1, 'conv1'), (p2, wants, 'shortcut')):
        mean, var = _merge_records(p, parts, c.Co, px, '%s %s records' % (c.id, name))
        _check_stats(mean, var, want, c, 'stats', fam)
    inst = (rec['family'], rec['NB'], rec['NCH'], rec['WAVES'], rec['rounds'] > 1)
    if inst not in FINALIZED:                           # the records through the launch that consumes them, once per instantiation
        FINALIZED.add(inst)
        mk = lambda: (torch.ones(c.Co).cuda(), torch.zeros(c.Co).cuda(), torch.zeros(c.Co).cuda(), torch.ones(c.Co).cuda(),
                      torch.zeros((), dtype=torch.int64).cuda(), 0.1, EPS)
        sa, sb = ops.bn_finalize_pair(p1, p2, parts, mk(), mk())
        for (mean, invstd, _, _), want in ((sa, want1), (sb, wants)):
            _check_stats(mean, invstd, want, c, 'stats', fam + ' finalize', is_invstd=True)
    (c1b, csb, none), recb = _launch_fwd(ops, c, 'nostats', xd, wp, wps)
    assert none is None
    assert torch.equal(c1b, c1) and torch.equal(csb, cs), '%s: the outputs without statistics are not bitwise those with' % c.id


def _dgrad_inputs(c):
    """Weights random (no symmetry), dy / ds i.i.d.; the upstream block's u, mean, invstd; its output's sign bytes from a random
    float64 y with |y| >= 0.1 (float32 and float64 cannot disagree on a bit)."""
    g = torch.Generator().manual_seed(_seed(c))
    Hd, Wd, px = _geo(c)
    w = torch.randn(c.Co, c.Ci, 3, 3, generator=g) / (c.Ci * 9) ** 0.5
    wsc = torch.randn(c.Co, c.Ci, 1, 1, generator=g) / c.Ci ** 0.5
    dy, ds = torch.randn(c.B, c.Co, Hd, Wd, generator=g), torch.randn(c.B, c.Co, Hd, Wd, generator=g)
    u = torch.randn(c.B, c.Ci, c.H, c.W, generator=g) * 1.5 + 0.4
    mean, invstd = torch.randn(c.Ci, generator=g) * 0.3, torch.rand(c.Ci, generator=g) + 0.5
    y = torch.randn(c.B, c.Ci, c.H, c.W, generator=g, dtype=torch.float64)
    y = y + 0.1 * torch.sign(y)
    mask = y > 0                                                    # [B, Ci, H, W]
    assert bool((y.abs() >= 0.1).all())
    share = mask.double().mean().item()
    assert mask.numel() < 64 or 0.25 <= share <= 0.75, (c.id, share)
    m = mask.permute(0, 2, 3, 1).reshape(c.B, c.H, c.W, c.Ci // 4, 4).to(torch.uint8)
    bits = (m[..., 0] | (m[..., 1] << 1) | (m[..., 2] << 2) | (m[..., 3] << 3)).contiguous()     # bit i of byte q: channel 4 q + i
    return w, wsc, dy, ds, u, mean, invstd, mask, bits


def _dgrad_oracle(c, w, wsc, dy, ds, u, mean, invstd, mask):
    """form -> float64 dx; form -> float64 (sum dz, sum dz * uhat, sum |dz|, sum |dz * uhat|) from the REFERENCE dx."""
    shape = (c.B, c.Ci, c.H, c.W)
    alone = torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), 2, 1, 1)
    dx = {'alone': alone, 'pair': alone + torch.nn.grad.conv2d_input(shape, wsc.double(), ds.double(), 2, 0, 1)}
    uhat = (u.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
    sums = {}
    for form in ('alone', 'pair'):
        dz = dx[form] * mask
        t2 = dz * uhat
        sums[form] = (dz.sum((0, 2, 3)), t2.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), t2.abs().sum((0, 2, 3)))
    return dx, sums


def _of_terms(diff, terms):
    """max over the channels of |diff| / sum |term|; a channel without a term (every pixel masked) must be exactly 0."""
    err = diff.abs()
    ratio = torch.where(terms > 0, err / terms.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return ratio.max().item()


def _launch_dgrad(ops, c, form, dev):
    dyd, dsd, wpt, wpst, ud, md, isd, bitsd = dev
    buf, out = _guarded((c.B, c.H, c.W, c.Ci))
    kw = dict(out=out)
    if 'pair' in form:
        kw['pair_1x1'] = (dsd, wpst)
    rbuf = None
    if 'sums' in form:
        rbuf, records = _guarded((ops._lib.lib().dam_bn_workspace_floats(c.Ci),))
        kw.update(bn_bwd=(ud, md, isd, None, None, bitsd), records=records)
    taken = ops.dgrad_s2_launches
    got = ops.conv2d_dgrad(dyd, wpt, c.Ci, c.H, c.W, 3, 3, 2, 1, 1, **kw)
    rec = _assert_record(ops, c, form)
    assert ops.dgrad_s2_launches == taken + (0 if c.family == 'pair_1x1' else 1), '%s %s: dgrad_s2_launches' % (c.id, form)
    torch.cuda.synchronize()
    dx, sums = got if 'sums' in form else (got, None)
    assert dx.data_ptr() == out.data_ptr()
    _bands_intact(buf, '%s %s dx' % (c.id, form))
    if rbuf is not None:
        assert (sums is None) == (rec['records'] == 0) and (sums is None or sums[1] == rec['records'])
        _bands_intact(rbuf, '%s %s records' % (c.id, form), written=rec['records'] * c.Ci * 2)
    return dx, sums, rec


def _check_dgrad(ops, c, monkeypatch):
    w, wsc, dy, ds, u, mean, invstd, mask, bits = _dgrad_inputs(c)
    want_dx, want_sums = _dgrad_oracle(c, w, wsc, dy, ds, u, mean, invstd, mask)
    dev = (_nhwc(dy).cuda(), _nhwc(ds).cuda(), ops.pack_weights(w.cuda(), transpose=True), ops.pack_weights(wsc.cuda(), transpose=True),
           _nhwc(u).cuda(), mean.cuda(), invstd.cuda(), bits.cuda())
    assert ops.DGRAD_S2
    if c.patch:
        monkeypatch.setattr(ops, 'DGRAD_S2', False)
    plain = {}
    for form in _forms(c):
        dx, sums, rec = _launch_dgrad(ops, c, form, dev)
        base = 'pair' if 'pair' in form else 'alone'
        fam = 'dgrad ' + (rec['family'] if rec['entry'] != 'none' else 'parity classes')
        _check_out(dx.permute(0, 3, 1, 2), want_dx[base], c, form, fam, 'dx')
        if 'sums' not in form:
            plain[base] = (dx, rec)
            continue
        same = {k: v for k, v in rec.items() if k not in ('sums', 'records')} == \
               {k: v for k, v in plain[base][1].items() if k not in ('sums', 'records')}
        assert not same or torch.equal(dx, plain[base][0]), '%s %s: dx differs from the launch without the sums' % (c.id, form)
        if c.family != 'resident':
            assert sums is None, '%s %s: a streaming kernel reported sums' % (c.id, form)
            continue
        records, parts = sums
        r = records[:parts * c.Ci * 2].view(parts, c.Ci, 2).double().sum(0).cpu()
        s1, s2, a1, a2 = want_sums[base]
        e1, e2 = _of_terms(r[:, 0] - s1, a1), _of_terms(r[:, 1] - s2, a2)
        _note(fam, 'sum dz', e1, c, form), _note(fam, 'sum dz uhat', e2, c, form)
        print('%s %s sums: %.2e, %.2e of the channel\'s sum |term|' % (c.id, form, e1, e2))
        assert e1 <= TOL_SUMS and e2 <= TOL_SUMS, '%s %s: sums off by %.3g, %.3g of sum |term|' % (c.id, form, e1, e2)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_s2_kernel(ops, monkeypatch, case):
    if case.kind == 'fwd':
        _check_fwd(ops, case)
    else:
        _check_dgrad(ops, case, monkeypatch)


# ------------------------------------------------------------------------------------------------------------------ retreats
def _fwd_retreat_inputs(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 32, H, W, generator=g) * 3 + 7
    w = (torch.randn(16, 32, 3, 3, generator=g) + 0.5) / (32 * 9) ** 0.5
    wsc = (torch.randn(16, 32, 1, 1, generator=g) + 0.5) / 32 ** 0.5
    return x, w, wsc


@pytest.mark.gpu
def test_retreat_forward_stream_statistics_at_the_record_limit(ops):
    """(2, 32 -> 16, 511, 512): 131 072 output pixels = exactly BN_RECORDS_MAX groups of 64: the streaming kernel writes 2048
    records."""
    c = C('retreat_2048', 'fwd', 2, 32, 16, 511, 512, 'stream_lds', n_xcd=8)
    assert _cdiv(_geo(c)[2], 64) == BN_RECORDS_MAX
    x, w, wsc = _fwd_retreat_inputs(c.H, c.W, 6001)
    want1, wants = _fwd_oracle(x, w, wsc)
    (c1, cs, (p1, p2, parts)), rec = _launch_fwd(ops, c, 'stats', _nhwc(x).cuda(), ops.pack_weights(w.cuda()), ops.pack_weights(wsc.cuda()))
    assert parts == BN_RECORDS_MAX
    _check_out(c1.permute(0, 3, 1, 2), want1, c, 'stats', 'fwd stream_lds', 'c1')
    _check_out(cs.permute(0, 3, 1, 2), wants, c, 'stats', 'fwd stream_lds', 'cs')
    for p, want, name in ((p1, want1, 'conv1'), (p2, wants, 'shortcut')):
        mean, var = _merge_records(p, parts, c.Co, _geo(c)[2], '%s %s records' % (c.id, name))
        _check_stats(mean, var, want, c, 'stats', 'fwd stream_lds')


@pytest.mark.gpu
def test_retreat_forward_stream_statistics_past_the_record_limit(ops):
    """(2, 32 -> 16, 513, 512): 2056 groups.  With statistics the entry point refuses (conv_s2_pair_fwd returns None, no record,
    every buffer keeps its fill pattern); without, the same shape runs and is right."""
    c = C('retreat_2056', 'fwd', 2, 32, 16, 513, 512, 'stream_lds', n_xcd=8)
    Hd, Wd, px = _geo(c)
    assert _cdiv(px, 64) == 2056 > BN_RECORDS_MAX
    x, w, wsc = _fwd_retreat_inputs(c.H, c.W, 6002)
    xd, wp, wps = _nhwc(x).cuda(), ops.pack_weights(w.cuda()), ops.pack_weights(wsc.cuda())
    n_rec = ops._lib.lib().dam_bn_workspace_floats(c.Co)
    bufs = [_guarded((c.B, Hd, Wd, c.Co)), _guarded((c.B, Hd, Wd, c.Co)), _guarded((n_rec,)), _guarded((n_rec,))]
    got = ops.conv_s2_pair_fwd(xd, wp, wps, c.Co, out=(bufs[0][1], bufs[1][1]), records=(bufs[2][1], bufs[3][1]))
    assert got is None and ops.s2_last_launch().entry == 'none', (got, ops.s2_last_launch())
    assert ops.s2_last_launch() == _plan(ops, c, 'stats')             # the refusal is the plan's
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert bool((buf == FILL).all()), 'a refused call wrote'
    want1, wants = _fwd_oracle(x, w, wsc)
    (c1, cs, none), rec = _launch_fwd(ops, c, 'nostats', xd, wp, wps)
    assert none is None
    _check_out(c1.permute(0, 3, 1, 2), want1, c, 'nostats', 'fwd stream_lds', 'c1')
    _check_out(cs.permute(0, 3, 1, 2), wants, c, 'nostats', 'fwd stream_lds', 'cs')


@pytest.mark.gpu
def test_retreat_block_forward_takes_the_separate_launches(ops):
    """One BasicBlock (32 -> 16, stride 2) in training mode at a shape the one-launch forward refuses ((2, 657, 400): 2057 groups
    of 64 output pixels): layers.py runs the two convolutions and the pair statistics as separate launches -- against the
    float64 block of the oracle, running statistics included.  (Rows of 480 and more pixels are no such shape: there
    dam_conv2d_tapgrid_f32 itself refuses the 3x3 / stride-2 convolution and the block raises.)"""
    from deep_audio_mixer_amd import layers
    from oracle import models_ref
    g = torch.Generator().manual_seed(6003)
    blk = layers.BasicBlock(32, 16, 2)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / m.weight[0].numel()) ** 0.5)
    ref = models_ref.RefBasicBlock(32, 16, 2).double().train()
    ref.load_state_dict({k: v.double() for k, v in blk.state_dict().items()})
    blk = blk.cuda().train()
    x = torch.relu(torch.randn((2, 657, 400, 32), generator=g))
    assert _cdiv(2 * 329 * 200, 64) > BN_RECORDS_MAX
    ops.conv_s2_pair_fwd(torch.zeros(1, 2, 2, 16, device='cuda'), ops.pack_weights(torch.zeros(32, 16, 3, 3, device='cuda')),
                         ops.pack_weights(torch.zeros(32, 16, 1, 1, device='cuda')), 32)
    assert ops.s2_last_launch().entry == 'pair_fwd'                    # a record the block's refused call must clear
    with torch.no_grad():
        out = blk(x.cuda())
        want = ref(x.permute(0, 3, 1, 2).double())
    assert ops.s2_last_launch().entry == 'none', ops.s2_last_launch()
    assert ops.s2_last_launch() == ops.conv_s2_pair_fwd_plan((2, 657, 400, 32), 16)
    err = float((out.permute(0, 3, 1, 2).double().cpu() - want).norm() / want.norm())
    print('block forward: %.2e of the norm' % err)
    assert err <= TOL_BLOCK, err
    for a, b in ((blk.bn1, ref.bn1), (blk.shortcut[1], ref.shortcut[1])):
        torch.testing.assert_close(a.running_mean.double().cpu(), b.running_mean, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(a.running_var.double().cpu(), b.running_var, rtol=1e-5, atol=0)


@pytest.mark.gpu
def test_retreat_strided_bn_bwd_on_a_refused_shape(ops):
    """bn_bwd at stride 2 on a shape the one-launch data gradient refuses (Co = 48): (dx, None), dx right, the record buffer
    untouched, the 1x1 pair launch recorded."""
    c = BY_ID['p16from48']
    w, wsc, dy, ds, u, mean, invstd, mask, bits = _dgrad_inputs(c)
    want_dx, _ = _dgrad_oracle(c, w, wsc, dy, ds, u, mean, invstd, mask)
    dev = (_nhwc(dy).cuda(), _nhwc(ds).cuda(), ops.pack_weights(w.cuda(), transpose=True), ops.pack_weights(wsc.cuda(), transpose=True),
           _nhwc(u).cuda(), mean.cuda(), invstd.cuda(), bits.cuda())
    for form in ('sums', 'pair_sums'):
        dx, sums, rec = _launch_dgrad(ops, c, form, dev)
        assert sums is None
        _check_out(dx.permute(0, 3, 1, 2), want_dx['pair' if 'pair' in form else 'alone'], c, form, 'dgrad parity classes', 'dx')


@pytest.mark.gpu
def test_out_and_records_are_validated(ops):
    """conv_s2_pair_fwd(out=, records=) and conv2d_dgrad(records=) refuse a wrong shape, dtype, layout, size or device."""
    x = torch.zeros(1, 4, 4, 16, device='cuda')
    wp, wps = ops.pack_weights(torch.zeros(32, 16, 3, 3, device='cuda')), ops.pack_weights(torch.zeros(32, 16, 1, 1, device='cuda'))
    good = lambda: torch.empty(1, 2, 2, 32, device='cuda')
    n = ops._lib.lib().dam_bn_workspace_floats(32)
    for bad in ((good(), torch.empty(1, 2, 2, 16, device='cuda')), (good(), good().double()), (good(), good().cpu()), (good(),),
                (good(), torch.empty(1, 2, 2, 64, device='cuda')[..., ::2])):
        with pytest.raises(ValueError):
            ops.conv_s2_pair_fwd(x, wp, wps, 32, out=bad)
    for bad in ((torch.empty(n, device='cuda'), torch.empty(n - 1, device='cuda')), (torch.empty(n, device='cuda'), torch.empty(n)),
                (torch.empty(n, device='cuda'), torch.empty(n, device='cuda', dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.conv_s2_pair_fwd(x, wp, wps, 32, records=bad)
    with pytest.raises(ValueError):
        ops.conv_s2_pair_fwd(x, wp, wps, 32, stats=False, records=(torch.empty(n, device='cuda'), torch.empty(n, device='cuda')))
    dy = torch.zeros(1, 2, 2, 32, device='cuda')
    wpt = ops.pack_weights(torch.zeros(32, 16, 3, 3, device='cuda'), transpose=True)
    n16 = ops._lib.lib().dam_bn_workspace_floats(16)
    with pytest.raises(ValueError):
        ops.conv2d_dgrad(dy, wpt, 16, 4, 4, 3, 3, 2, 1, 1, records=torch.empty(n16, device='cuda'))          # no bn_bwd
    bn = (x, torch.zeros(16, device='cuda'), torch.ones(16, device='cuda'), None, None, torch.zeros(1, 4, 4, 4, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.conv2d_dgrad(dy, wpt, 16, 4, 4, 3, 3, 2, 1, 1, bn_bwd=bn, records=torch.empty(n16 - 1, device='cuda'))


@pytest.mark.gpu
def test_coverage(ops, monkeypatch):
    """The union of the launches the table made covers REQUIRED.  (Cases that did not run in this process -- a -k selection --
    are launched here without their oracle, so the test stands on its own.)"""
    for c in CASES:
        missing = [f for f in _forms(c) if (c.id, f) not in SEEN]
        if not missing:
            continue
        if c.kind == 'fwd':
            x, w, wsc = _fwd_inputs(c)
            xd, wp, wps = _nhwc(x).cuda(), ops.pack_weights(w.cuda()), ops.pack_weights(wsc.cuda())
            for f in missing:
                _launch_fwd(ops, c, f, xd, wp, wps)
        else:
            w, wsc, dy, ds, u, mean, invstd, mask, bits = _dgrad_inputs(c)
            dev = (_nhwc(dy).cuda(), _nhwc(ds).cuda(), ops.pack_weights(w.cuda(), transpose=True),
                   ops.pack_weights(wsc.cuda(), transpose=True), _nhwc(u).cuda(), mean.cuda(), invstd.cuda(), bits.cuda())
            with monkeypatch.context() as m:
                if c.patch:
                    m.setattr(ops, 'DGRAD_S2', False)
                for f in missing:
                    _launch_dgrad(ops, c, f, dev)
    torch.cuda.synchronize()
    tags = set()
    for (cid, form), rec in SEEN.items():
        if cid in BY_ID:                                # (the retreat tests' shapes are not rows of the table)
            tags |= _tags(BY_ID[cid], form, rec)
    for key in sorted(WORST):
        print('worst error, %s / %s: %.2e (%s, %s)' % (key + WORST[key]))
    lacking = [r for r in REQUIRED if r not in tags]
    assert not lacking, 'launches no case made: %s' % lacking
