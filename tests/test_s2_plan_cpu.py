"""CPU: which kernel the three entry points of a down-sampling block (dam_conv_s2_pair_fwd_f32, dam_dgrad_s2_3x3_f32,
dam_conv1x1_pair_f32) give a layer, asked from their plan entries (ops.conv_s2_pair_fwd_plan, ops.conv2d_dgrad_s2_plan,
ops.conv1x1_pair_plan) without a GPU: the CU count and the occupancy answer, the only two things the decision takes from the
device, are arguments here.

The case table of tests/test_s2_kernels_gpu.py names, per (case, form), the whole record the launch must leave in
ops.s2_last_launch(); it passed on the device (256 CUs) before the dispatch became a plan, so agreement with it is agreement with
that dispatch.  Here every pair of the table is planned and compared with the same _record() -- no pair is skipped, the count is
asserted -- once with 2 and once with 3 resident workgroups per CU (the pinned grids do not depend on which), and the file's
REQUIRED coverage is asserted from the planned records.  The GPU tests assert the other half: the record a launch leaves equals
the plan of the same call.

Also here, each host arithmetic without a tensor: the occupancy answer as an input (the two grids the device gave the forward
at (8, 16 -> 32, 1025, 130)); the retreats of the GPU file and the refusals no test could reach with tensors (the 2^26 / 2^30
pixel limits, the 2 GiB byte offsets, the record limits of both persistent kernels, a CU count that is no multiple of 8); the
argument errors of the launching entries, with the same status."""
import ctypes

import pytest

import test_s2_kernels_gpu as sk

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
CUS = sk.CUS
NONE = dict(entry='none', family='none', NB=0, NCH=0, MB=0, WAVES=0, pair=0, sums=0, workgroups=0, units=0, rounds=0, n_xcd=0,
            records=0)
BN_BWD_RECORDS_MAX = 1024           # dam_common.h


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _dy_shape(c):
    Hd, Wd, _ = sk._geo(c)
    return (c.B, Hd, Wd, c.Co)


@pytest.mark.parametrize('resident', [2, 3])
def test_table(ops, resident):
    """Every (case, form) of tests/test_s2_kernels_gpu.py, all 13 fields; then REQUIRED from the planned records alone."""
    planned = {}
    for c in sk.CASES:
        for form in sk._forms(c):
            rec = planned[(c.id, form)] = sk._plan(ops, c, form, cus=CUS, resident=resident)._asdict()
            want = sk._record(c, form)
            assert rec == want, '%s %s: planned %s, the row names %s' % (c.id, form, rec, want)
    assert len(planned) == sum(len(sk._forms(c)) for c in sk.CASES) == 234
    tags = set()
    for (cid, form), rec in planned.items():
        tags |= sk._tags(sk.BY_ID[cid], form, rec)
    lacking = [r for r in sk.REQUIRED if r not in tags]
    assert not lacking, 'launches no case plans: %s' % lacking


def test_refused_rows_take_the_1x1_pair(ops):
    """Co = 48, 80, 144: 'none' from the one-launch data gradient in every form, the named <NB, R, BOTH> from the 1x1 plan; the
    model's shapes (patch rows) would take the one-launch kernel, and their 1x1 plan is what runs with it switched off."""
    for c in sk.CASES:
        if c.family != 'pair_1x1':
            continue
        for pair in (False, True):
            for sums in (False, True):
                one = ops.conv2d_dgrad_s2_plan(_dy_shape(c), c.Ci, c.H, c.W, pair=pair, sums=sums, cus=CUS, resident=2)
                assert (one.entry == 'none') == (not c.patch), (c.id, one)
        rec = ops.conv1x1_pair_plan(_dy_shape(c), c.Ci, c.H, c.W)
        assert (rec.entry, rec.family, rec.NB, rec.WAVES, bool(rec.pair)) == ('pair_1x1', 'pair_1x1') + c.inst, (c.id, rec)


def test_occupancy_is_an_input(ops):
    """The forward at (8, 16 -> 32, 1025, 130), 16 673 units: 2 workgroups per CU give 512 workgroups and 9 rounds, 3 give 768 and
    6 -- the two launches the device made with and without statistics (docstring of tests/test_s2_kernels_gpu.py)."""
    two = ops.conv_s2_pair_fwd_plan((8, 1025, 130, 16), 32, cus=CUS, resident=2)
    three = ops.conv_s2_pair_fwd_plan((8, 1025, 130, 16), 32, cus=CUS, resident=3)
    assert two.units == three.units == 16673
    assert (two.workgroups, two.rounds, two.n_xcd, two.records) == (512, 9, 8, 512), two
    assert (three.workgroups, three.rounds, three.n_xcd, three.records) == (768, 6, 8, 768), three
    # more than three per CU are never used; the 8-wave kernel takes one whatever the answer
    assert ops.conv_s2_pair_fwd_plan((8, 1025, 130, 16), 32, cus=CUS, resident=7) == three
    assert {ops.conv_s2_pair_fwd_plan((8, 513, 65, 32), 64, cus=CUS, resident=r).workgroups for r in (1, 2, 3)} == {CUS}
    # (8, 16 <- 32, 1025, 130), the data gradient's loop case of tests/test_conv_gpu.py: 768 workgroups, rounds 3
    d = ops.conv2d_dgrad_s2_plan((8, 513, 65, 32), 16, 1025, 130, cus=CUS, resident=3)
    assert (d.family, d.MB, d.workgroups, d.rounds, d.n_xcd) == ('resident', 2, 768, 3, 8), d


def test_forward_stream_record_limit(ops):
    """The shapes of the two test_retreat_forward_stream_* tests: exactly 2048 groups of 64 pixels plan 2048 records; 2056 groups
    plan 'none' with statistics and a launch without."""
    at = ops.conv_s2_pair_fwd_plan((2, 511, 512, 32), 16, cus=CUS, resident=2)
    assert at._asdict() == sk._record(sk.C('retreat_2048', 'fwd', 2, 32, 16, 511, 512, 'stream_lds', n_xcd=8), 'stats')
    assert at.records == sk.BN_RECORDS_MAX == 2048
    past = sk.C('retreat_2056', 'fwd', 2, 32, 16, 513, 512, 'stream_lds', n_xcd=8)
    assert ops.conv_s2_pair_fwd_plan((2, 513, 512, 32), 16, cus=CUS, resident=2)._asdict() == NONE
    assert ops.conv_s2_pair_fwd_plan((2, 513, 512, 32), 16, stats=False, cus=CUS, resident=2)._asdict() == sk._record(past, 'nostats')
    # the block of test_retreat_block_forward_takes_the_separate_launches: 2057 groups
    assert ops.conv_s2_pair_fwd_plan((2, 657, 400, 32), 16, cus=CUS, resident=2).entry == 'none'


def test_size_limits(ops):
    """The pixel-count and 2 GiB byte-offset refusals of the three entries, and the largest shapes in front of them."""
    fwd = lambda shape, co, **kw: ops.conv_s2_pair_fwd_plan(shape, co, stats=False, cus=CUS, resident=2, **kw).entry
    # forward: x of 2^31 bytes (resident: 16 channels; streaming: 32)
    assert fwd((1, 4096, 8192, 16), 32) == 'none' and fwd((1, 4096, 8191, 16), 32) == 'pair_fwd'
    assert fwd((1, 4096, 4096, 32), 16) == 'none' and fwd((1, 4096, 4095, 32), 16) == 'pair_fwd'
    # forward: 2^26 output pixels (x is 2^34 bytes by then: the byte limit is the one that binds)
    assert fwd((16, 4096, 4096, 16), 32) == 'none' and fwd((16, 4096, 4096, 32), 16) == 'none'
    # forward, streaming: weight images of 2^31 bytes
    assert fwd((1, 4, 4, 8192), 8192) == 'none' and fwd((1, 4, 4, 4096), 4096) == 'pair_fwd'
    dg = lambda dy, ci, H, W, **kw: ops.conv2d_dgrad_s2_plan(dy, ci, H, W, cus=CUS, resident=2, **kw).entry
    # data gradient: dy of 2^31 bytes (resident 32 channels: 2^24 pixels; streaming 96)
    assert dg((1, 4096, 4096, 32), 16, 8192, 8192) == 'none' and dg((1, 4096, 4095, 32), 16, 8192, 8190) == 'dgrad_s2'
    assert dg((1, 4096, 4096, 64), 32, 8192, 8192) == 'none'
    assert dg((3, 2048, 1024, 96), 48, 4096, 2048) == 'none' and dg((2, 2048, 1024, 96), 48, 4096, 2048) == 'dgrad_s2'
    # data gradient: 2^30 pixels in the resident kernels (dy is 2^37 bytes by then), 2^26 in the streaming ones
    assert dg((1, 32768, 32768, 32), 16, 65536, 65536) == 'none' and dg((1, 8192, 8192, 96), 48, 16384, 16384) == 'none'
    # data gradient, streaming: a weight image of 2^31 bytes
    assert dg((1, 2, 2, 8192), 8192, 4, 4) == 'none' and dg((1, 2, 2, 4096), 4096, 4, 4) == 'dgrad_s2'
    # 1x1 pair: an operand of 2^31 bytes
    p = lambda dy, ci, H, W: ops.conv1x1_pair_plan(dy, ci, H, W).entry
    assert p((1, 4096, 4096, 32), 16, 8192, 8192) == 'none' and p((1, 4096, 4095, 32), 16, 8192, 8192) == 'pair_1x1'


def test_record_limits_of_the_persistent_kernels(ops):
    """One record per workgroup.  The data gradient REFUSES a grid beyond BN_BWD_RECORDS_MAX when it is to write sums and runs
    it without; the forward LOWERS the workgroups per CU until cus * per_cu fits BN_RECORDS_MAX, and refuses a device with more
    CUs than records, statistics or not."""
    dy, args = (16, 513, 65, 32), (16, 1025, 130)                                  # 16 673 units of 32 pixels: three per CU
    free = ops.conv2d_dgrad_s2_plan(dy, *args, cus=512, resident=3)
    assert (free.workgroups, free.sums, free.records) == (1536, 0, 0) and free.workgroups > BN_BWD_RECORDS_MAX, free
    assert ops.conv2d_dgrad_s2_plan(dy, *args, sums=True, cus=512, resident=3)._asdict() == NONE
    # ... refused, not lowered: two per CU fit, where that is all the CU holds
    two = ops.conv2d_dgrad_s2_plan(dy, *args, sums=True, cus=512, resident=2)
    assert (two.workgroups, two.sums, two.records) == (1024, 1, 1024), two
    x = (8, 1000, 512, 16)                                                         # 64 000 units: three per CU cost 6 % more than one
    assert ops.conv_s2_pair_fwd_plan(x, 32, cus=500, resident=3).workgroups == 1500
    for stats in (True, False):                                                    # 3000 > 2048: two per CU
        assert ops.conv_s2_pair_fwd_plan(x, 32, stats=stats, cus=1000, resident=3).workgroups == 2000
    assert ops.conv_s2_pair_fwd_plan(x, 32, cus=2048, resident=3).workgroups == 2048
    for stats in (True, False):
        assert ops.conv_s2_pair_fwd_plan(x, 32, stats=stats, cus=2049, resident=3)._asdict() == NONE
        assert ops.conv_s2_pair_fwd_plan((1, 4, 4, 16), 32, stats=stats, cus=2049, resident=1)._asdict() == NONE


def test_cu_count_no_multiple_of_8(ops):
    """n_xcd 1 together with rounds >= 2: a full grid on a device whose CU count is no multiple of 8."""
    for rec in (ops.conv_s2_pair_fwd_plan((8, 1025, 130, 16), 32, cus=250, resident=2),
                ops.conv2d_dgrad_s2_plan((8, 513, 65, 32), 16, 1025, 130, sums=True, cus=250, resident=1)):
        assert rec.family == 'resident' and rec.workgroups % 250 == 0 and rec.workgroups % 8, rec
        assert rec.n_xcd == 1 and rec.rounds >= 2, rec
        n_xcd, counts, shares = sk._walk(rec.units, rec.workgroups, rec.WAVES)
        assert (n_xcd, max(counts)) == (1, rec.rounds) and sum(counts) == rec.units


def test_sums_on_a_streaming_layer(ops):
    """A request for the backward sums on a layer the streaming kernels take plans the launch without them."""
    c = sk.BY_ID['d48from96_b2_41x27']
    rec = ops.conv2d_dgrad_s2_plan(_dy_shape(c), c.Ci, c.H, c.W, pair=True, sums=True, cus=CUS, resident=2)
    assert (rec.entry, rec.family, rec.sums, rec.records) == ('dgrad_s2', 'stream_lds', 0, 0), rec


def test_plan_argument_errors(ops):
    """The refusals of the launching entries that depend on no pointer, from the plan entries, with the same status; a refused
    plan leaves the 'none' record."""
    from deep_audio_mixer_amd import _lib
    L = _lib.lib()

    def raw(name, args, **over):
        assert set(over) <= set(args)
        v = (ctypes.c_int * 16)(*([7] * 16))
        st = getattr(L, name)(*dict(args, **over).values(), v)
        assert st == OK or list(v) == [0] * 16, 'a refused plan left a record'
        return st

    f = dict(B=2, H=41, W=27, Ci=16, Co=32, stats=1, cus=CUS, resident=2)
    fwd = lambda **over: raw('dam_conv_s2_pair_fwd_plan', f, **over)
    assert fwd() == OK
    assert fwd(B=0) == BAD_ARG and fwd(H=0) == BAD_ARG and fwd(W=-1) == BAD_ARG
    assert fwd(Ci=16, Co=48) == UNSUPPORTED and fwd(Ci=48, Co=32) == UNSUPPORTED and fwd(Ci=32, Co=40) == UNSUPPORTED
    assert fwd(Ci=0, Co=32) == UNSUPPORTED and fwd(Ci=32, Co=0) == UNSUPPORTED and fwd(Ci=-32, Co=16) == UNSUPPORTED
    assert fwd(B=0, Co=48) == BAD_ARG                                 # a bad size is reported before an unsupported layer
    d = dict(B=2, Hd=21, Wd=14, Co=32, Ci=16, H=41, W=27, pair=1, sums=1, cus=CUS, resident=2)
    dg = lambda **over: raw('dam_dgrad_s2_3x3_plan', d, **over)
    assert dg() == OK and dg(H=42) == OK and dg(W=28) == OK
    assert dg(Hd=20) == BAD_ARG and dg(Hd=22) == BAD_ARG and dg(Wd=13) == BAD_ARG and dg(H=43) == BAD_ARG
    assert dg(B=0) == BAD_ARG and dg(Hd=0, H=0) == BAD_ARG and dg(Wd=0, W=-1) == BAD_ARG
    assert dg(Co=48) == UNSUPPORTED and dg(Co=64, Ci=24) == UNSUPPORTED and dg(Co=0) == UNSUPPORTED and dg(Ci=0) == UNSUPPORTED
    assert dg(Hd=20, Co=48) == BAD_ARG
    p = dict(B=2, H=5, W=11, C=48, n_out=16, OHt=9, OWt=21, out_stride=2, out_off_h=0, out_off_w=0)
    pair = lambda **over: raw('dam_conv1x1_pair_plan', p, **over)
    assert pair() == OK and pair(OHt=10, OWt=22, out_off_h=1, out_off_w=1) == OK
    assert pair(B=0) == BAD_ARG and pair(H=0) == BAD_ARG and pair(W=0) == BAD_ARG
    assert pair(out_stride=0) == BAD_ARG and pair(out_stride=1) == OK
    assert pair(out_off_h=1) == BAD_ARG and pair(out_off_w=1) == BAD_ARG             # (H - 1) * stride + off = OHt
    assert pair(out_off_h=-1) == BAD_ARG and pair(out_off_w=-1) == BAD_ARG and pair(OHt=8) == BAD_ARG and pair(OWt=20) == BAD_ARG
    assert pair(C=40) == UNSUPPORTED and pair(n_out=24) == UNSUPPORTED and pair(C=0) == UNSUPPORTED and pair(n_out=0) == UNSUPPORTED
    assert pair(C=40, out_stride=0) == BAD_ARG and pair(C=40, OHt=8) == UNSUPPORTED  # the order of the launching entry
    for name, n in (('dam_conv_s2_pair_fwd_plan', 8), ('dam_dgrad_s2_3x3_plan', 11), ('dam_conv1x1_pair_plan', 10)):
        assert getattr(L, name)(*([1] * n), None) == BAD_ARG
    # bad arguments raise from ops, a refusal is an answer
    with pytest.raises(RuntimeError, match='DAM_ERR_BAD_ARG'):
        ops.conv2d_dgrad_s2_plan((2, 20, 14, 32), 16, 41, 27, cus=CUS, resident=2)
    with pytest.raises(RuntimeError, match='DAM_ERR_BAD_ARG'):
        ops.conv_s2_pair_fwd_plan((0, 41, 27, 16), 32, cus=CUS, resident=2)
    assert ops.conv_s2_pair_fwd_plan((2, 41, 27, 16), 48, cus=CUS, resident=2)._asdict() == NONE
