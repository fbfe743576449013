"""CPU: which kernel dam_conv2d_tapgrid_f32 gives a layer, asked from the plan entry (dam_conv2d_tapgrid_plan through
ops.conv2d_fwd_plan / ops.conv2d_dgrad_plan) without a GPU.

The case tables of tests/test_conv_epilogue_gpu.py and tests/test_conv_training_epilogue_gpu.py name, per (case, epilogue) and
(case, form), the kernel family and template instantiation the launch must report through ops.conv_last_launch(); they passed
on the device before the dispatch became a plan, so agreement with them is agreement with that dispatch.  Here every pair of
both tables, the 'plain' call the data-gradient cases make beside their masked one, and the retreat cases (a launch that drops
its statistics or sums) are planned and compared with the same expected() records -- no pair is skipped, the counts are
asserted -- and both files' REQUIRED coverage sets are asserted from the planned records.  The GPU tests assert the other half:
the record a launch leaves equals the plan of the same call.

Also here: the plan entry answers DAM_OK with no GPU present (this whole file), and refuses the argument errors the launching
entry refuses, with the same status."""
import ctypes

import pytest

import test_conv_epilogue_gpu as inf
import test_conv_training_epilogue_gpu as trn

# pairs that cannot be expressed as one plan call: (table, case id, epilogue / form) -> reason.  None.
EXCEPTIONS = {}


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _check(rec, want, split, what):
    got = {k: getattr(rec, k) for k in want}
    assert got == want, '%s: planned %s' % (what, rec)
    if split is not None:
        assert (rec.ksplit > 1) == split, '%s: planned %s' % (what, rec)


def _env(monkeypatch, env):
    for name in ('DAM_NO_PIPE', 'DAM_TILE', 'DAM_PIPE_KS', 'DAM_PIPE_WGS'):
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------- the inference table
def _plan_inference(ops, c, epi):
    use_bias, use_res, relu = inf.EPILOGUES[epi]
    x_shape = (c.B, c.Ci, c.H, c.W) if c.nchw else (c.B, c.H, c.W, c.Ci)
    return ops.conv2d_fwd_plan(x_shape, c.Co, c.k, c.k, c.s, c.p, c.d, bias=use_bias, in_nchw=c.nchw, res=use_res,
                               relu_out=relu)


def test_inference_table(ops, monkeypatch):
    """Every (case, epilogue) of tests/test_conv_epilogue_gpu.py; then its REQUIRED coverage from the planned records."""
    planned = {}
    for c in inf.CASES:
        with monkeypatch.context() as mp:
            _env(mp, c.env)
            for epi, (_, use_res, _) in inf.EPILOGUES.items():
                if ('inference', c.id, epi) in EXCEPTIONS:
                    continue
                rec = planned[(c.id, epi)] = _plan_inference(ops, c, epi)
                _check(rec, inf.expected(c, use_res), c.expect.get('split'), '%s %s' % (c.id, epi))
    assert len(planned) + sum(k[0] == 'inference' for k in EXCEPTIONS) == len(inf.CASES) * len(inf.EPILOGUES)
    assert len(EXCEPTIONS) <= 5
    seen = {inf._variant(r) for r in planned.values()}
    lacking = [v for v in inf.REQUIRED if v not in seen]
    assert not lacking, 'kernel variants no case reached: %s' % lacking
    assert all(r.ranges >= 2 for r in planned.values() if r.family == 'pipe_ranges')


# -------------------------------------------------------------------------------------------------- the training table
def _dgrad_kw(form):
    kw = {}
    if form in ('mask', 'res_sums', 'res_bits'):
        kw.update(res=True, res_mask=True)
    if form == 'sums':
        kw.update(bn_bwd=(True, True, True, True, True))
    if form == 'res_sums':
        kw.update(res_mask_bits=True, bn_bwd=(True, True, True, True, True))
    if form == 'res_bits':
        kw.update(res_mask_bits=True, bn_bwd=(True, True, True, None, None, True))
    return kw


def _plan_training(ops, c, form):
    """-> (ConvLaunch, records) of the call trn._fwd_call / trn._dgrad_call makes for `form` ('plain': no residual, no records)."""
    if c.op == 'fwd':
        kw = dict(bn_partial=True)
        if form == 'stats_affine':
            kw.update(in_scale=True, in_shift=True, relu_in=True)
        if form == 'stats_bias':
            kw.update(bias=True)
        return ops.conv2d_fwd_plan((c.B, c.H, c.W, c.Ci), c.Co, c.k, c.k, c.s, c.p, c.d, parts=True, **kw)
    Ho, Wo = c.H + 2 * c.p - c.d * (c.k - 1), c.W + 2 * c.p - c.d * (c.k - 1)
    return ops.conv2d_dgrad_plan((c.B, Ho, Wo, c.Co), c.Ci, c.H, c.W, c.k, c.k, 1, c.p, c.d, parts=True, **_dgrad_kw(form))


def test_training_table(ops, monkeypatch):
    """Every (case, form) of tests/test_conv_training_epilogue_gpu.py with records (as its test asserts: parts > 0), the 'plain'
    data gradient beside every masked one; then its REQUIRED coverage from the planned records."""
    planned = {}
    for c in trn.CASES:
        forms = c.forms + (('plain',) if c.op == 'dgrad' and 'mask' in c.forms else ())
        with monkeypatch.context() as mp:
            _env(mp, c.env)
            for form in forms:
                if ('training', c.id, form) in EXCEPTIONS:
                    continue
                rec, parts = planned[(c.id, form)] = _plan_training(ops, c, form)
                _check(rec, trn.expected(c, form), c.expect.get('split'), '%s %s' % (c.id, form))
                assert (parts > 0) == (form not in ('mask', 'plain')), '%s %s: %d records from %s' % (c.id, form, parts, rec)
    n_pairs = sum(len(c.forms) + (c.op == 'dgrad' and 'mask' in c.forms) for c in trn.CASES)
    assert len(planned) + sum(k[0] == 'training' for k in EXCEPTIONS) == n_pairs
    for group, variants in trn.REQUIRED.items():
        seen = {trn._variant(rec, stats=parts > 0 and group == 'stats') for (cid, form), (rec, parts) in planned.items()
                if trn.GROUP.get(form) == group}
        lacking = [v for v in variants if v not in seen]
        assert not lacking, '%s: kernel variants no case reached: %s' % (group, lacking)


def test_training_retreats(ops, monkeypatch):
    """The launches of trn.test_retreat_*: no records, and the kernel that runs instead."""
    _env(monkeypatch, {})
    strip = lambda r: (r.family, r.MB, r.NB, r.NCH, r.T33, r.LW, r.EPI, r.SO)
    fwd = lambda Ci, Co, H, W, B, s=1, **kw: ops.conv2d_fwd_plan((B, H, W, Ci), Co, 3, 3, s, 1, 1, parts=True, **kw)
    # statistics with two channel workgroups
    rec, parts = fwd(16, 64, 9, 130, 3, bn_partial=True)
    assert parts == 0 and strip(rec) == ('strip', 4, 2, 1, 1, 0, 0, 0) and rec == fwd(16, 64, 9, 130, 3)[0]
    # 1024 strip records are still produced, 1025 are not
    assert fwd(16, 16, 3, 16, 1024, bn_partial=True) == (fwd(16, 16, 3, 16, 1024)[0]._replace(SO=2), 1024)
    assert fwd(16, 16, 3, 16, 1025, bn_partial=True) == (fwd(16, 16, 3, 16, 1025)[0], 0)
    assert strip(fwd(16, 16, 3, 16, 1025)[0]) == ('strip', 4, 1, 1, 1, 0, 0, 1)
    # statistics on a shape that runs column ranges: the tile kernel
    rec, parts = fwd(16, 32, 12, 130, 3, s=2, bn_partial=True)
    rec0 = fwd(16, 32, 12, 130, 3, s=2)[0]
    assert parts == 0 and rec.family == 'tile' and (rec0.family, rec0.ranges) == ('pipe_ranges', 2)
    # 2048 pipe records are still produced, 2049 are not
    rec, parts = fwd(64, 64, 5, 17, 256, bn_partial=True)
    assert (rec.family, rec.MB, rec.NB, rec.KS, rec.STATS, parts) == ('pipe', 1, 4, 1, 1, 2048)
    assert fwd(64, 64, 5, 17, 256)[0] == rec._replace(STATS=0)
    assert fwd(64, 64, 5, 17, 257, bn_partial=True) == (fwd(64, 64, 5, 17, 257)[0], 0)
    # bn_bwd on layers no sums kernel takes: the launch of the call without it
    for c, form, want_rec in trn.RETREATS:
        rec, parts = _plan_training(ops, c, form)
        base = _plan_training(ops, c, 'mask' if form.startswith('res') else 'plain')[0]
        assert parts == 0 and strip(rec) == want_rec and rec == base, (c.id, form, rec, base)


# ------------------------------------------------------------------------------------------------------ argument errors
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def _status(ops, g, **given):
    from deep_audio_mixer_amd import _lib
    has = 0
    for name in given:
        has |= ops._HAS[name]
    rec, parts = (ctypes.c_int * 16)(), ctypes.c_int(7)
    st = _lib.lib().dam_conv2d_tapgrid_plan(*g[:7], 0, 0, *g[7:], has, 0, rec, ctypes.byref(parts))
    if st != OK:
        assert rec[0] == 0 and parts.value == 0
    return st


def test_plan_argument_errors(ops, monkeypatch):
    """The refusals of dam_conv2d_tapgrid_f32 that depend on no pointer and no device, from the plan entry."""
    _env(monkeypatch, {})
    g = ops._fwd_grid((2, 9, 130, 16), 16, 3, 3, 1, 1, 1, False)
    assert _status(ops, g) == OK
    assert _status(ops, g._replace(n_out=24)) == UNSUPPORTED
    assert _status(ops, g._replace(in_stride=3)) == UNSUPPORTED
    assert _status(ops, g._replace(B=65536)) == UNSUPPORTED and _status(ops, g._replace(B=65535)) == OK
    assert _status(ops, g._replace(C=24)) == UNSUPPORTED and _status(ops, g._replace(k_chunks=2)) == UNSUPPORTED
    assert _status(ops, g._replace(B=0)) == BAD_ARG and _status(ops, g._replace(nA=0)) == BAD_ARG
    assert _status(ops, g, in_scale=1) == BAD_ARG and _status(ops, g, in_scale=1, in_shift=1) == OK
    # an unsupported shape is reported before the missing shift, as by the launching entry
    assert _status(ops, g._replace(n_out=24), in_scale=1) == UNSUPPORTED
    assert _status(ops, g, bn_bwd=1, bwd_mask_scale=1) == BAD_ARG
    assert _status(ops, g, bn_bwd=1, bn_partial=1, bwd_mask_scale=1) == OK
    assert _status(ops, g, bn_bwd=1, bn_partial=1) == BAD_ARG                                   # neither form of the mask
    assert _status(ops, g, bn_bwd=1, bn_partial=1, bwd_mask_bits=1) == BAD_ARG                  # sign bytes without a residual
    assert _status(ops, g, bn_bwd=1, bn_partial=1, bwd_mask_scale=1, res=1, res_mask=1) == BAD_ARG   # residual without its sign bytes
    assert _status(ops, g, bn_bwd=1, bn_partial=1, bwd_mask_scale=1, res=1, res_mask=1, bwd_res_mask_bits=1) == OK
    from deep_audio_mixer_amd import _lib
    assert _lib.lib().dam_conv2d_tapgrid_plan(*g[:7], 0, 0, *g[7:], 0, 0, None, None) == BAD_ARG
    with pytest.raises(RuntimeError, match='DAM_ERR_UNSUPPORTED'):
        ops.conv2d_fwd_plan((65536, 9, 130, 16), 16, 3, 3, 1, 1, 1)
    with pytest.raises(ValueError):
        ops.conv2d_dgrad_plan((2, 5, 65, 32), 16, 9, 130, 3, 3, 2, 1, 1)
