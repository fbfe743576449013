"""CPU: which kernel dam_conv2d_wgrad_f32 gives a layer, asked from the plan entry (dam_conv2d_wgrad_plan through
ops.conv2d_wgrad_plan) without a GPU.

The case table of tests/test_wgrad_kernels_gpu.py names, per (case, form), the kernel family and template instantiation the launch
must report through ops.wgrad_last_launch(); it passed on the device before the dispatch became a plan, so agreement with it is
agreement with that dispatch.  Here every pair of the table is planned and compared with the same _expected() record -- no pair is
skipped, the count is asserted -- and the file's REQUIRED coverage is asserted from the planned records, with the structural checks
its _launch makes on a record.  The fields the table does not name (grid, strips, pixels per tile) are pinned by
tests/golden/wgrad_launch_records.json: the 16 ints dam_wgrad_last_launch reported on the device for every pair, and for the twelve
jobs of test_direct_batched_jobs, from the library as it was before the dispatch became a plan.  The GPU tests assert the other
half: the record a launch leaves equals the plan of the same call.

Also here: the refusals of the launching entry that need no pointer and no device, with the same status, and per family the
smallest workspace that still plans."""
import ctypes
import json
import os

import pytest

import test_wgrad_kernels_gpu as wk

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'wgrad_launch_records.json')) as fh:
        return json.load(fh)


def _raw(ops, c, form='plain', workspace_floats=None, **over):
    """-> (status, the 16 ints) of the plan entry for the call wk._launch makes for (c, form); `over`: scalars replaced by name."""
    from deep_audio_mixer_amd import _lib
    n_out = c.Co - 12 if form == 'nout' else c.Co
    x_shape = (c.B, c.Ci, c.H, c.W) if c.nchw else (c.B, c.H, c.W, c.Ci)
    Ho, Wo = wk._out_hw(c)
    B, H, W, C, Ho, Wo, n_chan, cr, floats = ops._wgrad_call(x_shape, (c.B, Ho, Wo, c.Co), n_out, c.k, c.k, c.nchw, c.c_real)
    affine = form in ('relu', 'affine')
    a = dict(B=B, H=H, W=W, C=C, in_nchw=int(c.nchw), relu_in=int(form == 'relu'), Ho=Ho, Wo=Wo, n_chan=n_chan, n_out=n_out, kh=c.k,
             kw=c.k, stride=c.s, pad=c.p, dil=c.d, c_real=cr, has_affine=int(affine), has_shift=int(affine),
             queue_mode=(2 if ops.WGRAD_BATCH else 1) if form == 'defer' else 0,
             workspace_floats=floats if workspace_floats is None else workspace_floats)
    assert set(over) <= set(a)
    a.update(over)
    v = (ctypes.c_int * 16)(*([7] * 16))
    st = _lib.lib().dam_conv2d_wgrad_plan(*a.values(), v)
    if st != OK:
        assert list(v) == [0] * 16, 'a refused plan left a record'
    return st, list(v)


def _plan(ops, c, form):
    """ops.conv2d_wgrad_plan for the call wk._launch makes for (c, form)."""
    Ho, Wo = wk._out_hw(c)
    return ops.conv2d_wgrad_plan((c.B, c.Ci, c.H, c.W) if c.nchw else (c.B, c.H, c.W, c.Ci), (c.B, Ho, Wo, c.Co),
                                 c.Co - 12 if form == 'nout' else c.Co, c.k, c.k, c.s, c.p, c.d, affine=form in ('relu', 'affine'),
                                 relu_in=form == 'relu', in_nchw=c.nchw, c_real=c.c_real, defer=form == 'defer')


def test_table(ops, golden):
    """Every (case, form) of tests/test_wgrad_kernels_gpu.py: the expected record, the structural checks of its _launch, the
    device's 16 ints; then REQUIRED from the planned records."""
    planned = {}
    for c in wk.CASES:
        for form in wk.FORMS:
            want = wk._expected(c, form)
            st, v = _raw(ops, c, form)
            assert v == golden['records']['%s/%s' % (c.id, form)], '%s %s: planned %s' % (c.id, form, v)
            if wk._refused(c, form):
                assert st == UNSUPPORTED
                with pytest.raises(RuntimeError, match='DAM_ERR_UNSUPPORTED'):
                    _plan(ops, c, form)
                rec = planned[(c.id, form)] = ops._wgrad_launch(v)
                assert {k: getattr(rec, k) for k in want} == want
                continue
            assert st == OK
            rec = planned[(c.id, form)] = _plan(ops, c, form)
            assert rec == ops._wgrad_launch(v)
            assert {k: getattr(rec, k) for k in want} == want, '%s %s: planned %s' % (c.id, form, rec)
            assert rec.nx >= 1 and (rec.nsplit == 0) == (rec.family == 'tile' and rec.issued == 2), rec
            if rec.family in ('rows', 'rows_s2'):
                rows = c.H if rec.family == 'rows' else wk._out_hw(c)[0]
                assert rec.nsplit == c.B * rec.spi and rec.spi >= 1 and rec.spi * rec.rps >= rows and rec.TMW == 0, rec
            else:
                assert rec.spi == 0 and rec.rps == 0 and (rec.TMW > 0) == (rec.family == 'tile'), rec
    assert len(planned) == len(wk.CASES) * len(wk.FORMS) == len(golden['records'])
    seen = {wk._variant(r) for r in planned.values()}           # 'batched' from the defer forms, 'alone' from the others
    lacking = [v for v in wk.REQUIRED if v not in seen]
    assert not lacking, 'kernel variants no case reached: %s' % lacking
    for (cid, form), r in planned.items():
        if form in ('relu', 'affine'):
            assert r.family == 'none' if wk.BY_ID[cid].nchw else r.family in ('rows', 'tile'), (cid, form, r)


def test_direct_batched_jobs(ops, golden):
    """The twelve deferred jobs of wk.test_direct_batched_jobs: their instantiations, and the device's 16 ints."""
    A, Bj = wk._direct(2, 2, 1), wk._direct(2, 1, 1)
    plan = [(A, 2, 32, 64, 9, 21), (A, 1, 64, 64, 4, 35), (Bj, 2, 16, 32, 7, 66)]
    plan += [(A, 1 + i % 3, (32, 64, 96)[i % 3], (64, 32, 128)[(i // 3) % 3], 3 + 2 * i, 9 + 7 * i) for i in range(wk.WD_MAX_JOBS + 1)]
    assert len(plan) == 12 == len(golden['direct_batched_jobs'])
    for (exp, B, ci, co, H, W), want16 in zip(plan, golden['direct_batched_jobs']):
        rec = ops.conv2d_wgrad_plan((B, H, W, ci), (B, (H + 1) // 2, (W + 1) // 2, co), co, 1, 1, 2, 0, 1, defer=True)
        assert {k: getattr(rec, k) for k in exp} == exp and rec.issued == 2, rec
        assert rec == ops._wgrad_launch(want16), rec


def test_plan_argument_errors(ops):
    """The refusals of dam_conv2d_wgrad_f32 that depend on no pointer and no device, from the plan entry."""
    from deep_audio_mixer_amd import _lib
    c = wk.BY_ID['r9_w33_h3']
    st = lambda **over: _raw(ops, c, **over)[0]
    assert st() == OK
    assert st(B=0) == BAD_ARG and st(H=0) == BAD_ARG and st(Wo=0) == BAD_ARG
    assert st(c_real=c.Ci + 1) == BAD_ARG and st(c_real=-1) == BAD_ARG and st(c_real=c.Ci) == OK
    assert st(n_chan=24) == UNSUPPORTED
    assert st(n_out=c.Co + 1) == UNSUPPORTED
    assert st(stride=3) == UNSUPPORTED and st(stride=0) == UNSUPPORTED
    assert st(C=24, c_real=0) == UNSUPPORTED                        # NHWC: whole 16-channel chunks (c_real = 0: all of C)
    assert st(C=17, c_real=0, in_nchw=1) == UNSUPPORTED and st(C=16, c_real=0, in_nchw=1) == OK
    assert st(has_affine=1, has_shift=0) == BAD_ARG and st(has_affine=1, has_shift=1) == OK
    # an unsupported shape is reported before the missing shift, as by the launching entry
    assert st(n_chan=24, has_affine=1, has_shift=0) == UNSUPPORTED and st(stride=3, has_affine=1) == UNSUPPORTED
    assert st(C=8, c_real=0, in_nchw=1, has_affine=1, has_shift=1) == UNSUPPORTED
    assert st(kh=3, kw=4) == UNSUPPORTED and st(kh=1, kw=3) == UNSUPPORTED
    assert st(queue_mode=3) == BAD_ARG and st(queue_mode=1) == OK
    assert _lib.lib().dam_conv2d_wgrad_plan(*([1] * 19), 0, None) == BAD_ARG
    with pytest.raises(RuntimeError, match='DAM_ERR_UNSUPPORTED'):
        ops.conv2d_wgrad_plan((2, 9, 33, 24), (2, 9, 33, 32), 32, 3, 3, 1, 1, 1)


@pytest.mark.parametrize('cid', ['r9_w34_h22', 's7_wo27_w53_h23_16to32', 'd11_64to96', 'd33_wo23', 't_k9_64to128', 't256_w5'])
def test_smallest_workspace(ops, cid):
    """Per family: with room for one slab set -- nx workgroup slabs of NBLK blocks of 256 floats -- the call still plans, with one
    pixel split (row kernels: one strip per image); with one float less it is DAM_ERR_WORKSPACE and the record stays zero."""
    c = wk.BY_ID[cid]
    st, v = _raw(ops, c)
    rec = ops._wgrad_launch(v)
    rows = rec.family in ('rows', 'rows_s2')
    assert st == OK and (rec.spi if rows else rec.nsplit) > 1, rec
    nblk = rec.TNB * rec.TKB * (9 if rows else rec.TA * rec.TB)
    least = (c.B if rows else 1) * rec.nx * nblk * 256           # (a row kernel's strips never cross images: B slabs per tile at least)
    st1, v1 = _raw(ops, c, workspace_floats=least)
    one = ops._wgrad_launch(v1)
    assert st1 == OK and one.nsplit == (c.B if rows else 1) and one.spi == (1 if rows else 0), one
    assert one._replace(nsplit=0, spi=0, rps=0) == rec._replace(nsplit=0, spi=0, rps=0)
    assert _raw(ops, c, workspace_floats=least - 1) == (WORKSPACE, [0] * 16)
    if rec.family == 'tile':         # a recorded tile launch meets its workspace at the flush
        assert _raw(ops, c, 'defer', workspace_floats=least - 1)[0] == OK
