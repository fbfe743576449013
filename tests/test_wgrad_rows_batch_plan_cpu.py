"""CPU: what dam_conv2d_wgrad_plan answers for a stride-1 row-kernel call that goes to a queue in the row-batching mode
(queue_mode 4, ops.conv2d_wgrad(defer=True, batch_rows=True)), without a GPU.

The plan of such a call names the same kernel as the plan of the same call in the older modes -- family `rows`, the same
instantiation, the same grid (nx, nsplit), strips per image and rows per strip: a recorded job runs on exactly the grid a launch of
its own would have, which is what makes its slabs bitwise the same -- and differs in one field: issued == 2 (the launch itself is
recorded) for the instantiations of the batching table, issued == 1 (launched at once, the reduction queued) for the others.  The
older modes answer as before: every row record of tests/golden/wgrad_launch_records.json is re-planned in modes 0 and 2 (through
tests/test_wgrad_plan_cpu.py's helper) and compared with it, and queue_mode 3 stays no mode.

The shapes of tests/test_wgrad_rows_batch_gpu.py are planned here too: each must hit the instantiation it names, and its strips
must include one whose row count is 1 mod 4 (the split last slot) and one that is a multiple of 4."""
import json
import os

import pytest

import test_wgrad_kernels_gpu as wk
import test_wgrad_plan_cpu as wp

# instantiations a mode-4 queue records: <TNB, TKB, STEPS, KP, GPP, HV, NL>
BATCHED = {'r33', 'r17', 'r9', 'r5', 'r3'}
# The shapes of the GPU test, (B, H, W, C) per instantiation.  Widths and channels as first proposed (130 x 16, 65 x 32, 33 x 64,
# 17 x 96, 9 x 128, B = 2); the heights are not the 21 / 19 / 13 / 11 / 9 proposed with them: an image of H rows gets
# min(ceil(H / 4), 256 / (nx B)) strips of nearly equal size, so a short image has strips of 3 and 4 rows only.  Strips of 4 AND 5
# rows need 4 < H / strips < 5 with the strips capped by the chip: H = 4 * floor(256 / (nx B)) + 1.
GPU_SHAPES = {'r33': (2, 513, 130, 16), 'r17': (2, 257, 65, 32), 'r9': (2, 65, 33, 64), 'r5': (2, 29, 17, 96), 'r3': (2, 17, 9, 128)}


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def strip_rows(H, spi):
    return [(s + 1) * H // spi - s * H // spi for s in range(spi)]


def _row_cases():
    return [c for c in wk.CASES if c.expect['family'] == 'rows']


def test_new_mode_names_the_same_kernel(ops):
    """Every row case of the kernel table, plain and with the affine forms: mode 4 against mode 1."""
    seen = set()
    for c in _row_cases():
        name = c.id.split('_')[0]
        for form in ('plain', 'relu', 'affine', 'nout'):
            st1, v1 = wp._raw(ops, c, form, queue_mode=1)
            st4, v4 = wp._raw(ops, c, form, queue_mode=4)
            assert st1 == st4 == wp.OK
            a, b = ops._wgrad_launch(v1), ops._wgrad_launch(v4)
            assert a.family == b.family == 'rows' and a.issued == 1
            assert b.issued == (2 if name in BATCHED else 1), (c.id, form, b)
            assert b._replace(issued=1) == a, (c.id, form, a, b)
            assert (b.nx, b.nsplit, b.spi, b.rps) == (a.nx, a.nsplit, a.spi, a.rps)
            seen.add((name, b.issued))
    assert {n for n, i in seen if i == 2} == BATCHED
    assert {n for n, _ in seen} == set(wk.ROWS)


def test_ops_plan_keyword(ops):
    """ops.conv2d_wgrad_plan(defer=True, batch_rows=True) is queue_mode 4; without the keyword a deferred row call plans as before."""
    for name, (B, H, W, C) in GPU_SHAPES.items():
        exp = wk.ROWS[name][0]
        plain = ops.conv2d_wgrad_plan((B, H, W, C), (B, H, W, C), C, 3, 3, 1, 1, 1, defer=True)
        rec = ops.conv2d_wgrad_plan((B, H, W, C), (B, H, W, C), C, 3, 3, 1, 1, 1, defer=True, batch_rows=True)
        assert {k: getattr(rec, k) for k in exp} == exp, (name, rec)
        assert plain.issued == 1 and rec.issued == 2 and rec._replace(issued=1) == plain
        # batch_rows without defer: no queue, nothing to record
        assert ops.conv2d_wgrad_plan((B, H, W, C), (B, H, W, C), C, 3, 3, 1, 1, 1, batch_rows=True).issued == 0


def test_gpu_shapes_have_both_strip_kinds(ops):
    """The GPU test's shapes: a strip of 1 mod 4 rows (its last slot is split over the four compute waves by MFMA steps where the
    tile has one block, and is a one-row slot otherwise) and a strip of a multiple of 4 rows (whole slots only)."""
    for name, (B, H, W, C) in GPU_SHAPES.items():
        rec = ops.conv2d_wgrad_plan((B, H, W, C), (B, H, W, C), C, 3, 3, 1, 1, 1, defer=True, batch_rows=True)
        rows = strip_rows(H, rec.spi)
        assert sum(rows) == H and min(rows) >= 1
        assert any(r % 4 == 1 for r in rows) and any(r % 4 == 0 for r in rows), (name, rec.spi, rows)
        assert (W + 2 + 3) // 4 == exp_steps(name), name


def exp_steps(name):
    return wk.ROWS[name][0]['STEPS']


def test_other_families_unchanged_by_mode_4(ops):
    """Tile and direct calls are recorded in mode 4 exactly as in mode 2; the stride-2 row kernel is never recorded."""
    for c in wk.CASES:
        if c.expect['family'] == 'rows':
            continue
        st2, v2 = wp._raw(ops, c, 'plain', queue_mode=2)
        st4, v4 = wp._raw(ops, c, 'plain', queue_mode=4)
        assert (st2, v2) == (st4, v4), c.id


def test_old_modes_unchanged(ops, golden_dir):
    """Modes 0 and 2 (the table's forms) against the recorded device answers, mode 1 against mode 2 for the row kernel; 3 is refused."""
    with open(os.path.join(golden_dir, 'wgrad_launch_records.json')) as fh:
        golden = json.load(fh)
    for c in _row_cases():
        for form in wk.FORMS:
            st, v = wp._raw(ops, c, form)
            assert st == wp.OK and v == golden['records']['%s/%s' % (c.id, form)], (c.id, form, v)
        assert wp._raw(ops, c, 'plain', queue_mode=1) == wp._raw(ops, c, 'plain', queue_mode=2)
        assert wp._raw(ops, c, 'plain', queue_mode=3) == (wp.BAD_ARG, [0] * 16)
        assert wp._raw(ops, c, 'plain', queue_mode=5) == (wp.BAD_ARG, [0] * 16)
