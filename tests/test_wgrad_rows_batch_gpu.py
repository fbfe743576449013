"""GPU: recorded launches of the stride-1 row weight-gradient kernel (ops.conv2d_wgrad(defer=True, batch_rows=True),
dam_wgrad_queue_set_batching mode 2): the calls of one instantiation and geometry wait for each other and run as ONE launch of
wgrad_rows_kernel whose workgroups walk a job table, the loader waves asking for the next job's first rows while the current
job's last slots are multiplied.

Per instantiation of the batching table one shape (tests/test_wgrad_rows_batch_plan_cpu.py: GPU_SHAPES, B = 2, strips of 4 and
of 5 rows -- whole slots, and the last slot of one row that the one-block tile splits over its four compute waves), and per shape:
1, 2 and 5 jobs; a full table (ROWS_MAX_JOBS = 8: nothing launched before the flush); a full table plus one (the ninth call
launches the eight, its own job waits for the flush); a mix of plain, affine, affine + ReLU and c_real = 8 jobs; a job of another
geometry in mid-queue (it launches what is pending) and one of another instantiation; ops.wgrad_abandon() with jobs recorded,
then a clean step.

Every job's result must be
  * bitwise equal (torch.equal) to the same call made through the existing deferred path (batch_rows=False: launched at once), and
  * within 5e-5 of the max-abs of torch.nn.grad.conv2d_weight in float64 (tests/test_wgrad_kernels_gpu.py's bound for the family);
the `out` buffers and 64 guard words on either side are untouched until the flush (bit pattern), the guards afterwards too; every
call's launch record equals the plan of the same call, with issued == 2.  Which launches have run is read from the slab
workspaces (filled with a bit pattern beforehand): a recorded job has not written its slabs.

Block level: the backward of stem -> layer1.0 -> layer1.1 (five weight gradients of one geometry: one launch) at 33 x 130 and of
a 32-channel BasicBlock at 17 x 65, gradient slots bound, once with layers.WGRAD_ROWS_BATCH and once without: every parameter
gradient and dx bitwise equal."""
import ctypes

import pytest
import torch

import test_wgrad_kernels_gpu as wk
import test_wgrad_rows_batch_plan_cpu as bp

pytestmark = pytest.mark.gpu

ROWS_MAX_JOBS = 8                  # dam_wgrad_plan.h
GUARD = 64
FILL = 0x5EADBEEF
TOL = wk.TOL
NAMES = sorted(bp.GPU_SHAPES)
KINDS = ('plain', 'affine', 'relu', 'creal8')
N_DATA = 2                          # distinct (x, dy, scale, shift) sets per shape; jobs cycle through them

_DATA, _WANT = {}, {}


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    torch.set_num_threads(16)
    return ops


def _data(shape, i):
    """Inputs number i of a (B, H, W, C) shape: host NCHW tensors and their device NHWC forms.  |shift| 0.2 .. 1 with both signs."""
    key = (shape, i)
    if key not in _DATA:
        B, H, W, C = shape
        g = torch.Generator().manual_seed(9100 + 17 * i + H + 1000 * W)
        x, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        sc = torch.rand(C, generator=g) + 0.5
        sign = torch.ones(C)
        sign[(C + 1) // 2:] = -1
        sh = (0.2 + 0.8 * torch.rand(C, generator=g)) * sign[torch.randperm(C, generator=g)]
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
        _DATA[key] = dict(x=x, dy=dy, sc=sc, sh=sh, xd=nhwc(x), dyd=nhwc(dy), scd=sc.cuda(), shd=sh.cuda())
    return _DATA[key]


def _want(shape, i, kind):
    """float64 gradient of job kind `kind` on inputs i (computed once, shared, never modified)."""
    key = (shape, i, 'plain' if kind == 'creal8' else kind)
    if key not in _WANT:
        d, C = _data(shape, i), shape[3]
        a = d['x'].double()
        if kind in ('affine', 'relu'):
            a = a * d['sc'].double().view(1, -1, 1, 1) + d['sh'].double().view(1, -1, 1, 1)
            if kind == 'relu':
                neg = (a < 0).double().mean().item()
                assert 0.25 <= neg <= 0.75, neg
                a = a.clamp(min=0)
        _WANT[key] = torch.nn.grad.conv2d_weight(a, (C, C, 3, 3), d['dy'].double(), 1, 1, 1)
    w = _WANT[key]
    return w[:, :8].contiguous() if kind == 'creal8' else w


def _slabs(ops, dev, index, floats):
    """The slab workspace deferred call number `index` since the last flush will get, filled with the pattern."""
    ws = ops._grow(ops._workspaces, (dev.type, dev.index, 'wgrad slabs', index), dev, floats)
    ws.view(torch.int32).fill_(FILL)
    return ws


def _run(ops, jobs, batch, launched_after=None, abandon=False):
    """jobs: (shape, data index, kind) in call order, all deferred, batch_rows=batch; one flush at the end (abandon: none, the
    queue is dropped).  launched_after: {call index: set of call indices whose slab kernel must have run once that call returned};
    every other slab buffer must still hold the pattern then.  -> the gradients (host), or None after an abandon."""
    dev = torch.device('cuda', torch.cuda.current_device())
    q = ops._wgrad_queue(dev)
    L = ops._lib.lib()
    assert q[1] == 0 and L.dam_wgrad_queue_pending(ctypes.addressof(q[0])) == 0
    bufs, views, recs, slabs = [], [], [], []
    for n, (shape, i, kind) in enumerate(jobs):
        B, H, W, C = shape
        floats = L.dam_conv2d_wgrad_workspace_floats(C, C, 3, 3)
        slabs.append(_slabs(ops, dev, n, floats))
    for n, (shape, i, kind) in enumerate(jobs):
        B, H, W, C = shape
        d = _data(shape, i)
        kr = 8 if kind == 'creal8' else C
        numel = C * kr * 9
        buf = torch.full((2 * GUARD + numel,), FILL, dtype=torch.int32, device=dev)
        out = buf.view(torch.float32)[GUARD:GUARD + numel].view(C, kr, 3, 3)
        kw = {}
        if kind in ('affine', 'relu'):
            kw.update(in_scale=d['scd'], in_shift=d['shd'], relu_in=kind == 'relu')
        if kind == 'creal8':
            kw['c_real'] = 8
        ops.conv2d_wgrad(d['xd'], d['dyd'], C, 3, 3, 1, 1, 1, out=out, defer=True, batch_rows=batch, **kw)
        rec = ops.wgrad_last_launch()
        plan = wk.planned(ops, d['xd'], d['dyd'], C, 3, 1, 1, 1, defer=True, batch_rows=batch, affine=kind in ('affine', 'relu'),
                          relu_in=kind == 'relu', c_real=kr if kind == 'creal8' else None)
        assert rec == plan and rec.family == 'rows' and rec.issued == (2 if batch else 1), (n, rec, plan)
        bufs.append(buf), views.append(out), recs.append(rec)
        if launched_after is not None and n in launched_after:
            torch.cuda.synchronize()
            for m in range(len(jobs)):
                r = recs[m] if m < len(recs) else None
                used = None if r is None else r.nsplit * r.nx * r.TNB * r.TKB * 9 * 256
                pattern = slabs[m].view(torch.int32)[:used] == FILL
                if m in launched_after[n]:
                    assert not bool(pattern.any()), 'call %d: the slabs of job %d are not (all) written' % (n, m)
                else:
                    assert bool(pattern.all()), 'call %d: job %d has run' % (n, m)
    assert L.dam_wgrad_queue_pending(ctypes.addressof(q[0])) == len(jobs)
    torch.cuda.synchronize()
    for n, buf in enumerate(bufs):
        assert bool((buf == FILL).all()), 'job %d: result or guard words written before the flush' % n
    if abandon:
        ops.wgrad_abandon(dev)
        assert L.dam_wgrad_queue_pending(ctypes.addressof(q[0])) == 0 and q[1] == 0 and q[2] == []
        torch.cuda.synchronize()
        for n, buf in enumerate(bufs):
            assert bool((buf == FILL).all()), 'job %d: written by an abandoned queue' % n
        return None
    ops.wgrad_flush(dev)
    assert L.dam_wgrad_queue_pending(ctypes.addressof(q[0])) == 0 and q[2] == []
    torch.cuda.synchronize()
    got = []
    for n, buf in enumerate(bufs):
        host = buf.cpu()
        assert bool((host[:GUARD] == FILL).all()) and bool((host[-GUARD:] == FILL).all()), 'job %d: guard words written' % n
        got.append(views[n].cpu())
    return got


def _check(ops, jobs, launched_after=None):
    """The job list batched against the same list through the existing deferred path, and against float64."""
    alone = _run(ops, jobs, False, {n: set(range(n + 1)) for n in range(len(jobs))})     # each launched by its own call
    batched = _run(ops, jobs, True, launched_after)
    for n, (shape, i, kind) in enumerate(jobs):
        assert torch.equal(batched[n], alone[n]), 'job %d %s: not bitwise the result of a launch of its own' % (n, (shape, i, kind))
        w = _want(shape, i, kind)
        scale = w.abs().max().item()
        err = (batched[n].double() - w).abs().max().item()
        print('job %d %s data %d %s: err %.2e of scale %.3g' % (n, shape, i, kind, err / scale, scale))
        assert err <= TOL * scale, (n, shape, i, kind, err, scale)


def _cycle(shape, n, kinds=('plain',)):
    return [(shape, k % N_DATA, kinds[k % len(kinds)]) for k in range(n)]


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('njobs', [1, 2, 5])
def test_jobs(ops, name, njobs):
    """njobs recorded calls: nothing runs before the flush."""
    shape = bp.GPU_SHAPES[name]
    _check(ops, _cycle(shape, njobs, ('plain', 'relu')), {n: set() for n in range(njobs)})


@pytest.mark.parametrize('name', NAMES)
def test_full_table(ops, name):
    """ROWS_MAX_JOBS calls fill the table and still wait for the flush."""
    _check(ops, _cycle(bp.GPU_SHAPES[name], ROWS_MAX_JOBS, ('relu', 'plain', 'plain')), {n: set() for n in range(ROWS_MAX_JOBS)})


@pytest.mark.parametrize('name', NAMES)
def test_full_table_plus_one(ops, name):
    """The ninth call finds the table full: it launches the eight and is left for the flush -- two launches."""
    after = {n: set() for n in range(ROWS_MAX_JOBS)}
    after[ROWS_MAX_JOBS] = set(range(ROWS_MAX_JOBS))
    _check(ops, _cycle(bp.GPU_SHAPES[name], ROWS_MAX_JOBS + 1, ('plain', 'affine')), after)


@pytest.mark.parametrize('name', NAMES)
def test_mixed_jobs(ops, name):
    """Plain, affine, affine + ReLU and c_real = 8 jobs in one launch: the affine, the ReLU floor and the gradient's width are
    per job (a job that took its neighbour's would be off by far more than the bound)."""
    shape = bp.GPU_SHAPES[name]
    jobs = [(shape, 0, 'plain'), (shape, 1, 'relu'), (shape, 0, 'creal8'), (shape, 1, 'affine'), (shape, 0, 'relu'), (shape, 1, 'plain')]
    _check(ops, jobs, {n: set() for n in range(len(jobs))})


@pytest.mark.parametrize('name', NAMES)
def test_geometry_change(ops, name):
    """Two jobs, then one of the same instantiation and another height: its call launches the two; a fourth of the first geometry
    launches that one in turn.  The last is left for the flush."""
    shape = bp.GPU_SHAPES[name]
    other = (shape[0], 9, shape[2], shape[3])
    jobs = [(shape, 0, 'plain'), (shape, 1, 'relu'), (other, 0, 'relu'), (shape, 1, 'plain')]
    _check(ops, jobs, {0: set(), 1: set(), 2: {0, 1}, 3: {0, 1, 2}})


def test_instantiation_change(ops):
    """Jobs of two instantiations alternate: every change launches what is pending."""
    a, b = bp.GPU_SHAPES['r33'], bp.GPU_SHAPES['r17']
    jobs = [(a, 0, 'plain'), (a, 1, 'plain'), (b, 0, 'relu'), (b, 1, 'plain'), (a, 0, 'relu')]
    _check(ops, jobs, {0: set(), 1: set(), 2: {0, 1}, 3: {0, 1}, 4: {0, 1, 2, 3}})


@pytest.mark.parametrize('name', NAMES)
def test_abandon_then_clean_step(ops, name):
    """ops.wgrad_abandon() with three jobs recorded drops them (nothing is launched, nothing written); the next step is clean."""
    shape = bp.GPU_SHAPES[name]
    assert _run(ops, _cycle(shape, 3, ('relu', 'plain')), True, {n: set() for n in range(3)}, abandon=True) is None
    _check(ops, _cycle(shape, 2, ('plain', 'relu')), {0: set(), 1: set()})


def test_mode_switch_rules(ops):
    """dam_wgrad_queue_set_batching: 1 <-> 2 with launches recorded is allowed (the mode is that of the next call), to 0 it is not;
    values outside 0 .. 2 are refused."""
    dev = torch.device('cuda', torch.cuda.current_device())
    q, L = ops._wgrad_queue(dev), ops._lib.lib()
    addr = ctypes.addressof(q[0])
    shape = bp.GPU_SHAPES['r3']
    d, C = _data(shape, 0), shape[3]
    out = torch.empty(C, C, 3, 3, device=dev)
    ops.conv2d_wgrad(d['xd'], d['dyd'], C, 3, 3, 1, 1, 1, out=out, defer=True, batch_rows=True)
    assert L.dam_wgrad_queue_set_batching(addr, 1) == 0 and L.dam_wgrad_queue_set_batching(addr, 2) == 0
    assert L.dam_wgrad_queue_set_batching(addr, 0) == -1 and L.dam_wgrad_queue_set_batching(addr, 3) == -1
    assert L.dam_wgrad_queue_set_batching(addr, 1) == 0
    ops.wgrad_flush(dev)
    torch.cuda.synchronize()
    w = _want(shape, 0, 'plain')
    assert (out.cpu().double() - w).abs().max().item() <= TOL * w.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------- block level
def _randomize(module, gen):
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (2.0 / (m.weight[0].numel())) ** 0.5)
    return module


def _bind_slots(params):
    n = sum(p.numel() for p in params)
    flat = torch.full((n,), float('nan'), dtype=torch.float32, device='cuda')
    off = 0
    for p in params:
        p._dam_grad = flat[off:off + p.numel()].view(p.shape)
        off += p.numel()
    return flat


def _backward_twice(ops, layers, monkeypatch, params, forward, dout):
    """forward() -> (output, input that wants a gradient or None); backward with and without the opt-in -> the two (flat gradient
    buffer, dx) pairs and the number of row launches recorded with it."""
    res = []
    for batch in (False, True):
        monkeypatch.setattr(layers, 'WGRAD_ROWS_BATCH', batch)
        flat = _bind_slots(params)
        out, xin = forward()
        seen = []
        real = ops.conv2d_wgrad

        def spy(*a, **kw):
            r = real(*a, **kw)
            seen.append(ops.wgrad_last_launch())
            return r
        monkeypatch.setattr(ops, 'conv2d_wgrad', spy)
        out.backward(dout)
        monkeypatch.setattr(ops, 'conv2d_wgrad', real)
        ops.wgrad_flush()
        torch.cuda.synchronize()
        assert not bool(torch.isnan(flat).any())
        res.append((flat.clone(), None if xin is None else xin.grad.clone(), sum(r.family == 'rows' and r.issued == 2 for r in seen),
                    sum(r.family == 'rows' for r in seen)))
    return res


def test_chain_stem_layer1_bitwise(ops, monkeypatch):
    """stem -> layer1.0 -> layer1.1 at 2 x 8 x 33 x 130: five row weight gradients of one geometry, recorded, one launch."""
    from deep_audio_mixer_amd import layers
    gen = torch.Generator().manual_seed(21)
    S, B, H, W = 8, 2, 33, 130
    stem = _randomize(torch.nn.Sequential(torch.nn.Conv2d(S, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)), gen).cuda().train()
    blks = [_randomize(layers.BasicBlock(16, 16, 1), gen).cuda().train() for _ in range(2)]
    spec = layers.ConvSpec(S, 16, 3, 1, 1, in_nchw=True)
    params = list(stem.parameters()) + [p for b in blks for p in b.parameters()]
    x = (20.0 * torch.randn((B, S, H, W), generator=gen) - 40.0).cuda()
    dout = torch.randn((B, H, W, 16), generator=gen).cuda()

    def forward():
        a0 = layers.ConvBnReluFn.apply(x, stem[0].weight, None, stem[1].weight, stem[1].bias, spec, stem[1], True)
        return blks[1](blks[0](a0)), None
    (f0, _, rec0, rows0), (f1, _, rec1, rows1) = _backward_twice(ops, layers, monkeypatch, params, forward, dout)
    assert rows0 == rows1 == 5 and rec0 == 0 and rec1 == 5
    assert torch.equal(f0, f1)


def test_block32_bitwise(ops, monkeypatch):
    """A 32-channel identity BasicBlock at 2 x 17 x 65: two row weight gradients recorded; parameter gradients and dx."""
    from deep_audio_mixer_amd import layers
    gen = torch.Generator().manual_seed(22)
    B, H, W, C = 2, 17, 65, 32
    blk = _randomize(layers.BasicBlock(C, C, 1), gen).cuda().train()
    params = list(blk.parameters())
    x = torch.relu(torch.randn((B, H, W, C), generator=gen)).cuda()
    dout = torch.randn((B, H, W, C), generator=gen).cuda()

    def forward():
        xin = x.clone().requires_grad_(True)
        return blk(xin), xin
    (f0, dx0, rec0, rows0), (f1, dx1, rec1, rows1) = _backward_twice(ops, layers, monkeypatch, params, forward, dout)
    assert rows0 == rows1 == 2 and rec0 == 0 and rec1 == 2
    assert torch.equal(f0, f1) and torch.equal(dx0, dx1)
