"""GPU: the BatchNorm-backward apply inside the row loaders of the 16-channel data gradients (conv_strip_kernel's BNF forms,
ops.conv2d_dgrad(bn_in=) behind ops.bn_backward_finalize) against the two launches it replaces and against float64.

Per case (form x height), on the same inputs and the same records of the BatchNorm's two sums:
  unfused  ops.bn_backward(partials=) -> dc, dgamma, dbeta;  ops.conv2d_dgrad(dc, bn_bwd=..) -> dx, upstream-sum records
  fused    ops.bn_backward_finalize(partials) -> coef, dgamma, dbeta;  ops.conv2d_dgrad(dy, bn_bwd=.., bn_in=..) -> dx, records, dc
dc, dx, dgamma, dbeta, the record count and the records are BITWISE equal; dc and dx agree with the float64 reference of
tests/test_conv_training_epilogue_gpu.py (F.grad.conv2d_input on the CPU) at that file's tolerance, 2e-5 of the max-abs; the
launch record names the fused instantiation (EPI, SO 1, BNF).

Forms: `bits` = mask from sign bytes in front of the EPI 1 data gradient (a block's bn2 -> conv2's gradient, which takes bn1's
sums); `aff_e2` / `aff_e3` = mask recomputed as fma(c, scale, shift) > 0 in front of the residual data gradient that takes the
upstream BatchNorm's sums with its mask as (scale, shift) (EPI 2) or as sign bytes (EPI 3).
Shapes: batch 2, 16 channels, width 130 (what the instantiation requires); heights 5, 33, 34, 70, and the two heights on either side
of the first strip boundary as the plan reports it (records per image = strips: the largest single-strip height and one row more).
Channel 3 has gamma < 0 (scale < 0), channel 5's mask is zero everywhere; c is edited so that |fma(c, scale, shift)| >= 1e-3 (a
mask bit that differed between fp32 and float64 would move dc by a whole |dy|).
Not fused, by the launch record: 32 channels, width 216, sums not given (through layers._bn_bwd_dgrad, the only caller)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_conv_training_epilogue_gpu.py: of the max-abs of the float64 result
MARGIN = 1e-3
EPS = 1e-5
B, C, W = 2, 16, 130
HEIGHTS = (5, 33, 34, 70)
FORMS = {'bits': (1, 3), 'aff_e2': (2, 2), 'aff_e3': (3, 2)}        # form -> (EPI, BNF) of the instantiation


@pytest.fixture(scope='module')
def dam(dam_lib):
    import deep_audio_mixer_amd  # noqa: F401
    from deep_audio_mixer_amd import layers, ops
    return layers, ops


def _sign_bytes(positive):
    b, h, w, c = positive.shape
    weights = torch.tensor([1, 2, 4, 8], dtype=torch.int32)
    return (positive.view(b, h, w, c // 4, 4).to(torch.int32) * weights).sum(-1).to(torch.uint8).contiguous()


def _signed(shape, g):
    m = torch.randn(shape, generator=g)
    return torch.where(m >= 0, m + 0.1, m - 0.1)


def _bn_of(x, gamma, beta):
    mean = x.double().mean((0, 1, 2)).float()
    invstd = (1.0 / torch.sqrt(x.double().var((0, 1, 2), unbiased=False) + EPS)).float()
    sc = gamma * invstd
    return mean, invstd, sc, beta - mean * sc


@functools.lru_cache(maxsize=None)
def inputs(form, H, ch=C, width=W):
    """Everything of one case on the CPU, with the float64 references of dc and dx."""
    g = torch.Generator().manual_seed(8100 + 97 * sorted(FORMS).index(form) + H + 7 * width + ch)
    shape = (B, H, width, ch)
    dy, c = torch.randn(shape, generator=g), torch.randn(shape, generator=g) * 1.5 + 0.3
    gamma, beta = torch.rand(ch, generator=g) + 0.5, 0.3 * torch.randn(ch, generator=g)
    gamma[3] = -gamma[3]                                         # scale < 0
    beta[5] = -100.0                                             # fma(c, scale, shift) <= 0 everywhere: an all-zero mask
    mean, invstd, sc, sh = _bn_of(c, gamma, beta)
    t = c.double() * sc.double() + sh.double()
    moved = (torch.where(t >= 0, 2 * MARGIN, -2 * MARGIN) - sh.double()) / sc.double()
    c = torch.where(t.abs() < MARGIN, moved, c.double()).float()
    t = c.double() * sc.double() + sh.double()
    assert t.abs().min().item() >= MARGIN and not bool((t[..., 5] > 0).any()) and sc[3].item() < 0
    if form == 'bits':
        pos = _signed(shape, g) > 0
        pos[..., 5] = False
    else:
        pos = t > 0
    assert 0.2 <= pos.double().mean().item() <= 0.8
    dz = dy.double() * pos
    xhat = (c.double() - mean.double()) * invstd.double()
    s1, s2 = dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))
    n = B * H * width
    gi = gamma.double() * invstd.double()
    dc64 = gi * (dz - s1 / n - xhat * s2 / n)
    # the two sums as three records of a data-gradient epilogue would leave them: image 0's rows split in two, image 1
    cut = max(1, H // 3)
    parts = [(dz[0, :cut], xhat[0, :cut]), (dz[0, cut:], xhat[0, cut:]), (dz[1], xhat[1])]
    rec = torch.stack([torch.stack([a.sum((0, 1)), (a * b).sum((0, 1))], -1) for a, b in parts]).float().contiguous()
    w = torch.randn(ch, ch, 3, 3, generator=g) / (ch * 9) ** 0.5
    dx64 = torch.nn.grad.conv2d_input((B, ch, H, width), w.double(), dc64.permute(0, 3, 1, 2), 1, 1, 1).permute(0, 2, 3, 1)
    d = dict(dy=dy, c=c, gamma=gamma, mean=mean, invstd=invstd, sc=sc, sh=sh, bits=_sign_bytes(pos), rec=rec, w=w, dc64=dc64)
    # the data gradient's own operands: the upstream BatchNorm (x1, affine mask or sign bytes), the identity shortcut
    x1 = torch.randn(shape, generator=g) * 1.5 + 0.3
    m1, i1, sc1, sh1 = _bn_of(x1, torch.rand(ch, generator=g) + 0.5, 0.3 * torch.randn(ch, generator=g))
    d.update(x1=x1, m1=m1, i1=i1, sc1=sc1, sh1=sh1)
    if form != 'bits':
        res, rmask = torch.randn(shape, generator=g), _signed(shape, g)
        dx64 = dx64 + (res * (rmask > 0)).double()
        d.update(res=res, rmask=rmask, rbits=_sign_bytes(rmask > 0), ubits=_sign_bytes(_signed(shape, g) > 0))
    d['dx64'] = dx64.contiguous()
    return d


def _dev(d):
    return {k: (v.cuda() if torch.is_tensor(v) and v.dtype != torch.float64 else v) for k, v in d.items()}


def _dgrad_kw(form, v):
    if form == 'bits':
        return dict(bn_bwd=(v['x1'], v['m1'], v['i1'], v['sc1'], v['sh1']))
    up = (v['x1'], v['m1'], v['i1'], v['sc1'], v['sh1']) if form == 'aff_e2' else (v['x1'], v['m1'], v['i1'], None, None, v['ubits'])
    return dict(res=v['res'], res_mask=v['rmask'], res_mask_bits=v['rbits'], bn_bwd=up)


def _records(ops, v, ch=C):
    """A fresh record buffer of the size bn_backward's workspace has, holding the case's three records."""
    from deep_audio_mixer_amd import _lib
    buf = torch.zeros(int(_lib.lib().dam_bn_workspace_floats(ch)), dtype=torch.float32, device='cuda')
    buf[:v['rec'].numel()] = v['rec'].reshape(-1)
    return buf, v['rec'].shape[0]


def _mask_kw(form, v):
    return (None, v['bits']) if form == 'bits' else ((v['sc'], v['sh']), None)


def strips_per_image(ops, H):
    """Strips (workgroups per image) of the fused data gradient at height H, from the plan: one record per strip and image."""
    rec, parts = ops.conv2d_dgrad_plan((B, H, W, C), C, H, W, 3, 3, 1, 1, 1, bn_bwd=(True, True, True, True, True), parts=True)
    assert rec.family == 'strip' and rec.SO == 1 and parts % B == 0, rec
    return parts // B


def boundary_heights(ops):
    """The largest height one strip covers and one row more (two strips), by the plan's own geometry."""
    h = 1
    while strips_per_image(ops, h + 1) == 1:
        h += 1
    return h, h + 1


def all_heights(ops):
    return sorted(set(HEIGHTS) | set(boundary_heights(ops)))


def test_heights_cover_the_strip_geometry(dam):
    """One strip, two strips (a boundary inside a row or on one), several strips with a shorter last one."""
    _, ops = dam
    one, two = boundary_heights(ops)
    assert strips_per_image(ops, one) == 1 and strips_per_image(ops, two) == 2
    counts = {h: strips_per_image(ops, h) for h in all_heights(ops)}
    print('strips per image by height:', counts)
    assert min(counts.values()) == 1 and max(counts.values()) >= 3


@pytest.mark.parametrize('form', sorted(FORMS))
def test_fused_is_bitwise_the_two_launches(dam, form):
    _, ops = dam
    epi, bnf = FORMS[form]
    for H in all_heights(ops):
        d = inputs(form, H)
        v = _dev(d)
        wpt = ops.pack_weights(v['w'], transpose=True)
        aff, bits = _mask_kw(form, v)
        kw = _dgrad_kw(form, v)
        plan = ops.conv2d_dgrad_plan(v['dy'].shape, C, H, W, 3, 3, 1, 1, 1, bn_in=(True, True, aff, bits), **kw)
        assert (plan.family, plan.EPI, plan.SO, plan.BNF) == ('strip', epi, 1, bnf), plan
        # the two launches
        dc0, dg0, db0 = ops.bn_backward(v['dy'], None, v['c'], v['gamma'], v['mean'], v['invstd'], True, mask_affine=aff, mask_bits=bits,
                                        partials=_records(ops, v))
        dx0, sums0 = ops.conv2d_dgrad(dc0, wpt, C, H, W, 3, 3, 1, 1, 1, **kw)
        rec0 = ops.conv_last_launch()
        assert (rec0.EPI, rec0.SO, rec0.BNF) == (epi, 1, 0), rec0
        # finalize-only + the fused data gradient
        coef, dg1, db1 = ops.bn_backward_finalize(_records(ops, v), v['c'], v['gamma'], v['mean'], v['invstd'], True)
        dx1, sums1, dc1 = ops.conv2d_dgrad(v['dy'], wpt, C, H, W, 3, 3, 1, 1, 1, bn_in=(v['c'], coef, aff, bits), **kw)
        rec1 = ops.conv_last_launch()
        assert rec1 == plan, (rec1, plan)
        torch.cuda.synchronize()
        what = '%s H=%d' % (form, H)
        assert torch.equal(dg0, dg1) and torch.equal(db0, db1), what + ': dgamma / dbeta'
        assert torch.equal(dc0, dc1), '%s: dc differs in %d elements' % (what, int((dc0 != dc1).sum()))
        assert torch.equal(dx0, dx1), '%s: dx differs in %d elements' % (what, int((dx0 != dx1).sum()))
        assert sums0 is not None and sums1 is not None and sums0[1] == sums1[1] == strips_per_image(ops, H) * B, what
        n = sums0[1] * C * 2
        assert torch.equal(sums0[0][:n], sums1[0][:n]), what + ': upstream-sum records'
        for name, got, want in (('dc', dc1, d['dc64']), ('dx', dx1, d['dx64'])):
            scale = want.abs().max().item()
            err = (got.cpu().double() - want).abs().max().item()
            print('%s: %s err %.2e of scale %.3g' % (what, name, err / scale, scale))
            assert err <= TOL * scale, '%s: %s err %.3g > %.3g' % (what, name, err, TOL * scale)


def _spec_call(layers, ops, form, H, ch, width, partials):
    """layers._bn_bwd_dgrad (what BasicBlockFn.backward calls) on a case -> the launch record of its data gradient."""
    d = inputs(form, H, ch, width)
    v = _dev(d)
    spec = layers.ConvSpec(ch, ch, 3, 1, 1)
    aff, bits = _mask_kw(form, v)
    rec = _records(ops, v, ch) if partials else None
    seen = []
    layers._bn_bwd_dgrad(spec, v['w'], (H, width), v['dy'], v['c'], v['gamma'], v['mean'], v['invstd'], True, rec, None, None,
                         aff, bits, seen.append, **_dgrad_kw(form, v))
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].shape == v['c'].shape           # the weight gradient was handed dc
    got = ops.conv_last_launch()
    scale = d['dc64'].abs().max().item()
    assert (seen[0].cpu().double() - d['dc64']).abs().max().item() <= TOL * scale
    return got


@pytest.mark.parametrize('form', sorted(FORMS))
def test_eligible_shape_takes_the_fused_instantiation(dam, form):
    layers, ops = dam
    got = _spec_call(layers, ops, form, 5, C, W, True)
    assert (got.family, got.MB, got.NB, got.NCH, got.EPI, got.SO, got.BNF) == ('strip', 4, 1, 1) + (FORMS[form][0], 1, FORMS[form][1]), got


@pytest.mark.parametrize('ch,width,partials', [(32, 66, True), (16, 216, True), (16, W, False)], ids=['32ch', 'w216', 'no_sums'])
@pytest.mark.parametrize('form', ['bits', 'aff_e2'])
def test_everything_else_takes_the_unfused_launch(dam, form, ch, width, partials):
    """32 channels, the wide rows and a call without the sums: bn_backward's launches, then the data gradient without BNF."""
    layers, ops = dam
    got = _spec_call(layers, ops, form, 5, ch, width, partials)
    assert got.family == 'strip' and got.BNF == 0, got
    if ch == 16:
        assert got.EPI == FORMS[form][0] and got.LW == (1 if width == 216 else 0), got


def test_identity_block_backward_is_bitwise_the_unfused_one(dam, monkeypatch):
    """stem -> two identity blocks (B = 2, 5 x 130) through layers: every gradient with the fused launches is bitwise the gradient
    with the plan answering "not fused" (the apply launch + data gradient of before)."""
    layers, ops = dam
    from _randomize import _randomize
    from _inputs import model_input

    def run(fused):
        gen = torch.Generator().manual_seed(21)
        S, H = 8, 5
        stem = _randomize(torch.nn.Sequential(torch.nn.Conv2d(S, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)), gen).cuda().train()
        blks = [_randomize(layers.BasicBlock(16, 16, 1), gen).cuda().train() for _ in range(2)]
        spec = layers.ConvSpec(S, 16, 3, 1, 1, in_nchw=True)
        x = torch.from_numpy(model_input(B, S, H, W, seed=5)[0]).cuda()
        dout = torch.randn((B, H, W, 16), generator=gen).cuda()
        seen = []
        real = ops.conv2d_dgrad_plan
        with monkeypatch.context() as mp:
            def plan(*a, **kw):
                rec = real(*a, **kw)
                if 'bn_in' in kw:
                    rec = rec if fused else rec._replace(BNF=0)
                    seen.append(rec.BNF)
                return rec
            mp.setattr(ops, 'conv2d_dgrad_plan', plan)
            a0 = layers.ConvBnReluFn.apply(x, stem[0].weight, None, stem[1].weight, stem[1].bias, spec, stem[1], True)
            out = blks[1](blks[0](a0))
            out.backward(dout)
            ops.wgrad_flush()
        torch.cuda.synchronize()
        params = list(stem.parameters()) + [p for b in blks for p in b.parameters()]
        return [p.grad.clone() for p in params], seen

    g1, seen1 = run(True)
    g0, seen0 = run(False)
    # bn2 of the last block has no consumer that left its sums; the other three BatchNorm backwards sit behind an epilogue
    assert sorted(seen1) == [2, 2, 3] and seen0 == [0, 0, 0], (seen1, seen0)
    assert len(g0) == len(g1) == 3 + 2 * 6            # stem: conv weight, gamma, beta; a block: two convolutions, two BatchNorms
    for i, (a, b) in enumerate(zip(g0, g1)):
        assert torch.equal(a, b), 'parameter %d: %d elements differ' % (i, int((a != b).sum()))
