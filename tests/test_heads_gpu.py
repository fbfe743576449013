"""GPU: the conv-bias gradient (dam_channel_sum_f32), the gain heads, the gain-weighted sum and the fused MSE (dam_head.hip) at
the kernel level against float64, and the two branches of the heads' autograd Functions the training step never takes: a loss
that also uses the returned gains (HeadsFn: dg + dg_out) and a non-unit seed of forward_mse's loss (HeadsMseFn: dg * dloss).

Every reduction runs twice.  On small-integer inputs, chosen so that every partial and final sum stays below 2^24 in magnitude
(the test asserts that bound from the absolute values), each float32 sum is exact in any order: the result must EQUAL the
float64 one, which catches a dropped or doubled pixel, stem, record or tail element that a relative tolerance over 1e5-1e6
terms would not.  On random floats: 2e-5 of the norm, or 1e-6 of the sum of |term| for a single sum."""
import pytest
import torch
import torch.nn.functional as F

from _inputs import model_input
from _model_check import best_over_seeds
from oracle import models_ref

pytestmark = pytest.mark.gpu
TOL = 2e-5
EXACT = 2.0 ** 24


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double()
    return float((got - want).norm() / (want.norm() + 1e-300))


def _equal(name, got, want):
    got = got.detach().double().cpu()
    want = want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.equal(got, want), (name, float((got - want).abs().max()))


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


# ---------------------------------------------------------------------------------------------------------- A. channel_sum
def _bn_plan_r(C):
    """Pixel rows per workgroup of dam_bn.hip:bn_plan (threads = C/4 * r, ~16 pixels per thread, at most 1024 workgroups)."""
    return max(1, 256 // (C // 4))


def _pixel_counts(C):
    r = _bn_plan_r(C)
    prime = 100003 if C <= 128 else 30011                  # (a prime around 1e5 pixels; fewer for the widest rows)
    capped = 1024 * r * 16 + 4099                          # more than 1024 workgroups of r * 16 pixels: bn_plan caps parts
    return [1, 7, r * 16 + 1, prime, capped]


@pytest.mark.parametrize('C', [16, 32, 48, 64, 96, 128, 256, 1024])
@pytest.mark.parametrize('kind', ['exact', 'float'])
def test_channel_sum(ops, C, kind):
    """ops.channel_sum (the conv-bias gradient of ConvBlock2d) over 1, 7, one past a workgroup's 16 * r, a prime and a parts-capped
    pixel count; C = 48 / 96 give a non-power-of-two r in the tree reduction.  n_real < C writes n_real sums and nothing after."""
    gen = torch.Generator().manual_seed(C)
    worst = 0.0
    for P in _pixel_counts(C):
        x = _ints((P, C), -3, 3, gen) if kind == 'exact' else torch.randn((P, C), generator=gen)
        want = x.double().sum(0)
        mag = x.double().abs().sum(0)
        n_real = C - 5 if P % 2 else C
        out = torch.full((C,), float('nan'), device='cuda')
        got = ops.channel_sum(x.cuda(), n_real, out=out[:n_real])
        assert got.data_ptr() == out.data_ptr()
        assert torch.isnan(out[n_real:]).all(), 'channel_sum wrote past n_real'
        got = out[:n_real].double().cpu()
        if kind == 'exact':
            assert float(mag.max()) < EXACT
            _equal('channel_sum C=%d P=%d' % (C, P), got, want[:n_real])
        else:
            err = float(((got - want[:n_real]).abs() / mag[:n_real]).max())
            worst = max(worst, err)
            assert err <= 1e-6, (C, P, err)
    print('channel_sum C=%d %s: worst |err| / sum|x| %.1e' % (C, kind, worst))


# ---------------------------------------------------------------------------------------------------------- B. heads kernels
# S, C, P, B: every stem count, the three lane-group widths (C/4 <= 16 / <= 32 / more: 16 / 32 / 64 lanes per pixel), pixel counts
# past 1024 workgroups * pixels per workgroup (16384 / 8192 / 4096: the grid-stride loop turns), and S*C large enough that the
# weight-gradient pass shrinks its rows (16 x 256, 16 x 16, 16 x 1024)
HEAD_CASES = [(1, 16, 1, 1), (2, 64, 7, 3), (3, 128, 231, 8), (4, 256, 1320, 3), (5, 512, 20049, 1), (8, 1024, 231, 2),
              (16, 16, 20049, 2), (16, 256, 1320, 2), (16, 1024, 7, 1), (2, 256, 5003, 3), (3, 128, 9001, 1), (8, 128, 1320, 8)]


def _ref_heads(trunk, cw, cb, fw, fb, mask=None):
    """models_ref._Heads._run_heads (per stem: conv1x1 -> ReLU -> flatten -> Linear) on an NHWC trunk, with the ReLU decisions
    given (models_ref.masked_relu) -> (h [B, S, P], gains [B, S], pre-activations [B, S, P])."""
    B, C = trunk.shape[0], trunk.shape[-1]
    t = trunk.permute(0, 3, 1, 2)
    hs, gains, pre = [], [], []
    for s in range(cw.shape[0]):
        v = F.conv2d(t, cw[s].view(1, C, 1, 1), cb[s:s + 1])
        h, z = models_ref.masked_relu(v, None if mask is None else mask[:, s].view(v.shape))
        hs.append(h.reshape(B, -1)), pre.append(z.reshape(B, -1))
        gains.append(F.linear(h.reshape(B, -1), fw[s:s + 1], fb[s:s + 1]))
    return torch.stack(hs, 1), torch.cat(gains, 1), torch.stack(pre, 1)


def _head_inputs(S, C, P, B, kind, gen):
    shp = [(B, P, 1, C), (S, C), (S,), (S, P), (S,), (B, S)]
    if kind == 'exact':
        return [_ints(s, lo, hi, gen) for s, (lo, hi) in zip(shp, [(-1, 1), (-2, 2), (-3, 3), (-2, 2), (-3, 3), (-2, 2)])]
    trunk = torch.relu(torch.randn(shp[0], generator=gen))
    return [trunk, torch.randn(shp[1], generator=gen) * C ** -0.5, 0.1 * torch.randn(shp[2], generator=gen),
            torch.randn(shp[3], generator=gen) * P ** -0.5, torch.randn(shp[4], generator=gen), torch.randn(shp[5], generator=gen)]


@pytest.mark.parametrize('S,C,P,B', HEAD_CASES, ids=['S%d-C%d-P%d-B%d' % c for c in HEAD_CASES])
@pytest.mark.parametrize('kind', ['exact', 'float'])
def test_heads_fwd_bwd(ops, S, C, P, B, kind):
    """ops.heads_fwd / heads_bwd: h, gains, dtrunk, dconv_w, dconv_b, dfc_w, dfc_b against float64 autograd of the reference
    head.  Float inputs: the oracle takes the device's ReLU decisions, which may differ from its own only at rounding level."""
    gen = torch.Generator().manual_seed(1000 * S + C + P)
    trunk, cw, cb, fw, fb, dg = _head_inputs(S, C, P, B, kind, gen)
    h, g = ops.heads_fwd(trunk.cuda(), cw.cuda(), cb.cuda(), fw.cuda(), fb.cuda())
    dtrunk, dcw, dcb, dfw, dfb = ops.heads_bwd(dg.cuda(), h, trunk.cuda(), cw.cuda(), fw.cuda())
    torch.cuda.synchronize()
    leaves = [t.double().requires_grad_(True) for t in (trunk, cw, cb, fw, fb)]
    mask = None if kind == 'exact' else (h > 0).cpu()
    h_r, g_r, pre = _ref_heads(*leaves, mask=mask)
    grads = torch.autograd.grad(g_r, leaves, dg.double())
    got = [('h', h, h_r), ('gains', g, g_r), ('dtrunk', dtrunk, grads[0]), ('dconv_w', dcw, grads[1]), ('dconv_b', dcb, grads[2]),
           ('dfc_w', dfw, grads[3]), ('dfc_b', dfb, grads[4])]
    if kind == 'exact':
        # the same arithmetic on |inputs| with every ReLU open bounds every partial sum of every output
        absl = [t.double().abs().requires_grad_(True) for t in (trunk, cw, cb, fw, fb)]
        ha, ga, _ = _ref_heads(*absl, mask=torch.ones(B, S, P, dtype=torch.bool))
        bound = max([float(ha.max()), float(ga.max())] + [float(t.max()) for t in torch.autograd.grad(ga, absl, dg.double().abs())])
        assert bound < EXACT, bound
        for name, a, b in got:
            _equal(name, a, b)
        return
    diff = mask != (pre > 0)
    worst_flip = float(pre[diff].abs().max()) if diff.any() else 0.0
    assert worst_flip < 1e-5, ('ReLU decision differs at', worst_flip)
    errs = {name: _rel(a, b) for name, a, b in got}
    print('heads S=%d C=%d P=%d B=%d: %s' % (S, C, P, B, ', '.join('%s %.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs


# S, FT (= F * T), B: every stem count (2 / 4 / 8: the compile-time paths; the rest: the run-time one), odd and even plane
# lengths below 1024 and above 2 * 256 * 1024 (the stride walk of the partial pass wraps; U = 2 for the compile-time counts)
MASK_CASES = [(1, 7, 1), (2, 1000, 3), (4, 1023, 3), (3, 999, 8), (16, 231, 3), (3, 1320, 8), (4, 524289, 1), (5, 524294, 2),
              (8, 524296, 1), (2, 600001, 2), (16, 524290, 1), (8, 777, 2)]


def _ref_masked(x, g):
    """models_ref._Heads._run_heads: masked = sum_s g_s * x[:, s]."""
    masked = torch.zeros_like(x[:, 0])
    for s in range(x.shape[1]):
        masked = masked + g[:, s:s + 1].unsqueeze(2) * x[:, s]
    return masked


@pytest.mark.parametrize('S,FT,B', MASK_CASES, ids=['S%d-FT%d-B%d' % c for c in MASK_CASES])
@pytest.mark.parametrize('kind', ['exact', 'float'])
def test_masksum_and_mse(ops, S, FT, B, kind):
    """ops.masksum_fwd / masksum_bwd / masksum_mse: masked, dgains and the loss against float64 autograd."""
    gen = torch.Generator().manual_seed(S * 7 + FT)
    shape = (B, S, 1, FT)
    if kind == 'exact':
        x, g, dm = _ints(shape, -2, 2, gen), _ints((B, S), -3, 3, gen), _ints((B, 1, FT), -2, 2, gen)
        gt = _ref_masked(x.double(), g.double()) + _ints((B, 1, FT), -2, 2, gen).double()
        assert float(_ref_masked(x.abs().double(), g.abs().double()).max()) < EXACT
        # sum_i |d x_s|, sum_i d^2 per (b, s): both differences are at most 2 in magnitude
        assert 4.0 * FT < EXACT
        gt = gt.float()
    else:
        x = -20.0 + 15.0 * torch.randn(shape, generator=gen)
        g, dm = torch.randn((B, S), generator=gen), torch.randn((B, 1, FT), generator=gen)
        gt = (_ref_masked(x.double(), g.double()) + torch.randn((B, 1, FT), generator=gen).double()).float()
    xc, gc = x.cuda(), g.cuda()
    masked = ops.masksum_fwd(xc, gc)
    dg = ops.masksum_bwd(dm.cuda(), xc)
    m2, loss, dg2 = ops.masksum_mse(xc, gc, gt.cuda())
    torch.cuda.synchronize()
    xr, gr = x.double(), g.double().requires_grad_(True)
    masked_r = _ref_masked(xr, gr)
    dg_r, = torch.autograd.grad(masked_r, gr, dm.double())
    gr2 = g.double().requires_grad_(True)
    loss_r = F.mse_loss(_ref_masked(xr, gr2), gt.double())
    dg2_r, = torch.autograd.grad(loss_r, gr2)
    if kind == 'exact':
        n = B * FT
        d = masked_r.detach() - gt.double()
        _equal('masked', masked, masked_r)
        _equal('masked (mse)', m2, masked_r)
        _equal('dgains', dg, dg_r)
        # the kernel scales the exact sums in double: 1 / count and 2 / count
        _equal('loss', loss, torch.tensor([float((d * d).sum()) * (1.0 / n)], dtype=torch.float32))
        sdx = torch.stack([(d[:, 0] * xr[:, s, 0]).sum(-1) for s in range(S)], 1)
        _equal('dgains (mse)', dg2, (sdx * (2.0 / n)).float())
        assert float((dg2_r - sdx * (2.0 / n)).abs().max()) <= 1e-12 * float(sdx.abs().max() * (2.0 / n)) + 1e-300
        return
    mag = torch.stack([(dm.double().abs()[:, 0] * xr.abs()[:, s, 0]).sum(-1) for s in range(S)], 1)
    # the fused pass's d = sum_s' g_s' x_s' - gt is a difference of large numbers: its own rounding is of the order of
    # eps * (sum_s' |g_s' x_s'| + |gt|), the magnitude each term (d * x_s, d^2) carries
    d = (masked_r.detach() - gt.double()).abs()[:, 0]
    big = _ref_masked(xr.abs(), g.double().abs())[:, 0] + gt.double().abs()[:, 0]
    mag2 = torch.stack([((d + big) * xr.abs()[:, s, 0]).sum(-1) for s in range(S)], 1) * 2.0 / (B * FT)
    mag_loss = float((d * (d + 2 * big)).sum()) / (B * FT)
    errs = {'masked': _rel(masked, masked_r), 'masked (mse)': _rel(m2, masked_r),
            'dgains': float(((dg.double().cpu() - dg_r) / mag).abs().max()),
            'dgains (mse)': float(((dg2.double().cpu() - dg2_r) / mag2).abs().max()),
            'loss': abs(float(loss) - float(loss_r)) / mag_loss}
    print('masksum S=%d FT=%d B=%d: %s' % (S, FT, B, ', '.join('%s %.1e' % kv for kv in errs.items())))
    assert errs['masked'] <= TOL and errs['masked (mse)'] <= TOL, errs
    assert errs['dgains'] <= 1e-6 and errs['dgains (mse)'] <= 1e-6 and errs['loss'] <= 1e-6, errs


def test_heads_unsupported_shapes_fail_loudly(ops):
    """S > 16 stems, C % 16 in the backward, C % 4 in the forward: refused with an error, nothing launched."""
    gen = torch.Generator().manual_seed(5)
    cu = lambda *shape: torch.randn(shape, generator=gen).cuda()
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.heads_fwd(cu(2, 3, 1, 32), cu(17, 32), cu(17), cu(17, 3), cu(17))
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.heads_bwd(cu(2, 17), cu(2, 17, 3), cu(2, 3, 1, 32), cu(17, 32), cu(17, 3))
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.heads_fwd(cu(2, 3, 1, 18), cu(2, 18), cu(2), cu(2, 3), cu(2))
    # C = 20 (C % 4 == 0): the forward takes it, the backward does not
    trunk, cw, cb, fw, fb = cu(2, 3, 1, 20), cu(2, 20), cu(2), cu(2, 3), cu(2)
    h, g = ops.heads_fwd(trunk, cw, cb, fw, fb)
    h_r, g_r, _ = _ref_heads(*(t.double().cpu() for t in (trunk, cw, cb, fw, fb)))
    assert _rel(h, h_r) <= TOL and _rel(g, g_r) <= TOL
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.heads_bwd(cu(2, 2), h, trunk, cw, fw)
    x17 = cu(1, 17, 2, 8)
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.masksum_fwd(x17, cu(1, 17))
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.masksum_bwd(cu(1, 2, 8), x17)
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        ops.masksum_mse(x17, cu(1, 17), cu(1, 2, 8))


# ---------------------------------------------------------------------------------------------------------- C. autograd branches
@pytest.fixture(scope='module')
def layers(dam_lib):
    from deep_audio_mixer_amd import layers
    return layers


def _head_fn_case(seed, S=4, C=128, B=2, hw=(17, 3), FT=(257, 64)):
    gen = torch.Generator().manual_seed(seed)
    P = hw[0] * hw[1]
    trunk = torch.relu(torch.randn((B,) + hw + (C,), generator=gen))
    params = [torch.randn((S, C), generator=gen) * C ** -0.5, 0.1 * torch.randn(S, generator=gen),
              torch.randn((S, P), generator=gen) * P ** -0.5, torch.randn(S, generator=gen)]
    x, gt = model_input(B, S, FT[0], FT[1], seed=seed)
    return trunk, params, torch.from_numpy(x), torch.from_numpy(gt)


def test_heads_fn_loss_on_masked_and_gains(layers):
    """HeadsFn.backward with BOTH incoming gradients (dg + dg_out): loss = mse(masked, gt) + lam * sum(gains^2)."""
    trunk, params, x, gt = _head_fn_case(3)
    trunk_c = trunk.cuda().requires_grad_(True)
    params_c = [p.cuda().requires_grad_(True) for p in params]
    masked, g = layers.HeadsFn.apply(trunk_c, x.cuda(), *params_c)
    mse = F.mse_loss(masked, gt.cuda())
    lam = float(mse) / float((g * g).sum())             # both terms of the same size
    (mse + lam * (g * g).sum()).backward()
    h, _ = layers.ops.heads_fwd(trunk_c.detach(), *[p.detach() for p in params_c])
    leaves = [trunk.double().requires_grad_(True)] + [p.double().requires_grad_(True) for p in params]
    _, g_r, pre = _ref_heads(*leaves, mask=(h > 0).cpu())
    flips = (h > 0).cpu() != (pre > 0)
    assert not flips.any() or float(pre[flips].abs().max()) < 1e-5
    masked_r = _ref_masked(x.double(), g_r)
    (F.mse_loss(masked_r, gt.double()) + lam * (g_r * g_r).sum()).backward()
    errs = {n: _rel(a.grad, b.grad) for n, a, b in zip(('dtrunk', 'dconv_w', 'dconv_b', 'dfc_w', 'dfc_b'), [trunk_c] + params_c, leaves)}
    errs['masked'], errs['gains'] = _rel(masked, masked_r), _rel(g, g_r)
    print('HeadsFn, loss on masked and gains: %s' % ', '.join('%s %.1e' % kv for kv in errs.items()))
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize('form', ['scaled', 'sum'])
def test_heads_mse_fn_non_unit_seed(layers, form):
    """HeadsMseFn.backward with dloss != 1: (3 * loss).backward(), and loss + another loss on a head parameter."""
    trunk, params, x, gt = _head_fn_case(4)
    trunk_c = trunk.cuda().requires_grad_(True)
    params_c = [p.cuda().requires_grad_(True) for p in params]
    loss, masked, g = layers.HeadsMseFn.apply(trunk_c, x.cuda(), gt.cuda(), *params_c)
    total = 3.0 * loss if form == 'scaled' else loss + 0.5 * (params_c[3] ** 2).sum()
    total.backward()
    h, _ = layers.ops.heads_fwd(trunk_c.detach(), *[p.detach() for p in params_c])
    leaves = [trunk.double().requires_grad_(True)] + [p.double().requires_grad_(True) for p in params]
    _, g_r, _ = _ref_heads(*leaves, mask=(h > 0).cpu())
    loss_r = F.mse_loss(_ref_masked(x.double(), g_r), gt.double())
    (3.0 * loss_r if form == 'scaled' else loss_r + 0.5 * (leaves[4] ** 2).sum()).backward()
    errs = {n: _rel(a.grad, b.grad) for n, a, b in zip(('dtrunk', 'dconv_w', 'dconv_b', 'dfc_w', 'dfc_b'), [trunk_c] + params_c, leaves)}
    errs['loss'] = abs(float(loss) - float(loss_r)) / float(loss_r)
    print('HeadsMseFn, %s: %s' % (form, ', '.join('%s %.1e' % kv for kv in errs.items())))
    assert max(errs.values()) <= TOL, errs


@pytest.fixture(scope='module')
def models(dam_lib):
    import deep_audio_mixer_amd.models.model_resnet as mr
    import deep_audio_mixer_amd.models.model_scalar_1s as m1
    import deep_audio_mixer_amd.models.model_scalar_2s as m2
    return {'resnet18': (mr.ResNet18, models_ref.RefResNet18),
            'scalar1s': (m1.MixingModelScalar1s, models_ref.RefMixingModelScalar1s),
            'scalar2s': (m2.MixingModelScalar2s, models_ref.RefMixingModelScalar2s)}


MODEL_SHAPES = [('resnet18', (2, 4, 257, 64)), ('scalar1s', (2, 4, 257, 87)), ('scalar2s', (2, 4, 257, 93))]


@pytest.mark.parametrize('name,shape', MODEL_SHAPES, ids=[m[0] for m in MODEL_SHAPES])
def test_model_loss_on_masked_and_gains(models, name, shape):
    """model(x) with loss = mse(masked, gt) + lam * sum(gains^2) through the whole trunk, against the float64 oracle."""
    ctor, ref_ctor = models[name]
    lam = 1e-2

    def run(m, x, gt):
        masked, gains = m(x)
        g = torch.cat(gains, 1)
        return F.mse_loss(masked, gt) + lam * (g * g).sum(), g
    best_over_seeds(ctor, ref_ctor, shape, run, run)


@pytest.mark.parametrize('name,shape', MODEL_SHAPES, ids=[m[0] for m in MODEL_SHAPES])
def test_model_forward_mse_non_unit_seed(models, name, shape):
    """model.forward_mse seeded with 3, plus a second loss on the head biases, against the float64 oracle."""
    ctor, ref_ctor = models[name]

    def dev(m, x, gt):
        loss, _, gains = m.forward_mse(x, gt)
        return 3.0 * loss + 0.5 * (m._heads.fc_b ** 2).sum(), torch.cat(gains, 1)

    def ref(m, x, gt):
        masked, gains = m(x)
        reg = sum((getattr(m, 'fc_head%d' % (i + 1)).bias ** 2).sum() for i in range(m.n_stems))
        return 3.0 * F.mse_loss(masked, gt) + 0.5 * reg, torch.cat(gains, 1)
    best_over_seeds(ctor, ref_ctor, shape, dev, ref)
