"""GPU: backward through BatchNorm in eval mode (running statistics), against float64: fine-tuning with frozen BatchNorm, or
gradients of the gains with respect to a layer.  Kernels (ops.bn_backward / bn_backward_pair with training=False in every mask
mode, ops.bn_eval_affine), blocks (the identity and down-sampling residual blocks, the stem -> layer1 chain whose BatchNorm sums
come out of the next layer's data gradient, the scalar models' ConvBlock2d whose conv-bias gradient is NOT zero here) and the
three models.

The block tests use the construction of tests/test_blocks_gpu.py: the float64 oracle takes the device's ReLU decisions, and the
test asserts separately that those differ from the oracle's own only where the pre-activation is at rounding level."""
import pytest
import torch

from _inputs import model_input
from _model_check import best_over_seeds
from _randomize import _randomize, _running_stats
from oracle import models_ref

pytestmark = pytest.mark.gpu
TOL = 2e-5
FLIP_LEVEL = 2e-5
EXACT = 2.0 ** 24


@pytest.fixture(scope='module')
def dam(dam_lib):
    import deep_audio_mixer_amd  # noqa: F401
    from deep_audio_mixer_amd import layers, ops
    torch.set_num_threads(16)
    return layers, ops


def _rel(got, want):
    return float((got.detach().double().cpu() - want.detach().double()).norm() / (want.detach().double().norm() + 1e-300))


def _sign_bytes(mask):
    """bn_apply(sign_bits=True)'s layout: one byte per channel quad, bit i = channel 4q + i."""
    m = mask.view(*mask.shape[:-1], mask.shape[-1] // 4, 4).to(torch.uint8)
    return m[..., 0] | (m[..., 1] << 1) | (m[..., 2] << 2) | (m[..., 3] << 3)


# ---------------------------------------------------------------------------------------------------------------- kernels
BN_SHAPES = [(2, 37, 23, 16), (3, 9, 5, 256), (4, 129, 17, 96), (8, 65, 33, 64), (1, 5, 3, 16), (2, 33, 17, 1024)]


def _ref_bn_eval(x, gamma, beta, mean, var, eps, dy, mask):
    """float64 autograd of y = [mask *] bn_eval(x) -> (dx, dgamma, dbeta, pre-activation)."""
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    v = (xr - mean.double()) / torch.sqrt(var.double() + eps) * gr + br
    y = v if mask is None else models_ref.masked_relu(v, mask)[0]
    y.backward(dy.double())
    return xr.grad, gr.grad, br.grad, v.detach()


@pytest.mark.parametrize('B,H,W,C', BN_SHAPES, ids=['%dx%dx%dx%d' % s for s in BN_SHAPES])
def test_bn_backward_eval_float(dam, B, H, W, C):
    """bn_eval_affine, then bn_backward(training=False) with the mask from the saved output, from the fused affine, from the
    sign bytes and without a mask, and bn_backward_pair(training=False), against float64 autograd of relu(bn_eval(x))."""
    _, ops = dam
    gen = torch.Generator().manual_seed(C + H)
    eps = 1e-3
    shape = (B, H, W, C)
    rm, rv = _running_stats(C, gen)
    x = rm + torch.sqrt(rv) * torch.randn(shape, generator=gen) * 1.5
    gamma, beta, dy = torch.rand(C, generator=gen) + 0.5, 0.5 * torch.randn(C, generator=gen), torch.randn(shape, generator=gen)
    cu = lambda t: t.cuda()
    sm, si, sc, sh = ops.bn_eval_affine(cu(gamma), cu(beta), cu(rm), cu(rv), eps)
    inv = 1.0 / torch.sqrt(rv.double() + eps)
    errs = {'mean': _rel(sm, rm), 'invstd': _rel(si, inv), 'scale': _rel(sc, gamma.double() * inv),
            'shift': _rel(sh, beta.double() - rm.double() * gamma.double() * inv)}
    assert max(errs.values()) <= 1e-6, errs
    y, bits = ops.bn_apply(cu(x), sc, sh, relu=True, sign_bits=True)
    mask = (y > 0).cpu()
    dx_r, dg_r, db_r, pre = _ref_bn_eval(x, gamma, beta, rm, rv, eps, dy, mask)
    flips = mask != (pre > 0)
    assert not flips.any() or float(pre[flips].abs().max()) < FLIP_LEVEL
    assert torch.equal(bits.cpu(), _sign_bytes(mask))
    for mode, kw in (('saved', dict()), ('affine', dict(mask_affine=(sc, sh))), ('bits', dict(mask_bits=bits))):
        dx, dgm, dbt = ops.bn_backward(cu(dy), y if mode == 'saved' else None, cu(x), cu(gamma), sm, si, False, **kw)
        e = {'dx': _rel(dx, dx_r), 'dgamma': _rel(dgm, dg_r), 'dbeta': _rel(dbt, db_r)}
        errs.update({'%s %s' % (mode, k): v for k, v in e.items()})
    dx_n, dg_n, db_n, _ = _ref_bn_eval(x, gamma, beta, rm, rv, eps, dy, None)
    dx, dgm, dbt = ops.bn_backward(cu(dy), None, cu(x), cu(gamma), sm, si, False)
    errs.update({'none dx': _rel(dx, dx_n), 'none dgamma': _rel(dgm, dg_n), 'none dbeta': _rel(dbt, db_n)})
    # the pair: a second BatchNorm (its own input and statistics) behind the same dy and mask
    rm2, rv2 = _running_stats(C, gen)
    x2, gamma2 = rm2 + torch.sqrt(rv2) * torch.randn(shape, generator=gen), torch.rand(C, generator=gen) + 0.5
    sm2, si2, _, _ = ops.bn_eval_affine(cu(gamma2), cu(beta), cu(rm2), cu(rv2), eps)
    dx2_r, dg2_r, db2_r, _ = _ref_bn_eval(x2, gamma2, beta, rm2, rv2, eps, dy * mask, None)
    for mode in ('saved', 'bits'):
        (a, b) = ops.bn_backward_pair(cu(dy), y if mode == 'saved' else None, (cu(x), cu(gamma), sm, si, None, None),
                                      (cu(x2), cu(gamma2), sm2, si2, None, None), False, mask_bits=bits if mode == 'bits' else None)
        for tag, (d, want) in (('a', (a, (dx_r, dg_r, db_r))), ('b', (b, (dx2_r, dg2_r, db2_r)))):
            for k, got, w in zip(('dx', 'dgamma', 'dbeta'), d, want):
                errs['pair %s %s %s' % (mode, tag, k)] = _rel(got, w)
    worst = max(errs.items(), key=lambda kv: kv[1])
    print('bn eval backward %s: worst %s %.1e' % (shape, worst[0], worst[1]))
    assert worst[1] <= TOL, errs


@pytest.mark.parametrize('B,H,W,C', BN_SHAPES, ids=['%dx%dx%dx%d' % s for s in BN_SHAPES])
def test_bn_backward_eval_exact(dam, B, H, W, C):
    """Integer data, integer mean, power-of-two invstd and gamma: every sum of the eval-mode backward is exact in float32, so
    dx, dgamma and dbeta EQUAL the float64 result in every mask mode and in the pair (a dropped or doubled pixel, a stray
    batch-statistics term fails)."""
    _, ops = dam
    gen = torch.Generator().manual_seed(3 * C + W)
    shape = (B, H, W, C)
    ints = lambda shp, lo, hi: torch.randint(lo, hi + 1, shp, generator=gen).float()
    x, x2, dy = ints(shape, -8, 8), ints(shape, -8, 8), ints(shape, -3, 3)
    mean, mean2 = ints((C,), -2, 2), ints((C,), -2, 2)
    invstd, invstd2 = 2.0 ** ints((C,), -1, 1), 2.0 ** ints((C,), -1, 1)
    gamma, gamma2 = ints((C,), -2, 2), ints((C,), -2, 2)
    sc, sh = ints((C,), -1, 1), ints((C,), -3, 3)                   # mask = (x * sc + sh > 0), exact
    y = torch.relu(x * sc + sh)
    mask = y > 0
    n = B * H * W
    assert 3 * 10 * 2 * n < EXACT                                   # |dz| <= 3, |(x - mean) * invstd| <= 20

    def want(xx, mu, iv, gm, m):
        dz = (dy * m).double() if m is not None else dy.double()
        xhat = (xx.double() - mu.double()) * iv.double()
        return dz * (gm.double() * iv.double()), (dz * xhat).sum((0, 1, 2)), dz.sum((0, 1, 2))
    cu = lambda t: t.cuda()
    bits = cu(_sign_bytes(mask))
    for mode, kw in (('saved', dict()), ('affine', dict(mask_affine=(cu(sc), cu(sh)))), ('bits', dict(mask_bits=bits)),
                     ('none', dict())):
        got = ops.bn_backward(cu(dy), cu(y) if mode == 'saved' else None, cu(x), cu(gamma), cu(mean), cu(invstd), False, **kw)
        for k, a, b in zip(('dx', 'dgamma', 'dbeta'), got, want(x, mean, invstd, gamma, None if mode == 'none' else mask)):
            assert torch.equal(a.double().cpu(), b), (mode, k, float((a.double().cpu() - b).abs().max()))
    for mode in ('saved', 'bits'):
        pa, pb = ops.bn_backward_pair(cu(dy), cu(y) if mode == 'saved' else None, (cu(x), cu(gamma), cu(mean), cu(invstd), None, None),
                                      (cu(x2), cu(gamma2), cu(mean2), cu(invstd2), None, None), False,
                                      mask_bits=bits if mode == 'bits' else None)
        for tag, got, w in (('a', pa, want(x, mean, invstd, gamma, mask)), ('b', pb, want(x2, mean2, invstd2, gamma2, mask))):
            for k, a, b in zip(('dx', 'dgamma', 'dbeta'), got, w):
                assert torch.equal(a.double().cpu(), b), ('pair', mode, tag, k, float((a.double().cpu() - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- blocks
def _a1_mask(ops, out):
    saved = out.grad_fn.saved_tensors
    c1, sc1, sh1 = saved[5], saved[12], saved[13]
    return (ops.bn_apply(c1, sc1, sh1, relu=True) > 0).permute(0, 3, 1, 2).cpu()


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).double().cpu()


def _check_masks(name, pre, mask):
    diff = mask != (pre > 0)
    n = int(diff.sum())
    worst = float(pre[diff].abs().max()) if n else 0.0
    assert worst < FLIP_LEVEL, '%s: ReLU decision differs at |v| = %.3g' % (name, worst)
    assert mask.any(), '%s: no activation passes the ReLU' % name
    return n


def _compare(pairs):
    report = {name: _rel(got, want) for name, got, want in pairs}
    worst = max(report.items(), key=lambda kv: kv[1])
    return report, worst


def _ref_copy(ref, module):
    ref.load_state_dict({k: v.double() for k, v in module.state_dict().items()})
    return ref.eval()


BLOCKS = [('layer1', 16, 16, 1, 1025, 130), ('layer2.0', 16, 32, 2, 1025, 130), ('layer6.1', 256, 256, 1, 33, 5)]


@pytest.mark.parametrize('name,cin,cout,stride,H,W', BLOCKS, ids=[b[0] for b in BLOCKS])
def test_basic_block_eval(dam, name, cin, cout, stride, H, W):
    """A residual block in eval() with autograd on (BasicBlockFn, training=False): forward, dx and every parameter gradient
    within 2e-5 of the float64 oracle block in eval mode.  layer2.0: the strided pair and the shortcut in one dgrad launch."""
    layers, ops = dam
    B = 2
    gen = torch.Generator().manual_seed(101 + [b[0] for b in BLOCKS].index(name))
    blk = _randomize(layers.BasicBlock(cin, cout, stride), gen)
    ref = _ref_copy(models_ref.RefBasicBlock(cin, cout, stride).double(), blk)
    blk = blk.cuda().eval()
    x = torch.relu(torch.randn((B, H, W, cin), generator=gen))
    dout = torch.randn((B, (H - 1) // stride + 1, (W - 1) // stride + 1, cout), generator=gen)
    xc = x.cuda().requires_grad_(True)
    out = blk(xc)
    m1, m2 = _a1_mask(ops, out), (out > 0).permute(0, 3, 1, 2).cpu()
    out.backward(dout.cuda())
    ops.wgrad_flush()
    torch.cuda.synchronize()
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    out_r, v1, v2 = models_ref.block_forward_masked(ref, xr, m1, m2)
    flips = _check_masks(name + ' inner', v1, m1) + _check_masks(name + ' outer', v2, m2)
    out_r.backward(dout.permute(0, 3, 1, 2).double())
    pairs = [('out', _nchw(out), out_r), ('dx', _nchw(xc.grad), xr.grad)]
    pairs += [(n, p.grad, q.grad) for (n, p), (_, q) in zip(blk.named_parameters(), ref.named_parameters())]
    report, worst = _compare(pairs)
    print('%s eval B=%d: %d rounding-level ReLU decisions from the device; worst %s %.1e' % (name, B, flips, *worst))
    assert worst[1] <= TOL, report


def test_chain_stem_layer1_eval(dam):
    """stem -> layer1.0 -> layer1.1 in eval mode: the identity blocks' data gradients take the BatchNorm-backward sums of the
    activation in front of them (layers._UpstreamBn) with the running statistics."""
    layers, ops = dam
    B, S, H, W = 2, 8, 1025, 130
    gen = torch.Generator().manual_seed(111)
    stem = _randomize(torch.nn.Sequential(torch.nn.Conv2d(S, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)), gen)
    blks = [_randomize(layers.BasicBlock(16, 16, 1), gen) for _ in range(2)]
    ref_stem = _ref_copy(torch.nn.Sequential(torch.nn.Conv2d(S, 16, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(16)).double(), stem)
    refs = [_ref_copy(models_ref.RefBasicBlock(16, 16, 1).double(), b) for b in blks]
    with torch.no_grad():        # the stem's running mean where its dB-valued input puts the convolution output
        x = torch.from_numpy(model_input(B, S, H, W, seed=5)[0])
        c = torch.nn.functional.conv2d(x, stem[0].weight, padding=1)
        stem[1].running_mean.copy_(c.mean((0, 2, 3)) + 0.3 * torch.randn(16, generator=gen))
        stem[1].running_var.copy_(c.var((0, 2, 3)) * (0.5 + torch.rand(16, generator=gen)))
        ref_stem[1].running_mean.copy_(stem[1].running_mean), ref_stem[1].running_var.copy_(stem[1].running_var)
    stem, blks = stem.cuda().eval(), [b.cuda().eval() for b in blks]
    spec = layers.ConvSpec(S, 16, 3, 1, 1, in_nchw=True)
    dout = torch.randn((B, H, W, 16), generator=gen)
    a0 = layers.ConvBnReluFn.apply(x.cuda(), stem[0].weight, None, stem[1].weight, stem[1].bias, spec, stem[1], False)
    o1 = blks[0](a0)
    o2 = blks[1](o1)
    sign = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()
    masks = [sign(a0), _a1_mask(ops, o1), sign(o1), _a1_mask(ops, o2), sign(o2)]
    hits = layers._UpstreamBn.hits
    o2.backward(dout.cuda())
    ops.wgrad_flush()
    torch.cuda.synchronize()
    assert layers._UpstreamBn.hits == hits + 2 or not ops.DGRAD_BN_SUMS
    a0r, v0 = models_ref.stem_forward_masked(ref_stem[0], ref_stem[1], x.double(), masks[0])
    o1r, v1, v2 = models_ref.block_forward_masked(refs[0], a0r, masks[1], masks[2])
    o2r, v3, v4 = models_ref.block_forward_masked(refs[1], o1r, masks[3], masks[4])
    flips = sum(_check_masks('chain %d' % i, v, m) for i, (v, m) in enumerate(zip((v0, v1, v2, v3, v4), masks)))
    o2r.backward(dout.permute(0, 3, 1, 2).double())
    pairs = [('out', _nchw(o2), o2r)]
    pairs += [('stem.' + n, p.grad, q.grad) for (n, p), (_, q) in zip(stem.named_parameters(), ref_stem.named_parameters())]
    for i in range(2):
        pairs += [('layer1.%d.%s' % (i, n), p.grad, q.grad) for (n, p), (_, q) in zip(blks[i].named_parameters(), refs[i].named_parameters())]
    report, worst = _compare(pairs)
    print('stem -> layer1.0 -> layer1.1 eval: %d device ReLU decisions; worst %s %.1e' % (flips, *worst))
    assert worst[1] <= TOL, report


SCALAR_BLOCKS = [  # name, cin, cout, k, stride, dilation, input H, W, NCHW input   (tests/test_blocks_gpu.py: C2's five blocks)
    ('conv_b1', 4, 16, 3, 2, 2, 1025, 130, True), ('conv_b2', 16, 32, 5, 1, 1, 511, 63, False),
    ('conv_b3', 32, 48, 5, 1, 1, 507, 59, False), ('conv_b4', 48, 64, 7, 1, 1, 503, 55, False),
    ('conv_b5', 64, 128, 9, 1, 1, 497, 49, False)]


@pytest.mark.parametrize('name,cin,cout,k,stride,dil,H,W,nchw', SCALAR_BLOCKS, ids=[b[0] for b in SCALAR_BLOCKS])
def test_conv_block2d_eval(dam, name, cin, cout, k, stride, dil, H, W, nchw):
    """ConvBlock2d in eval() with autograd on: with the running statistics the conv-bias gradient is the channel sum of the
    BatchNorm's input gradient, not zero -- it must match the oracle at 2e-5 of its norm like every other tensor."""
    layers, ops = dam
    B = 2
    gen = torch.Generator().manual_seed(170 + [b[0] for b in SCALAR_BLOCKS].index(name))
    blk = _randomize(layers.ConvBlock2d(cin, cout, k, stride=stride, dilation=dil, dropout_p=-1.0, in_nchw=nchw), gen)
    ref = _ref_copy(models_ref.RefConvBlock2d(cin, cout, k, stride, dil, -1.0).double(), blk)
    Ho, Wo = (H - dil * (k - 1) - 1) // stride + 1, (W - dil * (k - 1) - 1) // stride + 1
    n16 = (cout + 15) // 16 * 16
    if nchw:
        x = -20.0 + 15.0 * torch.randn((B, cin, H, W), generator=gen)
        x_ref = x.double().requires_grad_(True)
        with torch.no_grad():     # running statistics around where the dB-valued input puts the convolution output
            c = ref.conv(x_ref.detach()).float()
            blk.batch_norm.running_mean.copy_(c.mean((0, 2, 3)) + 0.3 * c.std((0, 2, 3)) * torch.randn(cout, generator=gen))
            blk.batch_norm.running_var.copy_(c.var((0, 2, 3)) * (0.5 + torch.rand(cout, generator=gen)))
            ref = _ref_copy(ref, blk)
    else:
        x = torch.relu(torch.randn((B, H, W, cin), generator=gen))
        x_ref = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    blk = blk.cuda().eval()
    dout = torch.randn((B, Ho, Wo, n16), generator=gen)
    dout[..., cout:] = 0
    xc = x.cuda().requires_grad_(not nchw)
    out = blk(xc)
    assert tuple(out.shape) == (B, Ho, Wo, n16)
    mask = (out[..., :cout] > 0).permute(0, 3, 1, 2).cpu()
    out.backward(dout.cuda())
    ops.wgrad_flush()
    torch.cuda.synchronize()
    a_r, v = models_ref.stem_forward_masked(ref.conv, ref.batch_norm, x_ref, mask)
    flips = _check_masks(name, v, mask)
    a_r.backward(dout[..., :cout].permute(0, 3, 1, 2).double())
    pairs = [('out', _nchw(out[..., :cout]), a_r)] + ([] if nchw else [('dx', _nchw(xc.grad), x_ref.grad)])
    pairs += [(n, p.grad, q.grad) for (n, p), (_, q) in zip(blk.named_parameters(), ref.named_parameters())]
    assert float(ref.conv.bias.grad.norm()) > 1e-3 * float(ref.conv.weight.grad.norm())      # (not the training-mode zero)
    report, worst = _compare(pairs)
    print('%s eval B=%d: %d device ReLU decisions; conv.bias %.1e; worst %s %.1e' % (name, B, flips, report['conv.bias'], *worst))
    assert worst[1] <= TOL, report


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.fixture(scope='module')
def models(dam_lib):
    import deep_audio_mixer_amd.models.model_resnet as mr
    import deep_audio_mixer_amd.models.model_scalar_1s as m1
    import deep_audio_mixer_amd.models.model_scalar_2s as m2
    return {'resnet18': (mr.ResNet18, models_ref.RefResNet18),
            'scalar1s': (m1.MixingModelScalar1s, models_ref.RefMixingModelScalar1s),
            'scalar2s': (m2.MixingModelScalar2s, models_ref.RefMixingModelScalar2s)}


MODEL_SHAPES = [('resnet18', (2, 4, 257, 64)), ('scalar1s', (2, 4, 257, 87)), ('scalar2s', (2, 4, 257, 93))]


def _mse_of_forward(m, x, gt):
    masked, gains = m(x)
    return torch.nn.functional.mse_loss(masked, gt), torch.cat(gains, 1)


def _forward_mse(m, x, gt):
    loss, _, gains = m.forward_mse(x, gt)
    return loss, torch.cat(gains, 1)


@pytest.mark.parametrize('name,shape', MODEL_SHAPES, ids=[m[0] for m in MODEL_SHAPES])
@pytest.mark.parametrize('path', ['forward', 'forward_mse'])
def test_model_eval_backward(models, name, shape, path):
    """Each model in eval() (running statistics from three training-mode forwards), loss.backward() through model(x) or
    model.forward_mse, against the float64 oracle in eval mode: best-over-seeds rule (tests/_model_check.py)."""
    ctor, ref_ctor = models[name]
    best_over_seeds(ctor, ref_ctor, shape, _mse_of_forward if path == 'forward' else _forward_mse, _mse_of_forward, eval_mode=True)
