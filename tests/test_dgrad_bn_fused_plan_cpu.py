"""CPU: when does the plan give a stride-1 data gradient the strip instantiation that applies the BatchNorm backward in its row
loaders (ConvLaunch.BNF, ops.conv2d_dgrad_plan(bn_in=)), asked from the plan entry without a GPU.

Eligible is exactly: 16 channels in and out, 3x3 / stride 1 / pad 1, 130-pixel rows, the launch takes sums in its epilogue (EPI 1
-> the mask of the fused BatchNorm as sign bytes, EPI 2 / 3 -> as (scale, shift): the adopted instantiations), and bn_in given.
Every other call plans what it planned without bn_in, with BNF = 0 -- the launching entry refuses bn_in there."""
import pytest

AFF, BITS = (True, True), True
UP_AFF = (True, True, True, True, True)                 # the upstream BatchNorm of the sums epilogue: mask as (scale, shift)
UP_BITS = (True, True, True, None, None, True)          # ... as sign bytes (with the residual only)
RES = dict(res=True, res_mask=True, res_mask_bits=True)


@pytest.fixture(scope='module')
def ops(dam_lib):
    from deep_audio_mixer_amd import ops
    return ops


def _plan(ops, ch=16, H=9, W=130, k=3, pad=1, dil=1, cout=None, bn_in=None, **kw):
    cout = ch if cout is None else cout
    Ho, Wo = H + 2 * pad - dil * (k - 1), W + 2 * pad - dil * (k - 1)
    return ops.conv2d_dgrad_plan((2, Ho, Wo, cout), ch, H, W, k, k, 1, pad, dil, bn_in=bn_in, **kw)


def _bn_in(aff=None, bits=None):
    return (True, True, aff, bits)


ELIGIBLE = [  # id, bn_in mask, data-gradient operands, (EPI, BNF)
    ('bn2_bits_epi1', _bn_in(bits=BITS), dict(bn_bwd=UP_AFF), (1, 3)),
    ('bn1_aff_epi2', _bn_in(aff=AFF), dict(bn_bwd=UP_AFF, **RES), (2, 2)),
    ('bn1_aff_epi3', _bn_in(aff=AFF), dict(bn_bwd=UP_BITS, **RES), (3, 2)),
]


@pytest.mark.parametrize('cid,bn_in,kw,want', ELIGIBLE, ids=[e[0] for e in ELIGIBLE])
@pytest.mark.parametrize('H', [1, 5, 33, 70, 1025])
def test_eligible(ops, cid, bn_in, kw, want, H):
    rec = _plan(ops, H=H, bn_in=bn_in, **kw)
    assert (rec.family, rec.MB, rec.NB, rec.NCH, rec.T33, rec.LW, rec.EPI, rec.SO, rec.BNF) == ('strip', 4, 1, 1, 1, 0, want[0], 1, want[1]), rec
    base = _plan(ops, H=H, **kw)
    assert base.BNF == 0 and rec._replace(BNF=0) == base          # the same launch in everything but the loaders' transform


NOT_ELIGIBLE = [  # id, plan keywords: the mask form not adopted for the epilogue, other channels / widths / taps, no sums
    ('epi1_affine_mask', dict(bn_in=_bn_in(aff=AFF), bn_bwd=UP_AFF)),
    ('epi2_sign_bytes', dict(bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF, **RES)),
    ('epi3_sign_bytes', dict(bn_in=_bn_in(bits=BITS), bn_bwd=UP_BITS, **RES)),
    ('32_channels', dict(ch=32, W=65, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('32_channels_w130', dict(ch=32, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('16_to_32', dict(cout=32, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('32_to_16', dict(ch=32, cout=16, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('w216', dict(W=216, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('w216_residual', dict(W=216, bn_in=_bn_in(aff=AFF), bn_bwd=UP_AFF, **RES)),
    ('w129', dict(W=129, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('w131', dict(W=131, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('w142', dict(W=142, bn_in=_bn_in(aff=AFF), bn_bwd=UP_AFF, **RES)),
    ('dilated', dict(pad=2, dil=2, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('5x5', dict(k=5, pad=2, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('1x1', dict(k=1, pad=0, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('pad0', dict(H=11, pad=0, bn_in=_bn_in(bits=BITS), bn_bwd=UP_AFF)),
    ('no_epilogue', dict(bn_in=_bn_in(bits=BITS))),
    ('no_epilogue_residual', dict(bn_in=_bn_in(aff=AFF), res=True, res_mask=True)),
]


@pytest.mark.parametrize('cid,kw', NOT_ELIGIBLE, ids=[e[0] for e in NOT_ELIGIBLE])
def test_not_eligible(ops, cid, kw):
    rec = _plan(ops, **kw)
    assert rec.BNF == 0, rec
    assert rec == _plan(ops, **dict(kw, bn_in=None)), 'bn_in changed the plan of a launch that does not fuse it'


def test_without_bn_in_nothing_is_fused(ops):
    for _, _, kw, _ in ELIGIBLE:
        assert _plan(ops, **kw).BNF == 0
    assert ops.conv2d_fwd_plan((2, 9, 130, 16), 16, 3, 3, 1, 1, 1, bn_partial=True).BNF == 0
