"""CPU: the host restatement of the product's dropout generator (oracle/dropout_ref.py) against a scalar Python-int
splitmix64, its keep-rate, and the oracle block's hook that applies a mask given from outside."""
import numpy as np
import pytest
import torch

from oracle import dropout_ref, models_ref

M64 = (1 << 64) - 1


def _draw_scalar(seed, offset, i):
    """One draw in unbounded Python integers (the form oracle/features_ref.augment_gain_ref uses)."""
    z = (seed * 0xD1342543DE82EF95 + offset + i) & M64
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def _wrapping_offset(seed, n):
    """An offset for which base + i passes 2**64 in the middle of [0, n)."""
    return (-(seed * 0xD1342543DE82EF95) - n // 2) & M64


@pytest.mark.parametrize('seed,offset', [(0, 0), (1234, 7), (2 ** 32 + 5, 2 ** 32 + 12345), (2 ** 63 + 12345, 2 ** 40 + 3),
                                         (2 ** 64 - 1, 2 ** 62), (1234, _wrapping_offset(1234, 64)),
                                         (2 ** 63 + 12345, _wrapping_offset(2 ** 63 + 12345, 64))])
def test_keep_mask_equals_scalar_splitmix64(seed, offset):
    n = 64
    r = dropout_ref.draws(seed, offset, n)
    assert r.dtype == np.uint32 and r.shape == (n,)
    want = [_draw_scalar(seed, offset, i) for i in range(n)]
    assert r.tolist() == want
    base = (seed * 0xD1342543DE82EF95 + offset) & M64
    if offset == _wrapping_offset(seed, n):
        assert base + n - 1 > M64 >= base                      # the case really wraps
    for p in (0.0, 0.2, 0.3, 0.5, 0.999):
        thr = int(float(np.float32(p)) * 2 ** 32)
        assert int(dropout_ref.threshold(p)) == thr
        assert dropout_ref.keep_mask(seed, offset, n, p).tolist() == [w >= thr for w in want]
        assert dropout_ref.keep_mask(seed, offset, n, p, r).tolist() == [w >= thr for w in want]


def test_consecutive_ranges_are_one_stream():
    """A call at offset o with n elements followed by one at o + n draws what one call of both sizes draws."""
    a, b = dropout_ref.draws(99, 1000, 300), dropout_ref.draws(99, 1300, 212)
    assert np.array_equal(np.concatenate([a, b]), dropout_ref.draws(99, 1000, 512))


def test_scale_and_threshold():
    for p in (0.0, 0.2, 0.3, 0.5, 0.999):
        s = dropout_ref.scale(p)
        assert s.dtype == np.float32 and s == np.float32(1) / (np.float32(1) - np.float32(p))
    assert dropout_ref.scale(0.0) == 1 and dropout_ref.threshold(0.0) == 0 and dropout_ref.threshold(0.5) == 2 ** 31
    assert dropout_ref.keep_mask(5, 0, 4096, 0.0).all()
    for p in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            dropout_ref.threshold(p)


@pytest.mark.parametrize('p', [0.2, 0.3])
@pytest.mark.parametrize('seed,offset', [(0, 0), (2 ** 63 + 12345, 2 ** 33)])
def test_keep_rate(p, seed, offset):
    """2**22 draws: the keep-rate lies within 5 binomial standard deviations of 1 - p (9.8e-4 at 0.2, 1.1e-3 at 0.3)."""
    n = 1 << 22
    rate = float(dropout_ref.keep_mask(seed, offset, n, p).mean())
    bound = 5 * (p * (1 - p) / n) ** 0.5
    print('p %.1f seed %d: keep-rate %.5f (bound %.2e)' % (p, seed, rate, bound))
    assert abs(rate - (1 - p)) <= bound


def test_apply_ref():
    x = np.random.default_rng(0).standard_normal((3, 8)).astype(np.float32)
    keep = dropout_ref.keep_mask(7, 11, 24, 0.3).reshape(3, 8)
    y = dropout_ref.apply_ref(x, 7, 11, 0.3)
    assert y.dtype == np.float32 and np.array_equal(y != 0, keep)
    assert np.array_equal(y[keep], x[keep] * dropout_ref.scale(0.3))


def test_block_keep_masks_layout():
    """Masks are drawn over the NHWC tensor the device sees and handed to the oracle as NCHW; offsets run on."""
    shapes = [(2, 3, 5, 16), (2, 2, 4, 32)]
    masks, end = dropout_ref.block_keep_masks(42, 100, shapes, (0.2, 0.3))
    assert end == 100 + 2 * 3 * 5 * 16 + 2 * 2 * 4 * 32
    assert masks[0].shape == (2, 16, 3, 5) and masks[1].shape == (2, 32, 2, 4)
    flat0 = dropout_ref.keep_mask(42, 100, 480, 0.2)
    assert masks[0][1, 7, 2, 3] == flat0[((1 * 3 + 2) * 5 + 3) * 16 + 7]
    flat1 = dropout_ref.keep_mask(42, 580, 512, 0.3)
    assert masks[1][1, 31, 1, 2] == flat1[((1 * 2 + 1) * 4 + 2) * 32 + 31]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_oracle_block_hook(dtype):
    torch.manual_seed(0)
    p = 0.3
    blk = models_ref.RefConvBlock2d(3, 16, 3, 1, 1, p).to(dtype).train()
    plain = models_ref.RefConvBlock2d(3, 16, 3, 1, 1, -1.0).to(dtype).train()
    plain.load_state_dict(blk.state_dict())
    x = torch.randn(2, 3, 9, 8, dtype=dtype)
    y0 = plain(x)
    # all-true mask and p = 0 (scale 1): the identity
    blk.dropout_p, blk.keep_mask = 0.0, torch.ones(y0.shape, dtype=torch.bool)
    assert torch.equal(blk(x), y0)
    # a given mask: forward and autograd gradient are y * m / (1 - p)
    blk.dropout_p = p
    keep = torch.from_numpy(dropout_ref.keep_mask(3, 0, y0.numel(), p).reshape(2, 7, 6, 16).transpose(0, 3, 1, 2).copy())
    blk.keep_mask = keep
    xg = x.clone().requires_grad_(True)
    y = blk(xg)
    s = torch.ones((), dtype=dtype) / (1 - torch.tensor(p, dtype=dtype))
    if dtype == torch.float32:
        assert float(s) == float(dropout_ref.scale(p))
    assert torch.equal(y, y0 * keep.to(dtype) * s)
    dy = torch.randn(y.shape, dtype=dtype)
    y.backward(dy)
    x0 = x.clone().requires_grad_(True)
    plain.zero_grad()
    plain(x0).backward(dy * keep.to(dtype) * s)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert float((xg.grad - x0.grad).norm()) <= tol * float(x0.grad.norm())
    for a, b in zip(blk.parameters(), plain.parameters()):
        assert float((a.grad - b.grad).norm()) <= tol * float(b.grad.norm()) + 1e-12
    # a wrong shape or dtype is refused; eval mode ignores the mask; None is torch's own draw again
    blk.keep_mask = keep[:, :8]
    with pytest.raises(ValueError, match='keep_mask'):
        blk(x)
    blk.keep_mask = keep.float()
    with pytest.raises(ValueError, match='keep_mask'):
        blk(x)
    blk.keep_mask = keep
    plain.load_state_dict(blk.state_dict())                    # (the running statistics saw different numbers of forwards)
    plain.eval(), blk.eval()
    assert torch.equal(blk(x), plain(x))
    blk.train()
    blk.keep_mask = None
    torch.manual_seed(1)
    a = blk(x)
    torch.manual_seed(1)
    plain.train()
    assert torch.equal(a, torch.nn.functional.dropout(plain(x), p, True))


def test_set_keep_masks_and_block_shapes():
    ref = models_ref.RefMixingModelScalar2s(n_stems=4, input_shape=(257, 93)).train()
    shapes = models_ref.scalar_block_shapes(2, 257, 93, 2)
    assert shapes[0] == (2, 127, 45, 16) and [s[3] for s in shapes] == [16, 32, 48, 64, 128]
    assert shapes[-1][1:3] == models_ref.scalar_trunk_hw(257, 93, 2)
    ps = [b[2] for b in models_ref.SCALAR_BLOCKS]
    masks, _ = dropout_ref.block_keep_masks(5, 0, shapes, ps)
    models_ref.set_keep_masks(ref, [torch.from_numpy(m) for m in masks])
    x = torch.randn(2, 4, 257, 93)
    a, b = ref(x)[0], ref(x)[0]
    assert torch.equal(a, b)                                   # the given masks, not a fresh draw
    models_ref.set_keep_masks(ref, None)
    assert all(getattr(ref, 'conv_b%d' % i).keep_mask is None for i in range(1, 6))
    assert not torch.equal(ref(x)[0], ref(x)[0])
