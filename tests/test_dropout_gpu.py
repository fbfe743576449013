"""GPU: the dropout kernel (csrc/dam_dropout.hip through ops.dropout_tick / ops.dropout_apply and layers.DropoutFn) against
the host restatement of its generator (oracle/dropout_ref.py), BIT FOR BIT: the mask is a pure function of (seed, call
offset, element index) and the kept values are one float32 multiply by one float32 constant, so there is nothing to round
differently and every comparison here is exact equality on signed random inputs.

Sizes: the float4 minimum, around one block, the grid-stride boundary (the launch is capped at 4096 x 256 float4, larger
tensors take further passes), several passes, and the five ConvBlock2d activation sizes of bench configs C2 (batch 4) and
C1 (batch 8); every p of {0, 0.2, 0.3, 0.5, 0.999} at every size and seed (0, 1234, above 2**32, above 2**63 --
torch.initial_seed() of an unseeded process can be that large)."""
import numpy as np
import pytest
import torch

from oracle import dropout_ref, models_ref

pytestmark = pytest.mark.gpu

GRID = 4096 * 256 * 4                      # elements of one grid pass
PS = (0.0, 0.2, 0.3, 0.5, 0.999)
SEEDS = (0, 1234, 2 ** 32 + 5, 2 ** 63 + 12345)


def _activation_sizes(batch, f, t, first_dilation):
    """Element counts of the five block outputs, computed as the product model computes its shapes."""
    from deep_audio_mixer_amd.models._scalar import BLOCKS
    from deep_audio_mixer_amd.ops import conv_out_size
    out = []
    for i, (w, k, _) in enumerate(BLOCKS):
        s, d = (2, first_dilation) if i == 0 else (1, 1)
        f, t = conv_out_size(f, k, s, 0, d), conv_out_size(t, k, s, 0, d)
        out.append(batch * f * t * w)
    return out


def _sizes():
    sizes = [4, 1020, 1024, 256 * 4, GRID - 4, GRID, GRID + 4, 3 * GRID + 1028]
    sizes += _activation_sizes(4, 1025, 130, 2)       # C2: model_scalar_2s, 3 s @ 44.1 kHz hop 1024, batch 4
    sizes += _activation_sizes(8, 1025, 63, 1)        # C1: model_scalar_1s, 1 s @ 16 kHz hop 256, batch 8
    return sorted(set(sizes))


@pytest.fixture(scope='module')
def dam(dam_lib):
    import deep_audio_mixer_amd  # noqa: F401
    from deep_audio_mixer_amd import layers, ops
    return layers, ops


DEV = torch.device('cuda', 0)


def _randn(n, seed):
    return torch.randn(n, generator=torch.Generator(device='cuda').manual_seed(seed), device=DEV)


def test_sizes_cover_the_bench_activations(dam):
    """The size list holds what it says: C2's and C1's block outputs and the oracle's own shapes."""
    c2, c1 = _activation_sizes(4, 1025, 130, 2), _activation_sizes(8, 1025, 63, 1)
    assert c2 == [4 * 511 * 63 * 16, 4 * 507 * 59 * 32, 4 * 503 * 55 * 48, 4 * 497 * 49 * 64, 4 * 489 * 41 * 128]
    assert c1[-1] == 8 * 490 * 9 * 128
    assert c2 == [int(np.prod(s)) for s in models_ref.scalar_block_shapes(4, 1025, 130, 2)]
    assert c1 == [int(np.prod(s)) for s in models_ref.scalar_block_shapes(8, 1025, 63, 1)]
    assert all(n % 4 == 0 for n in _sizes()) and max(_sizes()) > 3 * GRID


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n', _sizes())
def test_apply_equals_host_mask(dam, n, seed):
    """ops.dropout_tick + ops.dropout_apply on signed random float32: y == where(keep, x * scale, 0) exactly, for every p;
    the tick returns the counter it found and advances it by n."""
    layers, ops = dam
    x = _randn(n, n % 1000 + 1)
    xh = x.cpu().numpy()
    c0 = ops.dropout_counter(DEV)
    r = dropout_ref.draws(seed, c0, n)      # one set of draws serves every p: the counter is put back to c0 before each call
    for p in PS:
        ops.set_dropout_counter(DEV, c0)
        snap = ops.dropout_tick(DEV, n)
        y = ops.dropout_apply(x, p, seed, snap)
        assert int(snap.item()) == c0
        want = dropout_ref.apply_ref(xh, seed, c0, p, r)
        got = y.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            pytest.fail('n %d seed %d p %g offset %d: %d elements differ, first at %d (got %r, want %r, x %r)'
                        % (n, seed, p, c0, bad.size, bad[0], got[bad[0]], want[bad[0]], xh[bad[0]]))
    assert ops.dropout_counter(DEV) == c0 + n
    assert torch.equal(x.cpu(), torch.from_numpy(xh))                  # the input is not written


def test_consecutive_calls_draw_adjacent_disjoint_ranges(dam):
    """The k-th tick returns the sum of the earlier n (from the counter's starting value); the k-th mask is the host mask at
    that sum, so the calls of one step use adjacent, disjoint counter ranges: concatenated, they are one stream."""
    layers, ops = dam
    seed, p = 1234, 0.3
    for start in (0, 977, 2 ** 32 + 4096, 2 ** 40 + 1):           # also from counters above 2**32, and an odd one
        ops.set_dropout_counter(DEV, start)
        assert ops.dropout_counter(DEV) == start
        ns = (1024, 4, 5 * 4096, 1020, GRID + 4)
        got, nonzero, total = [], [], 0
        for k, n in enumerate(ns):
            x = _randn(n, 10 + k)
            snap = ops.dropout_tick(DEV, n)
            y = ops.dropout_apply(x, p, seed, snap)
            assert int(snap.item()) == start + total
            assert np.array_equal(y.cpu().numpy(), dropout_ref.apply_ref(x.cpu().numpy(), seed, start + total, p))
            got.append((y != 0).cpu().numpy())
            nonzero.append((x != 0).cpu().numpy())
            total += n
        assert ops.dropout_counter(DEV) == start + total
        assert np.array_equal(np.concatenate(got), dropout_ref.keep_mask(seed, start, total, p) & np.concatenate(nonzero))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('shape,p', [((8, 1024), 0.3), ((4, 31, 9, 16), 0.2), ((2, 511, 63, 16), 0.2), ((GRID + 1028,), 0.5)])
def test_dropout_fn_forward_backward(dam, shape, p, seed):
    """layers.DropoutFn with torch's seed: forward and x.grad equal the host mask applied to x and to a random dy."""
    layers, ops = dam
    torch.manual_seed(seed)
    assert torch.initial_seed() == seed
    n = int(np.prod(shape))
    x = _randn(n, 3).view(shape).requires_grad_(True)
    dy = _randn(n, 4).view(shape)
    c0 = ops.dropout_counter(DEV)
    y = layers.DropoutFn.apply(x, p)
    assert ops.dropout_counter(DEV) == c0 + n
    y.backward(dy)
    assert ops.dropout_counter(DEV) == c0 + n                            # backward draws nothing
    assert np.array_equal(y.detach().cpu().numpy(), dropout_ref.apply_ref(x.detach().cpu().numpy(), seed, c0, p))
    assert np.array_equal(x.grad.cpu().numpy(), dropout_ref.apply_ref(dy.cpu().numpy(), seed, c0, p))
    torch.manual_seed(0)


def test_backward_uses_its_own_forwards_snapshot(dam):
    """Two other dropout calls (and a re-seeding of torch) happen between a forward and its backward, and dy arrives
    non-contiguous: the gradient mask is the forward's -- the saved snapshot and seed, not the live counter."""
    layers, ops = dam
    seed, p = 2 ** 63 + 12345, 0.2
    torch.manual_seed(seed)
    shape = (4, 24, 10, 32)
    n = int(np.prod(shape))
    x = _randn(n, 5).view(shape).requires_grad_(True)
    c0 = ops.dropout_counter(DEV)
    y = layers.DropoutFn.apply(x, p)
    other = _randn(4096, 6).requires_grad_(True)
    o1 = layers.DropoutFn.apply(other, 0.3)
    o2 = layers.DropoutFn.apply(other, 0.5)
    assert ops.dropout_counter(DEV) == c0 + n + 2 * 4096
    torch.manual_seed(99)
    dy = _randn(n, 7).view(shape[0], shape[3], shape[1], shape[2]).permute(0, 2, 3, 1)       # NCHW storage seen as NHWC
    assert not dy.is_contiguous() and tuple(dy.shape) == shape
    y.backward(dy)
    want = dropout_ref.apply_ref(dy.contiguous().cpu().numpy(), seed, c0, p)
    assert np.array_equal(x.grad.cpu().numpy(), want)
    assert tuple(x.grad.shape) == shape
    # and the two calls in between have their own ranges, in call order
    d1, d2 = _randn(4096, 8), _randn(4096, 9)
    (o1 * d1 + o2 * d2).sum().backward()
    want_o = dropout_ref.apply_ref(d1.cpu().numpy(), seed, c0 + n, 0.3) + dropout_ref.apply_ref(d2.cpu().numpy(), seed, c0 + n + 4096, 0.5)
    assert np.array_equal(other.grad.cpu().numpy(), want_o)
    torch.manual_seed(0)


def test_bad_arguments_raise_and_write_nothing(dam):
    """n % 4 != 0 and p outside [0, 1) are refused -- by the kernel's entry point and, before the counter is touched, by
    DropoutFn: a refused call draws nothing."""
    layers, ops = dam
    c0 = ops.dropout_counter(DEV)
    snap = torch.full((1,), c0, dtype=torch.int64, device=DEV)
    for n in (1, 2, 3, 6, 1022):
        with pytest.raises(RuntimeError, match='dam_dropout_apply_f32 failed'):
            ops.dropout_apply(torch.ones(n, device=DEV), 0.2, 0, snap)
        with pytest.raises(ValueError, match='multiple of 4'):
            layers.DropoutFn.apply(torch.ones(n, device=DEV, requires_grad=True), 0.2)
    for p in (1.0, 1.5, -0.1, float('nan')):
        with pytest.raises(RuntimeError, match='dam_dropout_apply_f32 failed'):
            ops.dropout_apply(torch.ones(8, device=DEV), p, 0, snap)
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            layers.DropoutFn.apply(torch.ones(8, device=DEV, requires_grad=True), p)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.dropout_apply(torch.ones(8), 0.2, 0, snap)
    torch.cuda.synchronize()
    assert ops.dropout_counter(DEV) == c0 and int(snap.item()) == c0


def test_captured_forward_backward_draws_fresh_masks_on_replay(dam):
    """DropoutFn forward + backward captured in one graph and replayed three times: the counter lives on the device, so
    every replay's mask is the host mask at the offset the counter had before THAT replay (not the capture's), the three
    differ, and every replay's gradient mask is its own forward's."""
    layers, ops = dam
    seed, p = 2 ** 32 + 5, 0.3
    torch.manual_seed(seed)
    shape = (4, 63, 31, 16)
    n = int(np.prod(shape))
    x = _randn(n, 11).view(shape).requires_grad_(True)
    dy = _randn(n, 12).view(shape)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            torch.autograd.grad(layers.DropoutFn.apply(x, p), x, dy)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    c_cap = ops.dropout_counter(DEV)
    with torch.cuda.graph(g):
        y = layers.DropoutFn.apply(x, p)
        (gx,) = torch.autograd.grad(y, x, dy)
    torch.cuda.synchronize()
    assert ops.dropout_counter(DEV) == c_cap                  # capturing launches nothing
    xh, dyh = x.detach().cpu().numpy(), dy.cpu().numpy()
    masks = []
    for k in range(3):
        if k == 2:
            # another call between two replays moves the counter; the next replay starts from where that left it
            layers.DropoutFn.apply(_randn(1024, 13), 0.5)
        c0 = ops.dropout_counter(DEV)
        assert c0 == c_cap + k * n + (1024 if k == 2 else 0)
        g.replay()
        torch.cuda.synchronize()
        assert ops.dropout_counter(DEV) == c0 + n
        assert np.array_equal(y.detach().cpu().numpy(), dropout_ref.apply_ref(xh, seed, c0, p)), 'replay %d forward' % k
        assert np.array_equal(gx.cpu().numpy(), dropout_ref.apply_ref(dyh, seed, c0, p)), 'replay %d backward' % k
        masks.append(dropout_ref.keep_mask(seed, c0, n, p))
        assert np.array_equal((gx != 0).cpu().numpy(), masks[-1].reshape(shape) & (dyh != 0))
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2]) and not np.array_equal(masks[0], masks[2])
    torch.manual_seed(0)
