"""GPU: the PCM encoder (ops.pcm_encode -> dam_pcm_encode) against tests/_pcm_ref.py.  Every comparison is exact equality
of the bytes and of clip_count: the arithmetic is fixed (one float64 product, an exact power-of-two scale, one float64
add for the dither, rint), so there is nothing to tolerate."""
import numpy as np
import pytest
import torch

import _pcm_ref

pytestmark = pytest.mark.gpu

SUBTYPES = ('PCM_16', 'PCM_24', 'PCM_32', 'FLOAT')
INT_SUBTYPES = SUBTYPES[:3]


def run(x, subtype, scale=None, dither_seed=None):
    """x: numpy planar [channels, n] -> (bytes ndarray, clip_count ndarray) from the device."""
    from deep_audio_mixer_amd import ops
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sd = None if scale is None else torch.tensor(np.atleast_1d(scale), dtype=torch.float64, device='cuda')
    clip = torch.full((xd.shape[0] if xd.dim() == 2 else 1,), -7, dtype=torch.int64, device='cuda')     # must be overwritten
    out = ops.pcm_encode(xd, subtype, scale=sd, dither_seed=dither_seed, clip_count=clip)
    assert out.dtype == torch.uint8 and out.is_cuda
    return out.cpu().numpy(), clip.cpu().numpy()


def check(x, subtype, scale=None, dither_seed=None):
    got, clip = run(x, subtype, scale, dither_seed)
    want, want_clip = _pcm_ref.encode(x, subtype, scale, dither_seed)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, 'first differing byte %d of %d (%s, shape %s)' % (bad[0], got.size, subtype, np.shape(x))
    assert clip.tolist() == want_clip.tolist()
    return got, clip


def test_every_int16_code(dam_lib):
    codes = np.arange(-32768, 32768, dtype=np.int64)
    mono = (codes / 32768.0).astype(np.float32)[None]
    got, clip = check(mono, 'PCM_16')
    assert np.array_equal(_pcm_ref.from_bytes(got, 'PCM_16', 1)[:, 0], codes) and clip.tolist() == [0]
    stereo = np.stack([mono[0], mono[0, ::-1]])
    got, clip = check(stereo, 'PCM_16')
    back = _pcm_ref.from_bytes(got, 'PCM_16', 2)
    assert np.array_equal(back[:, 0], codes) and np.array_equal(back[:, 1], codes[::-1]) and clip.tolist() == [0, 0]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('subtype', INT_SUBTYPES)
def test_edge_values(dam_lib, subtype, dtype):
    b = _pcm_ref.BITS[subtype]
    full = 2.0 ** (b - 1)
    v = [1.0, -1.0, 1.0 - 2.0 ** -(b - 1), 1.5, -1.5, np.inf, -np.inf, np.nan, 0.0, -0.0]
    v += [(k + 0.5) / full for k in (-2, -1, 0, 1, 2)]                                    # ties: round half to even
    # around the clamp: the last values that stay, the first that go (representable or not in `dtype`: the input is
    # whatever the cast makes of them, and the restatement sees the same array)
    v += [(full - 1.0) / full, (full - 0.5) / full, (full - 0.5) / full - 2.0 ** -40, (full - 0.49) / full,
          -(full + 0.5) / full, -(full + 0.5) / full - 2.0 ** -40, -(full + 0.51) / full, np.nextafter(1.0, 0.0),
          np.nextafter(-1.0, -2.0), float(np.nextafter(dtype(1.0), dtype(0.0))), float(np.nextafter(dtype(-1.0), dtype(-2.0)))]
    x = np.array(v, dtype=dtype)
    for row in (x[None], np.stack([x, x[::-1]]), np.stack([x, -x, x[::-1]])):
        _, clip = check(row, subtype)
        assert clip.min() >= 6                          # 1.0, +-1.5, +-inf and NaN at the least
    if dtype == np.float64 or b == 16:                  # the ties are exact in this dtype: show half-to-even itself
        ties = np.array([(k + 0.5) / full for k in (-2, -1, 0, 1, 2)], dtype=dtype)[None]
        got, _ = run(ties, subtype)
        assert _pcm_ref.from_bytes(got, subtype, 1)[:, 0].tolist() == [-2, 0, 0, 2, 2]


def _grid_frames(dtype):
    from deep_audio_mixer_amd import ops
    frames = ops.pcm_grid_frames(np.dtype(dtype).name)                  # one pass of the full grid, as the library states it
    assert frames >= 256 and frames % 256 == 0
    return frames


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('channels', [1, 2, 3, 6, 8])
def test_sizes_and_shapes(dam_lib, channels, dtype):
    rng = np.random.default_rng(channels)
    big = (0.5 * rng.standard_normal((channels, 4099))).astype(dtype)
    for subtype in SUBTYPES:
        for n in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099):
            check(np.ascontiguousarray(big[:, :n]), subtype)


@pytest.mark.parametrize('dtype,channels,subtype', [(np.float32, 2, 'PCM_16'), (np.float32, 1, 'PCM_24'),
                                                    (np.float64, 2, 'PCM_16'), (np.float32, 3, 'PCM_24'),
                                                    (np.float64, 1, 'PCM_24')])
def test_grid_stride_boundary(dam_lib, dtype, channels, subtype):
    """One full pass of the capped grid, one frame less, one more (the second pass starts with one frame)."""
    g = _grid_frames(dtype)
    rng = np.random.default_rng(11)
    big = (0.5 * rng.standard_normal((channels, g + 1))).astype(dtype)
    for n in (g - 1, g, g + 1):
        check(np.ascontiguousarray(big[:, :n]), subtype, dither_seed=3)


@pytest.mark.parametrize('channels', [1, 2, 3])
def test_scale(dam_lib, channels):
    rng = np.random.default_rng(2)
    x32 = (0.5 * rng.standard_normal((channels, 1031))).astype(np.float32)
    per_channel = np.array([0.37, 1.9, 3.3][:channels])
    for subtype in SUBTYPES:
        for x in (x32, x32.astype(np.float64)):
            check(x, subtype)
            check(x, subtype, scale=[0.37])
            check(x, subtype, scale=per_channel)
    # float32 input, float64 scale: the product is the float64 one, not a float32 product widened
    s = np.array([1.0 / 3.0])
    got, _ = check(x32, 'PCM_32', scale=s)
    narrow, _ = _pcm_ref.encode((x32 * np.float32(s[0])), 'PCM_32')
    assert not np.array_equal(got, narrow)
    # 0 * inf = NaN: zeros, every element counted
    zero = np.zeros((channels, 77), dtype=np.float32)
    for subtype in INT_SUBTYPES:
        got, clip = check(zero, subtype, scale=[np.inf])
        assert not got.any() and clip.tolist() == [77] * channels


@pytest.mark.parametrize('seed', [0, 1234, 2 ** 63 + 12345])
def test_dither(dam_lib, seed):
    rng = np.random.default_rng(4)
    for channels, dtype in ((1, np.float32), (2, np.float32), (3, np.float64), (2, np.float64)):
        x = (0.5 * rng.standard_normal((channels, 2051))).astype(dtype)
        for subtype in INT_SUBTYPES:
            long_bytes, _ = check(x, subtype, dither_seed=seed)
            n = 700
            short_bytes, _ = check(np.ascontiguousarray(x[:, :n]), subtype, dither_seed=seed)
            assert np.array_equal(short_bytes, long_bytes[:short_bytes.size])              # the value at an element, whatever n
        plain, _ = run(x, 'PCM_16')
        dithered, _ = run(x, 'PCM_16', dither_seed=seed)
        assert not np.array_equal(plain, dithered)
        flt, _ = run(x, 'FLOAT')
        flt_d, clip = run(x, 'FLOAT', dither_seed=seed)                                    # FLOAT: no dither, nothing counted
        assert np.array_equal(flt, flt_d) and not clip.any()


def test_graph_capture_and_replay(dam_lib):
    from deep_audio_mixer_amd import ops
    rng = np.random.default_rng(6)
    x = (0.5 * rng.standard_normal((2, 5003))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    scale = torch.tensor([0.8], dtype=torch.float64, device='cuda')
    out = torch.zeros(5003 * 2 * 3, dtype=torch.uint8, device='cuda')
    clip = torch.zeros(2, dtype=torch.int64, device='cuda')
    eager = ops.pcm_encode(xd, 'PCM_24', scale=scale, dither_seed=5).cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pcm_encode(xd, 'PCM_24', scale=scale, dither_seed=5, out=out, clip_count=clip)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.pcm_encode(xd, 'PCM_24', scale=scale, dither_seed=5, out=out, clip_count=clip)
    graph.replay()
    torch.cuda.synchronize()
    first, first_clip = _pcm_ref.encode(x, 'PCM_24', [0.8], 5)
    assert np.array_equal(eager, first) and np.array_equal(out.cpu().numpy(), eager) and clip.tolist() == first_clip.tolist()
    scale.fill_(40.0)                                                   # a device-side change: the replay reads it
    graph.replay()
    graph.replay()                                                      # (clip_count is overwritten, not accumulated)
    torch.cuda.synchronize()
    want, want_clip = _pcm_ref.encode(x, 'PCM_24', [40.0], 5)
    assert np.array_equal(out.cpu().numpy(), want) and clip.tolist() == want_clip.tolist() and want_clip.min() > 0


def test_argument_checks(dam_lib):
    from deep_audio_mixer_amd import _lib, ops
    L = dam_lib
    x = torch.zeros((3, 64), dtype=torch.float32, device='cuda')
    out = torch.full((3 * 64 * 2,), 0xAB, dtype=torch.uint8, device='cuda')
    scale = torch.ones(2, dtype=torch.float64, device='cuda')

    def call(channels, n_scale, fmt):
        return L.dam_pcm_encode(x.data_ptr(), 0, channels, 64, scale.data_ptr(), n_scale, fmt, 0, 0, out.data_ptr(), None,
                                _lib.stream())
    assert call(0, 0, 0) == -1 and call(9, 0, 0) == -1                  # DAM_ERR_BAD_ARG
    assert call(3, 2, 0) == -1 and call(3, 0, 4) == -1 and call(3, 0, -1) == -1
    with pytest.raises(ValueError):
        ops.pcm_encode(x, 'PCM_8', out=out)
    with pytest.raises(ValueError):
        ops.pcm_encode(x, 'PCM_16', scale=scale, out=out)
    with pytest.raises(ValueError):
        ops.pcm_encode(torch.zeros((64, 3), dtype=torch.float32, device='cuda').t(), 'PCM_16', out=out)       # non-contiguous
    with pytest.raises(ValueError):
        ops.pcm_encode(torch.zeros((9, 64), dtype=torch.float32, device='cuda'), 'PCM_16')
    with pytest.raises(RuntimeError):
        ops.pcm_encode(x.cpu(), 'PCM_16')
    with pytest.raises(TypeError):
        ops.pcm_encode(x.half(), 'PCM_16', out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())                                    # nothing was launched
    assert call(3, 0, 0) == 0
    torch.cuda.synchronize()
    assert not out.any()
