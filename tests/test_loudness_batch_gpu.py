"""GPU: the batched BS.1770 meter (dam_loudness_block_energy_batch: all rows in one set of launches, LDS-staged loads,
optional gain ramp at load, block energies from per-segment sums), the device gating (dam_loudness_gate) and the
normalisation gain (dam_loudness_target_gains) against the CPU oracle (oracle/loudness_ref.py) and the host gating.
Tolerances are those of tests/test_loudness_gpu.py: float64 recurrences and sums in another association order than one
sequential lfilter / np.sum -- 1e-9 relative on block energies, 1e-8 LU on the loudness, 1e-6 LU "at target".
Every test prints its largest observed error before asserting."""
import numpy as np
import pytest
import torch

from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

RATE = 44100
Z_RTOL, Z_ATOL, LU_TOL, TARGET_TOL = 1e-9, 1e-18, 1e-8, 1e-6


@pytest.fixture(scope='module')
def loud(dam_lib):
    from deep_audio_mixer_amd import loudness
    return loudness


def music_like(n, ch, seed, rate=44100):
    r = np.random.RandomState(seed)
    t = np.arange(n) / rate
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 0.3 * t + r.rand())
    x = np.stack([env * (0.2 * np.sin(2 * np.pi * (110 * (i + 1)) * t) + 0.05 * r.randn(n)) for i in range(ch)], axis=1)
    x[n // 3: n // 3 + rate] = 0.0            # a second of digital silence: gated blocks
    return x


def lu_err(got, want):
    """|got - want| with equal infinities counting as 0 (and unequal ones as inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(got == want, 0.0, np.abs(got - want))


def z_err(got, want):
    """Largest |got - want| as a fraction of the allowed Z_ATOL + Z_RTOL * |want| (<= 1 passes)."""
    return float(np.max(np.abs(got - want) / (Z_ATOL + Z_RTOL * np.abs(want))))


def threshold_distance(z):
    """Smallest distance (LU) of any block of z[channel][block] to the absolute or the relative gate; inf if none."""
    G = np.array([1.0, 1.0, 1.0, 1.41, 1.41])[:z.shape[0]]
    with np.errstate(divide='ignore', invalid='ignore'):
        l = -0.691 + 10.0 * np.log10(np.sum(G[:, None] * z, axis=0))
        a = l >= -70.0
        gr = -0.691 + 10.0 * np.log10(np.sum(G * z[:, a].mean(axis=1))) - 10.0 if a.any() else np.nan
    fin = l[np.isfinite(l)]
    d = [np.abs(fin + 70.0).min()] if len(fin) else []
    if len(fin) and np.isfinite(gr):
        d.append(np.abs(fin - gr).min())
    return min(d) if d else np.inf


@pytest.fixture(scope='module')
def five(loud):
    """The five stereo float32 tracks [5, n, 2], their oracle block energies and loudness (computed once, read-only)."""
    n = RATE * 3 + 123
    s = music_like(n, 2, 1, RATE).astype(np.float32)
    third = s.copy()
    third[:n // 3] *= np.float32(0.03)
    tone = np.repeat(np.sin(2 * np.pi * 997 * np.arange(n) / RATE)[:, None], 2, axis=1).astype(np.float32)
    x = np.stack([s, s * np.float32(1e-3), third, np.zeros_like(s), tone])
    z = np.stack([ref.block_energies(t.astype(np.float64), RATE) for t in x])
    lufs = np.array([ref.integrated_loudness(t.astype(np.float64), RATE) for t in x])
    for a in (x, z, lufs):
        a.setflags(write=False)
    return x, z, lufs


def test_batch_matches_oracle(loud, five):
    x, z_want, lufs_want = five
    # a condition on the inputs: no block sits on a gate threshold, so the kept sets cannot differ by rounding
    dist = min(threshold_distance(z) for z in z_want)
    print('smallest block-to-threshold distance %.4f LU' % dist)
    assert dist >= 1e-3
    assert z_want.shape[2] == 27 and lufs_want[1] == -np.inf and lufs_want[3] == -np.inf and np.isfinite(lufs_want[[0, 2, 4]]).all()
    m = loud.Meter(RATE)
    xd = torch.from_numpy(x.copy()).cuda()
    z = m.block_energies_batch(xd)
    lufs = m.integrated_loudness_batch(xd)
    assert z.is_cuda and z.dtype == torch.float64 and tuple(z.shape) == z_want.shape
    assert lufs.is_cuda and lufs.dtype == torch.float64 and tuple(lufs.shape) == (5,)
    z, lufs = z.cpu().numpy(), lufs.cpu().numpy()
    print('block energies: max err %.3g of the bound' % z_err(z, z_want))
    print('loudness: max err %.3g LU (bound %g)' % (lu_err(lufs, lufs_want).max(), LU_TOL))
    np.testing.assert_allclose(z, z_want, rtol=Z_RTOL, atol=Z_ATOL)
    assert np.array_equal(np.isneginf(lufs), np.isneginf(lufs_want))
    assert lu_err(lufs, lufs_want).max() < LU_TOL


@pytest.mark.parametrize('N,n,ch,dtype,rate,planar', [
    (1, 17640, 2, np.float64, 44100, False),                 # one block, 18 chunks
    (3, 2 * 44100 + 1, 5, np.float32, 44100, False),
    (2, 48000 * 3, 1, np.float32, 48000, False),
    (2, 8000 * 6 + 77, 2, np.float64, 8000, False),          # the 800-sample hop is below the 1024-sample chunk
    (3, 44100 + 4321, 2, np.float32, 44100, True),           # [N, channels, n] storage passed as .transpose(1, 2)
])
def test_geometries(loud, N, n, ch, dtype, rate, planar):
    x = np.stack([(0.3 + 0.5 * t) * music_like(n, ch, 7 * t + n % 97, rate) for t in range(N)]).astype(dtype)
    if n > 3 * rate // 2:
        x[-1, n // 3 + rate:] *= 0.05                         # a quiet tail: blocks under the relative gate
    m = loud.Meter(rate)
    if planar:
        xd = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
        assert not xd.is_contiguous()
    else:
        xd = torch.from_numpy(x).cuda()
    z = m.block_energies_batch(xd).cpu().numpy()
    lufs = m.integrated_loudness_batch(xd).cpu().numpy()
    z_want = np.stack([ref.block_energies(t.astype(np.float64), rate) for t in x])
    lufs_want = np.array([ref.integrated_loudness(t.astype(np.float64), rate) for t in x])
    assert min(threshold_distance(zz) for zz in z_want) >= 1e-3
    assert z.shape == z_want.shape
    print('block energies: max err %.3g of the bound; loudness: max err %.3g LU' % (z_err(z, z_want), lu_err(lufs, lufs_want).max()))
    np.testing.assert_allclose(z, z_want, rtol=Z_RTOL, atol=Z_ATOL)
    assert lu_err(lufs, lufs_want).max() < LU_TOL


def test_batch_invariance_is_bitwise(loud, five):
    x = torch.from_numpy(five[0].copy()).cuda()
    m = loud.Meter(RATE)
    z, lufs = m.block_energies_batch(x), m.integrated_loudness_batch(x)
    for t in range(x.shape[0]):
        assert torch.equal(m.block_energies_batch(x[t:t + 1])[0], z[t])
        one = m.integrated_loudness_batch(x[t:t + 1])
        assert one[0].item() == lufs[t].item() or (torch.isnan(one[0]) and torch.isnan(lufs[t]))


@pytest.mark.parametrize('n_gains', [7, 1])
def test_gain_fusion(loud, five, n_gains):
    from deep_audio_mixer_amd import ops
    x = five[0][[0, 2, 4]]
    N, n, ch = x.shape
    assert n_gains == 1 or n % n_gains
    gains = np.random.RandomState(n_gains).uniform(0.3, 1.7, (N, n_gains))
    m = loud.Meter(RATE)
    planar = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()            # [N, ch, n]
    gd = torch.from_numpy(gains).cuda()
    z = m.block_energies_batch(planar.transpose(1, 2), gains=gd)
    lufs = m.integrated_loudness_batch(planar.transpose(1, 2), gains=gd)
    scaled = ops.gain_ramp_apply(planar, gd, out_dtype=torch.float64)
    assert torch.equal(z, m.block_energies_batch(scaled.transpose(1, 2)))
    assert torch.equal(lufs, m.integrated_loudness_batch(scaled.transpose(1, 2)))
    masks = np.stack([inference_ref.interpolate_mask(g, n) if n_gains > 1 else np.full(n, g[0]) for g in gains])
    want_audio = x.astype(np.float64) * masks[:, :, None]
    z_want = np.stack([ref.block_energies(t, RATE) for t in want_audio])
    lufs_want = np.array([ref.integrated_loudness(t, RATE) for t in want_audio])
    assert min(threshold_distance(zz) for zz in z_want) >= 1e-3
    print('block energies: max err %.3g of the bound; loudness: max err %.3g LU' % (
        z_err(z.cpu().numpy(), z_want), lu_err(lufs.cpu().numpy(), lufs_want).max()))
    np.testing.assert_allclose(z.cpu().numpy(), z_want, rtol=Z_RTOL, atol=Z_ATOL)
    assert lu_err(lufs.cpu().numpy(), lufs_want).max() < LU_TOL


@pytest.mark.parametrize('n_blocks', [1, 2, 257, 3000])
@pytest.mark.parametrize('ch', [1, 2, 5])
def test_gate_alone(loud, n_blocks, ch):
    r = np.random.RandomState(n_blocks * 16 + ch)
    # block energies spread over ~40 dB around -30 LUFS, some blocks under the absolute gate, some zero
    level = r.uniform(-50.0, -10.0, n_blocks)
    level[r.rand(n_blocks) < 0.2] = -90.0
    base = 10.0 ** (level / 10.0)
    z = base[None, :] * r.uniform(0.5, 1.5, (ch, n_blocks))
    z[:, r.rand(n_blocks) < 0.1] = 0.0
    quiet = 10.0 ** (r.uniform(-120.0, -80.0, (ch, n_blocks)) / 10.0)              # everything below -70: -inf
    one = np.full((ch, n_blocks), 10.0 ** (-45.0 / 10.0))                           # one block above, the rest 15 LU below
    one[:, n_blocks // 2] = 10.0 ** (-30.0 / 10.0)
    batch = np.stack([z, quiet, one])
    want = np.array([loud.gated_loudness(t) for t in batch])
    assert want[1] == -np.inf
    for t in (0, 2):
        assert threshold_distance(batch[t]) >= 1e-3
    got = loud.gate_loudness_device(torch.from_numpy(batch).cuda()).cpu().numpy()
    print('gate: max err %.3g LU (bound %g)' % (lu_err(got, want).max(), LU_TOL))
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    assert lu_err(got, want).max() < LU_TOL


def test_capture_and_replay(loud, five):
    """Meter + gate with gains inside torch.cuda.graph on a static buffer: capturing proves nothing synchronises; the
    replay on new buffer contents equals the eager result on those contents."""
    x = five[0]
    m = loud.Meter(RATE)
    buf = torch.from_numpy(x[[0, 2]]).cuda()
    gains = torch.from_numpy(np.random.RandomState(3).uniform(0.3, 1.7, (2, 5))).cuda()
    out = torch.empty(2, dtype=torch.float64, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.integrated_loudness_batch(buf, gains=gains, out=out)           # warm-up: uploads the block bounds
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.integrated_loudness_batch(buf, gains=gains, out=out)
    first = out.clone()
    buf.copy_(torch.from_numpy(x[[4, 0]]).cuda())
    gains.copy_(torch.from_numpy(np.random.RandomState(4).uniform(0.3, 1.7, (2, 5))).cuda())
    graph.replay()
    torch.cuda.synchronize()
    eager = m.integrated_loudness_batch(buf.clone(), gains=gains.clone())
    assert torch.equal(out, eager) and not torch.equal(out, first)
    assert torch.isfinite(out).all()


def test_target_gains_and_normalise(loud, five):
    from deep_audio_mixer_amd import ops
    x, _, lufs_want = five
    m = loud.Meter(RATE)
    planar = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda()
    lufs = m.integrated_loudness_batch(planar.transpose(1, 2))
    target = np.array([-23.0, -20.0, -16.0, -20.0, -30.0])
    g = loud.target_gains_device(lufs, target)
    gh = g.cpu().numpy()
    assert gh[1] == np.inf and gh[3] == np.inf                              # silent tracks: 10 ** (+inf), not special-cased
    keep = [0, 2, 4]
    with np.errstate(over='ignore'):
        np.testing.assert_allclose(gh[keep], np.power(10.0, (target[keep] - lufs_want[keep]) / 20.0), rtol=1e-9)
    out = ops.gain_ramp_apply(planar[keep], g[keep].view(-1, 1), out_dtype=torch.float64)
    again = m.integrated_loudness_batch(out.transpose(1, 2)).cpu().numpy()
    print('at target: max err %.3g LU (bound %g)' % (np.abs(again - target[keep]).max(), TARGET_TOL))
    assert np.abs(again - target[keep]).max() < TARGET_TOL
    # normalize_loudness_device: the same through the public helper, a float target, on the [N, n, ch] view
    norm = loud.normalize_loudness_device(planar[keep].transpose(1, 2), lufs[keep], -20.0)
    assert tuple(norm.shape) == (3, x.shape[1], 2) and norm.dtype == torch.float64
    for i, t in enumerate(keep):
        assert abs(ref.integrated_loudness(norm[i].cpu().numpy(), RATE) - (-20.0)) < TARGET_TOL


def test_mean_loudness_model_forward_device(loud):
    from deep_audio_mixer_amd.models.baselines.mean_loudness_model import MeanLoudnessModel
    names = ('bass', 'drums', 'vocals', 'other')
    tracks = {k: torch.from_numpy(music_like(RATE * 2 + 11, 2, 40 + i, RATE).T.copy()).cuda() for i, k in enumerate(names)}
    target = {'bass': -25.0, 'drums': -20.0, 'vocals': -18.0, 'other': -22.0}
    model = MeanLoudnessModel(target, RATE)
    dev, host = model.forward_device(tracks), model.forward(tracks)
    m = loud.Meter(RATE)
    for k in names:
        assert dev[k].shape == tracks[k].shape and dev[k].is_cuda
        a, b = m.integrated_loudness(dev[k].T), m.integrated_loudness(host[k].T)
        print('%s: device %.9f host %.9f target %g' % (k, a, b, target[k]))
        assert abs(a - target[k]) < TARGET_TOL and abs(b - target[k]) < TARGET_TOL


def test_errors(loud):
    m = loud.Meter(RATE)
    with pytest.raises(ValueError, match='five channels or less'):
        m.integrated_loudness_batch(torch.zeros((1, RATE, 6), device='cuda'))
    with pytest.raises(ValueError, match='length greater than the block size'):
        m.integrated_loudness_batch(torch.zeros((2, 100, 2), device='cuda'))
    with pytest.raises(RuntimeError, match='GPU only'):
        m.integrated_loudness_batch(torch.zeros((1, RATE, 2)))
    with pytest.raises(ValueError):
        m.block_energies_batch(torch.zeros((RATE, 2), device='cuda'))
