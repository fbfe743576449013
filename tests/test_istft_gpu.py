"""GPU: the complex front-end (dam_stft_complex_f32) and the inverse STFT (dam_istft_f32) against torch.stft / torch.istft
in float64 on the CPU, with torch's float32 periodic Hann table up-cast to float64.

Bounds.  Forward: |got - want| over the frame's peak magnitude, every bin, <= 2e-6 -- the bound tests/test_features_gpu.py
holds the dB front-end to (REL_LIN); torch's own float32 stft sits at 1.0e-7 ... 3.0e-7 on these inputs.  Inverse, round trip
and the mag_db form: max|got - want| <= 2e-6 * max|want|; torch's float32 istft is at 1.3e-8 ... 3.9e-7 of the peak on these
inputs, its float32 round trip at <= 6e-7."""
import numpy as np
import pytest
import torch

from _inputs import make_audio
from test_features_gpu import ABS_DB, REL_LIN

pytestmark = pytest.mark.gpu

BOUND = 2e-6
CASES = [(132300, 2048, 1024), (132300, 2048, 512), (16000, 2048, 256), (44100, 256, 64), (88200, 4096, 1024),
         (220500, 2048, 1024)]
KINDS = ['noise', 'sweep', 'impulse']


@pytest.fixture(scope='module')
def features(dam_lib):
    from deep_audio_mixer_amd import features
    return features


def window64(n_fft):
    return torch.hann_window(n_fft, dtype=torch.float32).double()


def stft64(x, n_fft, hop):
    """x: float64 array [n] -> complex128 [bins, T]"""
    return torch.stft(torch.as_tensor(np.asarray(x, dtype=np.float64)), n_fft, hop, window=window64(n_fft), center=True,
                      return_complex=True)


def istft64(spec, n_fft, hop, length):
    return torch.istft(spec, n_fft, hop, window=window64(n_fft), center=True, normalized=False, onesided=True,
                       length=length).numpy()


def forward_error(got, want):
    got, want = np.asarray(got, dtype=np.complex128), want.numpy()
    peak = np.abs(want).max(axis=0, keepdims=True)
    return (np.abs(got - want) / np.maximum(peak, 1e-30)).max()


def check_wave(got, want, what):
    got = np.asarray(got, dtype=np.float64)
    err, peak = np.abs(got - want).max(), np.abs(want).max()
    print('%s: max err %.3e of peak %.3e = %.3e' % (what, err, peak, err / max(peak, 1e-300)))
    assert err <= BOUND * peak, what


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,n_fft,hop', CASES)
def test_forward_complex_matches_torch_f64(features, n, n_fft, hop, kind, dtype):
    x = make_audio(kind, n, seed=n + hop).astype(dtype)
    got = features.stft(torch.from_numpy(x[None]).cuda(), n_fft, hop)
    assert got.dtype == torch.complex64 and tuple(got.shape) == (1, n_fft // 2 + 1, 1 + n // hop)
    want = stft64(x, n_fft, hop)
    err = forward_error(got[0].cpu().numpy(), want)
    print('forward %s %s n=%d n_fft=%d hop=%d: %.3e' % (kind, np.dtype(dtype).name, n, n_fft, hop, err))
    assert err <= REL_LIN == BOUND
    # the dB front-end computes the magnitude of the same bins
    db = features.stft_logmag(torch.from_numpy(x[None]).cuda(), n_fft, hop)[0].cpu().numpy().astype(np.float64)
    mine = 20.0 * np.log10(np.maximum(np.abs(got[0].cpu().numpy().astype(np.complex128)), 1e-5))
    mag = np.abs(want.numpy())
    strong = mag > 1e-3 * mag.max(axis=0, keepdims=True)                 # bins within 60 dB of the frame peak
    if strong.any():
        assert np.abs(mine - db)[strong].max() <= ABS_DB


def test_forward_stereo_gain_int16_and_summed_tracks(features):
    n, n_fft, hop = 44100, 2048, 1024
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal((3, n, 2))).astype(np.float32)
    gain = np.array([0.6, 1.0, 1.4], dtype=np.float32)
    got = features.stft(torch.from_numpy(x).cuda(), n_fft, hop, gain=torch.from_numpy(gain).cuda()).cpu().numpy()
    for k in range(3):
        want = stft64(x[k].astype(np.float64).mean(1) * float(gain[k]), n_fft, hop)
        assert forward_error(got[k], want) <= BOUND
    pcm = np.round(32767 * 0.5 * np.sin(np.arange(n) * 0.01) + 200 * rng.standard_normal(n)).astype(np.int16)
    got = features.stft(torch.from_numpy(pcm[None]).cuda(), n_fft, hop)[0].cpu().numpy()
    assert forward_error(got, stft64(pcm.astype(np.float64) / 32768.0, n_fft, hop)) <= BOUND
    # stems summed at load: all chunks of a planar song, one launch
    S, ch, chunk, n_chunks = 4, 2, 22050, 5
    song = (0.1 * rng.standard_normal((S, ch, chunk * n_chunks + 99))).astype(np.float32)
    got = features.stft_song_chunks_sum(torch.from_numpy(song).cuda(), n_chunks, chunk, n_fft, hop).cpu().numpy()
    assert got.shape == (n_chunks, 1025, 1 + chunk // hop)
    for c in range(n_chunks):
        mono = song[:, :, c * chunk:(c + 1) * chunk].astype(np.float64).mean(1).sum(0)
        assert forward_error(got[c], stft64(mono, n_fft, hop)) <= BOUND


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,n_fft,hop', CASES)
def test_inverse_matches_torch_f64(features, n, n_fft, hop, kind):
    """The same float64 spectrum (rounded to complex64 for the GPU) through torch.istft in float64 and dam_istft_f32."""
    spec = stft64(make_audio(kind, n, seed=n + hop), n_fft, hop)
    spec32 = spec.to(torch.complex64)
    dev = spec32[None].cuda()
    t = spec.shape[1]
    for length in (n, hop * (t - 1), n - 777):
        got = features.istft(dev, hop, length)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, length)
        check_wave(got[0].cpu().numpy(), istft64(spec32.to(torch.complex128), n_fft, hop, length),
                   'inverse %s n=%d n_fft=%d hop=%d length=%d' % (kind, n, n_fft, hop, length))
    assert np.array_equal(features.istft(dev, hop).cpu().numpy(), features.istft(dev, hop, hop * (t - 1)).cpu().numpy())
    # the float32 [..., 2] view is the same call
    assert torch.equal(features.istft(torch.view_as_real(dev), hop, n), features.istft(dev, hop, n))


def test_inverse_zero_spectrum_and_uncovered_tail(features):
    n, n_fft, hop = 44100, 2048, 512
    t = 1 + n // hop
    zero = torch.zeros((2, n_fft // 2 + 1, t), dtype=torch.complex64, device='cuda')
    out = features.istft(zero, hop, n)
    assert out.abs().max().item() == 0.0 and not torch.signbit(out).any()
    # the last frame reaches padded position hop*(t-1) + n_fft, i.e. output sample hop*(t-1) + n_fft/2: nothing beyond
    spec = stft64(make_audio('noise', n, seed=1), n_fft, hop).to(torch.complex64)
    reach = hop * (t - 1) + n_fft // 2
    out = features.istft(spec[None].cuda(), hop, reach + 5000)[0].cpu().numpy()
    assert np.all(out[reach:] == 0.0)
    check_wave(out[:n], istft64(spec.to(torch.complex128), n_fft, hop, n), 'covered part of an over-long output')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,n_fft,hop', CASES)
def test_round_trip(features, n, n_fft, hop, kind):
    x = make_audio(kind, n, seed=n + hop).astype(np.float32)
    got = features.istft(features.stft(torch.from_numpy(x[None]).cuda(), n_fft, hop), hop, n)
    check_wave(got[0].cpu().numpy(), x.astype(np.float64), 'round trip %s n=%d n_fft=%d hop=%d' % (kind, n, n_fft, hop))


@pytest.mark.parametrize('n,n_fft,hop', [(20013, 8192, 2048), (20013, 16384, 4096)])
def test_large_windows_raise_the_lds_limit(features, n, n_fft, hop):
    """8192- and 16384-point windows hold 64 / 128 KB of LDS, above a kernel's default limit: the complex front-end and the
    inverse transform raise theirs on the first call and find it raised on the second."""
    x = make_audio('noise', n, seed=n + hop).astype(np.float32)
    want = stft64(x, n_fft, hop)
    dev = torch.from_numpy(x[None]).cuda()
    for call in ('first', 'second'):
        spec = features.stft(dev, n_fft, hop)
        assert tuple(spec.shape) == (1, n_fft // 2 + 1, 1 + n // hop)
        err = forward_error(spec[0].cpu().numpy(), want)
        print('forward n=%d n_fft=%d hop=%d, %s call: %.3e' % (n, n_fft, hop, call, err))
        assert err <= BOUND
        check_wave(features.istft(spec, hop, n)[0].cpu().numpy(), x.astype(np.float64),
                   'round trip n=%d n_fft=%d hop=%d, %s call' % (n, n_fft, hop, call))


def _compose64(spec32, db32):
    """10^(0.05 db) * X/|X| in float64, (1, 0) where X == 0."""
    x = spec32.to(torch.complex128)
    mag = x.abs()
    unit = torch.where(mag > 0, x / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.ones_like(x))
    return torch.pow(10.0, 0.05 * db32.double()) * unit


@pytest.mark.parametrize('n,n_fft,hop', CASES)
def test_mag_db_form(features, n, n_fft, hop):
    """The magnitudes come from ANOTHER signal than the phases: a kernel that ignores mag_db fails."""
    spec32 = stft64(make_audio('noise', n, seed=11), n_fft, hop).to(torch.complex64)
    other = stft64(make_audio('noise', n, seed=12) + make_audio('sweep', n, seed=0), n_fft, hop)
    db32 = (20.0 * torch.log10(other.abs().clamp_min(1e-5))).float()
    got = features.istft(spec32[None].cuda(), hop, n, mag_db=db32[None].cuda())[0].cpu().numpy()
    want = istft64(_compose64(spec32, db32), n_fft, hop, n)
    check_wave(got, want, 'mag_db n=%d n_fft=%d hop=%d' % (n, n_fft, hop))
    plain = features.istft(spec32[None].cuda(), hop, n)[0].cpu().numpy()
    assert np.abs(plain - want).max() > 1e-2 * np.abs(want).max()          # the two spectra really differ


def test_mag_db_zero_bins_take_phase_one(features):
    n, n_fft, hop = 44100, 2048, 1024
    spec32 = stft64(make_audio('noise', n, seed=21), n_fft, hop).to(torch.complex64)
    spec32[100:300, :] = 0
    spec32[::7, 3] = 0
    db32 = (20.0 * torch.log10(stft64(make_audio('noise', n, seed=22), n_fft, hop).abs().clamp_min(1e-5))).float()
    got = features.istft(spec32[None].cuda(), hop, n, mag_db=db32[None].cuda())[0].cpu().numpy()
    check_wave(got, istft64(_compose64(spec32, db32), n_fft, hop, n), 'mag_db with zero bins')


@pytest.mark.parametrize('n_tracks', [59, 72])
def test_batch_independence_and_determinism(features, n_tracks):
    n, n_fft, hop = 33000, 2048, 1024
    rng = np.random.default_rng(n_tracks)
    x = torch.from_numpy((0.1 * rng.standard_normal((n_tracks, n))).astype(np.float32)).cuda()
    spec = features.stft(x, n_fft, hop)
    db = (20.0 * torch.log10(spec.abs().clamp_min(1e-5))).roll(1, 0).contiguous()
    wave, wave_db = features.istft(spec, hop, n), features.istft(spec, hop, n, mag_db=db)
    assert torch.equal(features.stft(x, n_fft, hop), spec)
    assert torch.equal(features.istft(spec, hop, n), wave) and torch.equal(features.istft(spec, hop, n, mag_db=db), wave_db)
    for k in (0, 1, n_tracks // 2, n_tracks - 1):
        one = features.stft(x[k:k + 1], n_fft, hop)
        assert torch.equal(one[0], spec[k])
        assert torch.equal(features.istft(one, hop, n)[0], wave[k])
        assert torch.equal(features.istft(one, hop, n, mag_db=db[k:k + 1])[0], wave_db[k])


def test_capture_equals_eager(features):
    n, n_fft, hop = 44100, 2048, 512
    rng = np.random.default_rng(0)
    xs = [torch.from_numpy((0.1 * rng.standard_normal((3, n))).astype(np.float32)).cuda() for _ in range(3)]
    x = xs[0].clone()
    spec = torch.empty((3, n_fft // 2 + 1, 1 + n // hop), dtype=torch.complex64, device='cuda')
    out = torch.empty((3, n), dtype=torch.float32, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        features.istft(features.stft(x, n_fft, hop, out=spec), hop, n, out=out)      # warm-up: tables are uploaded
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        features.istft(features.stft(x, n_fft, hop, out=spec), hop, n, out=out)
    for fresh in xs[1:]:
        x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, features.istft(features.stft(fresh, n_fft, hop), hop, n))


def test_argument_checks(features):
    spec = torch.zeros((1, 1025, 10), dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError):
        features.istft(spec, hop=1025)
    with pytest.raises(ValueError):
        features.istft(torch.zeros((1, 51, 10), dtype=torch.complex64, device='cuda'), hop=25)      # n_fft 100
    with pytest.raises(TypeError):
        features.istft(spec.to(torch.complex128), hop=1024)
    with pytest.raises(ValueError):
        features.istft(spec, hop=1024, mag_db=torch.zeros((1, 1025, 9), device='cuda'))
    with pytest.raises(ValueError):
        features.stft(torch.zeros((1, 4096), device='cuda'), n_fft=100, hop=25)
    with pytest.raises(TypeError):
        features.stft(torch.zeros((1, 4096), device='cuda', dtype=torch.float16))
    with pytest.raises(ValueError):          # reflect padding needs N > n_fft / 2, as torch.stft
        features.stft(torch.zeros((1, 1024), device='cuda'))
    with pytest.raises(ValueError):
        features.stft_song_chunks_sum(torch.zeros((2, 2, 4096), device='cuda'), 4, 1024)
    with pytest.raises(ValueError):
        features.istft(spec, hop=1024, length=-5)
    with pytest.raises(TypeError):
        features.istft(spec, hop=1024, length=4096.5)
    with pytest.raises(TypeError):
        features.istft(spec, hop=512.0)
    assert features.istft(spec, hop=np.int64(1024), length=np.int64(4096)).shape == (1, 4096)


def test_length_beyond_the_last_frame_centre(features):
    """length > hop*(T-1), where torch.istft raises: up to the last frame's reach the samples are covered by the falling
    half of the last frame alone, so the output is that frame's irfft sample over the window, w x[j] / w^2 = x[j] / w[j]
    (for a consistent spectrum x is the windowed signal, and this is the signal again).  The numerator's error
    is w times the transform's error (<= 2e-6 of the frame's peak, the bound of the inverse above), the division by w^2
    makes it 2e-6 * peak / w: checked where w >= 0.1.  The last sample of the reach has w^2 below torch's 1e-11 threshold
    and is 0 like everything past it."""
    n, n_fft, hop = 44100, 2048, 1024
    t = 1 + n // hop
    spec = stft64(make_audio('noise', n, seed=5), n_fft, hop).to(torch.complex64)
    centre, reach = hop * (t - 1), hop * (t - 1) + n_fft // 2
    out = features.istft(spec[None].cuda(), hop, reach + 100)[0].cpu().numpy().astype(np.float64)
    frame = torch.fft.irfft(spec[:, -1].to(torch.complex128), n=n_fft).numpy()       # sample j of the last frame
    w = window64(n_fft).numpy()
    j = np.arange(n_fft // 2 + 1, n_fft)          # hop = n_fft/2: past its centre the last frame is alone
    keep = w[j] >= 0.1
    got = out[centre + (j - n_fft // 2)]
    assert keep.sum() > 500
    assert np.all(np.abs(got - frame[j] / w[j])[keep] <= 2e-6 * np.abs(frame).max() / w[j][keep])
    assert np.all(out[reach - 1:] == 0.0) and np.isfinite(out).all()
