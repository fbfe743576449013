"""GPU: what the alignment is for -- the gain fit on a mix whose stems entered it late or early.

Stems times known constants, each delayed by its own d_s in [-40, 40] before the sum.  Without ``align`` the fit compares
every stem with a copy of itself that sits somewhere else: the gains and the residual are wrong.  With ``align=64`` the lags
come back exactly, the shifted stems ARE the delayed copies the mix holds (zeros shifted in on both sides), and the gains
come back to the end-to-end bound tests/test_gainfit_gpu.py uses for a fit from samples: with u = 2^-53, N the addends of one
moment and kappa the reference's cond(R) of the window, gains within 64 kappa N u max|g|, residual within
64 kappa N u (1 + sum|g|)^2 of 0.  The unaligned fit is only asserted to be worse than the aligned one by a clear factor, FACTOR
= 1e6, not to reach a value.
Observed (1 x MI355X): aligned gains 8.0e-6 and residual 8.4e-7 of the bounds (2.9e-11, 5.6e-10; kappa <= 1.142), that is gains
to 2.2e-16 and residual 4.5e-16; unaligned gain error 1.48 .. 1.53 and residual 0.998 .. 1 -- 5e10 and 2e9 times the bounds.
Evaluator (W 12, kappa <= 1.033): aligned oracle gains within 4.4e-16 of the undelayed run, unaligned off by 2.25 .. 2.28."""

import numpy as np
import pytest
import torch

import _align_ref as ref
import _gainfit_ref as gf

pytestmark = pytest.mark.gpu

U = gf.U_ROUND
S0, C0, N0, W0, L0 = 4, 2, 6007, 5, 64
CONSTANTS = (0.75, 1.25, 1.5, 0.875)
DELAYS = [-40, 7, 23, 40]
FACTOR = 1e6


def up_stems(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)


def up_mix(y):
    return torch.from_numpy(np.ascontiguousarray(y.T)).cuda().transpose(0, 1)


def bits_equal(a, b):
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


@pytest.fixture(scope='module')
def delayed(dam_lib):
    """Independent float32 stems at 0.1 RMS; mix = sum_s CONSTANTS[s] * (stem s delayed by DELAYS[s]) in float64."""
    rng = np.random.default_rng(41)
    x = (0.1 * rng.standard_normal((S0, N0, C0))).astype(np.float32)
    moved = ref.shift(x, DELAYS)                                        # float32: exactly what the aligned stems must be
    y = np.zeros((N0, C0))
    for s in range(S0):
        y = y + moved[s].astype(np.float64) * CONSTANTS[s]
    return x, moved, y, up_stems(x), up_mix(y)


def test_fit_needs_the_alignment_and_gets_it(delayed):
    from deep_audio_mixer_amd import align, gainfit
    x, moved, y, dx, dy = delayed
    lag, frac, peak, sign, status = align.estimate_lag(dx, dy, L0)
    assert lag.tolist() == DELAYS and sign.tolist() == [1] * S0 and status.tolist() == [1] * S0
    assert np.array_equal(align.shift_tracks(dx, lag).cpu().numpy(), moved)
    want = np.array(CONSTANTS)[:, None]
    # the reference's solution of the aligned problem, its kappa and N: the bound of tests/test_gainfit_gpu.py, end to end
    g_ref, r_ref, s_ref, kappa = gf.solve(gf.moments(moved, y, W0))
    N = gf.addends(N0, W0, C0)
    bound_g = 64.0 * kappa * N * U * max(CONSTANTS)
    bound_r = 64.0 * kappa * N * U * (1.0 + sum(CONSTANTS)) ** 2
    assert s_ref.tolist() == [S0] * W0
    gains, residual, st = gainfit.fit_gains(dx, dy, W0, align=L0)
    g, r = gains.cpu().numpy(), residual.cpu().numpy()
    eg, er = np.abs(g - want).max(axis=0), r
    print('aligned: gains %.3g, residual %.3g of the end-to-end bounds (%.3g, %.3g); kappa <= %.3f'
          % ((eg / bound_g).max(), (er / bound_r).max(), bound_g.max(), bound_r.max(), kappa.max()))
    assert st.tolist() == [S0] * W0 and np.all(eg <= bound_g) and np.all(er <= bound_r) and np.all(r >= 0.0)
    assert np.abs(g - g_ref).max() <= bound_g.max()
    # the same call as its parts
    parts = gainfit.fit_gains(align.shift_tracks(dx, lag), dy, W0)
    assert all(bits_equal(a, b) for a, b in zip((gains, residual, st), parts))
    # ... and without the alignment: worse by a clear factor, in the gains and in the residual
    g0, r0, _ = gainfit.fit_gains(dx, dy, W0)
    eg0, er0 = np.abs(g0.cpu().numpy() - want).max(axis=0), r0.cpu().numpy()
    print('unaligned: gain error %.3g .. %.3g (aligned %.3g), residual %.3g .. %.3g (aligned %.3g)'
          % (eg0.min(), eg0.max(), eg.max(), er0.min(), er0.max(), er.max()))
    assert np.all(eg0 >= FACTOR * np.maximum(eg, bound_g)) and np.all(er0 >= FACTOR * np.maximum(er, bound_r))


def test_align_none_is_todays_path_bit_for_bit(delayed):
    from deep_audio_mixer_amd import gainfit
    x, moved, y, dx, dy = delayed
    today = gainfit.solve(gainfit.moments(dx, dy, W0), pool=1, ridge=1e-9)
    for got in (gainfit.fit_gains(dx, dy, W0, pool=1, ridge=1e-9), gainfit.fit_gains(dx, dy, W0, pool=1, ridge=1e-9, align=None)):
        assert all(bits_equal(a, b) for a, b in zip(got, today))
    with pytest.raises(ValueError):
        gainfit.fit_gains(dx, dy, W0, align=0)
    with pytest.raises(ValueError):
        gainfit.fit_gains(dx, dy, W0, align=ref.MAX_LAG + 1)


def test_loader_aligns_stems_to_the_mix(dam_lib, tmp_path):
    """load_tracks_musdb18(align_to_mix=...) on files whose mix holds the stems at other offsets: float WAVs, so that the
    loaded arrays are the written ones and the shifted stems can be compared exactly."""
    from deep_audio_mixer_amd.data import dataset_utils
    rng = np.random.default_rng(8)
    n, sr, names, delays = 3000, 8000, ('bass', 'drums'), [-12, 30]
    x = (0.1 * rng.standard_normal((2, n, 2))).astype(np.float32)
    mix = ref.shift(x, delays).sum(axis=0).astype(np.float32)
    os_dir = tmp_path / 'song'
    os_dir.mkdir()
    for name, a in zip(names + ('mixture',), (x[0], x[1], mix)):
        dataset_utils.write_wav(str(os_dir / (name + '.wav')), a, sr, subtype='FLOAT')
    plain = dataset_utils.load_tracks_musdb18(str(tmp_path), 'song', tracklist=names + ('mix',), sr=sr)
    moved = dataset_utils.load_tracks_musdb18(str(tmp_path), 'song', tracklist=names + ('mix',), sr=sr, align_to_mix=64)
    assert list(moved) == list(plain) and np.array_equal(moved['mix'], plain['mix'])
    for i, name in enumerate(names):
        assert np.array_equal(plain[name], x[i].T) and moved[name].dtype == np.float32
        assert np.array_equal(moved[name], ref.shift(x, delays)[i].T), name
    with pytest.raises(ValueError, match='mix'):
        dataset_utils.load_tracks_musdb18(str(tmp_path), 'song', tracklist=names, sr=sr, align_to_mix=64)


# ---- the evaluator: LoudnessEvaluator.process_song_tracks(gain_fit={'align': ...}) on the song of tests/test_gainfit_gpu.py
SR, CHUNK_LENGTH = 8000, 2
N_SONG = SR * 26 + 77
KEYS = ('bass', 'drums', 'vocals', 'other')
MEAN_LOUDNESS = {'bass': -25.0, 'drums': -21.0, 'vocals': -19.0, 'other': -23.0}
SONG_DELAYS = {'bass': 0, 'drums': -37, 'vocals': 12, 'other': 40}
OLD_KEYS = ['song_name', 'sum_error', 'loudnorm_error', 'mix_error', 'random_error', 'smooth_gains']
FIT_KEYS = ['sum_gain_error', 'loudnorm_gain_error', 'mix_gain_error', 'random_gain_error', 'oracle_gains', 'oracle_residual']
LAG_KEYS = ['oracle_lag', 'oracle_lag_peak']


def song(seed):
    """tests/test_gainfit_gpu.py's song: four spectrally distinct stereo stems on the 16-bit grid, so that a stem times a
    constant of three significant bits is exact in float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(N_SONG) / SR
    tone = lambda f, ph: np.sin(2 * np.pi * f * t[None, :] + np.array([[0.0], [ph]]))
    noise = lambda a: a * rng.standard_normal((2, N_SONG))
    tracks = {'bass': 0.20 * tone(80.0, 0.3) + noise(0.002),
              'drums': noise(0.08),
              'vocals': 0.10 * tone(400.0, 0.5) + 0.06 * tone(800.0, 1.1) + noise(0.002),
              'other': 0.07 * tone(2500.0, 0.7) + noise(0.002)}
    return {k: (np.round(tracks[k] * 32768.0) / 32768.0).astype(np.float32) for k in KEYS}


def delay_tracks(tracks, delays):
    """{name: [channels, n]} with every track delayed by delays[name] samples, zeros shifted in."""
    return {k: np.ascontiguousarray(ref.shift(v.T[None], [delays[k]])[0].T) for k, v in tracks.items()}


@pytest.fixture(scope='module')
def evaluator(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(3)
    model = ResNet18(n_stems=4, input_shape=(1025, 16)).cuda().eval()
    a = song(0)
    d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :SR * 2].T for k, v in a.items()}, 'mix': a['bass'][:, :SR * 2].T}},
                                           chunk_length=CHUNK_LENGTH, sr=SR, tracklist=list(KEYS) + ['mix'])
    reference = {k: v * np.float32(c) for (k, v), c in zip(a.items(), CONSTANTS)}

    def evaluate(tracks, reference_tracks, **kw):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        stats = ev.process_song_tracks(tracks, reference_tracks, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH, **kw)
        return stats, float(np.random.uniform())                        # the next value of the seeded generator
    yield a, reference, evaluate
    inference_utils._mixers.clear()


def test_evaluator_aligns_the_stems_to_the_reference(evaluator):
    a, reference, evaluate = evaluator
    # the reference holds every stem late or early by SONG_DELAYS: the raw stems are the undelayed ones
    late = delay_tracks(reference, SONG_DELAYS)
    (plain, next_plain), (fit, next_fit) = evaluate(a, late), evaluate(a, late, gain_fit=True)
    aligned, next_aligned = evaluate(a, late, gain_fit={'align': L0})
    undelayed, next_undelayed = evaluate(a, reference, gain_fit={'align': L0})
    assert list(plain) == OLD_KEYS and list(fit) == OLD_KEYS + FIT_KEYS and list(aligned) == OLD_KEYS + FIT_KEYS + LAG_KEYS
    for key in OLD_KEYS:                                                # the old keys and the next seeded draw do not move
        assert aligned[key] == plain[key] == fit[key], key
    assert next_aligned == next_plain == next_fit == next_undelayed
    assert aligned['oracle_lag'] == SONG_DELAYS and undelayed['oracle_lag'] == {k: 0 for k in KEYS}
    assert list(aligned['oracle_lag_peak']) == list(KEYS) and all(0.0 < v <= 1.0 + 1e-6 for v in aligned['oracle_lag_peak'].values())
    # the oracle gains equal the undelayed run's, within the end-to-end bound of this song (tests/test_gainfit_gpu.py: its
    # kappa <= 1.023; here computed from the aligned problem itself)
    W = len(aligned['smooth_gains'][KEYS[0]])
    x = np.stack([a[k].T for k in KEYS])
    y = np.zeros((N_SONG, 2))
    for k in KEYS:
        y = y + late[k].T.astype(np.float64)
    moved = ref.shift(x, [SONG_DELAYS[k] for k in KEYS])
    from deep_audio_mixer_amd import gainfit
    M = gainfit.moments(up_stems(moved), up_mix(y), W)
    _, _, s_ref, kappa = gf.solve(M.cpu().numpy())
    assert s_ref.tolist() == [4] * W
    N = gf.addends(N_SONG, W, 2)
    bound_g = 64.0 * kappa * N * U * max(CONSTANTS)
    got = np.array([aligned['oracle_gains'][k] for k in KEYS])
    base = np.array([undelayed['oracle_gains'][k] for k in KEYS])
    raw = np.array([fit['oracle_gains'][k] for k in KEYS])
    d_aligned, d_raw = np.abs(got - base).max(axis=0), np.abs(raw - base)[1:].max(axis=0)
    print('evaluator: W %d, kappa <= %.3f; aligned oracle gains within %.3g of the undelayed run (%.3g of the bound), '
          'unaligned off by %.3g .. %.3g on the delayed stems' % (W, kappa.max(), d_aligned.max(), (d_aligned / (2.0 * bound_g)).max(),
                                                                    d_raw.min(), d_raw.max()))
    assert np.all(d_aligned <= 2.0 * bound_g)                           # both runs within the bound of the planted constants
    assert np.abs(got - np.array(CONSTANTS)[:, None]).max() <= bound_g.max()
    assert np.all(d_raw >= FACTOR * bound_g)                            # the reason the key exists
    with pytest.raises(ValueError):
        evaluate(a, late, gain_fit={'align': 0})
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, late, gain_fit={'aline': 64})
