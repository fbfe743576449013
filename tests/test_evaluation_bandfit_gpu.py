"""GPU: LoudnessEvaluator.process_song_tracks(band_fit=...) -- the band gain fit inside the whole-song evaluation.

The song is tests/test_gainfit_gpu.py's (four spectrally distinct stereo stems at 8 kHz, the reference = stems x constants
exactly), fitted in octave bands at n_fft 256.  Bounds: with c the moment bound of tests/test_bandfit_gpu.py (8 x what a float32
transform costs the reference on this very input) and kappa the reference's cond(R) of a cell, the oracle band gains lie
within c kappa max|g_ref| of the reference's, the band residuals within c kappa (1 + sum|g_ref|)^2, the total likewise with
the largest kappa of the window; the band gain errors equal numpy's on the device's own gains to 1e-10 dB.
Largest observed (1 x MI355X; W 12, 6 bands, c 3.9e-6, kappa <= 2.5): gains 0.25, residual 6.6e-10, total 1.7e-10 of their bounds,
the planted constants back to 1.6e-6, band residuals <= 7.7e-14; band gain errors equal numpy's to 4.4e-16 dB; two-band
reference: oracle_residual 2.4e-2 .. 2.5e-2, band total 2.7e-10 .. 3.4e-6, 38.5 .. 79.6 dB under it."""
import math
from statistics import mean

import numpy as np
import pytest
import torch

import _bandfit_ref as ref
import _gainfit_ref as gref
from test_gainfit_gpu import CHUNK_LENGTH, CONSTANTS, FIT_KEYS, KEYS, MEAN_LOUDNESS, N_SONG, OLD_KEYS, SR, song

pytestmark = pytest.mark.gpu

BAND = {'n_fft': 256, 'hop': 128, 'fraction': 1, 'f_lo': 100.0}
BAND_KEYS = ['sum_band_gain_error', 'loudnorm_band_gain_error', 'mix_band_gain_error', 'random_band_gain_error',
             'oracle_band_centres', 'oracle_band_gains', 'oracle_band_residual', 'oracle_band_residual_total']


def same(a, b):
    """two stats values, bit for bit (lists and dicts of floats, arrays, NaN equal to NaN)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


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

    def make():
        return LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)

    def evaluate(tracks, reference_tracks, **kw):
        stats = make().process_song_tracks(tracks, reference_tracks, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH, **kw)
        return stats, float(np.random.uniform())                        # the next value of the seeded generator

    runs = {'off': evaluate(a, reference), 'explicit_off': evaluate(a, reference, band_fit=False),
            'gain': evaluate(a, reference, gain_fit=True), 'both': evaluate(a, reference, gain_fit=True, band_fit=BAND),
            'band': evaluate(a, reference, band_fit=BAND)}
    yield a, reference, evaluate, runs, make
    inference_utils._mixers.clear()


def test_switch_leaves_todays_stats_alone(evaluator):
    a, reference, evaluate, runs, _ = evaluator
    (off, n_off), (explicit, n_explicit), (gain, n_gain), (both, n_both), (band, n_band) = (runs[k] for k in
                                                                                          ('off', 'explicit_off', 'gain', 'both', 'band'))
    assert list(off) == OLD_KEYS and list(explicit) == OLD_KEYS and same(explicit, off)
    assert list(gain) == OLD_KEYS + FIT_KEYS and list(both) == OLD_KEYS + FIT_KEYS + BAND_KEYS
    assert list(band) == OLD_KEYS + BAND_KEYS
    for key in OLD_KEYS:
        assert same(both[key], off[key]) and same(band[key], off[key]) and same(gain[key], off[key]), key
    for key in FIT_KEYS:
        assert same(both[key], gain[key]), key
    for key in BAND_KEYS:
        assert same(both[key], band[key]), key                          # the band fit does not depend on the gain fit
    assert n_off == n_explicit == n_gain == n_both == n_band            # the same number of draws, in the same order
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, reference, band_fit={'nfft': 256})
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, reference, gain_fit={'n_fft': 256})
    with pytest.raises(ValueError, match='length'):
        evaluate(a, {k: v[:, :-1] for k, v in reference.items()}, band_fit=BAND)


def song_arrays(a, reference):
    x = np.stack([a[k].T for k in KEYS])                                # [S, n, C]
    y = np.zeros((N_SONG, 2))
    for k in KEYS:
        y = y + reference[k].T.astype(np.float64)
    return x, y


def test_oracle_band_stats_against_reference(evaluator):
    from deep_audio_mixer_amd import spectrum
    a, reference, evaluate, runs, _ = evaluator
    stats = runs['both'][0]
    W = len(stats['smooth_gains'][KEYS[0]])
    edges, centres = spectrum.band_edges(SR, 256, 1, 100.0, 20000.0)
    B = len(centres)
    assert B >= 5 and isinstance(stats['oracle_band_centres'], np.ndarray) and np.array_equal(stats['oracle_band_centres'], centres)
    gains = np.array([stats['oracle_band_gains'][k] for k in KEYS]).transpose(1, 0, 2)              # [B, S, W]
    residual, total = np.array(stats['oracle_band_residual']), np.array(stats['oracle_band_residual_total'])
    assert gains.shape == (B, 4, W) and residual.shape == (B, W) and total.shape == (W,) and list(stats['oracle_band_gains']) == list(KEYS)
    x, y = song_arrays(a, reference)
    want = ref.moments(x, y, W, 256, 128, edges)
    c = 8.0 * ref.moment_ratio(ref.moments(x, y, W, 256, 128, edges, transform='f32'), want)
    g_ref, r_ref, t_ref, s_ref, kappa = ref.solve_bands(want)
    assert np.all(s_ref == 4) and np.array_equal(np.isnan(gains), np.isnan(g_ref)) and not np.isnan(gains).any()
    bound_g = c * kappa * np.abs(g_ref).max(axis=1)
    bound_r = c * kappa * (1.0 + np.abs(g_ref).sum(axis=1)) ** 2
    eg = np.abs(gains - g_ref).max(axis=1) / bound_g
    er = np.abs(residual - r_ref) / bound_r
    et = np.abs(total - ref.summary(r_ref, t_ref, s_ref)) / bound_r.max(axis=0)
    known = np.abs(gains - np.array(CONSTANTS)[None, :, None]).max()
    print('evaluator band fit: W %d, %d bands, c %.3g, kappa <= %.3g; gains %.3g, residual %.3g, total %.3g of their bounds; '
          'against the planted constants %.3g; residual <= %.3g' % (W, B, c, kappa.max(), eg.max(), er.max(), et.max(), known, residual.max()))
    assert np.all(eg <= 1.0) and np.all(er <= 1.0) and np.all(et <= 1.0) and np.all(residual >= 0.0)
    # the band gain errors: numpy's on the device's own gains, every (band, window) a window, the curves repeated over the bands
    fit = gains.transpose(1, 0, 2).reshape(4, B * W)
    smooth = np.array([stats['smooth_gains'][k] for k in KEYS])
    np.random.seed(7)
    drawn = np.array([[float(np.random.uniform(0.5, 1.5)) for _ in KEYS] for _ in range(2)])
    repeat = lambda curve: np.broadcast_to(curve[:, None, :], (4, B, W)).reshape(4, B * W)
    want_sum = gref.gain_error(fit, np.ones((1, 4, 1)))[0][0]
    want_mix = gref.gain_error(fit, repeat(smooth)[None])[0][0]
    want_random = float(np.mean(gref.gain_error(fit, drawn[:, :, None])[0]))
    for key, value in (('sum_band_gain_error', want_sum), ('mix_band_gain_error', want_mix), ('random_band_gain_error', want_random)):
        print('%s: %.12f dB (numpy %.12f, |diff| %.3g)' % (key, stats[key], value, abs(stats[key] - value)))
    for key, value in (('sum_band_gain_error', want_sum), ('mix_band_gain_error', want_mix), ('random_band_gain_error', want_random)):
        assert abs(stats[key] - value) <= 1e-10, key
    assert want_sum > 1.0 and math.isfinite(stats['loudnorm_band_gain_error']) and stats['loudnorm_band_gain_error'] > 0.0


def test_two_band_reference_has_30_db_of_headroom(evaluator):
    """A reference that gives every stem one gain below 700 Hz and another above 1.4 kHz: no gain-only mixer explains it
    ('oracle_residual'), a band-gain mixer does ('oracle_band_residual_total')."""
    a, reference, evaluate, runs, _ = evaluator
    rng = np.random.default_rng(11)
    low = {k: np.stack([ref.band_limited_noise(rng, N_SONG, SR, 150.0, 700.0) for _ in range(2)]) for k in KEYS}
    high = {k: np.stack([ref.band_limited_noise(rng, N_SONG, SR, 1400.0, 3500.0) for _ in range(2)]) for k in KEYS}
    ga, gb = rng.uniform(0.5, 1.5, 4), rng.uniform(0.5, 1.5, 4)
    tracks = {k: (low[k] + high[k]).astype(np.float32) for k in KEYS}
    planted = {k: (ga[i] * low[k] + gb[i] * high[k]).astype(np.float32) for i, k in enumerate(KEYS)}
    stats, _ = evaluate(tracks, planted, gain_fit=True, band_fit={'n_fft': 256, 'hop': 128})
    broadband, total = np.array(stats['oracle_residual']), np.array(stats['oracle_band_residual_total'])
    headroom = 10.0 * np.log10(total / broadband)
    print('two-band reference: oracle_residual %.3g .. %.3g, band total %.3g .. %.3g: %.1f .. %.1f dB'
          % (broadband.min(), broadband.max(), total.min(), total.max(), headroom.max(), headroom.min()))
    assert np.all(broadband > 1e-3) and np.all(headroom <= -30.0)


def test_songlist_averages_the_band_errors(evaluator, monkeypatch):
    a, reference, evaluate, runs, make = evaluator
    ev = make()
    other = song(1)
    songs = {'first': (a, reference), 'second': (other, {k: v * np.float32(c) for (k, v), c in zip(other.items(), CONSTANTS[::-1])})}

    def from_arrays(base_dir, song_name, n_random_samples, chunk_length, *args, **kw):
        return ev.process_song_tracks(songs[song_name][0], songs[song_name][1], song_name, 2, CHUNK_LENGTH, **kw)
    monkeypatch.setattr(ev, 'process_song', from_arrays)
    rows, means = ev.process_songlist('.', list(songs), band_fit=BAND)
    keys = [k for k in BAND_KEYS if k.endswith('_error')]
    assert len(rows) == 2 and all(list(row) == OLD_KEYS + BAND_KEYS for row in rows)
    assert rows[0]['sum_band_gain_error'] != rows[1]['sum_band_gain_error']
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} | set(keys)
    for key in keys:
        assert math.isfinite(means[key]) and means[key] == mean(row[key] for row in rows), key
