"""GPU: LoudnessEvaluator.process_song_tracks(band_fit=..., band_render=...) -- the fitted band gains rendered to audio inside
the whole-song evaluation, on tests/test_evaluation_bandfit_gpu.py's song (four spectrally distinct stereo stems at 8 kHz, the
reference = stems x constants exactly; octave bands at n_fft 256).  What is checked: the new key and only the new key, its
agreement with the same quantity formed in numpy float64 from a render of the reported gains, and the exported file.
Largest observed (1 x MI355X; W 12, 6 bands): 'oracle_band_render_residual' 1.95e-14 .. 2.03e-14 beside a frame-domain total of
2.2e-14; a numpy float64 render of the reported gains leaves 2.4e-18 .. 7.3e-18, a float32 one 1.8e-14 .. 1.9e-14; in amplitude the
device's 1.4e-7 against 1.1e-6 allowed; the exported file within one 16-bit step of reference.wav at a peak of 9079; fill 0:
7.0e-2 .. 7.1e-2."""
import os
import wave

import numpy as np
import pytest
import torch

import _bandmix_ref as mref
import _gainfit_ref as gref
from test_evaluation_bandfit_gpu import BAND, BAND_KEYS, same, song_arrays
from test_gainfit_gpu import CHUNK_LENGTH, CONSTANTS, FIT_KEYS, KEYS, MEAN_LOUDNESS, N_SONG, OLD_KEYS, SR, song

pytestmark = pytest.mark.gpu

KEY = 'oracle_band_render_residual'


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

    runs = {'off': evaluate(a, reference), 'explicit_off': evaluate(a, reference, band_render=False),
            'band': evaluate(a, reference, band_fit=BAND), 'render': evaluate(a, reference, band_fit=BAND, band_render=True),
            'both': evaluate(a, reference, gain_fit=True, band_fit=BAND, band_render={'fill': 'broadband'})}
    yield a, reference, evaluate, runs
    inference_utils._mixers.clear()


def test_switch_adds_one_key_and_changes_nothing_else(evaluator):
    a, reference, evaluate, runs = evaluator
    (off, n_off), (explicit, n_explicit), (band, n_band), (render, n_render), (both, n_both) = (
        runs[k] for k in ('off', 'explicit_off', 'band', 'render', 'both'))
    assert list(off) == OLD_KEYS and same(explicit, off)                # the default call: the keys and the values of before
    assert list(band) == OLD_KEYS + BAND_KEYS
    assert list(render) == OLD_KEYS + BAND_KEYS + [KEY] and list(both) == OLD_KEYS + FIT_KEYS + BAND_KEYS + [KEY]
    for key in OLD_KEYS + BAND_KEYS:
        assert same(render[key], band[key]) and same(both[key], band[key]), key
    assert n_off == n_explicit == n_band == n_render == n_both          # the same number of draws, in the same order
    W = len(render['smooth_gains'][KEYS[0]])
    got, total = np.array(render[KEY]), np.array(render['oracle_band_residual_total'])
    assert got.shape == (W,) and np.all(np.isfinite(got[np.isfinite(total)])) and np.all(got >= 0.0)
    # the broadband fill fitted for the render and the gain fit's own (pool 0, ridge 0, no lag: the same arguments) are one
    assert same(both[KEY], render[KEY])
    print('%s: %.3g .. %.3g beside a frame-domain total of %.3g .. %.3g' % (KEY, got.min(), got.max(), total.min(), total.max()))
    for kw in (dict(band_render=True), dict(gain_fit=True, band_render=True), dict(band_fit=BAND, band_render={'fil': 1.0}),
               dict(band_fit=BAND, band_render={'fill': 'unit'}), dict(band_fit=dict(BAND, hop=200), band_render=True)):
        with pytest.raises(ValueError):
            evaluate(a, reference, **kw)


def test_residual_is_that_of_a_render_of_the_reported_gains(evaluator):
    """The reference is stems x constants, so per-band gains explain all of it: what the render leaves is float32 arithmetic.  The
    reported figure equals, to the float32 of the render, the one numpy forms from its own float64 render of the gains and the
    broadband fill the stats report."""
    from deep_audio_mixer_amd import spectrum
    a, reference, evaluate, runs = evaluator
    stats = runs['both'][0]
    W = len(stats['smooth_gains'][KEYS[0]])
    edges = spectrum.band_edges(SR, 256, 1, 100.0, 20000.0)[0]
    gains = np.array([stats['oracle_band_gains'][k] for k in KEYS]).transpose(1, 0, 2)              # [B, S, W]
    fill = np.array([stats['oracle_gains'][k] for k in KEYS])                                       # [S, W]
    x, y = song_arrays(a, reference)
    want64 = mref.render(x, gains, fill, edges, 256, 128)
    want32 = mref.render(x, gains, fill, edges, 256, 128, transform='f32')
    bounds = gref.window_bounds(N_SONG, W)

    def shares(r):
        d = y - r.T
        return np.array([(d[lo:hi] ** 2).sum() / (y[lo:hi] ** 2).sum() for lo, hi in bounds])
    s64, s32, got = shares(want64), shares(want32), np.array(stats[KEY])
    print('%s: device %.3g .. %.3g, numpy float64 render %.3g .. %.3g, numpy float32 render %.3g .. %.3g'
          % (KEY, got.min(), got.max(), s64.min(), s64.max(), s32.min(), s32.max()))
    # amplitudes: sqrt(share) of the device's render lies within the float64 figure plus 8 x what float32 costs the reference
    c = 8.0 * np.sqrt(np.array([((want32 - want64).T[lo:hi] ** 2).sum() / (y[lo:hi] ** 2).sum() for lo, hi in bounds]))
    print('sqrt: device %.3g .. %.3g, allowed above float64 %.3g .. %.3g' % (np.sqrt(got).min(), np.sqrt(got).max(), c.min(), c.max()))
    assert np.all(c > 0.0) and np.all(np.sqrt(got) <= np.sqrt(s64) + c)


def test_constant_fill_and_the_exported_file(evaluator, tmp_path):
    a, reference, evaluate, runs = evaluator
    results = tmp_path / 'out'
    stats, _ = evaluate(a, reference, band_fit=BAND, band_render=True, write_wavs_to_disk=True, results_dir=str(results))
    base = runs['render'][0]
    for key in OLD_KEYS + BAND_KEYS + [KEY]:
        assert same(stats[key], base[key]), key                         # writing files changes no key
    # fill 0 silences the bins the octave bands from 100 Hz leave out, the 80 Hz of the bass among them: only the new key moves
    silent, _ = evaluate(a, reference, band_fit=BAND, band_render={'fill': 0.0})
    for key in OLD_KEYS + BAND_KEYS:
        assert same(silent[key], base[key]), key
    assert np.all(np.isfinite(silent[KEY])) and np.all(np.array(silent[KEY]) > np.array(base[KEY]))
    names = sorted(os.listdir(str(results)))
    assert 'song a_oracle_band.wav' in names and len(names) == 4 + 2 + 1
    with wave.open(str(results / 'song a_oracle_band.wav'), 'rb') as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, SR, N_SONG)
        pcm = np.frombuffer(w.readframes(N_SONG), dtype='<i2').astype(np.float64)
    with wave.open(str(results / 'song a_reference.wav'), 'rb') as w:
        ref_pcm = np.frombuffer(w.readframes(N_SONG), dtype='<i2').astype(np.float64)
    # both files are at -20 LUFS and per-band gains explain this reference: the same audio but for two 16-bit roundings, each at
    # most half a step -- and a step of slack for the two loudness measurements
    worst = float(np.abs(pcm - ref_pcm).max())
    got = np.array(silent[KEY])
    print('oracle_band.wav against reference.wav (16 bit, both at -20 LUFS): largest difference %.3g steps, peak %.0f; %s with '
          'fill 0: %.3g .. %.3g' % (worst, np.abs(pcm).max(), KEY, got.min(), got.max()))
    assert np.abs(pcm).max() > 1000.0 and worst <= 2.0
