"""GPU: the spectral part of the whole-song evaluation (LoudnessEvaluator.process_song_tracks(spectral=...)): every
variant's long-term average spectrum in third-octave bands against the reference mix's -- against the same quantities
composed in numpy (tests/_spectrum_ref.py) from the gains the call returns and numpy's seeded draws.  The model and the
evaluator are built as tests/test_evaluation_dynamics_gpu.py builds them; the song has spectrally distinct stems (white-noise
stems would make every variant read about 0).
Bound per figure: the mean over the kept bands of |dL_ref| + |dL_cand|, |dL[b]| <= (10 / ln 10) (beta[b] / P[b] + beta_tot /
P_tot) 1.05 with beta the band-power bound of tests/test_spectrum_gpu.py (a few 1e-5 dB here).  The loudnorm variant's gains
are formed on the device from its own loudness values, within 1e-8 dB of the oracle's: five orders below that bound.
Largest observed errors (1 x MI355X; the test prints them): 4.1e-8 dB on 'mix_spec_error' against a bound of 1.0e-3 dB, 4e-5
of it; the four figures read 1.788 (sum), 1.475 (loudnorm), 0.769 (mix) and 2.869 dB (random), 22 of 22 bands kept."""
from statistics import mean

import numpy as np
import pytest
import torch

import _spectrum_ref as sref
from oracle import loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH = 8000, 2
N = SR * 26 + 77
N_FFT = 1024
KEYS = ('bass', 'drums', 'vocals', 'other')
MEAN_LOUDNESS = {'bass': -25.0, 'drums': -21.0, 'vocals': -19.0, 'other': -23.0}
OLD_KEYS = ['song_name', 'sum_error', 'loudnorm_error', 'mix_error', 'random_error', 'smooth_gains']
ST_KEYS = ['sum_st_error', 'loudnorm_st_error', 'mix_st_error', 'random_st_error']
SPEC_KEYS = ['sum_spec_error', 'loudnorm_spec_error', 'mix_spec_error', 'random_spec_error']


def song(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N) / SR
    tone = lambda f, ph: np.sin(2 * np.pi * f * t[None, :] + np.array([[0.0], [ph]]))
    noise = lambda a: a * rng.standard_normal((2, N))
    tracks = {'bass': 0.20 * tone(80.0, 0.3) + noise(0.002),
              'drums': noise(0.08),
              'vocals': 0.10 * tone(400.0, 0.5) + 0.06 * tone(800.0, 1.1),
              'other': 0.07 * tone(2500.0, 0.7) + noise(0.002)}
    return {k: tracks[k].astype(np.float32) for k in KEYS}


def stack(tracks):
    """{name: [channels, n]} -> [stems, n, channels], the reference's layout."""
    return np.stack([tracks[k].T for k in KEYS])


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(3)
    model = ResNet18(n_stems=4, input_shape=(1025, 16)).cuda().eval()
    a = song(0)
    d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :SR * 2].T for k, v in a.items()}, 'mix': a['bass'][:, :SR * 2].T}},
                                           chunk_length=CHUNK_LENGTH, sr=SR, tracklist=list(KEYS) + ['mix'])
    reference = {k: (v * g).astype(np.float32) for (k, v), g in zip(a.items(), (0.7, 1.2, 1.5, 0.9))}

    def evaluate(tracks, reference_tracks, **kw):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        stats = ev.process_song_tracks(tracks, reference_tracks, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH, **kw)
        return ev, stats, float(np.random.uniform())                        # the next value of the seeded generator

    yield a, reference, evaluate
    inference_utils._mixers.clear()


def test_spectral_switch_leaves_todays_stats_alone(env):
    a, reference, evaluate = env
    _, off, next_off = evaluate(a, reference)
    _, on, next_on = evaluate(a, reference, spectral={'n_fft': N_FFT})
    _, both, next_both = evaluate(a, reference, dynamics=True, spectral={'n_fft': N_FFT})
    assert list(off) == OLD_KEYS and list(on) == OLD_KEYS + SPEC_KEYS + ['ltas']
    assert list(both) == OLD_KEYS + ST_KEYS + ['lra'] + SPEC_KEYS + ['ltas']
    for key in OLD_KEYS:
        assert on[key] == off[key] and both[key] == off[key], key           # the floats exactly, smooth gains included
    for key in SPEC_KEYS + ['ltas']:
        assert both[key] == on[key], key
    assert next_on == next_off == next_both                                 # the same number of draws, in the same order
    assert list(on['ltas']) == ['centres', 'reference', 'mix'] and len(on['ltas']['centres']) == 22
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, reference, spectral={'nfft': N_FFT})


def test_spectral_errors_against_numpy(env):
    from deep_audio_mixer_amd import spectrum
    a, reference, evaluate = env
    ev, stats, _ = evaluate(a, reference, spectral={'n_fft': N_FFT})
    np.random.seed(7)
    drawn = [[float(np.random.uniform(0.5, 1.5)) for _ in KEYS] for _ in range(2)]
    plain = np.array([ref.integrated_loudness(a[k].astype(np.float64).T, SR) for k in KEYS])
    loudnorm = [10.0 ** ((MEAN_LOUDNESS[k] - plain[i]) / 20.0) for i, k in enumerate(KEYS)]
    edges, centres = sref.band_edges(SR, N_FFT)
    assert len(centres) == 22 and stats['ltas']['centres'] == centres.tolist()
    stems, hop = stack(a), N_FFT // 2
    R, R_beta = sref.band_power(stack(reference), None, N_FFT, hop, edges)

    def figure(gains):
        P, beta = sref.band_power(stems, None if gains is None else np.asarray(gains, dtype=np.float64).reshape(4, -1), N_FFT, hop, edges)
        err, kept = sref.balance_error(R, P)
        assert kept == 22 and min(sref.gate_margin(P), sref.gate_margin(R)) > 1e-6      # a condition on the inputs
        return err, sref.balance_error_bound(R, R_beta, P, beta)
    smooth = [stats['smooth_gains'][k] for k in KEYS]
    want = {'sum_spec_error': figure(None), 'loudnorm_spec_error': figure(loudnorm), 'mix_spec_error': figure(smooth)}
    rnd = [figure(g) for g in drawn]
    want['random_spec_error'] = (mean(e for e, _ in rnd), mean(b for _, b in rnd))
    for key, (value, bound) in want.items():
        print('%s: %.9f dB (numpy %.9f, |diff| %.3g = %.2e of the bound %.3g); per song loudness: %.6f'
              % (key, stats[key], value, abs(stats[key] - value), abs(stats[key] - value) / bound, bound,
                 stats[key.replace('_spec', '')]))
    for key, (value, bound) in want.items():
        assert abs(stats[key] - value) <= bound, key
    values = [v for v, _ in want.values()]
    assert len({round(v, 3) for v in values}) == 4 and min(values) > 0.5     # four clearly different figures
    # the evaluator's own spectrum call is what the stats are made of
    dev = lambda tracks: {k: torch.from_numpy(tracks[k]).cuda() for k in KEYS}
    got = ev.evaluate_spectrum_batch(dev(reference), n_fft=N_FFT)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (1, 22)
    assert spectrum.relative_levels_db(got)[0].cpu().tolist() == stats['ltas']['reference']
    mix = ev.evaluate_spectrum_batch(dev(a), torch.tensor(smooth, dtype=torch.float64, device='cuda'), n_fft=N_FFT)
    assert spectrum.relative_levels_db(mix)[0].cpu().tolist() == stats['ltas']['mix']
    assert np.all(np.abs(got[0].cpu().numpy() - R) <= R_beta)
    assert np.abs(np.array(stats['ltas']['reference']) - sref.relative_levels_db(R)).max() <= sref.level_bound(R, R_beta).max()


def test_level_invariance_identity_and_lengths(env):
    a, reference, evaluate = env
    _, stats, _ = evaluate(a, reference, spectral={'n_fft': N_FFT})
    _, half, _ = evaluate({k: v * np.float32(0.5) for k, v in a.items()}, reference, spectral={'n_fft': N_FFT})
    print('sum_spec_error %.17g, all stems at half level %.17g (bitwise expected)' % (stats['sum_spec_error'], half['sum_spec_error']))
    assert half['sum_spec_error'] == stats['sum_spec_error'] and stats['sum_spec_error'] > 0.5
    _, same, _ = evaluate(a, a, spectral={'n_fft': N_FFT})
    assert same['sum_spec_error'] == 0.0 and same['sum_error'] == 0.0
    _, shorter, _ = evaluate(a, {k: v[:, :-1] for k, v in reference.items()}, spectral={'n_fft': N_FFT})
    assert abs(shorter['sum_spec_error'] - stats['sum_spec_error']) < 0.05   # a long-term average: one sample is nothing


def test_songlist_passes_the_switch(env, monkeypatch):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator(SR, KEYS)
    seen = []

    def fake(base_dir, song_name, *args, **kw):
        seen.append((len(args), kw))
        row = {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
        if kw.get('spectral'):
            row.update({k: 5.0 + len(song_name) for k in SPEC_KEYS})
        return row
    monkeypatch.setattr(ev, 'process_song', fake)
    _, means = ev.process_songlist('.', ['a', 'bcd'])
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} and seen == [(6, {}), (6, {})]
    _, means = ev.process_songlist('.', ['a', 'bcd'], spectral={'n_fft': N_FFT})
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} | set(SPEC_KEYS)
    assert seen[2:] == [(6, {'spectral': {'n_fft': N_FFT}})] * 2 and means['mix_spec_error'] == 7.0
