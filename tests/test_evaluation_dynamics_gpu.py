"""GPU: the time-resolved part of the whole-song evaluation (LoudnessEvaluator.process_song_tracks(dynamics=True)): every
variant's short-term loudness profile against the reference mix's, window by window, and the loudness range of the
reference stems -- against the same quantities composed in numpy (tests/_dynamics_ref.py) from the gains the call
returns and numpy's seeded draws.  The song and the model are those of tests/test_evaluation_gpu.py.
Bounds: 1e-7 LU per '*_st_error', the existing process_song_tracks bound (a mean of absolute differences of profiles whose
values are within 1e-8 LU of their host counterparts); 2e-8 LU for the loudness range.
Largest observed errors: NOT YET RECORDED -- no GPU could be obtained while this file was written."""
from statistics import mean

import numpy as np
import pytest
import torch

import _dynamics_ref as dyn
from oracle import loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH = 8000, 2
N = SR * 26 + 77
KEYS = ('bass', 'drums', 'vocals', 'other')
MEAN_LOUDNESS = {'bass': -25.0, 'drums': -21.0, 'vocals': -19.0, 'other': -23.0}
OLD_KEYS = ['song_name', 'sum_error', 'loudnorm_error', 'mix_error', 'random_error', 'smooth_gains']
ST_KEYS = ['sum_st_error', 'loudnorm_st_error', 'mix_st_error', 'random_st_error']


def song(seed):
    rng = np.random.default_rng(seed)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * np.arange(N) / (SR * 7.0))
    return {k: ((0.04 + 0.03 * i) * rng.standard_normal((2, N)) * np.roll(env, i * SR * 2)[None]).astype(np.float32)
            for i, k in enumerate(KEYS)}


def short_term(tracks, gains=None):
    """[stems, windows] from the numpy definition; gains {name: scalar or sequence} are applied as a gain ramp."""
    return np.stack([dyn.dynamics(tracks[k].T, SR, None if gains is None else gains[k])['short_term'] for k in KEYS])


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
    # a reference mix that moves in time: the vocals come up by 6 dB over the song, the drums go down by 6 dB
    ramp = np.linspace(-0.5, 0.5, N, dtype=np.float32)
    reference['vocals'] = (reference['vocals'] * 2.0 ** ramp).astype(np.float32)
    reference['drums'] = (reference['drums'] * 2.0 ** -ramp).astype(np.float32)

    def evaluate(tracks, reference_tracks, dynamics):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        stats = ev.process_song_tracks(tracks, reference_tracks, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH,
                                       dynamics=dynamics)
        return ev, stats, float(np.random.uniform())                        # the next value of the seeded generator

    yield a, reference, evaluate
    inference_utils._mixers.clear()


def test_dynamics_switch_leaves_todays_stats_alone(env):
    a, reference, evaluate = env
    _, off, next_off = evaluate(a, reference, False)
    _, on, next_on = evaluate(a, reference, True)
    assert list(off) == OLD_KEYS and list(on) == OLD_KEYS + ST_KEYS + ['lra']
    for key in OLD_KEYS:
        assert on[key] == off[key], key                                     # the floats exactly, smooth gains included
    assert next_on == next_off                                              # the same number of draws, in the same order


def test_short_term_errors_against_numpy(env):
    a, reference, evaluate = env
    ev, stats, _ = evaluate(a, reference, True)
    np.random.seed(7)
    drawn = [{k: float(np.random.uniform(0.5, 1.5)) for k in KEYS} for _ in range(2)]
    plain = np.array([ref.integrated_loudness(a[k].astype(np.float64).T, SR) for k in KEYS])
    loudnorm = {k: 10.0 ** ((MEAN_LOUDNESS[k] - plain[i]) / 20.0) for i, k in enumerate(KEYS)}
    R = short_term(reference)
    want = {'sum_st_error': dyn.profile_error(R, short_term(a))[0],
            'loudnorm_st_error': dyn.profile_error(R, short_term(a, loudnorm))[0],
            'mix_st_error': dyn.profile_error(R, short_term(a, stats['smooth_gains']))[0],
            'random_st_error': mean(dyn.profile_error(R, short_term(a, g))[0] for g in drawn)}
    for key, value in want.items():
        print('%s: %.9f (numpy %.9f, diff %.3g, bound 1e-7); per song: %s %.9f'
              % (key, stats[key], value, abs(stats[key] - value), key.replace('_st', ''), stats[key.replace('_st', '')]))
    for key, value in want.items():
        assert abs(stats[key] - value) < 1e-7, key
    assert len({round(v, 6) for v in want.values()}) == 4                   # four different figures
    lra = {k: dyn.dynamics(reference[k].T, SR)['lra'] for k in KEYS}
    print('lra: %s (numpy %s)' % (stats['lra'], lra))
    assert list(stats['lra']) == list(KEYS)
    for k in KEYS:
        assert abs(stats['lra'][k] - lra[k]) < 2e-8 and lra[k] > 0.5
    # the evaluator's own curve call is what the stats are made of
    got = ev.evaluate_short_term_batch({k: torch.from_numpy(reference[k]).cuda() for k in KEYS})
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == R.shape
    assert np.abs(got.cpu().numpy() - R).max() < 1e-8


def test_profile_invariance_and_identity(env):
    a, reference, evaluate = env
    _, stats, _ = evaluate(a, reference, True)
    _, half, _ = evaluate({k: v * np.float32(0.5) for k, v in a.items()}, reference, True)
    print('sum_st_error %.12f, all stems at half level %.12f (bound 1e-9)' % (stats['sum_st_error'], half['sum_st_error']))
    assert abs(half['sum_st_error'] - stats['sum_st_error']) < 1e-9 and stats['sum_st_error'] > 0.1
    _, same, _ = evaluate(a, a, True)
    assert same['sum_st_error'] == 0.0 and same['sum_error'] == 0.0
    with pytest.raises(ValueError, match='length'):
        evaluate(a, {k: v[:, :-1] for k, v in a.items()}, True)


def test_songlist_passes_the_switch(env, monkeypatch):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator(SR, KEYS)
    seen = []

    def fake(base_dir, song_name, *args):
        seen.append(args[-1])
        row = {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
        if args[-1]:
            row.update({k: 5.0 + len(song_name) for k in ST_KEYS})
        return row
    monkeypatch.setattr(ev, 'process_song', fake)
    _, means = ev.process_songlist('.', ['a', 'bcd'])
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} and seen == [False, False]
    _, means = ev.process_songlist('.', ['a', 'bcd'], dynamics=True)
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} | set(ST_KEYS) and seen[2:] == [True, True]
    assert means['mix_st_error'] == 7.0
