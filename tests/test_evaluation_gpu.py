"""GPU: whole-song loudness evaluation (evaluation.py:77-145) -- the 'loudness' kind of SongMixer (model gains -> smoothing
-> batched BS.1770 meter with the gain ramp applied at load -> device gating, one hipGraph), the master at a target
loudness, and LoudnessEvaluator.process_song_tracks / process_songlist against the same quantities composed on the host
from the CPU oracle meter, the gains the calls return and numpy's seeded draws.
Bounds: 1e-8 LU per loudness and 1e-6 LU "at target" (tests/test_loudness_gpu.py); a loudness error is a mean of four
absolute differences of two profiles, each value within 1e-8 of its host counterpart up to the profile's mean: 1e-7."""
import os
from statistics import mean

import numpy as np
import pytest
import torch

from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH = 8000, 2
N = SR * 26 + 77                                   # 13 chunks of 2 s (16 frames each), 12 gains, Savitzky-Golay window 3
KEYS = ('bass', 'drums', 'vocals', 'other')
MEAN_LOUDNESS = {'bass': -25.0, 'drums': -21.0, 'vocals': -19.0, 'other': -23.0}


def song(seed):
    rng = np.random.default_rng(seed)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * np.arange(N) / (SR * 7.0))
    return {k: ((0.04 + 0.03 * i) * rng.standard_normal((2, N)) * np.roll(env, i * SR * 2)[None]).astype(np.float32)
            for i, k in enumerate(KEYS)}


def lufs_of(tracks, gains=None):
    """Oracle loudness of every stem ([channels, n]), optionally times its gain: a scalar or a chunk gain sequence."""
    out = []
    for k in KEYS:
        a = tracks[k].astype(np.float64)
        if gains is not None:
            g = np.atleast_1d(np.asarray(gains[k], dtype=np.float64))
            a = a * (inference_ref.interpolate_mask(g, a.shape[1]) if len(g) > 1 else g[0])
        out.append(ref.integrated_loudness(a.T, SR))
    return np.array(out)


def profile(lufs):
    return lufs - lufs.mean()


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(3)
    model = ResNet18(n_stems=4, input_shape=(1025, 16)).cuda().eval()
    a = song(0)
    d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :SR * 2].T for k, v in a.items()}, 'mix': a['bass'][:, :SR * 2].T}},
                                           chunk_length=CHUNK_LENGTH, sr=SR, tracklist=list(KEYS) + ['mix'])
    yield model, d, a, song(1)
    inference_utils._mixers.clear()


def test_mix_song_loudness(env):
    from deep_audio_mixer_amd import inference_utils
    model, d, a, b = env
    lufs, raw, smooth = inference_utils.mix_song_loudness(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR)
    mixer = next(iter(inference_utils._mixers.values()))
    assert mixer.kind == 'loudness' and mixer.graph is not None and mixer.n_proc == 12
    assert list(lufs) == list(KEYS) and len(raw['bass']) == len(smooth['bass']) == 12
    err = np.abs(np.array([lufs[k] for k in KEYS]) - lufs_of(a, smooth)).max()
    print('mix_song_loudness: max err %.3g LU (bound 1e-8)' % err)
    assert err < 1e-8
    graph = mixer.graph
    lufs_b, _, smooth_b = inference_utils.mix_song_loudness(d, model, b, chunk_length=CHUNK_LENGTH, sr=SR)
    assert next(iter(inference_utils._mixers.values())).graph is graph                    # a replay, not a new capture
    assert not np.allclose(smooth_b['bass'], smooth['bass'])
    assert np.abs(np.array([lufs_b[k] for k in KEYS]) - lufs_of(b, smooth_b)).max() < 1e-8
    inference_utils._mixers.clear()                      # (a mixer keeps the graph of its last eval-mode launch)
    model.train()
    try:
        lufs_t, _, smooth_t = inference_utils.mix_song_loudness(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR)
        assert next(iter(inference_utils._mixers.values())).graph is None                 # chunk by chunk, eagerly
        assert np.abs(np.array([lufs_t[k] for k in KEYS]) - lufs_of(a, smooth_t)).max() < 1e-8
    finally:
        model.eval()
        inference_utils._mixers.clear()


def test_master_at_target_loudness(env):
    from deep_audio_mixer_amd import inference_utils
    model, d, a, _ = env
    master, raw, smooth = inference_utils.mix_song_to_master(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR,
                                                             normalize='loudness', target_lufs=-20.0)
    assert next(iter(inference_utils._mixers.values())).graph is not None
    assert master.shape == (2, N) and master.dtype == np.float64
    got = ref.integrated_loudness(master.T, SR)
    print('master: %.9f LUFS (target -20, bound 1e-6)' % got)
    assert abs(got - (-20.0)) < 1e-6
    mixed = np.sum(np.array([a[k].astype(np.float64) * inference_ref.interpolate_mask(smooth[k], N) for k in KEYS]), axis=0)
    want = ref.normalize_loudness(mixed.T, ref.integrated_loudness(mixed.T, SR), -20.0).T
    print('master: max rel err %.3g (bound 1e-9)' % np.max(np.abs(master - want) / np.maximum(np.abs(want), 1e-300)))
    np.testing.assert_allclose(master, want, rtol=1e-9)
    # normalize=True / False keep their meaning
    peak, _, _ = inference_utils.mix_song_to_master(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR, normalize=True)
    assert np.allclose(np.abs(peak).max(axis=1), 1.0)
    plain, _, smooth_p = inference_utils.mix_song_to_master(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR, normalize=False)
    np.testing.assert_allclose(plain, mixed, rtol=1e-6, atol=1e-9)


def host_stats(tracks, reference_tracks, smooth_gains, random_gains):
    """evaluation.py:77-116 composed on the host from the oracle meter."""
    want_ref = profile(lufs_of(reference_tracks))

    def error(lufs):
        return float(np.mean(np.abs(profile(lufs) - want_ref)))
    plain = lufs_of(tracks)
    loudnorm = {k: 10.0 ** ((MEAN_LOUDNESS[k] - plain[i]) / 20.0) for i, k in enumerate(KEYS)}
    return {'sum_error': error(plain), 'loudnorm_error': error(lufs_of(tracks, loudnorm)),
            'mix_error': error(lufs_of(tracks, smooth_gains)),
            'random_error': mean(error(lufs_of(tracks, g)) for g in random_gains)}


def test_process_song_tracks_and_songlist(env, tmp_path):
    from scipy.io import wavfile
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d, a, b = env
    reference = {k: (v * g).astype(np.float32) for (k, v), g in zip(a.items(), (0.7, 1.2, 1.5, 0.9))}
    ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
    stats = ev.process_song_tracks(a, reference, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH)
    np.random.seed(7)
    drawn = [{k: float(np.random.uniform(0.5, 1.5)) for k in KEYS} for _ in range(2)]      # the reference's draw order
    assert stats['song_name'] == 'song a' and list(stats['smooth_gains']) == list(KEYS)
    want = host_stats(a, reference, stats['smooth_gains'], drawn)
    for key, value in want.items():
        print('%s: %.9f (host %.9f, diff %.3g, bound 1e-7)' % (key, stats[key], value, abs(stats[key] - value)))
    for key, value in want.items():
        assert abs(stats[key] - value) < 1e-7, key
    assert len({round(v, 6) for v in want.values()}) == 4               # four different figures: nothing matched trivially
    # process_songlist: two songs from disk (MUSDB18-HQ layout), rows plus the per-key means
    for name, tracks, refs in (('song a', a, reference), ('song b', b, {k: (0.8 * v).astype(np.float32) for k, v in a.items()})):
        for sub, src in (('test', tracks), ('manual_gain_mixes', refs)):
            os.makedirs(tmp_path / sub / name)
            for k in KEYS:
                wavfile.write(str(tmp_path / sub / name / (k + '.wav')), SR, np.ascontiguousarray(src[k].T))
    rows, means = ev.process_songlist(str(tmp_path), ['song a', 'song b'], n_random_samples=2, chunk_length=CHUNK_LENGTH)
    assert [r['song_name'] for r in rows] == ['song a', 'song b']
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'}
    for key in means:
        assert means[key] == mean(r[key] for r in rows)
    for key in ('sum_error', 'loudnorm_error', 'mix_error'):            # (the random draws have moved on)
        assert abs(rows[0][key] - want[key]) < 1e-7, key
    assert abs(rows[1]['sum_error'] - rows[0]['sum_error']) > 1e-3
