"""GPU: the song's master as a WAV file -- the PCM encoder as the last node of SongMixer's graph (mix_song_to_wav), the
evaluator's WAV export (LoudnessEvaluator.process_song_tracks(write_wavs_to_disk=True)) and the listening-test excerpts
(data/listening_test_data_preparation), on the song of tests/test_evaluation_gpu.py.

The encoder quantises the very float64 values mix_song_to_master returns (peak path: the same buffer; loudness path: the
same single float64 rounding of mix * gain, then an exact power-of-two scale), so those comparisons are exact.  Files the
evaluator renders are compared with a HOST composition (oracle mixdown x oracle gain), which agrees with the device to
rtol 1e-9 (tests/test_evaluation_gpu.py::test_master_at_target_loudness): a value that close to a rounding boundary may
land on the neighbouring code, hence +-1 LSB there.  "At -20 LUFS" is asserted within 1e-3 LU: 16-bit rounding noise is
1/12 LSB^2 ~ 8e-11 against a signal power near 1e-2, below 1e-7 dB -- four orders of margin, and still far below what
a wrong gain or a swapped variant would give."""
import os
import wave

import numpy as np
import pytest
import torch

import _pcm_ref
import test_evaluation_gpu as te
from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH, N, KEYS, MEAN_LOUDNESS = te.SR, te.CHUNK_LENGTH, te.N, te.KEYS, te.MEAN_LOUDNESS


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(3)
    model = ResNet18(n_stems=4, input_shape=(1025, 16)).cuda().eval()
    a = te.song(0)
    d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :SR * 2].T for k, v in a.items()}, 'mix': a['bass'][:, :SR * 2].T}},
                                           chunk_length=CHUNK_LENGTH, sr=SR, tracklist=list(KEYS) + ['mix'])
    yield model, d, a, te.song(1)
    inference_utils._mixers.clear()


def read_codes(path, channels=2, frames=N, width=2):
    with wave.open(str(path), 'rb') as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (SR, channels, width, frames)
        return _pcm_ref.from_bytes(w.readframes(frames), {2: 'PCM_16', 3: 'PCM_24', 4: 'PCM_32'}[width], channels)


def file_lufs(path):
    from deep_audio_mixer_amd.data import dataset_utils as du
    data, rate = du.read_wav(str(path), dtype=np.float64)
    assert rate == SR
    return ref.integrated_loudness(data, SR), data


@pytest.mark.parametrize('normalize', [True, False, 'loudness'])
def test_mix_song_to_wav_equals_quantised_master(env, normalize, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    model, d, a, _ = env
    master, raw_m, smooth_m = inference_utils.mix_song_to_master(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR,
                                                                 normalize=normalize, dtype=np.float64)
    subtype, width = ('PCM_24', 3) if normalize is True else ('PCM_16', 2)
    path = tmp_path / 'master.wav'
    clipped, raw, smooth = inference_utils.mix_song_to_wav(d, model, a, str(path), chunk_length=CHUNK_LENGTH, sr=SR,
                                                           normalize=normalize, subtype=subtype)
    mixer = next(iter(inference_utils._mixers.values()))
    assert mixer.encode == subtype and mixer.graph is not None
    assert raw == raw_m and {k: list(v) for k, v in smooth.items()} == {k: list(v) for k, v in smooth_m.items()}
    want, want_clip = _pcm_ref.quantize(master, subtype)
    got = read_codes(path, width=width)
    print('normalize=%r: %d differing samples, clipped %d (restatement %d), peak %.4f'
          % (normalize, int((got != want).sum()), clipped, int(want_clip.sum()), np.abs(master).max()))
    assert np.array_equal(got, want)
    assert clipped == int(want_clip.sum())
    if normalize is True:
        # librosa.util.normalize puts each channel's peak at exactly +-1.0, and +1.0 is one code above full scale: a channel
        # whose peak is positive clips that one sample
        assert clipped == int((master.max(axis=1) == 1.0).sum()) <= 2
    if normalize == 'loudness':
        assert clipped == 0
        # the -20 LUFS master of this song stays inside [-1, 1): nothing to clip, confirmed on the host
        assert abs(ref.integrated_loudness(master.T, SR) + 20.0) < 1e-6 and np.abs(master).max() < 1.0
        lufs, _ = file_lufs(path)
        assert abs(lufs + 20.0) < 1e-3


def test_dither_seed_reaches_the_graph(env, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    model, d, a, _ = env
    master, _, _ = inference_utils.mix_song_to_master(d, model, a, chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness')
    path = tmp_path / 'dithered.wav'
    inference_utils.mix_song_to_wav(d, model, a, str(path), chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness',
                                    dither_seed=77)
    want, _ = _pcm_ref.quantize(master, 'PCM_16', dither_seed=77)
    assert np.array_equal(read_codes(path), want)


def test_graph_replay_and_encode_none(env, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.inference_utils import SongMixer
    model, d, a, b = env
    pa, pb = tmp_path / 'a.wav', tmp_path / 'b.wav'
    inference_utils.mix_song_to_wav(d, model, a, str(pa), chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness')
    mixer = next(iter(inference_utils._mixers.values()))
    graph = mixer.graph
    assert graph is not None and not hasattr(mixer, 'out')          # no float master is kept beside the encoded one
    inference_utils.mix_song_to_wav(d, model, b, str(pb), chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness')
    assert len(inference_utils._mixers) == 1 and next(iter(inference_utils._mixers.values())).graph is graph      # a replay
    master_b, _, _ = inference_utils.mix_song_to_master(d, model, b, chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness')
    assert np.array_equal(read_codes(pb), _pcm_ref.quantize(master_b, 'PCM_16')[0])
    assert not np.array_equal(read_codes(pa), read_codes(pb))
    inference_utils._mixers.clear()
    # encode=None: the mixer of before, bit for bit
    arrays = [a[k] for k in KEYS]
    outs = []
    for kwargs in ({}, {'encode': None}):
        m = SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', 'loudness', sr=SR, **kwargs)
        out, gains = m.run(arrays)
        assert m.graph is not None and out.dtype == np.float64 and out.shape == (2, N)
        outs.append((out, gains))
        del m
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError):
        SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'stems', False, sr=SR, encode='PCM_16')
    with pytest.raises(ValueError):
        SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', True, sr=SR, encode='PCM_8')


def _at_target(mixed):
    return ref.normalize_loudness(mixed.T, ref.integrated_loudness(mixed.T, SR), -20.0).T


def test_process_song_tracks_writes_wavs(env, tmp_path):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d, a, _ = env
    reference = {k: (v * g).astype(np.float32) for (k, v), g in zip(a.items(), (0.7, 1.2, 1.5, 0.9))}
    results = tmp_path / 'experiment'
    stats = {}
    for on in (False, True):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        stats[on] = ev.process_song_tracks(a, reference, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH,
                                           write_wavs_to_disk=on, results_dir=str(results))
        if not on:
            assert not results.exists()
        follow = np.random.uniform()                                     # the generator is where the switch-off run left it
        stats[on]['next_draw'] = follow
    assert stats[True] == stats[False]
    names = ['reference', 'sum', 'loudnorm', 'mix', 'random_0', 'random_1']
    assert sorted(os.listdir(results)) == sorted('song a_%s.wav' % n for n in names)
    # the host composition of every variant
    np.random.seed(7)
    drawn = [{k: float(np.random.uniform(0.5, 1.5)) for k in KEYS} for _ in range(2)]
    plain = te.lufs_of(a)
    smooth = stats[True]['smooth_gains']
    gains = {'reference': None, 'sum': {k: 1.0 for k in KEYS},
             'loudnorm': {k: 10.0 ** ((MEAN_LOUDNESS[k] - plain[i]) / 20.0) for i, k in enumerate(KEYS)},
             'mix': {k: inference_ref.interpolate_mask(np.asarray(smooth[k], dtype=np.float64), N) for k in KEYS},
             'random_0': drawn[0], 'random_1': drawn[1]}
    seen = []
    for name in names:
        path = results / ('song a_%s.wav' % name)
        if gains[name] is None:
            mixed = np.sum(np.array([reference[k].astype(np.float64) for k in KEYS]), axis=0)
        else:
            mixed = np.sum(np.array([a[k].astype(np.float64) * gains[name][k] for k in KEYS]), axis=0)
        want, want_clip = _pcm_ref.quantize(_at_target(mixed), 'PCM_16')
        got = read_codes(path)
        lufs, _ = file_lufs(path)
        diff = np.abs(got - want)
        print('%s: %.6f LUFS (bound 1e-3 around -20), %d samples off by one LSB, max diff %d'
              % (name, lufs, int((diff == 1).sum()), diff.max()))
        assert abs(lufs + 20.0) < 1e-3, name
        assert diff.max() <= 1, name
        assert (diff != 0).mean() < 1e-3, name                          # rounding-boundary cases only, not a shifted signal
        assert want_clip.sum() == 0
        seen.append(got)
    for i in range(len(seen)):                                           # six different files: no variant written twice
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j])


def test_listening_test_excerpts(env, tmp_path):
    from scipy.io import wavfile
    from deep_audio_mixer_amd.data import listening_test_data_preparation as prep
    from deep_audio_mixer_amd.models.baselines.mean_loudness_model import MeanLoudnessModel
    from deep_audio_mixer_amd.models.baselines.random_model import RandomModel
    model, d, a, b = env
    base, save = tmp_path / 'musdb', tmp_path / 'test_data'
    for name, tracks in (('song a', a), ('song b', b)):
        for sub, scale in (('test', 1.0), ('manual_gain_mixes', 0.8)):
            os.makedirs(base / sub / name)
            for k in KEYS:
                wavfile.write(str(base / sub / name / (k + '.wav')), SR, np.ascontiguousarray((scale * tracks[k]).T.astype(np.float32)))
    np.random.seed(5)
    models = {'random': RandomModel(), 'loudnorm': MeanLoudnessModel(MEAN_LOUDNESS, SR)}
    prep.process_songlist(str(base), ['song a', 'song b'], [(2, 12), (2, 12)], models, d, save_dir=str(save), sr=SR)
    want_files = sorted('%s_%s.wav' % (s, i) for s in ('song a', 'song b') for i in ('reference', 'sum', 'random', 'loudnorm'))
    assert sorted(os.listdir(save)) == want_files
    for f in want_files:
        lufs, data = file_lufs(save / f)
        print('%s: %d frames, %.6f LUFS' % (f, data.shape[0], lufs))
        assert data.shape == (10 * SR, 2), f
        assert abs(lufs + 20.0) < 1e-3, f
    # the excerpt is the interval: the raw sum of seconds 2..12, at -20 LUFS
    mixed = np.sum(np.array([a[k][:, 2 * SR:12 * SR].astype(np.float64) for k in KEYS]), axis=0)
    want, _ = _pcm_ref.quantize(_at_target(mixed), 'PCM_16')
    assert np.abs(read_codes(save / 'song a_sum.wav', frames=10 * SR) - want).max() <= 1
    # a mixing network goes through mix_song_smooth under the name 'mix' (the whole song: 13 chunks of 2 s)
    whole = tmp_path / 'whole'
    os.makedirs(whole)
    prep.process_song(str(base), 'song a', (0, 27), {'mix': model}, d, str(whole), sr=SR)          # (the song ends at 26.01 s)
    assert sorted(os.listdir(whole)) == ['song a_mix.wav', 'song a_reference.wav', 'song a_sum.wav']
    lufs, data = file_lufs(whole / 'song a_mix.wav')
    assert data.shape == (N, 2) and abs(lufs + 20.0) < 1e-3
    assert not np.array_equal(read_codes(whole / 'song a_mix.wav'), read_codes(whole / 'song a_sum.wav'))
