"""GPU: the true-peak ceiling of rendered masters -- SongMixer / mix_song_to_master / mix_song_to_wav with
``ceiling_dbtp`` and ``normalize='true_peak'``, and the evaluator's WAV export under a ceiling -- on the song geometry of
tests/test_evaluation_gpu.py (8 kHz, 13 chunks of 2 s, 4 stereo stems; its model recipe too: tests/_inputs.py holds no
model or song fixture, its make_audio supplies the impulse the click stems are built from).

Bounds: "at the ceiling" is asserted with tests/_truepeak_ref.py on the returned float64 master to 1e-12 relative -- the
device peak agrees with the definition to 1e-13 of max|x| (tests/test_truepeak_gpu.py), the gain is one division and the
master one rounding per sample, each ~1e-16.  One gain for all channels: the ratio of two float64 values, 1e-15.
Everything else here is bitwise, the song's WAV against the evaluator's export of the same PCM and gains included (both run
inference_utils.MasterChain).  Largest observed errors: NOT YET RECORDED -- no GPU could be obtained while this file was
written; each test prints its figures before asserting."""
import os
import warnings
import wave

import numpy as np
import pytest
import torch

import _pcm_ref
import _truepeak_ref as tpref
import test_evaluation_gpu as te
from _inputs import make_audio
from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH, N, KEYS, MEAN_LOUDNESS = te.SR, te.CHUNK_LENGTH, te.N, te.KEYS, te.MEAN_LOUDNESS


def tone_song():
    """A steady mix: one sine per stem and channel.  At -20 LUFS its peaks stay far under full scale."""
    t = np.arange(N) / SR
    return {k: np.stack([0.1 * np.sin(2 * np.pi * (110.0 * (i + 1) + 7 * c) * t + i) for c in range(2)]).astype(np.float32)
            for i, k in enumerate(KEYS)}


def click_song():
    """A sparse mix: every stem is a train of 4-sample fs/4 bursts (the impulse of _inputs.make_audio convolved with the
    burst, repeated every 0.75 s at a stem-specific offset) over a very quiet bed.  Its loudness is low, so the gain to
    -20 LUFS drives the bursts above full scale (on the host, with the oracle meter and unit gains: +1.3 dBFS sample peak,
    +3.9 dBTP); fs/4 at 45 degrees puts the waveform's peak between the samples."""
    rng = np.random.default_rng(11)
    burst = np.sin(2 * np.pi * np.arange(4) / 4 + np.pi / 4)
    period = make_audio('impulse', 6000, 0)                             # one unit impulse at 2000
    out = {}
    for i, k in enumerate(KEYS):
        train = np.roll(np.tile(period, N // 6000 + 1)[:N], 700 * i)
        x = 0.2 * np.convolve(train, burst)[:N]
        out[k] = np.stack([x, 0.8 * np.roll(x, 3)]).astype(np.float32) + (1e-4 * rng.standard_normal((2, N))).astype(np.float32)
    return out


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
    yield model, d, a, tone_song(), click_song()
    inference_utils._mixers.clear()


def master(env, tracks, **kw):
    from deep_audio_mixer_amd import inference_utils
    model, d = env[0], env[1]
    out = inference_utils.mix_song_to_master(d, model, tracks, chunk_length=CHUNK_LENGTH, sr=SR, **kw)
    return out, next(iter(inference_utils._mixers.values()))


def true_peak_of(master_array):
    return tpref.true_peak(master_array.T).max()


def read_codes(path):
    with wave.open(str(path), 'rb') as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (SR, 2, 2, N)
        return _pcm_ref.from_bytes(w.readframes(N), 'PCM_16', 2)


@pytest.mark.parametrize('normalize', [True, False, 'loudness'])
def test_no_ceiling_is_bit_identical(env, normalize):
    a = env[2]
    (plain, raw, smooth), _ = master(env, a, normalize=normalize)
    (same, raw2, smooth2), mixer = master(env, a, normalize=normalize, ceiling_dbtp=None)
    assert mixer.ceiling is None and mixer.graph is not None
    assert np.array_equal(plain, same) and raw == raw2
    assert {k: list(v) for k, v in smooth.items()} == {k: list(v) for k, v in smooth2.items()}
    with pytest.raises(ValueError):
        mixer.peaks()


def test_ceiling_needs_a_gain_it_can_clamp(env):
    from deep_audio_mixer_amd.inference_utils import SongMixer
    model = env[0]
    for normalize in (True, False):
        with pytest.raises(ValueError):
            SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', normalize, sr=SR, ceiling_dbtp=-1.0)
    with pytest.raises(ValueError):
        SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'stems', 'loudness', sr=SR, ceiling_dbtp=-1.0)


@pytest.mark.parametrize('ceiling', [-1.0, -6.0])
def test_normalize_true_peak(env, ceiling):
    a = env[2]
    (plain, _, _), _ = master(env, a, normalize=False)
    (out, _, smooth), mixer = master(env, a, normalize='true_peak', ceiling_dbtp=ceiling)
    assert mixer.graph is not None and out.dtype == np.float64 and out.shape == (2, N)
    want = 10.0 ** (ceiling / 20.0)
    got = true_peak_of(out)
    ratio = out[plain != 0] / plain[plain != 0]
    spread = ratio.max() / ratio.min() - 1.0
    print('ceiling %g dBTP: true peak %.15f (want %.15f, rel err %.3g, bound 1e-12); gain %.6f, ratio spread %.3g (bound 1e-15)'
          % (ceiling, got, want, abs(got / want - 1.0), ratio.mean(), spread))
    assert abs(got / want - 1.0) <= 1e-12
    assert spread <= 1e-15
    peaks = mixer.peaks()
    assert peaks['limited'] and abs(max(peaks['true_peak_db']) - ceiling) < 1e-9
    assert all(s <= t for s, t in zip(peaks['sample_peak_db'], peaks['true_peak_db']))
    if ceiling == -1.0:                                                  # the default ceiling of normalize='true_peak'
        (dflt, _, _), _ = master(env, a, normalize='true_peak')
        assert np.array_equal(dflt, out)


def test_loudness_with_ceiling_under_and_over(env):
    tone, click = env[3], env[4]
    # under the ceiling: nothing changes, bit for bit
    (free, _, _), _ = master(env, tone, normalize='loudness')
    (held, _, _), mixer = master(env, tone, normalize='loudness', ceiling_dbtp=-1.0)
    peaks = mixer.peaks()
    print('tone mix at -20 LUFS: true peak %.3f dBTP, limited %s' % (max(peaks['true_peak_db']), peaks['limited']))
    assert mixer.graph is not None and np.array_equal(free, held) and peaks['limited'] is False
    assert max(peaks['true_peak_db']) < -1.0
    assert abs(max(peaks['true_peak_db']) - tpref.to_db(true_peak_of(held))) < 1e-9
    # over it: the host composition (oracle meter, the gains the call returned) shows by how much
    (held, _, smooth), mixer = master(env, click, normalize='loudness', ceiling_dbtp=-1.0)
    mixed = np.sum(np.array([click[k].astype(np.float64) * inference_ref.interpolate_mask(smooth[k], N) for k in KEYS]), axis=0)
    unclamped = ref.normalize_loudness(mixed.T, ref.integrated_loudness(mixed.T, SR), -20.0).T
    over = tpref.to_db(true_peak_of(unclamped)) + 1.0
    print('click mix at -20 LUFS: %.2f dB over the ceiling, sample peak %.2f dBFS' % (over, tpref.to_db(np.abs(unclamped).max())))
    assert over >= 1.0
    want = 10.0 ** (-1.0 / 20.0)
    got = true_peak_of(held)
    peaks = mixer.peaks()
    print('held master: true peak %.15f (want %.15f, rel err %.3g, bound 1e-12), %.3f LUFS, limited %s'
          % (got, want, abs(got / want - 1.0), ref.integrated_loudness(held.T, SR), peaks['limited']))
    assert abs(got / want - 1.0) <= 1e-12
    assert peaks['limited'] is True and abs(max(peaks['true_peak_db']) + 1.0) < 1e-9
    assert abs(ref.integrated_loudness(held.T, SR) - (-20.0 - over)) < 1e-6      # quieter than the target by what the peaks cost
    # a second song through the same graph: a replay, and the measurement follows the contents
    (again, _, _), mixer2 = master(env, tone, normalize='loudness', ceiling_dbtp=-1.0)
    assert mixer2 is mixer and mixer.peaks()['limited'] is False and np.array_equal(again, free)


def test_wav_under_the_ceiling_does_not_clip(env, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    model, d, click = env[0], env[1], env[4]
    (held, raw_m, _), _ = master(env, click, normalize='loudness', ceiling_dbtp=-1.0)
    path = tmp_path / 'held.wav'
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)                   # the clip warning of write_wav_bytes
        clipped, raw, _ = inference_utils.mix_song_to_wav(d, model, click, str(path), chunk_length=CHUNK_LENGTH, sr=SR,
                                                          normalize='loudness', ceiling_dbtp=-1.0)
    mixer = next(iter(inference_utils._mixers.values()))
    assert mixer.graph is not None and mixer.encode == 'PCM_16' and mixer.peaks()['limited'] is True
    want, want_clip = _pcm_ref.quantize(held, 'PCM_16')
    got = read_codes(path)
    print('ceiling -1 dBTP: clipped %d, %d samples differ from the quantised master, largest code %d'
          % (clipped, int((got != want).sum()), np.abs(got).max()))
    assert clipped == 0 and want_clip.sum() == 0 and raw == raw_m
    assert np.array_equal(got, want)
    with pytest.warns(RuntimeWarning, match='clipped'):
        unheld, _, _ = inference_utils.mix_song_to_wav(d, model, click, str(tmp_path / 'free.wav'), chunk_length=CHUNK_LENGTH,
                                                       sr=SR, normalize='loudness')
    print('no ceiling: clipped %d' % unheld)
    assert unheld > 0


def test_evaluator_export_under_the_ceiling(env, tmp_path):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d, click = env[0], env[1], env[4]
    reference = {k: (v * g).astype(np.float32) for (k, v), g in zip(click.items(), (0.7, 1.2, 1.5, 0.9))}
    stats = {}
    for ceiling in (None, -1.0):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        results = tmp_path / ('ceiling_%s' % ceiling)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            stats[ceiling] = ev.process_song_tracks(click, reference, 'clicks', n_random_samples=2, chunk_length=CHUNK_LENGTH,
                                                    write_wavs_to_disk=True, results_dir=str(results), ceiling_dbtp=ceiling)
        stats[ceiling]['next_draw'] = np.random.uniform()
        clip_warnings = [w for w in caught if issubclass(w.category, RuntimeWarning) and 'clipped' in str(w.message)]
        files = sorted(os.listdir(results))
        assert files == sorted('clicks_%s.wav' % n for n in ('reference', 'sum', 'loudnorm', 'mix', 'random_0', 'random_1'))
        largest = {f: int(np.abs(read_codes(results / f)).max()) for f in files}
        print('ceiling %s: %d files warned about clipping; largest code per file %s' % (ceiling, len(clip_warnings), largest))
        if ceiling is None:
            assert len(clip_warnings) >= 1                               # at -20 LUFS this song clips
        else:
            assert not clip_warnings                                      # clip count 0 for every file
            # the sample peak is under the true peak: no code beyond the ceiling (+ half an LSB of rounding)
            assert max(largest.values()) <= int(np.ceil(10.0 ** (-1.0 / 20.0) * 32768.0))
    assert stats[None] == stats[-1.0]


@pytest.mark.parametrize('ceiling', [None, -1.0])
def test_song_wav_and_evaluator_export_are_one_chain(env, tmp_path, ceiling):
    """mix_song_to_wav (the chain inside the song's graph) and LoudnessEvaluator.write_sum_to_target (the chain run
    eagerly) on the same resident PCM and the same smoothed gains: the same deterministic launches, so the same file."""
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d, click = env[0], env[1], env[4]
    song, export = tmp_path / 'song.wav', tmp_path / 'export.wav'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                  # without the ceiling this song clips
        clipped = inference_utils.mix_song_to_wav(d, model, click, str(song), chunk_length=CHUNK_LENGTH, sr=SR,
                                                  normalize='loudness', subtype='PCM_16', ceiling_dbtp=ceiling)[0]
        m = next(iter(inference_utils._mixers.values()))
        exported = LoudnessEvaluator(SR, KEYS).write_sum_to_target(m.pcm, m.gains[1], str(export), target_lufs=-20.0,
                                                                   subtype='PCM_16', ceiling_dbtp=ceiling)
    a, b = song.read_bytes(), export.read_bytes()
    print('ceiling %s: clipped %d (song) / %d (export); %d of %d file bytes differ'
          % (ceiling, clipped, exported, sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b)), len(a)))
    assert m.graph is not None and a == b and clipped == exported


# What SongMixer(kind='master') did with (normalize, ceiling_dbtp) before MasterChain existed: the ceiling it ended up
# with, or ValueError.  An encode outside ops.PCM_FORMATS ('PCM_8') raised whatever the other two were.
MASTER_RULES = {(True, None): None, (True, -1.0): ValueError, (False, None): None, (False, -1.0): ValueError,
                ('loudness', None): None, ('loudness', -1.0): -1.0, ('true_peak', None): -1.0, ('true_peak', -1.0): -1.0}


@pytest.mark.parametrize('encode', [None, 'PCM_16', 'PCM_8'])
@pytest.mark.parametrize('normalize,ceiling', sorted(MASTER_RULES, key=str))
def test_master_rules_live_in_one_place(env, normalize, ceiling, encode):
    from deep_audio_mixer_amd.inference_utils import MasterChain, SongMixer
    model = env[0]
    want = ValueError if encode == 'PCM_8' else MASTER_RULES[normalize, ceiling]

    def chain():
        return MasterChain(2, 64, torch.device('cuda'), normalize=normalize, out_dtype=torch.float64, sr=SR, target_lufs=-20.0,
                           ceiling_dbtp=ceiling, encode=encode, dither_seed=None)

    def mixer():
        return SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', normalize, sr=SR, encode=encode,
                         ceiling_dbtp=ceiling)

    if want is ValueError:
        for build in (chain, mixer):
            with pytest.raises(ValueError):
                build()
    else:
        assert chain().ceiling == want and mixer().ceiling == want
