"""GPU: the compressor as a stage of the master chain -- SongMixer / mix_song_to_master / mix_song_to_wav and the evaluator's
WAV export with ``compressor=`` -- on the song geometry and with the helpers of tests/test_master_truepeak_gpu.py (8 kHz,
26 s, 4 stereo stems) and the bed-plus-bursts song of tests/_limiter_inputs.py.

Bounds.  The device master against the host composition (the returned smoothed gains, the oracle meter, tests/_compressor_ref.py,
the oracle meter again): tests/test_compressor_gpu.py's bound on ``out``, max|xs| (ln10/20 TOL_Q + 4 * 2^-53), times the
second gain, plus one float64 ulp; xs is the stem sum at the first target gain.  Both gains are functions of the device
meter's reading, which has a bound of its own (1e-8 LU, tests/test_loudness_gpu.py: 1.2e-9 relative as a gain, asserted
here), so the composition takes the gains the chain used.  Loudness of the master: 1e-6 LU, as the other test_master_*
files.  "At or under the ceiling": 1e-12 relative, as tests/test_master_limiter_gpu.py.  Everything else is bitwise.
Largest observed (1 x MI355X): master against the composition 5.3e-16 (bound 3.7e-13), both gains 2.2e-16 relative (1.2e-9),
loudness of the master -20.000000000 LUFS, max reduction equal to the reference's to all printed digits (bound 8.9e-12 dB),
true peak behind compressor and limiter 1.4e-5 under the ceiling; 0 codes / bytes / samples differ in the bitwise tests.  Each
test prints its figures before asserting."""
import warnings

import numpy as np
import pytest
import torch

import _compressor_ref as cref
import _limiter_inputs as li
import _pcm_ref
import test_master_truepeak_gpu as tm
from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH, N, KEYS = tm.SR, tm.CHUNK_LENGTH, tm.N, tm.KEYS
CEILING = 10.0 ** (-1.0 / 20.0)
NEW_BUFFERS = ('comp_gain', 'compressed', 'comp_max', 'comp_over', 'compressed_lufs', 'comp_ws', 'comp_args')

env = tm.env                               # (model, dataset, noise song, tone song, click song)
master = tm.master


@pytest.fixture(scope='module')
def bursts():
    return li.burst_song(3.0)


def mixer_of():
    from deep_audio_mixer_amd import inference_utils
    return next(iter(inference_utils._mixers.values()))


def curve_args(shape=None):
    """MasterChain.COMPRESSOR_DEFAULTS (or ``shape``) as the seven arguments of ref.compress behind x."""
    from deep_audio_mixer_amd import ops
    from deep_audio_mixer_amd.inference_utils import MasterChain
    p = dict(MasterChain.COMPRESSOR_DEFAULTS, **(shape or {}))
    return (p['threshold_db'], p['ratio'], p['knee_db']) + ops.compressor_constants(
        p['threshold_db'], p['knee_db'], p['attack_ms'], p['release_ms'], SR), p


def host_mix(song, smooth):
    return np.sum(np.array([song[k].astype(np.float64) * inference_ref.interpolate_mask(smooth[k], N) for k in KEYS]), axis=0)


@pytest.mark.parametrize('shape', [None, {'threshold_db': -18.0, 'ratio': 4.0, 'knee_db': 0.0, 'attack_ms': 2.0, 'release_ms': 250.0}])
def test_master_against_the_composition_of_the_references(env, shape):
    a = env[2]
    (out, _, smooth), mixer = master(env, a, normalize='loudness', compressor=True if shape is None else shape)
    chain = mixer.chain
    info = mixer.compression()
    assert mixer.graph is not None and out.dtype == np.float64 and out.shape == (2, N) and chain.ceiling is None
    args, p = curve_args(shape)
    mixed = host_mix(a, smooth)
    g1, g2 = float(chain.comp_gain.cpu()[0]), float(chain.master_gain.cpu()[0])
    g1_oracle = 10.0 ** ((-20.0 - ref.integrated_loudness(mixed.T, SR)) / 20.0)
    want = cref.compress(mixed.T, *args, pre_gain=g1)
    g2_oracle = 10.0 ** ((-20.0 - ref.integrated_loudness(want['out'], SR)) / 20.0)
    print('first gain %.9f (oracle %.9f, rel %.3g), make-up gain %.9f (oracle %.9f, rel %.3g); bound 1.2e-9'
          % (g1, g1_oracle, abs(g1 / g1_oracle - 1.0), g2, g2_oracle, abs(g2 / g2_oracle - 1.0)))
    assert abs(g1 / g1_oracle - 1.0) <= 1.2e-9 and abs(g2 / g2_oracle - 1.0) <= 1.2e-9
    tol = cref.tol_q(p['attack_ms'] * 1e-3 * SR, p['release_ms'] * 1e-3 * SR, want['c'].max())
    composition = (want['out'] * g2).T
    bound = np.abs(want['xs']).max() * (cref.LN10_20 * tol + 4 * 2.0 ** -53) * g2
    err = (np.abs(out - composition) - np.spacing(np.abs(composition))).max()
    lufs = ref.integrated_loudness(out.T, SR)
    print('master against the composition: max err %.3g (bound %.3g); loudness %.9f LUFS (target -20, bound 1e-6)'
          % (err, bound, lufs))
    assert err <= bound
    assert abs(lufs + 20.0) <= 1e-6
    print('compression(): %s; reference max reduction %.9f dB (bound %.3g), over share %.6f, make-up %.9f dB'
          % (info, want['max_reduction'], tol, want['n_over'] / N, 20.0 * np.log10(g2_oracle)))
    assert want['max_reduction'] > 0.1 and 0.0 < want['n_over'] < N
    assert abs(info['max_reduction_db'] - want['max_reduction']) <= tol
    assert info['over_share'] == want['n_over'] / N
    assert abs(info['makeup_db'] - 20.0 * np.log10(g2_oracle)) <= 20.0 * np.log10(1.0 + 1.2e-9) + 1e-15
    assert info['makeup_db'] > 0.0 and abs(info['loudness_lufs'] + 20.0) <= 1e-6
    with pytest.raises(ValueError):
        mixer.peaks()                                   # no ceiling was asked for


def test_compressor_in_front_of_the_limiter(env, bursts):
    (out, _, smooth), mixer = master(env, bursts, normalize='loudness', compressor=True, limiter=True, ceiling_dbtp=-1.0)
    peaks, info = mixer.peaks(), mixer.compression()
    got = tm.true_peak_of(out)
    (plain, _, _), _ = master(env, bursts, normalize='loudness', limiter=True, ceiling_dbtp=-1.0)
    print('true peak %.15f (ceiling %.15f, rel %.3g, bound 1e-12); peaks %s; compression %s; %d samples differ from the master '
          'without a compressor' % (got, CEILING, got / CEILING - 1.0, peaks, info, int((out != plain).sum())))
    assert mixer.graph is not None and out.shape == (2, N)
    assert got <= CEILING * (1.0 + 1e-12)
    assert info['max_reduction_db'] > 1.0 and info['over_share'] > 0.0 and peaks['limited'] is True
    assert not np.array_equal(out, plain)
    # the limiter read the compressed signal at the make-up gain: its input's loudness is the target
    assert abs(info['loudness_lufs'] + 20.0) <= 1e-6


def test_wav_with_the_compressor(env, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    model, d, a = env[0], env[1], env[2]
    (compressed, raw_m, _), _ = master(env, a, normalize='loudness', compressor=True)
    path = tmp_path / 'compressed.wav'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        clipped, raw, _ = inference_utils.mix_song_to_wav(d, model, a, str(path), chunk_length=CHUNK_LENGTH, sr=SR,
                                                          normalize='loudness', compressor=True)
    mixer = mixer_of()
    want, want_clip = _pcm_ref.quantize(compressed, 'PCM_16')
    got = tm.read_codes(path)
    print('compressor: clipped %d (reference %d), %d codes differ from the quantised master (bound 0), largest code %d'
          % (clipped, int(want_clip.sum()), int((got != want).sum()), np.abs(got).max()))
    assert mixer.graph is not None and mixer.encode == 'PCM_16' and mixer.compression()['max_reduction_db'] > 0.1
    assert clipped == int(want_clip.sum()) and raw == raw_m
    assert np.array_equal(got, want)


def test_captured_mixer_equals_the_eager_chain(env):
    from deep_audio_mixer_amd.inference_utils import MasterChain
    a = env[2]
    shape = {'threshold_db': -15.0, 'release_ms': 60.0}
    (out, _, _), mixer = master(env, a, normalize='loudness', compressor=shape, ceiling_dbtp=-1.0)
    assert mixer.graph is not None
    chain = MasterChain(2, N, torch.device('cuda'), 'loudness', sr=SR, ceiling_dbtp=-1.0, compressor=shape)
    chain.render(mixer.pcm, mixer.gains[1])
    torch.cuda.synchronize()
    differ = int((chain.out != mixer.chain.out).sum())
    print('captured SongMixer against the eager MasterChain: %d samples differ (bound 0); compression %s' % (differ, chain.compression()))
    assert differ == 0 and np.array_equal(out, chain.out.cpu().numpy())
    for name in ('comp_gain', 'comp_max', 'comp_over', 'compressed_lufs', 'master_gain', 'free_gain', 'compressed'):
        assert torch.equal(getattr(chain, name), getattr(mixer.chain, name)), name
    assert chain.compression() == mixer.compression() and chain.peaks() == mixer.peaks()
    assert chain.compression()['max_reduction_db'] > 0.1


def test_song_wav_and_evaluator_export_are_one_file(env, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d, a = env[0], env[1], env[2]
    song, export = tmp_path / 'song.wav', tmp_path / 'export.wav'
    shape = {'ratio': 3.0}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        clipped = inference_utils.mix_song_to_wav(d, model, a, str(song), chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness',
                                                  subtype='PCM_16', compressor=shape)[0]
        m = mixer_of()
        exported = LoudnessEvaluator(SR, KEYS).write_sum_to_target(m.pcm, m.gains[1], str(export), target_lufs=-20.0,
                                                                   subtype='PCM_16', compressor=shape)
    x, y = song.read_bytes(), export.read_bytes()
    print('clipped %d (song) / %d (export); %d of %d file bytes differ (bound 0)'
          % (clipped, exported, sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y)), len(x)))
    assert m.graph is not None and m.chain.compressor[1] == 3.0 and x == y and clipped == exported


def test_compressor_rules(env):
    from deep_audio_mixer_amd.inference_utils import MasterChain, SongMixer
    model = env[0]
    dev = torch.device('cuda')
    for normalize in (True, False, 'true_peak'):
        with pytest.raises(ValueError):
            MasterChain(2, 64, dev, normalize=normalize, sr=SR, compressor=True)
        with pytest.raises(ValueError):
            SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', normalize, sr=SR, compressor=True)
    for kind in ('stems', 'loudness', 'spectral'):
        with pytest.raises(ValueError):
            SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, kind, 'loudness', sr=SR, compressor=True)
    for bad in ({'threshold': -12.0}, {'ratio': 2.0, 'makeup_db': 3.0}, {'ratio': 0.5}, {'knee_db': -1.0}, {'attack_ms': 0.0},
                'soft', 3):
        with pytest.raises(ValueError):
            MasterChain(2, 64, dev, normalize='loudness', sr=SR, compressor=bad)
    with pytest.raises(ValueError):                                      # beyond the kernel's cap at this rate
        MasterChain(2, 64, dev, normalize='loudness', sr=SR, compressor={'release_ms': 1e5})
    assert MasterChain.compressor_rules(None, True) is None and MasterChain.compressor_rules(False, 'loudness') is None
    assert MasterChain.compressor_rules(True, 'loudness') == (-12.0, 2.0, 6.0, 10.0, 100.0)
    assert MasterChain.compressor_rules({'ratio': float('inf')}, 'loudness') == (-12.0, float('inf'), 6.0, 10.0, 100.0)
    chain = MasterChain(2, 64, dev, normalize='loudness', sr=SR)
    with pytest.raises(ValueError):
        chain.compression()


@pytest.mark.parametrize('normalize,ceiling,limiter', [(True, None, None), ('loudness', None, None), ('loudness', -1.0, True)])
def test_compressor_off_is_a_no_op(env, normalize, ceiling, limiter):
    a = env[2]
    (plain, raw, smooth), mixer = master(env, a, normalize=normalize, ceiling_dbtp=ceiling, limiter=limiter)
    for off in (None, False):
        (same, raw2, smooth2), mixer2 = master(env, a, normalize=normalize, ceiling_dbtp=ceiling, limiter=limiter, compressor=off)
        print('normalize %r ceiling %r limiter %r compressor %r: %d samples differ (bound 0), same mixer %s'
              % (normalize, ceiling, limiter, off, int((plain != same).sum()), mixer2 is mixer))
        assert mixer2 is mixer and mixer.compressor is None and mixer.chain.compressor is None
        assert np.array_equal(plain, same) and raw == raw2
    assert not any(hasattr(mixer.chain, name) for name in NEW_BUFFERS)
    with pytest.raises(ValueError):
        mixer.compression()
    from deep_audio_mixer_amd.inference_utils import MasterChain
    on = MasterChain(2, 64, torch.device('cuda'), normalize='loudness', sr=SR, compressor=True)
    assert all(hasattr(on, name) for name in NEW_BUFFERS)


def test_songlist_passes_the_compressor(env, monkeypatch):
    """process_songlist hands ``compressor`` to process_song by keyword, and only when one is asked for."""
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator(SR, KEYS)
    seen = []

    def fake(base_dir, song_name, *args, **kw):
        seen.append((len(args), kw))
        return {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
    monkeypatch.setattr(ev, 'process_song', fake)
    ev.process_songlist('.', ['a'])
    ev.process_songlist('.', ['a'], compressor=False)
    ev.process_songlist('.', ['a'], compressor={'ratio': 4.0})
    print('process_song saw %s' % seen)
    assert seen == [(6, {}), (6, {}), (6, {'compressor': {'ratio': 4.0}})]
