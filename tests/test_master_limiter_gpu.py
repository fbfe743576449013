"""GPU: the look-ahead limiter as a stage of the master chain -- SongMixer / mix_song_to_master / mix_song_to_wav and the
evaluator's WAV export with ``limiter=`` -- on the song geometry and with the helpers of tests/test_master_truepeak_gpu.py,
and the bed-plus-bursts song of tests/_limiter_inputs.py.

Bounds.  The device master against the host composition (the returned smoothed gains, the oracle meter, tests/_limiter_ref.py,
the reference trim): tests/test_limiter_gpu.py's tolerance, 1e-13 * max(1, max|xs| / ceil) * max|xs| plus one float64 ulp,
xs being the stem sum at the target gain.  That gain is a function of the device meter's reading, which has a bound of its
own (1e-8 LU, tests/test_loudness_gpu.py: 1.2e-9 relative as a gain, asserted here), so the composition takes the gain the
chain used.  "At the ceiling": 1e-12 relative by tests/_truepeak_ref.py, as in test_master_truepeak_gpu.py -- the meter agrees
with the definition to 1e-13 of the peak, so "at or under the ceiling" is asserted to that precision too.  Loudness: 1e-6 LU.
Everything else is bitwise.  Each test prints its figures before asserting.
Largest observed (1 x MI355X): master against the composition 7.8e-16 (bound 1.9e-13), target gain 2.2e-16 relative (1.2e-9),
true peak at the ceiling 0 relative (1e-12), trim -2.3e-5 dB (> -1e-3), loudness 1e-7 LU or less (1e-6), 4.72 LU over the
static clamp (>= 3), unlimited master 5.60 dB over the ceiling (>= 3)."""
import os
import warnings

import numpy as np
import pytest
import torch

import _limiter_inputs as li
import _limiter_ref as lref
import _pcm_ref
import _truepeak_ref as tpref
import test_master_truepeak_gpu as tm
from oracle import inference_ref, loudness_ref as ref

pytestmark = pytest.mark.gpu

SR, CHUNK_LENGTH, N, KEYS = tm.SR, tm.CHUNK_LENGTH, tm.N, tm.KEYS
CEILING = 10.0 ** (-1.0 / 20.0)
BURST_AMPLITUDE = 3.0                      # raised here, not the 3 dB precondition lowered, if the model's gains pull the peaks under

env = tm.env                               # (model, dataset, noise song, tone song, click song)
master = tm.master


@pytest.fixture(scope='module')
def bursts():
    return li.burst_song(BURST_AMPLITUDE)


def mixer_of():
    from deep_audio_mixer_amd import inference_utils
    return next(iter(inference_utils._mixers.values()))


@pytest.mark.parametrize('normalize,ceiling', [(True, None), (False, None), ('loudness', None), ('loudness', -1.0)])
def test_limiter_off_is_a_no_op(env, normalize, ceiling):
    a = env[2]
    (plain, raw, smooth), mixer = master(env, a, normalize=normalize, ceiling_dbtp=ceiling)
    for off in (None, False):
        (same, raw2, smooth2), mixer2 = master(env, a, normalize=normalize, ceiling_dbtp=ceiling, limiter=off)
        print('normalize %r ceiling %r limiter %r: %d samples differ (bound 0), same mixer %s'
              % (normalize, ceiling, off, int((plain != same).sum()), mixer2 is mixer))
        assert mixer2 is mixer and mixer.limiter is None and mixer.chain.limiter is None
        assert np.array_equal(plain, same) and raw == raw2
        assert {k: list(v) for k, v in smooth.items()} == {k: list(v) for k, v in smooth2.items()}
    assert mixer.ceiling == ceiling and not hasattr(mixer.chain, 'limited') and not hasattr(mixer.chain, 'limiter_ws')


def test_limiter_rules(env):
    from deep_audio_mixer_amd.inference_utils import MasterChain, SongMixer
    model = env[0]
    dev = torch.device('cuda')
    for normalize in (True, False, 'true_peak'):
        with pytest.raises(ValueError):
            MasterChain(2, 64, dev, normalize=normalize, sr=SR, limiter=True)
        with pytest.raises(ValueError):
            SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, 'master', normalize, sr=SR, limiter=True)
    for kind in ('stems', 'loudness', 'spectral'):
        with pytest.raises(ValueError):
            SongMixer(model, 4, 2, N, torch.float32, CHUNK_LENGTH * SR, kind, 'loudness', sr=SR, limiter=True)
    for bad in ({'lookahead': 5.0}, {'lookahead_ms': 5.0, 'release_ms': 50.0}, 'fast', 3):
        with pytest.raises(ValueError):
            MasterChain(2, 64, dev, normalize='loudness', sr=SR, limiter=bad)
    with pytest.raises(ValueError):                                      # beyond the kernel's caps at this rate
        MasterChain(2, 64, dev, normalize='loudness', sr=SR, limiter={'hold_ms': 1e4})
    assert MasterChain.rules('loudness', None, None) == ('loudness', None)               # three arguments, a two-tuple
    assert MasterChain.limiter_rules(True, 'loudness', None) == ((5.0, 20.0), -1.0)
    assert MasterChain.limiter_rules({'hold_ms': 10}, 'loudness', -2.0) == ((5.0, 10.0), -2.0)
    chain = MasterChain(2, 64, dev, normalize='loudness', sr=SR, limiter=True)
    assert chain.ceiling == -1.0 and (chain.lookahead, chain.hold) == (lref.samples(5.0, SR), lref.samples(20.0, SR)) == (40, 160)


def test_tone_song_passes_untouched(env):
    tone = env[3]
    for dtype in (np.float64, np.float32):
        (free, _, _), _ = master(env, tone, normalize='loudness', dtype=dtype)
        (limited, _, _), mixer = master(env, tone, normalize='loudness', limiter=True, dtype=dtype)
        peaks = mixer.peaks()
        print('tone song, %s: %d samples differ from the unlimited master (bound 0); peaks %s'
              % (np.dtype(dtype).name, int((free != limited).sum()), peaks))
        assert mixer.graph is not None and limited.dtype == dtype
        if dtype == np.float64:
            assert np.array_equal(free, limited)
        else:
            # dam_gain_ramp_apply forms a float32 master as (float)mix * (float)gain: three float32 roundings, each 2^-24
            # relative; the limited one is the float64 product rounded once.  They differ by 4 * 2^-24 relative at the most.
            rel = float((np.abs(free.astype(np.float64) - limited) / np.abs(limited.astype(np.float64)).clip(1e-30)).max())
            print('float32: largest relative difference %.3g (bound %.3g)' % (rel, 4 * 2.0 ** -24))
            assert rel <= 4 * 2.0 ** -24
        assert peaks['limited'] is False and peaks['max_reduction_db'] == 0.0 and peaks['limited_share'] == 0.0
        assert peaks['trim_db'] == 0.0 and max(peaks['true_peak_db']) < -1.0
        assert abs(peaks['loudness_lufs'] + 20.0) < 1e-6


def test_bed_plus_bursts_song(env, bursts):
    (limited, _, smooth), mixer = master(env, bursts, normalize='loudness', limiter=True)
    peaks = mixer.peaks()
    free_gain = float(mixer.chain.free_gain.cpu()[0])
    assert mixer.graph is not None and limited.dtype == np.float64 and limited.shape == (2, N)
    # the host composition
    mixed = np.sum(np.array([bursts[k].astype(np.float64) * inference_ref.interpolate_mask(smooth[k], N) for k in KEYS]), axis=0)
    oracle_gain = 10.0 ** ((-20.0 - ref.integrated_loudness(mixed.T, SR)) / 20.0)
    unlimited = mixed * oracle_gain
    over = tpref.to_db(tm.true_peak_of(unlimited) / CEILING)
    print('unlimited master at -20 LUFS: %.3f dB over -1 dBTP (precondition >= 3); target gain %.9f on the device, %.9f by the '
          'oracle: rel diff %.3g (bound 1.2e-9)' % (over, free_gain, oracle_gain, abs(free_gain / oracle_gain - 1.0)))
    assert over >= 3.0
    assert abs(free_gain / oracle_gain - 1.0) <= 1.2e-9
    L, H = lref.samples(5.0, SR), lref.samples(20.0, SR)
    want = lref.limit(mixed.T, CEILING, L, H, pre_gain=free_gain)
    trim = min(1.0, CEILING / tpref.true_peak(want['out']).max())
    composition = (want['out'] * trim).T
    peak = np.abs(want['xs']).max()
    bound = 1e-13 * max(1.0, peak / CEILING) * peak
    err = (np.abs(limited - composition) - np.spacing(np.abs(composition))).max()
    print('device master against the host composition: max err %.3g (bound %.3g); min gain %.6f / %.6f, limited share %.5f / %.5f'
          % (err, bound, 10.0 ** (peaks['max_reduction_db'] / 20.0), want['min_gain'], peaks['limited_share'], want['n_limited'] / N))
    assert err <= bound
    assert abs(10.0 ** (peaks['max_reduction_db'] / 20.0) - want['min_gain']) <= 1e-13 * max(1.0, peak / CEILING)
    assert abs(peaks['limited_share'] - want['n_limited'] / N) <= 1e-3 and peaks['limited'] is True
    # the ceiling, exactly; the residual trim is small
    got = tm.true_peak_of(limited)
    print('true peak %.15f (ceiling %.15f, rel %.3g, bound 1e-12); trim %.3g dB (bound > -1e-3), reference trim %.3g dB'
          % (got, CEILING, got / CEILING - 1.0, peaks['trim_db'], 20.0 * np.log10(trim)))
    assert got <= CEILING * (1.0 + 1e-12)
    if peaks['trim_db'] < 0.0:
        assert abs(got / CEILING - 1.0) <= 1e-12 and abs(max(peaks['true_peak_db']) + 1.0) < 1e-9
    assert -1e-3 < peaks['trim_db'] <= 0.0
    # the loudness it reports, and what the limiter buys over the static clamp
    lufs = ref.integrated_loudness(limited.T, SR)
    (clamped, _, _), _ = master(env, bursts, normalize='loudness', ceiling_dbtp=-1.0)
    clamped_lufs = ref.integrated_loudness(clamped.T, SR)
    print('loudness: %.6f LUFS reported, %.6f by the oracle (bound 1e-6); static clamp %.3f LUFS: the limiter is %.3f LU louder '
          '(bound 3)' % (peaks['loudness_lufs'], lufs, clamped_lufs, lufs - clamped_lufs))
    assert abs(peaks['loudness_lufs'] - lufs) <= 1e-6
    assert lufs - clamped_lufs >= 3.0


def test_wav_with_the_limiter(env, bursts, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    model, d = env[0], env[1]
    (limited, raw_m, _), _ = master(env, bursts, normalize='loudness', limiter=True)
    path = tmp_path / 'limited.wav'
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        clipped, raw, _ = inference_utils.mix_song_to_wav(d, model, bursts, str(path), chunk_length=CHUNK_LENGTH, sr=SR,
                                                          normalize='loudness', limiter=True)
    mixer = mixer_of()
    want, want_clip = _pcm_ref.quantize(limited, 'PCM_16')
    got = tm.read_codes(path)
    print('limiter: clipped %d, %d codes differ from the quantised master (bound 0), largest code %d'
          % (clipped, int((got != want).sum()), np.abs(got).max()))
    assert mixer.graph is not None and mixer.encode == 'PCM_16' and mixer.peaks()['limited'] is True
    assert clipped == 0 and want_clip.sum() == 0 and raw == raw_m
    assert np.array_equal(got, want)


def test_song_wav_and_evaluator_export_are_one_file(env, bursts, tmp_path):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d = env[0], env[1]
    song, export = tmp_path / 'song.wav', tmp_path / 'export.wav'
    limiter = {'lookahead_ms': 2.5, 'hold_ms': 10.0}
    clipped = inference_utils.mix_song_to_wav(d, model, bursts, str(song), chunk_length=CHUNK_LENGTH, sr=SR, normalize='loudness',
                                              subtype='PCM_16', limiter=limiter)[0]
    m = mixer_of()
    assert (m.chain.lookahead, m.chain.hold) == (20, 80)
    exported = LoudnessEvaluator(SR, KEYS).write_sum_to_target(m.pcm, m.gains[1], str(export), target_lufs=-20.0,
                                                               subtype='PCM_16', limiter=limiter)
    a, b = song.read_bytes(), export.read_bytes()
    print('clipped %d (song) / %d (export); %d of %d file bytes differ (bound 0)'
          % (clipped, exported, sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b)), len(a)))
    assert m.graph is not None and a == b and clipped == exported == 0


def test_evaluator_stats_do_not_depend_on_the_limiter(env, bursts, tmp_path):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    model, d = env[0], env[1]
    reference = {k: (v * g).astype(np.float32) for (k, v), g in zip(bursts.items(), (0.7, 1.2, 1.5, 0.9))}
    stats = {}
    for limiter in (None, True):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=tm.MEAN_LOUDNESS, mix_model=model, seed=7)
        results = tmp_path / ('limiter_%s' % limiter)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            stats[limiter] = ev.process_song_tracks(bursts, reference, 'bursts', n_random_samples=2, chunk_length=CHUNK_LENGTH,
                                                    write_wavs_to_disk=True, results_dir=str(results), limiter=limiter)
        stats[limiter]['next_draw'] = np.random.uniform()
        clip_warnings = [w for w in caught if issubclass(w.category, RuntimeWarning) and 'clipped' in str(w.message)]
        files = sorted(os.listdir(results))
        assert files == sorted('bursts_%s.wav' % n for n in ('reference', 'sum', 'loudnorm', 'mix', 'random_0', 'random_1'))
        largest = {f: int(np.abs(tm.read_codes(results / f)).max()) for f in files}
        print('limiter %s: %d files warned about clipping; largest code per file %s' % (limiter, len(clip_warnings), largest))
        if limiter:
            assert not clip_warnings
            assert max(largest.values()) <= int(np.ceil(CEILING * 32768.0))
    assert stats[None] == stats[True]


def test_second_song_is_a_replay(env, bursts):
    tone = env[3]
    (free, _, _), _ = master(env, tone, normalize='loudness')
    (first, _, _), mixer = master(env, bursts, normalize='loudness', limiter=True)
    graph = mixer.graph
    assert graph is not None and mixer.peaks()['limited'] is True
    (other, _, _), mixer2 = master(env, tone, normalize='loudness', limiter=True)
    peaks = mixer2.peaks()
    print('second song through the same mixer: same graph %s, peaks %s' % (mixer2.graph is graph, peaks))
    assert mixer2 is mixer and mixer2.graph is graph
    assert peaks['limited'] is False and peaks['max_reduction_db'] == 0.0 and np.array_equal(other, free)
    (third, _, _), mixer3 = master(env, bursts, normalize='loudness', limiter=True)
    assert mixer3 is mixer and mixer3.graph is graph and mixer3.peaks()['limited'] is True and np.array_equal(third, first)


def test_songlist_passes_the_limiter(env, monkeypatch):
    """process_songlist hands ``limiter`` to process_song by keyword, and only when one is asked for: without it the call is
    the call of before, argument for argument."""
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator(SR, KEYS)
    seen = []

    def fake(base_dir, song_name, *args, **kw):
        seen.append((len(args), kw))
        return {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
    monkeypatch.setattr(ev, 'process_song', fake)
    ev.process_songlist('.', ['a'])
    ev.process_songlist('.', ['a'], limiter=False)
    ev.process_songlist('.', ['a'], limiter={'hold_ms': 10.0})
    print('process_song saw %s' % seen)
    assert seen == [(6, {}), (6, {}), (6, {'limiter': {'hold_ms': 10.0}})]
