"""CPU: the host-side pieces of the whole-song loudness evaluation -- the random-gain baseline draws what the reference
draws (models/baselines/random_model.py: one np.random.uniform per stem, in tracklist order), its numpy forward is
``gain * x``, and LoudnessEvaluator keeps its positional ``(sr, keys)`` constructor."""
import inspect

import numpy as np


def test_random_model_draw_order_and_range():
    from deep_audio_mixer_amd.models.baselines.random_model import RandomModel
    m = RandomModel()
    assert m.tracklist == ('bass', 'drums', 'vocals', 'other')
    np.random.seed(11)
    want = [float(np.random.uniform(0.5, 1.5)) for _ in range(8)]
    np.random.seed(11)
    first, second = m.draw(), m.draw()
    assert list(first) == list(m.tracklist)
    assert [first[t] for t in m.tracklist] + [second[t] for t in m.tracklist] == want
    lo_hi = RandomModel(2.0, 3.0)
    for _ in range(50):
        assert all(2.0 <= g < 3.0 for g in lo_hi.draw().values())


def test_random_model_numpy_forward_is_gain_times_x():
    from deep_audio_mixer_amd.models.baselines.random_model import RandomModel
    rng = np.random.default_rng(0)
    x = {t: rng.standard_normal((2, 100)).astype(np.float32) for t in ('bass', 'drums', 'vocals', 'other')}
    np.random.seed(5)
    out = RandomModel().forward(x)
    np.random.seed(5)
    for t in ('bass', 'drums', 'vocals', 'other'):             # the reference's expression, drawn in the same order
        want = float(np.random.uniform(0.5, 1.5)) * x[t]
        assert out[t].dtype == want.dtype and np.array_equal(out[t], want)


def test_evaluator_constructor_surface():
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    params = inspect.signature(LoudnessEvaluator.__init__).parameters
    assert list(params)[:3] == ['self', 'sr', 'keys']
    for name in ('dataset', 'd_mean_loudness', 'mix_model', 'seed'):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None
    for name in ('evaluate_loudness_batch', 'process_song_tracks', 'process_song', 'process_songlist'):
        assert callable(getattr(LoudnessEvaluator, name))


def test_evaluator_constructs_positionally(dam_lib):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    keys = ('bass', 'drums', 'vocals', 'other')
    ev = LoudnessEvaluator(44100, keys)
    assert ev.sr == 44100 and ev.keys == keys and ev.meter.rate == 44100
    assert ev.d is None and ev.mix_model is None and ev.mean_loudness_model is None
    np.random.seed(1)
    a = np.random.uniform()
    LoudnessEvaluator(44100, keys, seed=1)                         # evaluation.py:23-24: seeds numpy's global generator
    assert np.random.uniform() == a
