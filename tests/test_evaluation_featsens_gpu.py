"""GPU: the sensitivity part of the whole-song evaluation (LoudnessEvaluator.process_song_tracks(feature_distance={'sensitivity':
True, ...})): '*_feat_sens' [stems][windows], the change of a variant's '*_feat_mse' in dB^2 per dB of a stem in a gain window
-- against the numpy reference of the gradient (tests/_specgrad_ref.py) from the gains the call returns and numpy's seeded
draws.  The model, the evaluator and the song are those of tests/test_evaluation_featdist_gpu.py.
Bound: the reference's per-entry bound on the gradient, times g ln 10 / (20 N).  The loudnorm variant's gains are formed on the
device from its own loudness values, within 1e-8 dB of the oracle's: orders below that bound."""
import numpy as np
import pytest
import torch

import _specgrad_ref as gref
from oracle import loudness_ref as ref
from test_evaluation_featdist_gpu import FEAT_KEYS, HOP, KEYS, MEAN_LOUDNESS, N, N_FFT, OLD_KEYS, SR, env, stack  # noqa: F401

pytestmark = pytest.mark.gpu

SENS_KEYS = ['sum_feat_sens', 'loudnorm_feat_sens', 'mix_feat_sens', 'random_feat_sens']


def reference_sensitivity(tracks, gains, reference):
    """gains [rows, stems, W] -> (sens [rows, stems, W], bound alike) of the numpy reference."""
    out = gref.gradient(stack(tracks), gains, stack(reference), None, N_FFT, HOP)
    scale = gains * np.log(10.0) / 20.0 / ((1 + N // HOP) * (N_FFT // 2 + 1))
    return out['grad'] * scale, out['grad_bound'] * np.abs(scale)


def test_switch_leaves_every_earlier_key_alone(env):
    a, reference, evaluate = env
    _, absent, next_absent = evaluate(a, reference, feature_distance=True)
    _, off, next_off = evaluate(a, reference, feature_distance={'sensitivity': False})
    _, on, next_on = evaluate(a, reference, feature_distance={'sensitivity': True, 'n_fft': N_FFT, 'hop': HOP})
    assert list(absent) == OLD_KEYS + FEAT_KEYS + ['feat_profile'] == list(off)
    assert list(on) == OLD_KEYS + FEAT_KEYS + ['feat_profile'] + SENS_KEYS
    for key in absent:
        assert on[key] == absent[key] and off[key] == absent[key], key
    assert next_on == next_off == next_absent                               # the same number of draws, in the same order
    W = len(on['smooth_gains']['bass'])
    for key in SENS_KEYS:
        assert np.asarray(on[key]).shape == (len(KEYS), W) and np.all(np.isfinite(on[key])), key
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, reference, feature_distance={'sensitivity': True, 'nfft': N_FFT})


def test_sensitivity_against_numpy(env):
    a, reference, evaluate = env
    _, stats, _ = evaluate(a, reference, feature_distance={'sensitivity': True})
    np.random.seed(7)
    drawn = [[float(np.random.uniform(0.5, 1.5)) for _ in KEYS] for _ in range(2)]
    plain = np.array([ref.integrated_loudness(a[k].astype(np.float64).T, SR) for k in KEYS])
    loudnorm = [10.0 ** ((MEAN_LOUDNESS[k] - plain[i]) / 20.0) for i, k in enumerate(KEYS)]
    smooth = np.array([stats['smooth_gains'][k] for k in KEYS], dtype=np.float64)
    W = smooth.shape[1]
    assert N // W >= N_FFT
    const = lambda g: np.repeat(np.asarray(g, dtype=np.float64)[:, None], W, axis=1)
    gains = np.stack([np.ones((4, W)), const(loudnorm), smooth] + [const(g) for g in drawn])
    sens, bound = reference_sensitivity(a, gains, reference)
    rows = {'sum': [0], 'loudnorm': [1], 'mix': [2], 'random': [3, 4]}
    for name, rr in rows.items():
        got = np.asarray(stats[name + '_feat_sens'])
        want, tol = sens[rr].mean(axis=0), bound[rr].mean(axis=0)
        ratio = np.abs(got - want) / tol
        print('%s_feat_sens: largest |entry| %.4g dB^2/dB, largest |difference| / bound = %.3g (largest bound %.3g)'
              % (name, np.abs(want).max(), ratio.max(), tol.max()))
        assert np.all(ratio <= 1.0), name


def test_planted_stem_reads_positive_where_it_is_too_loud(env):
    """The drums of the plain sum are 3 dB above the reference's in the second half of the song: in the gain windows of that half
    the drums' sensitivity is positive (turning them up makes it worse) and larger in magnitude than every other stem's.
    (tests/_specgrad_ref.py reads the same on this input: asserted here first.)"""
    a, reference, evaluate = env
    planted = {k: v.copy() for k, v in a.items()}
    planted['drums'][:, N // 2:] *= np.float32(10.0 ** (3.0 / 20.0))
    _, stats, _ = evaluate(planted, a, feature_distance={'sensitivity': True})
    got = np.asarray(stats['sum_feat_sens'])
    W, drums = got.shape[1], KEYS.index('drums')
    second = [w for w in range(W) if w * (N // W) >= N // 2]
    others = [s for s in range(len(KEYS)) if s != drums]
    want = reference_sensitivity(planted, np.ones((1, 4, W)), a)[0][0]
    print('planted +3 dB on the drums from window %d on: drums %s; largest other stem %s'
          % (second[0], ' '.join('%.3f' % v for v in got[drums]), ' '.join('%.3f' % v for v in np.abs(got[others]).max(axis=0))))
    assert len(second) >= 3
    for sens in (want, got):
        assert np.all(sens[drums, second] > 0.0)
        assert np.all(sens[drums, second] > np.abs(sens[others][:, second]).max(axis=0))
