"""CPU: the numpy reference of the gain fit (tests/_gainfit_ref.py) against known answers -- so that the GPU tests compare
the kernels with something that has itself been checked -- the new ctypes entries against the header, and the host-side
argument checks of gainfit.py (no GPU is touched)."""
import math
import os
import re

import numpy as np
import pytest

import _gainfit_ref as ref

S, C, N, W = 4, 2, 6007, 5


def test_window_convention_is_the_gain_ramps():
    assert ref.window_bounds(N, W) == [(0, 1201), (1201, 2402), (2402, 3603), (3603, 4804), (4804, 6007)]
    assert ref.window_bounds(7, 7)[-1] == (6, 7) and ref.window_bounds(9, 1) == [(0, 9)]
    assert ref.addends(N, W, C) == 1203 * 2


def test_moments_are_exactly_rounded():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 40, 2))                                 # float64: the products need the error-free split
    y = rng.standard_normal((40, 2))
    M = ref.moments(x, y, 3)
    from fractions import Fraction
    u = np.concatenate([x, y[None]])
    for w, (a, b) in enumerate(ref.window_bounds(40, 3)):
        for i in range(3):
            for j in range(3):
                exact = sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(u[i, a:b].ravel(), u[j, a:b].ravel()))
                assert M[w, i, j] == float(exact), (w, i, j)
    assert np.array_equal(M, M.transpose(0, 2, 1))


def test_known_gains_float64_target():
    x, y, g = ref.base_input(np.float64)
    gains, residual, status, cond = ref.solve(ref.moments(x, y, W))
    print('float64 target: largest gain error %.3g, cond(R) <= %.3f, residual <= %.3g' % (np.abs(gains - g).max(), cond.max(), residual.max()))
    assert np.abs(gains - g).max() <= 7e-16
    assert np.all(cond <= 5.6) and np.all(cond >= 1.0)
    assert np.all(residual <= 1e-15) and np.all(residual >= 0.0)
    assert status.tolist() == [S] * W


def test_known_gains_float32_target():
    x, y, g = ref.base_input(np.float32)
    assert y.dtype == np.float32
    gains, residual, status, cond = ref.solve(ref.moments(x, y, W))
    print('float32 target: largest gain error %.3g, residual <= %.3g' % (np.abs(gains - g).max(), residual.max()))
    assert np.abs(gains - g).max() <= 6.3e-9 and np.all(cond <= 5.6) and status.tolist() == [S] * W
    assert np.all(residual <= 1e-15)


def test_pooling_adds_neighbouring_windows():
    x, y, _ = ref.base_input(np.float64)
    M = ref.moments(x, y, W)
    pooled = ref.solve(M, pool=1)
    for w in range(W):
        alone = ref.solve(M[max(0, w - 1):w + 2].sum(axis=0, keepdims=True))
        assert np.allclose(pooled[0][:, w], alone[0][:, 0], rtol=1e-13, atol=0) and pooled[2][w] == S
    everything = ref.solve(M, pool=W)
    assert np.allclose(everything[0], everything[0][:, :1], rtol=1e-13, atol=0)


def test_planted_cases():
    x, y, g = ref.base_input(np.float64)
    # a zeroed stem: NaN, three stems fitted -- everywhere, and in one window only
    z = x.copy()
    z[2] = 0.0
    gains, residual, status, _ = ref.solve(ref.moments(z, y, W))
    assert np.all(np.isnan(gains[2])) and not np.any(np.isnan(gains[[0, 1, 3]])) and status.tolist() == [3] * W
    assert np.all(residual > 0.01)                                      # its share of y is not explained
    z = x.copy()
    z[1, 1201:2402] = 0.0
    yz = ref.mix(z, g)
    gains, residual, status, _ = ref.solve(ref.moments(z, yz, W))
    assert status.tolist() == [4, 3, 4, 4, 4] and np.isnan(gains[1, 1]) and np.isnan(gains).sum() == 1
    assert np.nanmax(np.abs(gains - g)) <= 7e-16 and np.all(residual <= 1e-15)
    # a silent target window: status 0, everything NaN there
    y0 = y.copy()
    y0[3603:4804] = 0.0
    gains, residual, status, _ = ref.solve(ref.moments(x, y0, W))
    assert status.tolist() == [4, 4, 4, 0, 4] and np.all(np.isnan(gains[:, 3])) and math.isnan(residual[3])
    assert np.isnan(gains).sum() == S and np.isnan(residual).sum() == 1
    # two identical stems: rank-deficient without a ridge, equal gains with one
    t = x.copy()
    t[3] = t[0]
    yt = ref.mix(t, g)
    gains, residual, status, cond = ref.solve(ref.moments(t, yt, W))
    assert status.tolist() == [-1] * W and np.all(np.isnan(gains)) and np.all(np.isnan(residual)) and np.all(np.isnan(cond))
    gains, residual, status, cond = ref.solve(ref.moments(t, yt, W), ridge=1e-6)
    assert status.tolist() == [4] * W and np.all(cond > 1e6) and np.all(cond < 1e7)
    assert np.abs(gains[0] - gains[3]).max() <= 64 * cond.max() * ref.U_ROUND * np.abs(gains).max()
    assert np.abs(gains[0] - 0.5 * (g[0] + g[3])).max() < 1e-5          # the two share their sum; the ridge costs ~1e-6
    # inverted polarity: a negative gain, nothing else changes
    gn = g.copy()
    gn[1] = -gn[1]
    gains, residual, status, _ = ref.solve(ref.moments(x, ref.mix(x, gn), W))
    assert np.abs(gains - gn).max() <= 7e-16 and status.tolist() == [4] * W and np.all(gains[1] < 0)


def test_gain_error_known_answers():
    rng = np.random.default_rng(3)
    fit = rng.uniform(0.5, 1.5, (3, 4))
    err, err_stem, kept = ref.gain_error(fit, fit[None])
    assert err.tolist() == [0.0] and err_stem.tolist() == [[0.0] * 3] and kept.tolist() == [12]
    err, _, kept = ref.gain_error(fit, np.stack([2.0 * fit, fit * rng.uniform(0.1, 9.0, (1, 4))]))
    assert np.all(err <= 1e-12) and kept.tolist() == [12, 12]           # a common gain per window is a master fader
    # one stem 6.02 dB up against two: d = (D, 0, 0), mean D / 3 -> contributions 2D/3, D/3, D/3
    cand = fit.copy()
    cand[0] *= 2.0
    D = 20.0 * math.log10(2.0)
    err, err_stem, kept = ref.gain_error(fit, cand[None])
    assert abs(err[0] - 4.0 * D / 9.0) < 1e-13 and np.allclose(err_stem[0], [2 * D / 3, D / 3, D / 3], atol=1e-13)
    # constants: [V, S, 1] is the broadcast
    const = rng.uniform(0.5, 1.5, (2, 3, 1))
    a, b = ref.gain_error(fit, const), ref.gain_error(fit, np.broadcast_to(const, (2, 3, 4)))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    # what is not a level is left out: NaN, a negative fitted gain, and a window with a single stem left
    f2 = fit.copy()
    f2[0, 0] = np.nan
    f2[1, 1] = -0.7
    f2[0, 2] = f2[1, 2] = np.nan
    err, err_stem, kept = ref.gain_error(f2, cand[None])
    assert kept.tolist() == [2 + 2 + 0 + 3]
    assert abs(err_stem[0, 0] - 0.5 * (D / 2 + 2 * D / 3)) < 1e-13      # stem 0: windows 1 (two kept) and 3 (three kept)
    err, err_stem, kept = ref.gain_error(np.full((3, 4), np.nan), cand[None])
    assert kept.tolist() == [0] and math.isnan(err[0]) and np.all(np.isnan(err_stem))


def test_ctypes_table_has_the_gainfit_entries():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 25
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_gainfit_\w+)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        args = [a.strip() for a in m.group(3).split(',')] if m.group(3).strip() not in ('', 'void') else []
        found[m.group(2)] = (m.group(1), args)
    assert set(found) == {'dam_gainfit_tile_samples', 'dam_gainfit_workspace_bytes', 'dam_gainfit_moments',
                          'dam_gainfit_solve', 'dam_gainfit_gain_error'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        want = [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args]
        assert argtypes == want, name
    assert float.fromhex(re.search(r'#define DAM_GAINFIT_GATE (\S+)', header).group(1)) == ref.GATE == 1e-8
    assert float.fromhex(re.search(r'#define DAM_GAINFIT_PIVOT (\S+)', header).group(1)) == ref.PIVOT == 2.0 ** -40
    assert int(re.search(r'#define DAM_GAINFIT_MAX_STEMS (\d+)', header).group(1)) == ref.MAX_STEMS == 8


def test_host_side_argument_checks():
    import torch
    from deep_audio_mixer_amd import gainfit, ops
    assert ops.GAINFIT_MAX_STEMS == ref.MAX_STEMS
    x, y = torch.zeros((4, 100, 2)), torch.zeros((100, 2))
    for stems, mix, n_windows in ((x[0], y, 5), (torch.zeros((9, 100, 2)), y, 5), (torch.zeros((0, 100, 2)), y, 5),
                                  (torch.zeros((4, 100, 3)), torch.zeros((100, 3)), 5), (x, y[:99], 5), (x, y[:, :1], 5),
                                  (x, y, 0), (x, y, 101), (x, y, -1)):
        for fn in (gainfit.moments, gainfit.fit_gains):
            with pytest.raises(ValueError):
                fn(stems, mix, n_windows)
    with pytest.raises(TypeError):
        gainfit.moments(x, y, 2.0)
    for kw in (dict(pool=-1), dict(ridge=-1e-9), dict(ridge=float('nan'))):
        with pytest.raises(ValueError):
            gainfit.fit_gains(x, y, 5, **kw)
        with pytest.raises(ValueError):
            gainfit.solve(torch.zeros((5, 5, 5), dtype=torch.float64), **kw)
    for kw in (dict(pool=1.5), dict(ridge='0')):
        with pytest.raises(TypeError):
            gainfit.fit_gains(x, y, 5, **kw)
    if not torch.cuda.is_available():                                   # what is well-formed still needs the GPU
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.fit_gains(x, y, 5)
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.gain_error_device(torch.ones((4, 5), dtype=torch.float64), torch.ones((1, 4, 5), dtype=torch.float64))
    r = np.array([1.0, 0.1, 0.0])
    assert np.allclose(gainfit.residual_db(r)[:2], [0.0, -10.0], atol=1e-13) and gainfit.residual_db(r)[2] == -np.inf
    got = gainfit.residual_db(torch.from_numpy(r))
    assert torch.is_tensor(got) and got[2].item() == -math.inf and abs(got[1].item() + 10.0) < 1e-13


def test_evaluator_switch_checks_its_keys():
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator.__new__(LoudnessEvaluator)                   # (the meter needs the library; the check does not)
    assert ev._gain_fit_args(True) == (0, 0.0) and ev._gain_fit_args({'pool': 2, 'ridge': 1e-6}) == (2, 1e-6)
    with pytest.raises(ValueError, match='unknown'):
        ev._gain_fit_args({'pol': 1})
    with pytest.raises(ValueError):
        ev._gain_fit_args({'pool': -1})


def test_songlist_passes_the_switch_and_skips_nan_rows(monkeypatch):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator.__new__(LoudnessEvaluator)
    fit_keys = ['sum_gain_error', 'random_gain_error', 'loudnorm_gain_error', 'mix_gain_error']
    seen = []

    def fake(base_dir, song_name, *args, **kw):
        seen.append((len(args), kw))
        row = {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
        if kw.get('gain_fit'):
            row.update({k: 5.0 + len(song_name) for k in fit_keys})
            if song_name == 'bcd':
                row['mix_gain_error'] = float('nan')
            row['loudnorm_gain_error'] = float('nan')
        return row
    monkeypatch.setattr(ev, 'process_song', fake)
    _, means = ev.process_songlist('.', ['a', 'bcd'])
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} and seen == [(6, {}), (6, {})]
    _, means = ev.process_songlist('.', ['a', 'bcd'], gain_fit={'pool': 1})
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} | set(fit_keys)
    assert seen[2:] == [(6, {'gain_fit': {'pool': 1}})] * 2
    assert means['sum_gain_error'] == 7.0 and means['mix_gain_error'] == 6.0 and math.isnan(means['loudnorm_gain_error'])
