"""CPU: the numpy reference of the spectrogram distance (tests/_specdist_ref.py) against known answers of its own conventions
-- so that the GPU tests compare the kernels with something that has itself been checked -- the inputs of the GPU parity
sweep (their bounds must be tight beside the values they guard), the new ctypes entries against the header and the
host-side argument checks of ops.py and spectrum.py (no GPU is touched)."""
import os
import re

import numpy as np
import pytest

import _bandfit_ref as bref
import _specdist_ref as ref
import _spectrum_ref as sref


def noise(seed, S, n, C, scale=0.1):
    return (scale * np.random.default_rng(seed).standard_normal((S, n, C))).astype(np.float32)


def test_common_gain_is_a_pure_bias():
    """cand = c * ref with every level above the floor: d = 20 log10 c in every bin."""
    x = noise(1, 3, 4000, 2)
    c = 0.5                                                                  # (a power of two: the float32 mix scales exactly)
    sums, count, bound, d, Lc, Lr = ref.distance(x, np.full((1, 3, 1), c), x, None, 256, 128, sref.band_edges(44100, 256)[0], 3)
    assert Lr.min() > -99.0 and Lc.min() > -99.0
    fig = ref.summary(sums, count)
    want = 20.0 * np.log10(c)
    print('common gain %.3g: bias %.12f dB (want %.12f), centred rms up to %.3g dB' % (c, fig[0, 0, 1], want, fig[0, :, 2].max()))
    assert np.abs(d - want).max() <= 1e-9 and np.std(d) <= 1e-9             # bin by bin, and the centred rms taken directly
    assert np.abs(fig[0, :, 1] - want).max() <= 1e-9 and np.abs(fig[0, :, 0] - want * want).max() <= 1e-9
    # from the SUMS the centred rms is sqrt(mse - bias^2), a difference of two numbers near 36: each is good to a few ulp
    # (2^-52 relative), so the root cannot be told from 0 below sqrt(8 * 2^-52 * mse) = 2.5e-7 dB -- the floor of the figure
    assert fig[0, :, 2].max() <= np.sqrt(8.0 * 2.0 ** -52 * want * want)


def test_identical_and_silent_inputs_give_exact_zeros():
    x = noise(2, 2, 3000, 1)
    edges = ref.edge_tables(64)[2]
    sums, count, bound, d, Lc, Lr = ref.distance(x, None, x, None, 64, 23, edges, 5)
    assert np.all(sums == 0.0) and np.all(d == 0.0) and np.all(bound > 0.0)
    z = np.zeros_like(x)
    sums, count, bound, d, Lc, Lr = ref.distance(z, None, z, None, 64, 23, edges, 5)
    assert np.all(sums == 0.0) and np.all(Lc == -100.0) and np.all(Lr == -100.0)
    # silence in the reference only: L_ref = -100 exactly, d = L_cand + 100
    sums, count, bound, d, Lc, Lr = ref.distance(x, None, z, None, 64, 23, np.array([0, 33]), 1)
    assert np.all(Lr == -100.0) and np.array_equal(d[0], Lc[0] + 100.0) and sums[0, 0, 0, 0] == (Lc[0] + 100.0).sum()
    # another floor: amin = 1e-3 -> -60 dB
    assert np.all(ref.levels(np.zeros(100, dtype=np.float32), 64, 32, amin=1e-3)[0] == -60.0)


@pytest.mark.parametrize('n, W, hop', [(6007, 5, 128), (6007, 7, 77), (129, 2, 64), (1000, 3, 23), (33, 1, 64), (4096, 4, 1024)])
def test_windows_and_counts(n, W, hop):
    first = bref.frame_windows(n, W, hop)
    w_of = ref.window_of_frames(n, W, hop)
    T = 1 + n // hop
    assert len(w_of) == T
    for w in range(W):
        assert np.array_equal(np.nonzero(w_of == w)[0], np.arange(first[w], first[w + 1]))
    from deep_audio_mixer_amd import ops
    assert ops.gainfit_band_frame_windows(n, W, hop) == list(first)
    n_fft = 64
    if n > n_fft // 2:
        edges = ref.edge_tables(n_fft)[2]
        x = noise(n, 1, n, 1)
        count = ref.distance(x, None, x, None, n_fft, hop, edges, W)[1]
        frames = np.array([first[w + 1] - first[w] for w in range(W)])
        assert np.array_equal(count, np.diff(edges)[:, None] * frames[None, :])


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_extended_tables_cover_every_bin_and_total_is_the_criterion(n_fft):
    from deep_audio_mixer_amd import spectrum
    edges = spectrum.band_edges(44100, n_fft)[0]
    ext, low, high = spectrum.extend_edges(edges, n_fft)
    assert np.array_equal(ext, ref.extend_edges(edges, n_fft))
    assert ext[0] == 0 and ext[-1] == n_fft // 2 + 1 and np.all(np.diff(ext) > 0)
    assert len(ext) == len(edges) + int(low) + int(high) and np.array_equal(ext[int(low):len(ext) - int(high)], edges)
    full = np.array([0, n_fft // 2 + 1])
    assert np.array_equal(spectrum.extend_edges(full, n_fft)[0], full)
    rng = np.random.default_rng(n_fft)
    n = 5 * n_fft + 11
    x, y = noise(n_fft, 3, n, 2), noise(n_fft + 1, 1, n, 2)
    g = rng.uniform(0.5, 1.5, (2, 3, 4))
    sums, count, bound, d, Lc, Lr = ref.distance(x, g, y, None, n_fft, n_fft // 2, ext, 3)
    fig = ref.summary(sums, count)
    for r in range(2):
        plain = np.mean((Lc[r] - Lr) ** 2)
        assert abs(fig[r, 0, 0] - plain) <= 1e-12 * plain
        assert abs(fig[r, 0, 1] - np.mean(Lc[r] - Lr)) <= 1e-12 * np.abs(Lc[r] - Lr).mean()
    assert count.sum() == Lr.size


def test_summary_places_nan_at_zero_counts():
    sums = np.random.default_rng(0).uniform(1.0, 2.0, (2, 3, 2, 2))
    count = np.array([[4, 0], [0, 0], [2, 0]])
    fig = ref.summary(sums, count)
    assert np.all(np.isnan(fig[:, 2])) and np.all(np.isnan(fig[:, 1 + 3 + 1]))          # band 1, window 1: no count
    assert np.all(np.isfinite(fig[:, 0])) and np.all(np.isfinite(fig[:, 1])) and np.all(np.isfinite(fig[:, 4]))


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_sweep_inputs_keep_the_bounds_informative(n_fft):
    """The inputs of the GPU parity sweep: on every cell the bound on sum d^2 is at most 1e-2 of the value, so that a device
    result cannot be wrong by a per cent and still pass; every axis of the sweep takes every value."""
    cases = ref.sweep_cases(n_fft)
    worst, seen = 0.0, {k: set() for k in ('T', 'W', 'S', 'S_ref', 'R', 'ch', 'n_gains', 'dtype', 'planar', 'B')}
    for c in cases:
        sums, count, bound, d, Lc, Lr = ref.distance(c['stems'], c['gains'], c['ref_stems'], c['ref_gains'], n_fft, c['hop'],
                                                     c['edges'], c['W'])
        ratio = bound[..., 1] / np.abs(sums[..., 1])
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1e-2), (c['hop'], c['n'], float(ratio.max()))
        for r in c['zero_rows']:
            assert np.all(Lc[r] == -100.0)
        seen['T'].add(c['T']); seen['W'].add(c['W']); seen['S'].add(c['stems'].shape[0]); seen['S_ref'].add(c['ref_stems'].shape[0])
        seen['R'].add(d.shape[0]); seen['ch'].add(c['stems'].shape[2]); seen['dtype'].add(c['stems'].dtype.name)
        seen['n_gains'].add(None if c['gains'] is None else c['gains'].shape[2] if c['gains'].shape[2] < c['n'] else 'n')
        seen['planar'].add(c['planar']); seen['B'].add(len(c['edges']) - 1)
        assert c['n'] > n_fft // 2 and 1 + c['n'] // c['hop'] == c['T']
        assert len(set(ref.window_of_frames(c['n'], c['W'], c['hop']).tolist())) == c['W']
    print('n_fft %d: %d cases, largest bound / |sum d^2| = %.3g' % (n_fft, len(cases), worst))
    assert seen['T'] == {1, 2, 9, 19} and seen['W'] == {1, 3, 5} and seen['S'] == {1, 2, 3, 5} and seen['R'] == {1, 5}
    assert seen['ch'] == {1, 2} and seen['dtype'] == {'float32', 'float64'} and seen['planar'] == {False, True}
    assert seen['n_gains'] == {None, 1, 3, 7, 'n'} and len(seen['B']) == 3
    assert any(c['n'] == n_fft // 2 + 1 for c in cases) and any(c['n'] % c['hop'] for c in cases)
    assert any(c['ref_stems'].shape[0] != c['stems'].shape[0] for c in cases)
    # a last window of one frame
    assert any(c['W'] > 1 and int((ref.window_of_frames(c['n'], c['W'], c['hop']) == c['W'] - 1).sum()) == 1 for c in cases)


def test_ctypes_table_has_the_specdist_entries():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 34
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_specdist_\w+)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        found[m.group(2)] = (m.group(1), [a.strip() for a in m.group(3).split(',')])
    assert set(found) == {'dam_specdist_workspace_bytes', 'dam_specdist_sums', 'dam_specdist_summary'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d, 'float': _lib.c_f}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        assert argtypes == [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args], name
    source = open(os.path.join(ROOT, 'deep-audio-mixer_amd', 'csrc', 'dam_specdist.hip')).read()
    for name in found:
        assert re.search(r'extern "C" \w+ %s\(' % name, source), name
    assert '#pragma clang fp contract(off)' in source


def test_shape_checks_refuse_before_anything_runs():
    from deep_audio_mixer_amd import ops
    ok = dict(stems_shape=(3, 6007, 2), gains_shape=(5, 3, 7), ref_shape=(2, 6007, 1), ref_gains_shape=(2, 3), n_fft=256,
              hop=None, n_windows=5)
    assert ops.specdist_check_shapes(**ok) == (5, 3, 6007, 2, 2, 1, 256, 128, 5)
    assert ops.specdist_check_shapes(**dict(ok, gains_shape=None, ref_gains_shape=None))[0] == 1
    bad = [dict(ref_shape=(2, 6008, 1)), dict(n_fft=100), dict(n_fft=32), dict(n_fft=32768), dict(hop=0),
           dict(stems_shape=(3, 128, 2), ref_shape=(2, 128, 1), n_windows=1, gains_shape=None, ref_gains_shape=None),
           dict(stems_shape=(3, 6007, 3)), dict(ref_shape=(2, 6007, 4)), dict(gains_shape=(5, 2, 7)), dict(gains_shape=(0, 3, 7)),
           dict(gains_shape=(65536, 3, 1)), dict(gains_shape=(5, 3, 6008)), dict(ref_gains_shape=(3, 3)),
           dict(ref_gains_shape=(2, 0)), dict(n_windows=0), dict(n_windows=6008), dict(n_windows=40, hop=256),
           dict(n_bands=0), dict(n_bands=65), dict(amin=0.0), dict(amin=-1.0), dict(amin=1e-60), dict(amin=float('nan')),
           dict(stems_shape=(6007, 2))]
    for change in bad:
        with pytest.raises(ValueError):
            ops.specdist_check_shapes(**dict(ok, **change))
    for change in (dict(n_fft=256.0), dict(hop=1.5), dict(n_windows=True)):
        with pytest.raises(TypeError):
            ops.specdist_check_shapes(**dict(ok, **change))


def test_python_surface_refuses_cpu_tensors():
    import torch
    from deep_audio_mixer_amd import spectrum
    x = torch.zeros(2, 4000, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        spectrum.spectrogram_distance(x, None, x)
    with pytest.raises(RuntimeError, match='GPU only'):
        spectrum.distance_summary(torch.zeros(1, 1, 1, 2, dtype=torch.float64), torch.ones(1, 1, dtype=torch.int64))
