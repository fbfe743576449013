"""CPU: the reference of the spectrogram-distance gradient (tests/_specgrad_ref.py) against finite differences of the
distance's own reference, its homogeneity identity, the size of its error bound on the inputs of the GPU sweep, and the host
side of the new entries (header, ctypes table, shape rules)."""
import os
import re

import numpy as np
import pytest

import _specdist_ref as dref
import _specgrad_ref as ref
import _spectrum_ref as sref


@pytest.fixture
def float64_frames(monkeypatch):
    """_specdist_ref.distance with the float32 roundings of the mix signal and of the frame switched off, for this file's
    finite differences only: a step of 1e-6 in a gain moves the mix signal by less than a float32 ulp."""
    frames = sref.frames
    monkeypatch.setattr(sref, 'mix_signal', lambda stems, gains=None: ref._mix(np.asarray(stems), gains, True))
    monkeypatch.setattr(sref, 'frames', lambda xm, n_fft, hop, exact=False: frames(xm, n_fft, hop, exact=True))


def fd_inputs(n_fft):
    rng = np.random.default_rng(40 + n_fft)
    n, S, G = 4 * n_fft + 13, 3, 3
    stems = rng.standard_normal((S, n, 2)) * rng.uniform(0.05, 0.2, (S, 1, 1))
    ref_stems = (stems[:2] * 0.8 + 0.1 * rng.standard_normal((2, n, 2)))[:, :, :1]
    gains = rng.uniform(0.5, 1.5, (2, S, G))
    return stems, gains, ref_stems, rng.uniform(0.9, 1.1, (2, 2))


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_formula_against_finite_differences(float64_frames, n_fft):
    stems, gains, ref_stems, ref_gains = fd_inputs(n_fft)
    hop, h = n_fft // 2, 1e-6
    edges = np.array([0, n_fft // 2 + 1])
    out = ref.gradient(stems, gains, ref_stems, ref_gains, n_fft, hop, exact=True, want_bound=False)
    S2 = lambda g: dref.distance(stems, g, ref_stems, ref_gains, n_fft, hop, edges, 1)[0][:, 0, 0, 1]
    assert np.allclose(S2(gains), out['value'][:, 1], rtol=1e-12, atol=0) and out['floored'].sum() == 0
    worst = 0.0
    for s in range(gains.shape[1]):
        for j in range(gains.shape[2]):
            up, dn = gains.copy(), gains.copy()
            up[:, s, j] += h
            dn[:, s, j] -= h
            fd = (S2(up) - S2(dn)) / (2.0 * h)
            worst = max(worst, float((np.abs(fd - out['grad'][:, s, j]) / np.abs(out['grad']).max(axis=(1, 2))).max()))
    print('n_fft %d: largest |FD - analytic| = %.3g of the row\'s largest entry' % (n_fft, worst))
    assert worst <= 1e-4


@pytest.mark.parametrize('n_fft', [64, 2048])
def test_homogeneity_identity(n_fft):
    """Every level rises by 20 log10(c) under a common gain c where nothing is floored: sum g dJ/dg = (40 / ln 10) S1."""
    stems, gains, ref_stems, ref_gains = fd_inputs(n_fft)
    out = ref.gradient(stems, gains, ref_stems, ref_gains, n_fft, n_fft // 2, exact=True, want_bound=False)
    assert out['floored'].sum() == 0
    lhs, rhs = (gains * out['grad']).sum(axis=(1, 2)), ref.SCALE * out['value'][:, 0]
    assert np.all(np.abs(lhs - rhs) <= 1e-9 * np.abs(rhs)), (lhs, rhs)
    # (with the mix signal and the frame rounded to float32, as the definition has them, the two sides differ by that rounding
    # amplified at the near-null bins -- 3e-6 relative here; the GPU test takes the reference's own difference into its bound)


def sweep(n_fft):
    return ref.sweep_cases(n_fft) if n_fft <= 2048 else [ref.large_case(n_fft)]


@pytest.mark.parametrize('n_fft', [64, 256, 2048, 8192, 16384])
def test_sweep_inputs_keep_the_bounds_informative(n_fft):
    """A condition on the inputs of the GPU sweep, not a measurement: every entry's bound is at most 1e-2 of its row's largest
    |gradient entry|, so that a device result cannot be wrong by a per cent of the row's scale and still pass."""
    cases = sweep(n_fft)
    worst, seen = 0.0, {k: set() for k in ('T', 'hop', 'S', 'S_ref', 'R', 'ch', 'n_gains', 'dtype', 'ref_dtype', 'planar', 'clips')}
    for c in cases:
        out = ref.gradient_clips(c['stems'], c['gains'], c['ref_stems'], c['ref_gains'], n_fft, c['hop'])
        for clip in range(len(c['stems'])):
            for r in range(out['grad'].shape[1]):
                if r in c['zero_rows']:
                    assert np.all(out['grad'][clip, r] == 0.0) and np.all(out['grad_bound'][clip, r] == 0.0)
                    continue
                ratio = float((out['grad_bound'][clip, r] / np.abs(out['grad'][clip, r]).max()).max())
                worst = max(worst, ratio)
                assert ratio <= 1e-2, (c['hop'], c['n'], clip, r, ratio)
        G = None if c['gains'] is None else c['gains'].shape[3]
        assert G in (None, 1) or c['n'] // G >= n_fft
        assert c['n'] > n_fft // 2 and 1 + c['n'] // c['hop'] == c['T'] and c['n'] % c['hop']
        seen['T'].add(c['T']); seen['hop'].add(c['hop']); seen['S'].add(c['stems'].shape[1]); seen['S_ref'].add(c['ref_stems'].shape[1])
        seen['R'].add(out['grad'].shape[1]); seen['ch'].add(c['stems'].shape[3]); seen['n_gains'].add(G)
        seen['dtype'].add(c['stems'].dtype.name); seen['ref_dtype'].add(c['ref_stems'].dtype.name)
        seen['planar'].add(c['planar']); seen['clips'].add(len(c['stems']))
    print('n_fft %d: %d cases, largest bound / largest |entry| of the row = %.3g' % (n_fft, len(cases), worst))
    if n_fft <= 2048:
        assert seen['T'] >= {2, 9} and seen['R'] == {1, 5} and seen['ch'] == {1, 2} and seen['clips'] == {1, 3}
        assert seen['dtype'] == seen['ref_dtype'] == {'float32', 'float64'} and seen['planar'] == {False, True}
        assert seen['n_gains'] >= {None, 1, 2} and len(seen['S']) >= 3 and len(seen['S_ref']) >= 2
        assert seen['hop'] >= {n_fft // 2, n_fft}
    else:
        c = cases[0]
        assert c['n'] == 2 * n_fft + n_fft // 2 + 37 and c['gains'].shape[3] == 2
        assert ref.frames_owned(c['n'], 2, n_fft, c['hop']).tolist() == [2, 1]           # a node that owns exactly one frame


def test_sweep_covers_every_axis_value():
    """Over the three small sizes together: T 2 / 9 / 19, hop 23, S 1 / 2 / 3 / 5, S_ref 1 / 2 / 4, n_gains None / 1 / 2 / 3."""
    cases = [c for n_fft in (64, 256, 2048) for c in ref.sweep_cases(n_fft)]
    assert {c['T'] for c in cases} == {2, 9, 19} and 23 in {c['hop'] for c in cases}
    assert {c['stems'].shape[1] for c in cases} == {1, 2, 3, 5} and {c['ref_stems'].shape[1] for c in cases} == {1, 2, 4}
    assert {None if c['gains'] is None else c['gains'].shape[3] for c in cases} == {None, 1, 2, 3}
    assert any(c['stems'].shape[3] == 2 and c['ref_stems'].shape[3] == 1 for c in cases)


def test_ctypes_table_has_the_specgrad_entries():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 39
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_specgrad\w*)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        found[m.group(2)] = (m.group(1), [a.strip() for a in m.group(3).split(',')])
    assert set(found) == {'dam_specgrad_workspace_bytes', 'dam_specgrad'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d, 'float': _lib.c_f}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        assert argtypes == [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args], name
    source = open(os.path.join(ROOT, 'deep-audio-mixer_amd', 'csrc', 'dam_specgrad.hip')).read()
    for name in found:
        assert re.search(r'extern "C" \w+ %s\(' % name, source), name
    assert '#pragma clang fp contract(off)' in source


def test_workspace_size_and_refusals_of_the_library(dam_lib):
    T = 1 + 6007 // 128
    assert dam_lib.dam_specgrad_workspace_bytes(2, 5, 3, 6007, 256, 128, 3) == 16 * 2 * 5 * T * 4
    assert dam_lib.dam_specgrad_workspace_bytes(2, 5, 3, 6007, 256, 128, 0) == 16 * 2 * 5 * T * 4       # gains NULL
    for args in [(0, 5, 3, 6007, 256, 128, 3), (65536, 5, 3, 6007, 256, 128, 3), (2, 0, 3, 6007, 256, 128, 3),
                 (2, 5, 0, 6007, 256, 128, 3), (2, 5, 3, 128, 256, 128, 1), (2, 5, 3, 6007, 100, 128, 3),
                 (2, 5, 3, 6007, 256, 0, 3), (2, 5, 3, 6007, 256, 128, 24), (2, 5, 3, 6007, 256, 128, 6008)]:
        assert dam_lib.dam_specgrad_workspace_bytes(*args) == 0, args


def test_shape_checks_refuse_before_anything_runs():
    from deep_audio_mixer_amd import ops
    ok = dict(stems_shape=(2, 3, 6007, 2), gains_shape=(2, 5, 3, 7), ref_shape=(2, 2, 6007, 1), ref_gains_shape=(2, 2, 3),
              n_fft=256, hop=None)
    assert ops.specgrad_check_shapes(**ok) == (2, 5, 3, 6007, 2, 2, 1, 256, 128, 7)
    assert ops.specgrad_check_shapes(**dict(ok, gains_shape=None, ref_gains_shape=None))[1::8] == (1, 1)
    assert ops.specgrad_check_shapes(**dict(ok, gains_shape=(2, 5, 3, 23)))[9] == 23          # 6007 // 23 = 261 >= 256
    bad = [dict(ref_shape=(2, 2, 6008, 1)), dict(ref_shape=(3, 2, 6007, 1)), dict(n_fft=100), dict(n_fft=32), dict(n_fft=32768),
           dict(hop=0), dict(stems_shape=(2, 3, 128, 2), ref_shape=(2, 2, 128, 1), gains_shape=None, ref_gains_shape=None),
           dict(stems_shape=(2, 3, 6007, 3)), dict(ref_shape=(2, 2, 6007, 4)), dict(gains_shape=(2, 5, 2, 7)),
           dict(gains_shape=(2, 0, 3, 7)), dict(gains_shape=(2, 65536, 3, 1)), dict(gains_shape=(1, 5, 3, 7)),
           dict(gains_shape=(5, 3, 7)), dict(ref_gains_shape=(2, 3, 3)), dict(ref_gains_shape=(2, 2, 0)),
           dict(ref_gains_shape=(2, 3)), dict(amin=0.0), dict(amin=-1.0), dict(amin=1e-60), dict(amin=float('nan')),
           dict(stems_shape=(3, 6007, 2)), dict(stems_shape=(0, 3, 6007, 2), ref_shape=(0, 2, 6007, 1)),
           dict(gains_shape=(2, 5, 3, 24)),                              # the gain-segment rule: 6007 // 24 = 250 < 256
           dict(gains_shape=(2, 5, 3, 6007))]
    for change in bad:
        with pytest.raises(ValueError):
            ops.specgrad_check_shapes(**dict(ok, **change))
    with pytest.raises(ValueError, match='unsupported'):
        ops.specgrad_check_shapes(**dict(ok, gains_shape=(2, 5, 3, 24)))
    for change in (dict(n_fft=256.0), dict(hop=1.5)):
        with pytest.raises(TypeError):
            ops.specgrad_check_shapes(**dict(ok, **change))


def test_python_surface_refuses_cpu_tensors_and_converts_sensitivity():
    import torch
    from deep_audio_mixer_amd import spectrum
    x = torch.zeros(2, 4000, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        spectrum.spectrogram_distance_grad(x, None, x)
    with pytest.raises(RuntimeError):
        spectrum.rendered_spectrogram_mse(x, torch.ones(2, dtype=torch.float64), x)
    with pytest.raises(ValueError):
        spectrum.rendered_spectrogram_mse(x, None, x)
    g, dg = np.array([[2.0, 0.5]]), np.array([[3.0, -4.0]])
    want = g * dg * np.log(10.0) / 20.0
    assert np.array_equal(spectrum.gain_sensitivity_db(g, dg), want)
    assert np.array_equal(spectrum.gain_sensitivity_db(torch.from_numpy(g), torch.from_numpy(dg)).numpy(), want)
