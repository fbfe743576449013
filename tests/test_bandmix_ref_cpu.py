"""CPU: the numpy reference of the band-gain mixer (tests/_bandmix_ref.py) against the consequences include/dam_hip.h states -- so
that the GPU tests compare the kernels with something that has itself been checked -- the new ctypes entries against the header,
and the host-side argument checks of ops.py, gainfit.py and evaluation.py (no GPU is touched).

Figures of the reference (44.1 kHz, third-octave tables unless stated):
  identity, six geometries: the stems' sum back to 8.3e-17 .. 3.7e-15;
  broadband gains over the table [2, 3, 40, 100] of n_fft 256 (bins uncovered on both sides), W = 1: sum g_s x_s to 4.3e-15;
  gain steps, W = 5, n_fft 256, hops 128 / 77 / 32: the 4983 samples at least n_fft/2 inside their window are the gain-ramp mix's
  to 6.4e-15 / 3.3e-16 / 2.2e-16; the other 1024 deviate by up to 0.42 / 0.33 / 0.22 (the frames that straddle a border
  cross-fade the two windows' gains where the mix steps);
  two-band case, W = 1: the render of the reference's own fitted band gains, broadband fit as fill, leaves 1.4e-6 of the mix's
  energy against a broadband residual of 3.5e-2 (4.0e-5 of it); with fill = 0: 6.0e-5."""
import os
import re

import numpy as np
import pytest

import _bandfit_ref as bref
import _bandmix_ref as ref
import _gainfit_ref as gref

SR = 44100
# S, C, n, n_fft, hop
GEOMETRIES = [(3, 2, 6007, 256, 128), (2, 1, 6007, 256, 77), (4, 2, 129, 256, 128), (1, 1, 6007, 64, 32),
              (2, 2, 6007, 2048, 1024), (1, 1, 20000, 16384, 8192)]
WIDE = np.array([2, 3, 40, 100], dtype=np.int32)                        # n_fft 256: bins 0, 1 and 100 .. 128 lie in no band


def third_octaves(n_fft):
    from deep_audio_mixer_amd import spectrum
    return spectrum.band_edges(SR, n_fft, 3)[0]


def stems_of(seed, S, n, C, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal((S, n, C)) + 0.05 * rng.standard_normal((1, n, C))).astype(dtype)


def f32_values(a):
    """The gains the definition uses are float32 values: tables that hold such values make the consequences exact."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize('case', range(len(GEOMETRIES)))
def test_unit_gains_give_back_the_sum(case):
    S, C, n, n_fft, hop = GEOMETRIES[case]
    x = stems_of(300 + case, S, n, C)
    edges = third_octaves(n_fft)
    out = ref.render(x, np.ones((len(edges) - 1, S, 1)), 1.0, edges, n_fft, hop)
    want = x.astype(np.float64).sum(0).T
    worst = float(np.abs(out - want).max())
    print('identity S %d C %d n %d n_fft %d hop %d: largest deviation %.3g' % (S, C, n, n_fft, hop, worst))
    assert out.shape == (C, n) and worst <= 1e-12


def test_constant_gains_are_a_broadband_mix():
    S, C, n = 3, 2, 6007
    x = stems_of(311, S, n, C)
    g = f32_values(np.random.default_rng(5).uniform(0.5, 1.5, (S, 1)))
    out = ref.render(x, np.broadcast_to(g[None], (3, S, 1)), g, WIDE, 256, 128)
    worst = float(np.abs(out - gref.mix(x, g).T).max())
    print('constant gains over [2, 3, 40, 100] and as fill: largest deviation from sum g_s x_s %.3g' % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize('hop', (128, 77, 32))
def test_gain_steps_hold_inside_the_windows(hop):
    S, C, n, W, n_fft = 4, 2, 6007, 5, 256
    x = stems_of(312, S, n, C)
    g = f32_values(np.random.default_rng(6).uniform(0.5, 1.5, (S, W)))
    edges = third_octaves(n_fft)
    out = ref.render(x, np.broadcast_to(g[None], (len(edges) - 1, S, W)), g, edges, n_fft, hop)
    keep = ref.interior(n, W, n_fft)
    d = np.abs(out - gref.mix(x, g).T)
    print('gain steps, hop %d: %d of %d samples inside their window to %.3g; largest deviation near the borders %.3g'
          % (hop, keep.sum(), n, d[:, keep].max(), d[:, ~keep].max()))
    assert keep.sum() == 4983 and float(d[:, keep].max()) <= 1e-12


def test_nan_rule():
    S, C, n, W, n_fft, hop = 3, 2, 6007, 3, 256, 128
    x = stems_of(313, S, n, C)
    rng = np.random.default_rng(7)
    gains = rng.uniform(0.5, 1.5, (3, S, W))
    fill = rng.uniform(0.5, 1.5, (S, W))
    gains[0, 1, 2] = gains[2, 0, 0] = gains[1, 2, 1] = np.nan
    gains[1, 1, 0] = np.inf                                             # not finite: the fill as well
    fill[2, 1] = fill[0, 2] = np.nan                                    # (a NaN gain over a NaN fill: 0)
    out = ref.render(x, gains, fill, WIDE, n_fft, hop)
    g2, f2 = ref.substituted(gains, fill)
    assert g2[1, 2, 1] == 0.0 and g2[0, 1, 2] == fill[1, 2] and g2[1, 1, 0] == fill[1, 0] and np.isfinite(g2).all()
    assert np.isfinite(out).all() and np.array_equal(out, ref.render(x, g2, f2, WIDE, n_fft, hop))


def test_two_band_case_closes_the_loop():
    x, y, a, b = bref.two_band_case()
    edges = third_octaves(256)
    assert len(edges) - 1 == 18
    gains = bref.solve_bands(bref.moments(x, y, 1, 256, 128, edges))[0]
    broad_gains, broad_residual = gref.solve(gref.moments(x, y, 1))[:2]
    share = ref.residual_share(y, ref.render(x, gains, broad_gains, edges, 256, 128))
    silent = ref.residual_share(y, ref.render(x, gains, 0.0, edges, 256, 128))
    print('two-band case: the render of the fitted band gains leaves %.3g of the mix against a broadband residual of %.3g '
          '(%.3g of it); with fill = 0: %.3g' % (share, broad_residual[0], share / broad_residual[0], silent))
    assert share <= 1e-3 * float(broad_residual[0])


def test_ctypes_table_has_the_bandmix_entries():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 33
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_bandmix_\w+)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        found[m.group(2)] = (m.group(1), [a.strip() for a in m.group(3).split(',')])
    assert set(found) == {'dam_bandmix_workspace_bytes', 'dam_bandmix_render'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        assert argtypes == [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args], name
    source = open(os.path.join(ROOT, 'deep-audio-mixer_amd', 'csrc', 'dam_bandmix.hip')).read()
    for name in found:
        assert re.search(r'extern "C" (int|int64_t) %s\(' % name, source), name
    assert 'rendering the fitted band gains to audio' not in header     # the band fit's "not covered" clause is gone


def test_host_side_argument_checks():
    import torch
    from deep_audio_mixer_amd import gainfit, ops
    S, n, C, B, W = 4, 1000, 2, 18, 3
    ok = ((S, n, C), (B, S, W), (), 256, 128)
    assert ops.bandmix_check_shapes(*ok) == (S, n, C, B, W, 256, 128)
    assert ops.bandmix_check_shapes((S, n, C), (B, S, W), (S, 1), 256, None)[5:] == (256, 128)
    for fill_shape in ((), (S,), (S, 1), (S, W)):
        ops.bandmix_check_shapes((S, n, C), (B, S, W), fill_shape, 256, 77)

    def bad(stems=(S, n, C), gains=(B, S, W), fill=(), n_fft=256, hop=128):
        return stems, gains, fill, n_fft, hop
    for args in (bad(stems=(0, n, C)), bad(stems=(9, n, C), gains=(B, 9, W)), bad(stems=(S, n, 3)), bad(stems=(S, n, 0)),
                 bad(stems=(S, n)), bad(stems=(S, 128, C)),                                 # n <= n_fft / 2
                 bad(n_fft=100), bad(n_fft=32), bad(n_fft=32768), bad(hop=0), bad(hop=129), bad(hop=-1),
                 bad(gains=(B, W)), bad(gains=(B, S + 1, W)), bad(gains=(0, S, W)), bad(gains=(65, S, W)), bad(gains=(B, S, 0)),
                 bad(gains=(B, S, n + 1)),
                 bad(fill=(W,)), bad(fill=(S, 2)), bad(fill=(1, W)), bad(fill=(S, W, 1)),
                 bad(gains=(B, S, 9))):                                                     # 8 frames: a window without a frame
        with pytest.raises(ValueError):
            ops.bandmix_check_shapes(*args)
    for args in (bad(n_fft=256.0), bad(hop=64.0), bad(n_fft=True)):
        with pytest.raises(TypeError):
            ops.bandmix_check_shapes(*args)
    x = torch.zeros((S, n, C))
    edges = third_octaves(256)
    g = torch.ones((len(edges) - 1, S, W), dtype=torch.float64)
    with pytest.raises(ValueError):                                     # a table of another band count
        gainfit.render_band_gains(x, g[:5], n_fft=256, edges=edges)
    with pytest.raises(ValueError):
        gainfit.render_band_gains(x, g, n_fft=256, edges=np.array([0, 5, 5, 9]))
    with pytest.raises(ValueError):
        gainfit.render_band_gains(x, g, n_fft=256, hop=200, edges=edges)
    with pytest.raises(TypeError):
        gainfit.render_band_gains(x, g, n_fft=256, edges=edges, fill='broadband')
    with pytest.raises(TypeError):
        gainfit.render_band_gains(x, g.numpy(), n_fft=256, edges=edges)
    if not torch.cuda.is_available():                                   # what is well-formed still needs the GPU
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.render_band_gains(x, g, n_fft=256, edges=edges)


def test_evaluator_switch_needs_the_band_fit():
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator.__new__(LoudnessEvaluator)
    ev.sr = SR
    assert set(ev.BAND_FIT_DEFAULTS) == {'n_fft', 'hop', 'fraction', 'f_lo', 'f_hi', 'pool', 'ridge', 'align'}
    assert ev._band_render_args(False, False) is None and ev._band_render_args(False, True) is None
    assert ev._band_render_args(True, True) == 'broadband' and ev._band_render_args({}, {'n_fft': 256}) is None
    assert ev._band_render_args({'fill': 0}, True) == 0.0 and ev._band_render_args({'fill': 'broadband'}, True) == 'broadband'
    for render, fit in ((True, False), ({'fill': 1.0}, False), ({'fil': 1.0}, True), ({'fill': 'unit'}, True),
                        ({'fill': None}, True), ({'fill': True}, True)):
        with pytest.raises(ValueError):
            ev._band_render_args(render, fit)
    # every whole-song method refuses it before a file is read or a byte uploaded (the evaluator has no dataset here)
    with pytest.raises(ValueError, match='needs band_fit'):
        ev.process_song_tracks({}, {}, 'song', band_render=True)
    with pytest.raises(ValueError, match='needs band_fit'):
        ev.process_song('/nonexistent', 'song', band_render=True)
    with pytest.raises(ValueError, match='needs band_fit'):
        ev.process_songlist('/nonexistent', ['song'], band_render={'fill': 1.0})
