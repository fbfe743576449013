"""CPU: the numpy reference of the band gain fit (tests/_bandfit_ref.py) against known answers -- so that the GPU tests compare
the kernels with something that has itself been checked -- the new ctypes entries against the header, and the host-side
argument checks of gainfit.py and evaluation.py (no GPU is touched).

Figures of the reference (n_fft 256, hop 128, 44.1 kHz, _gainfit_ref.base_input at n = 6007):
  planted gains, W = 1, 8 octave bands of 1 .. 63 bins: back to 9.4e-15 in every band, cond(R) 5.1 .. 6.9, status 4;
  gain steps, W = 3: the frames that straddle a step limit the recovery to 2.7e-2 in gain, residual <= 1.2e-3 per band;
  one band over all bins / the time-domain moments: 192.17 .. 195.03 (n_fft sum(w^2) / hop = 192 but for the reflected edges);
  two-band case, 18 third-octave bands: the low gains back to 2.7e-4 in the bands inside 600 .. 1100 Hz, the high gains to
  6.6e-5 inside 5.5 .. 10 kHz; broadband residual 3.5e-2, band total 9.0e-7."""
import math
import os
import re

import numpy as np
import pytest

import _bandfit_ref as ref
import _gainfit_ref as gref

SR, NF, HOP, N = 44100, 256, 128, 6007


def band_edges(fraction, f_lo=25.0, f_hi=20000.0):
    from deep_audio_mixer_amd import spectrum
    return spectrum.band_edges(SR, NF, fraction, f_lo, f_hi)


def test_window_of_a_frame_is_the_gain_index_of_its_centre():
    from deep_audio_mixer_amd import ops
    assert ref.frame_windows(N, 5, HOP) == [0, 10, 19, 29, 38, 47]
    for n, W, hop in ((N, 5, HOP), (N, 1, 77), (129, 1, 128), (1000, 7, 33), (640, 5, 128), (1024, 4, 256), (6007, 46, 128)):
        assert ops.gainfit_band_frame_windows(n, W, hop) == ref.frame_windows(n, W, hop), (n, W, hop)
    assert ref.frame_windows(640, 5, 128) == [0, 1, 2, 3, 4, 6]         # hop divides n: the last frame is centred on sample n


def test_planted_gains_come_back_in_every_band():
    x, _, g = gref.base_input(np.float64, W=1)
    y = gref.mix(x, g)
    edges, centres = band_edges(1, 100.0)
    assert len(centres) == 8 and np.diff(edges).min() == 1 and np.diff(edges).max() == 63
    gains, residual, target, status, cond = ref.solve_bands(ref.moments(x, y, 1, NF, HOP, edges))
    worst = float(np.abs(gains - g[None]).max())
    print('planted gains, 8 octave bands: largest error %.3g, cond(R) %.2f .. %.2f' % (worst, cond.min(), cond.max()))
    assert worst <= 1e-12 and np.all(status == 4) and np.all(target > 0.0) and np.all(residual <= 1e-12)


def test_gain_steps_are_smeared_over_one_frame():
    """Documents the smear, claims no parity: frames reach n_fft / 2 samples over a window's borders."""
    x, y, g = gref.base_input(np.float64, W=3)
    edges, _ = band_edges(1, 100.0)
    gains, residual, _, status, _ = ref.solve_bands(ref.moments(x, y, 3, NF, HOP, edges))
    print('gain steps, W = 3: largest gain error %.3g, largest residual %.3g' % (np.abs(gains - g[None]).max(), residual.max()))
    assert np.all(status == 4) and float(residual.max()) < 5e-3


def test_one_band_over_all_bins_is_parseval():
    x, y, _ = gref.base_input(np.float64, W=1)
    Mb = ref.moments(x, y, 1, NF, HOP, [0, NF // 2 + 1])[0, 0]
    Mt = gref.moments(x, y, 1)[0]
    w = ref.hann(NF).astype(np.float64)
    factor = NF * float((w * w).sum()) / HOP
    ratio = Mb / Mt
    print('band moments / time-domain moments: %.2f .. %.2f (n_fft sum(w^2) / hop = %.2f)' % (ratio.min(), ratio.max(), factor))
    assert abs(factor - 192.0) < 1e-4 and np.all(np.abs(ratio / factor - 1.0) <= 0.03)
    assert np.array_equal(Mb, Mb.T)


def inside(edges, f_lo, f_hi):
    """the bands whose bins all lie within f_lo .. f_hi"""
    lo, hi = edges[:-1] * SR / NF, (edges[1:] - 1) * SR / NF
    return [b for b in range(len(edges) - 1) if lo[b] >= f_lo and hi[b] <= f_hi]


def check_two_band(gains, residual, target, status, a, b, edges, broadband, total):
    """The meaning test's assertions, shared with the GPU test: gains [B, S], the rest [B]; broadband, total scalars."""
    low, high = inside(edges, 600.0, 1100.0), inside(edges, 5500.0, 10000.0)
    assert len(low) >= 2 and len(high) >= 2
    ea, eb = float(np.abs(gains[low] - a[None]).max()), float(np.abs(gains[high] - b[None]).max())
    print('two bands: low gains to %.3g in bands %s, high gains to %.3g in bands %s; broadband residual %.3g, band total %.3g'
          % (ea, low, eb, high, broadband, total))
    assert ea <= 2e-3 and eb <= 2e-4
    assert total <= 1e-3 * broadband
    assert np.all(status[low + high] == gains.shape[1])
    return ea, eb


def test_two_band_case_needs_band_gains():
    x, y, a, b = ref.two_band_case()
    assert x.dtype == np.float32 and np.abs(a - b).max() > 0.3
    edges, centres = band_edges(3)
    assert len(centres) == 18
    gains, residual, target, status, _ = ref.solve_bands(ref.moments(x, y, 1, NF, HOP, edges))
    broadband = float(gref.solve(gref.moments(x, y, 1))[1][0])
    total = float(ref.summary(residual, target, status)[0])
    check_two_band(gains[:, :, 0], residual[:, 0], target[:, 0], status[:, 0], a, b, edges, broadband, total)
    assert broadband > 1e-2                                             # no scalar gain per stem explains this mix


def test_summary_rules():
    x, _, g = gref.base_input(np.float64, W=1)
    edges, _ = band_edges(1, 100.0)
    # silent bands: the mix's row and column zeroed in bands 5 .. 7 -- Y = 0 there adds nothing
    y = gref.mix(x, g)
    M = ref.moments(x, y, 1, NF, HOP, edges)
    M[5:, :, 4, :] = 0.0
    M[5:, :, :, 4] = 0.0
    gains, residual, target, status, _ = ref.solve_bands(M)
    assert status[:, 0].tolist() == [4] * 5 + [0] * 3 and np.all(target[5:] == 0.0) and np.all(np.isnan(residual[5:]))
    total = ref.summary(residual, target, status)
    want = float((residual[:5, 0] * target[:5, 0]).sum() / target[:5, 0].sum())
    assert abs(total[0] - want) <= 1e-15 * max(want, 1e-300) + 1e-30
    # a rank-deficient band: two identical stems, status -1 counts as unexplained
    t = x.copy()
    t[3] = t[0]
    yt = gref.mix(t, g)
    Mt = ref.moments(t, yt, 1, NF, HOP, edges)
    Mt[:, :, 3, :] = Mt[:, :, 0, :]                                     # (exactly dependent, as the device's moments are)
    Mt[:, :, :, 3] = Mt[:, :, :, 0]
    gains, residual, target, status, _ = ref.solve_bands(Mt)
    assert np.all(status == -1) and np.all(np.isnan(residual)) and np.all(target > 0.0)
    assert ref.summary(residual, target, status).tolist() == [1.0]
    mixed = status.copy()
    mixed[:4] = 4
    res = np.where(mixed > 0, 0.25, np.nan)
    want = (0.25 * target[:4, 0].sum() + target[4:, 0].sum()) / target[:, 0].sum()
    assert abs(ref.summary(res, target, mixed)[0] - want) <= 1e-15
    # status 0 with energy in the mix (every stem gated out): unexplained as well
    st0 = np.zeros_like(status)
    assert ref.summary(np.full_like(residual, np.nan), target, st0).tolist() == [1.0]
    # an all-silent mix: NaN
    gains, residual, target, status, _ = ref.solve_bands(ref.moments(x, np.zeros_like(y), 1, NF, HOP, edges))
    assert np.all(status == 0) and math.isnan(ref.summary(residual, target, status)[0])


def test_ctypes_table_has_the_bandfit_entries():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 30
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_bandfit_\w+)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        args = [a.strip() for a in m.group(3).split(',')] if m.group(3).strip() not in ('', 'void') else []
        found[m.group(2)] = (m.group(1), args)
    assert set(found) == {'dam_bandfit_tile_elements', 'dam_bandfit_workspace_bytes', 'dam_bandfit_moments',
                          'dam_bandfit_solve_grouped', 'dam_bandfit_summary'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        want = [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args]
        assert argtypes == want, name
    assert int(re.search(r'#define DAM_BANDFIT_SLAB_BYTES (\d+)', header).group(1)) == 128 << 20
    assert ops.GAINFIT_BAND_MAX_BANDS == 64
    csrc = os.path.join(ROOT, 'deep-audio-mixer_amd', 'csrc')
    exported = open(os.path.join(csrc, 'dam_bandfit.hip')).read() + open(os.path.join(csrc, 'dam_gainfit.hip')).read()
    for name in found:
        assert re.search(r'extern "C" (int|int64_t) %s\(' % name, exported), name


def test_host_side_argument_checks():
    import torch
    from deep_audio_mixer_amd import gainfit, ops
    x, y = torch.zeros((4, 1000, 2)), torch.zeros((1000, 2))
    edges = band_edges(3)[0]
    ok = dict(n_fft=NF, hop=HOP, edges=edges)
    assert ops.gainfit_band_check_shapes(x.shape, y.shape, 3, NF, None, 18) == (4, 1000, 2, 3, NF, HOP)
    for fn in (gainfit.band_moments, gainfit.fit_band_gains):
        for stems, mix, W, kw in (
                (x, y, 9, ok),                                          # 8 frames: a window without a frame
                (x, y, 0, ok), (x, y, -1, ok), (x, y, 1001, ok),
                (torch.zeros((9, 1000, 2)), y, 3, ok), (torch.zeros((4, 1000, 3)), torch.zeros((1000, 3)), 3, ok),
                (x, y[:999], 3, ok),
                (x, y, 3, dict(ok, n_fft=100)), (x, y, 3, dict(ok, n_fft=32)), (x, y, 3, dict(ok, n_fft=32768)),
                (x, y, 3, dict(ok, hop=0)),
                (x[:, :128], y[:128], 1, ok),                           # n <= n_fft / 2
                (x, y, 3, dict(ok, edges=np.arange(66, dtype=np.int32))),                  # 65 bands
                (x, y, 3, dict(ok, edges=np.array([0, 5, 5, 9]))), (x, y, 3, dict(ok, edges=np.array([0, 130]))),
                (x, y, 3, dict(ok, edges=np.array([3])))):
            with pytest.raises(ValueError):
                fn(stems, mix, W, **kw)
        for W, kw in ((2.0, ok), (3, dict(ok, n_fft=256.0)), (3, dict(ok, hop=1.5)), (3, dict(ok, edges=np.array([0.0, 4.0])))):
            with pytest.raises(TypeError):
                fn(x, y, W, **kw)
    for kw in (dict(pool=-1), dict(ridge=-1e-9), dict(ridge=float('nan'))):
        with pytest.raises(ValueError):
            gainfit.fit_band_gains(x, y, 3, **ok, **kw)
        with pytest.raises(ValueError):
            gainfit.solve_bands(torch.zeros((2, 3, 5, 5), dtype=torch.float64), **kw)
    with pytest.raises(TypeError):
        gainfit.fit_band_gains(x, y, 3, **ok, pool=1.5)
    for shape in ((3, 5, 5), (2, 3, 5, 4), (2, 3, 10, 10), (2, 3, 1, 1), (0, 3, 5, 5), (2, 0, 5, 5)):
        with pytest.raises(ValueError):
            gainfit.solve_bands(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        gainfit.fit_band_gains(x, y, 3, **ok, align=0)
    if not torch.cuda.is_available():                                   # what is well-formed still needs the GPU
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.fit_band_gains(x, y, 3, **ok)
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.solve_bands(torch.zeros((2, 3, 5, 5), dtype=torch.float64))
        with pytest.raises(RuntimeError, match='GPU only'):
            gainfit.band_residual_total(torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.float64),
                                        torch.zeros((2, 3), dtype=torch.int32))


def test_evaluator_switch_checks_its_keys():
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator.__new__(LoudnessEvaluator)                   # (the meter needs the library; the check does not)
    ev.sr = SR
    assert set(ev.BAND_FIT_DEFAULTS) == {'n_fft', 'hop', 'fraction', 'f_lo', 'f_hi', 'pool', 'ridge', 'align'}
    o = ev._band_fit_args(True)
    assert (o['n_fft'], o['hop'], o['pool'], o['ridge'], o['align']) == (4096, 2048, 0, 0.0, None)
    assert len(o['centres']) == len(o['edges']) - 1 >= 20
    o = ev._band_fit_args({'n_fft': 256, 'hop': 64, 'fraction': 1, 'f_lo': 100.0, 'pool': 2, 'ridge': 1e-6, 'align': 50})
    assert (o['n_fft'], o['hop'], o['pool'], o['ridge'], o['align'], len(o['centres'])) == (256, 64, 2, 1e-6, 50, 8)
    with pytest.raises(ValueError, match='unknown'):
        ev._band_fit_args({'nfft': 256})
    with pytest.raises(ValueError):
        ev._band_fit_args({'pool': -1})
    with pytest.raises(ValueError):
        ev._band_fit_args({'n_fft': 100})
    with pytest.raises(ValueError, match='unknown'):                    # a new keyword, not a new key of gain_fit
        ev._gain_fit_args({'n_fft': 256})


def test_songlist_passes_the_switch_and_averages_the_band_errors(monkeypatch):
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    ev = LoudnessEvaluator.__new__(LoudnessEvaluator)
    band_keys = ['sum_band_gain_error', 'random_band_gain_error', 'loudnorm_band_gain_error', 'mix_band_gain_error']
    seen = []

    def fake(base_dir, song_name, *args, **kw):
        seen.append((len(args), kw))
        row = {'song_name': song_name, 'sum_error': 1.0, 'random_error': 2.0, 'loudnorm_error': 3.0, 'mix_error': 4.0}
        if kw.get('band_fit'):
            row.update({k: 5.0 + len(song_name) for k in band_keys})
            if song_name == 'bcd':
                row['mix_band_gain_error'] = float('nan')
            row['loudnorm_band_gain_error'] = float('nan')
        return row
    monkeypatch.setattr(ev, 'process_song', fake)
    _, means = ev.process_songlist('.', ['a', 'bcd'])
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} and seen == [(6, {}), (6, {})]
    _, means = ev.process_songlist('.', ['a', 'bcd'], band_fit={'n_fft': 256})
    assert set(means) == {'sum_error', 'random_error', 'loudnorm_error', 'mix_error'} | set(band_keys)
    assert seen[2:] == [(6, {'band_fit': {'n_fft': 256}})] * 2
    assert means['sum_band_gain_error'] == 7.0 and means['mix_band_gain_error'] == 6.0
    assert math.isnan(means['loudnorm_band_gain_error'])
