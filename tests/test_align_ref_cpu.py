"""CPU: the numpy reference of the alignment (tests/_align_ref.py) against known answers that need no FFT, the header's
constants against the reference's, and the package's host-side argument checks -- so that the GPU tests compare the kernels
with something that has itself been checked."""
import math
import os
import re

import numpy as np
import pytest

import _align_ref as ref


def test_fft_size_table():
    assert [ref.fft_size(L) for L in (1, 2, 15, 16, 17, 64, 65, 2048, 2049, 4096)] == \
        [64, 64, 64, 64, 128, 256, 512, 8192, 16384, 16384]
    for L in (1, 16, 17, 100, 4096):
        assert ref.fft_size(L) // 4 >= L                                 # every lag asked for is free of wrap-around


@pytest.mark.parametrize('n', [1, 7, 8, 9, 100, 1000])
@pytest.mark.parametrize('N', [16, 64, 256])
def test_framed_sum_is_the_direct_correlation(n, N):
    """irfft(sum_t conj(A'_t) Y'_t)[l + N/4] = sum_p a[p] y[p + l] for every lag in [-N/4, N/4], whatever n is: within
    1e-12 sqrt(E_a E_y)."""
    rng = np.random.default_rng(1000 * N + n)
    a, y = rng.standard_normal(n), rng.standard_normal(n)
    L = N // 4
    C, _ = ref.cross_spectrum(a, y, N)
    framed = ref.curve(C, N, L, 'plain')
    direct = ref.correlation_direct(a, y, L)
    worst = float(np.abs(framed - direct).max()) / math.sqrt(float(a @ a) * float(y @ y))
    print('n %d N %d: largest |framed - direct| = %.3g sqrt(Ea Ey)' % (n, N, worst))
    assert worst <= 1e-12
    # the direct sum itself, spelt out for one lag
    l = min(3, L)
    assert abs(direct[l + L] - sum(a[p] * y[p + l] for p in range(n) if 0 <= p + l < n)) <= 1e-12 * max(1.0, abs(direct[l + L]))


L0, N_PLANTED = 64, 3001


@pytest.mark.parametrize('weighting', ['plain', 'phat'])
@pytest.mark.parametrize('d', [-L0, -17, 0, 5, L0])
def test_planted_delay_comes_back_exactly(weighting, d):
    stems, mix = ref.planted(N_PLANTED, [d], seed=3)
    r = ref.analyse(stems[0], mix, L0, weighting)
    print('%s d %d: lag %d frac %.3f peak %.3f lead %.3g, bound %.3g' % (weighting, d, r['lag'], r['frac'], r['peak'], r['lead'], r['bound']))
    assert r['lag'] == d and r['sign'] == 1 and r['status'] == 1 and r['lead'] > 2.0 * r['bound']
    assert abs(r['frac']) <= 0.5 and (abs(d) < L0 or r['frac'] == 0.0)
    if weighting == 'plain':                                            # ... and the direct sum agrees, with no FFT in it
        q = ref.analyse(stems[0], mix, L0, 'plain', framed=False)
        assert q['lag'] == d and abs(q['peak'] - r['peak']) <= 1e-12
        assert 0.4 < r['peak'] < 0.7                                    # 0.7 E_a / sqrt(E_a (0.49 + 1 + 0.01) E_a) = 0.57


@pytest.mark.parametrize('weighting', ['plain', 'phat'])
def test_inverted_polarity_and_silence(weighting):
    stems, mix = ref.planted(N_PLANTED, [9], seed=4, invert=(0,))
    r = ref.analyse(stems[0], mix, L0, weighting)
    assert (r['lag'], r['sign'], r['status']) == (9, -1, 1)
    for a, y in ((np.zeros_like(stems[0]), mix), (stems[0], np.zeros_like(mix))):
        r = ref.analyse(a, y, L0, weighting)
        assert (r['lag'], r['frac'], r['sign'], r['status']) == (0, 0.0, 0, 0) and math.isnan(r['peak'])
        assert np.all(r['curve'] == 0.0)


def test_tie_rule_on_a_periodic_signal():
    n, L, p0 = 200, 16, 100
    a = np.zeros(n)
    a[p0] = 1.0

    def lag_of(positions):
        y = np.zeros(n)
        y[positions] = 1.0                                              # R[l] = 1 exactly at l = position - p0
        return ref.estimate(ref.correlation_direct(a, y, L), L, 1.0, float(len(positions)), 'plain')['lag']
    assert lag_of([p0 + 3 + 6 * k for k in range(-3, 3)]) == -3          # period 6: lags -15, -9, -3, 3, 9, 15 -> |3|, negative
    assert lag_of([p0 + 6 * k for k in range(-2, 3)]) == 0               # lag 0 is among them
    assert lag_of([p0 + 2, p0 - 3]) == 2                                 # the smaller |lag| before the negative one
    assert lag_of([p0 + 5, p0 + 11]) == 5
    assert ref.pick(np.ones(2 * L + 1), L) == 0
    # equal magnitude, opposite sign: still a tie
    y = np.zeros(n)
    y[p0 - 4], y[p0 + 4] = 1.0, -1.0
    r = ref.estimate(ref.correlation_direct(a, y, L), L, 1.0, 2.0, 'plain')
    assert (r['lag'], r['sign']) == (-4, 1)


def band_limited(t, rng_seed=11):
    rng = np.random.default_rng(rng_seed)
    f = rng.uniform(0.002, 0.02, 40)                                    # cycles per sample: all below 0.02 of the rate
    ph = rng.uniform(0, 2 * np.pi, 40)
    env = 0.5 - 0.5 * np.cos(2 * np.pi * np.clip(t / 4000.0, 0.0, 1.0))  # silent at both ends: the delay cuts nothing off
    return env * np.sin(2 * np.pi * f[:, None] * t[None, :] + ph[:, None]).sum(axis=0)


HALF_SAMPLE_MARGIN = 0.02


def test_parabola_recovers_a_half_sample_delay():
    """a band-limited signal (40 sines below 0.02 of the rate under a Hann envelope), delayed by 5.5 and by 5.25 samples by
    evaluating it there.  The parabola through three samples of the correlation peak is not the peak's true shape: on this
    input the reference itself is off by 7.5e-11 (5.5: symmetric) and 1.5e-4 (5.25) samples; HALF_SAMPLE_MARGIN = 0.02 samples is
    that error with two orders of margin, and still a fiftieth of the half sample the integer lag leaves open."""
    t = np.arange(4000, dtype=np.float64)
    a = band_limited(t)
    for delay in (5.5, 5.25):
        y = band_limited(t - delay)
        r = ref.estimate(ref.correlation_direct(a, y, 32), 32, float(a @ a), float(y @ y), 'plain')
        err = abs(r['lag'] + r['frac'] - delay)
        print('delay %.2f: lag %d frac %+.6f, |error| %.3g samples' % (delay, r['lag'], r['frac'], err))
        assert r['lag'] in (5, 6) and err <= HALF_SAMPLE_MARGIN and r['peak'] > 0.999


def test_shift_is_numpy_slicing():
    x = np.arange(2 * 7 * 2, dtype=np.float32).reshape(2, 7, 2) + 1.0
    out = ref.shift(x, [2, -3])
    assert np.array_equal(out[0, 2:], x[0, :5]) and np.all(out[0, :2] == 0.0)
    assert np.array_equal(out[1, :4], x[1, 3:]) and np.all(out[1, 4:] == 0.0)
    assert np.all(ref.shift(x, [7, -7]) == 0.0) and np.all(ref.shift(x, [12, -12]) == 0.0)
    assert np.array_equal(ref.shift(x, [0, 0]), x)
    six = ref.shift(x, [6, -6])
    assert np.array_equal(six[0, 6], x[0, 0]) and np.array_equal(six[1, 0], x[1, 6]) and np.count_nonzero(six) == 4


def test_header_constants_and_ctypes_table():
    from conftest import ROOT
    from deep_audio_mixer_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'dam_hip.h')).read()
    assert int(re.search(r'#define DAM_ABI_VERSION (\d+)', header).group(1)) == _lib.EXPECTED_ABI >= 28
    assert float.fromhex(re.search(r'#define DAM_ALIGN_PHAT_FLOOR (\S+)', header).group(1)) == ref.PHAT_FLOOR == 1e-2
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define DAM_ALIGN_(PLAIN|PHAT) (\d+)', header)}
    assert codes == ref.WEIGHTINGS == ops.ALIGN_WEIGHTINGS
    assert ops.ALIGN_MAX_LAG == ref.MAX_LAG and ops.ALIGN_MAX_STEMS == ref.MAX_STEMS
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = {}
    for m in re.finditer(r'\b(int|int64_t)\s+(dam_align_\w+)\s*\(([^;]*?)\)\s*;', code, flags=re.S):
        args = [a.strip() for a in m.group(3).split(',')] if m.group(3).strip() not in ('', 'void') else []
        found[m.group(2)] = (m.group(1), args)
    assert set(found) == {'dam_align_max_lag', 'dam_align_frames_per_block', 'dam_align_fft_size', 'dam_align_workspace_bytes',
                          'dam_align_estimate', 'dam_align_shift'}
    kinds = {'int': _lib.c_i, 'int64_t': _lib.c_i64, 'double': _lib.c_d}
    for name, (res, args) in found.items():
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[res], name
        assert argtypes == [_lib.c_p if '*' in a else kinds[a.split()[0]] for a in args], name


def test_library_geometry_without_gpu(dam_lib):
    """The getters are host code: they answer without a GPU, and as the reference does."""
    from deep_audio_mixer_amd import ops
    assert dam_lib.dam_align_max_lag() == ref.MAX_LAG and dam_lib.dam_align_frames_per_block() >= 1
    for L in (1, 16, 17, 64, 100, 2048, 2049, 4096):
        assert dam_lib.dam_align_fft_size(L) == ref.fft_size(L) == ops.align_geometry(L)[2]
    for L in (0, -1, 4097):
        assert dam_lib.dam_align_fft_size(L) == 0 and dam_lib.dam_align_workspace_bytes(2, 1000, L) == 0
    F = dam_lib.dam_align_frames_per_block()
    for S, n, L in ((1, 1, 16), (3, 32 * F, 16), (3, 32 * F + 1, 16), (8, 100000, 2048)):
        N = ref.fft_size(L)
        blocks = -(-(-(-n // (N // 2))) // F)
        assert dam_lib.dam_align_workspace_bytes(S, n, L) == S * (blocks + 1) * (2 * (N // 2 + 1) + 2) * 8
    assert dam_lib.dam_align_workspace_bytes(1, 1000, 4096) > dam_lib.dam_align_workspace_bytes(1, 1000, 2048) * 2
    for S, n in ((0, 100), (9, 100), (2, 0)):
        assert dam_lib.dam_align_workspace_bytes(S, n, 16) == 0


def test_host_side_argument_checks():
    import torch
    from deep_audio_mixer_amd import align, gainfit
    x, y = torch.zeros((4, 100, 2)), torch.zeros((100, 2))
    for stems, mix, max_lag in ((x[0], y, 5), (torch.zeros((9, 100, 2)), y, 5), (torch.zeros((0, 100, 2)), y, 5),
                                (torch.zeros((4, 100, 3)), torch.zeros((100, 3)), 5), (x, y[:99], 5), (x, y[:, :1], 5),
                                (x, y, 0), (x, y, 4097), (x, y, -1), (torch.zeros((4, 0, 2)), torch.zeros((0, 2)), 5)):
        for fn in (align.cross_correlation, align.estimate_lag):
            with pytest.raises(ValueError):
                fn(stems, mix, max_lag)
    with pytest.raises(TypeError):
        align.estimate_lag(x, y, 5.0)
    with pytest.raises(ValueError, match='weighting'):
        align.estimate_lag(x, y, 5, weighting='scot')
    for fn in (align.cross_correlation, align.estimate_lag):
        with pytest.raises(RuntimeError, match='GPU only'):              # well-formed CPU tensors: no CPU fallback
            fn(x, y, 5)
    with pytest.raises(RuntimeError, match='GPU only'):
        align.shift_tracks(x, 3)
    with pytest.raises(RuntimeError, match='GPU only'):
        align.shift_tracks(x, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        align.shift_tracks(x, 1.5)
    with pytest.raises(ValueError):
        gainfit.fit_gains(x, y, 4, align=0)
    with pytest.raises(TypeError):
        gainfit.fit_gains(x, y, 4, align=2.5)
    with pytest.raises(RuntimeError, match='GPU only'):
        gainfit.fit_gains(x, y, 4, align=8)
    assert align.lag_from_ms(10, 44100) == 441 and align.lag_from_ms(0.001, 8000) == 1 and align.lag_from_ms(92.88, 44100) == 4097
    for bad in ((0, 44100), (-1, 44100), (10, 0)):
        with pytest.raises(ValueError):
            align.lag_from_ms(*bad)
    with pytest.raises(TypeError):
        align.lag_from_ms('10', 44100)
    assert align.WEIGHTINGS == ('phat', 'plain')
