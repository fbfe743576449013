"""CPU: the compressor's definition (tests/_compressor_ref.py) against known answers, the properties of its static curve, and
its chunked restatement (the kernel's parallel form, on the host) against the sequential loops.

Known answers with T = -24 dB, R = 4, W = 6 dB, 10 / 100 ms at 44.1 kHz; every margin is derived where it is used.
Chunked against sequential: the bound is TOL_Q of tests/_compressor_ref.py (8 u tau max(1, max c)); measured on the host
9e-14 dB against 8e-11."""
import math

import numpy as np
import pytest

import _compressor_ref as ref

SR = 44100
T, R, W, ATTACK_MS, RELEASE_MS = -24.0, 4.0, 6.0, 10.0, 100.0


@pytest.fixture(scope='module')
def constants():
    from deep_audio_mixer_amd import ops
    knee_start, a_att, a_rel, makeup = ops.compressor_constants(T, W, ATTACK_MS, RELEASE_MS, SR)
    assert makeup == 1.0 and knee_start == 10.0 ** (-27.0 / 20.0)
    assert a_att == math.exp(-1.0 / 441.0) and a_rel == math.exp(-1.0 / 4410.0)
    assert ops.compressor_constants(T, W, ATTACK_MS, RELEASE_MS, SR, makeup_db=6.0)[3] == 10.0 ** 0.3
    return knee_start, a_att, a_rel


def run(x, constants, **kw):
    knee_start, a_att, a_rel = constants
    return ref.compress(x, T, R, W, knee_start, a_att, a_rel, **kw)


def test_constant_input_settles_on_the_curve(constants):
    n = SR
    got = run(np.full(n, 0.5), constants)
    want = 0.75 * (20.0 * math.log10(0.5) - T)
    attack = int(ATTACK_MS * SR / 1000)
    print('q at the end %.9f dB (want %.9f); q after %d samples %.6f of it (want 1 - 1/e = %.6f)'
          % (got['q'][-1], want, attack, got['q'][attack - 1] / want, 1.0 - math.exp(-1.0)))
    assert abs(want - 13.48455) < 1e-5
    # the remainder after n samples of one pole: exp(-n / 441) = e^-100; roundings: a few ulp of 13.5
    assert abs(got['q'][-1] - want) < 1e-12
    # p jumps to c at once and stays, so q[i] = c (1 - aA^(i+1)): after attack_ms exactly 1 - 1/e, up to roundings
    assert abs(got['q'][attack - 1] / want - (1.0 - math.exp(-1.0))) < 1e-12
    assert np.all(got['p'] == got['c']) and got['n_over'] == n and got['max_reduction'] == got['q'][-1]
    assert np.allclose(got['out'][:, 0], 0.5 * 10.0 ** (-got['q'] / 20.0), rtol=1e-14, atol=0.0)


def test_release_decays_with_the_slower_pole(constants):
    knee_start, a_att, a_rel = constants
    x = np.concatenate([np.full(SR // 2, 0.5), np.zeros(SR // 2)])
    q = run(x, constants)['q']
    ratio = q[-1] / q[-2]
    print('q[i+1] / q[i] at the end of the silence: %.12f (max(aA, aR) = %.12f)' % (ratio, max(a_att, a_rel)))
    # q = u aR^i + v aA^i: the ratio tends to the larger pole as (aA / aR)^i = exp(-i (1/441 - 1/4410)) -> e^-45 after 0.5 s
    assert abs(ratio - max(a_att, a_rel)) < 1e-12
    assert np.all(np.diff(q[SR // 2 + 2000:]) < 0.0)


def test_input_under_the_knee_passes_bitwise(constants):
    rng = np.random.default_rng(5)
    x = 0.004 * rng.standard_normal((20000, 2))
    got = run(x, constants)
    print('largest |x| %.5f against knee_start %.5f; n_over %d, %d samples differ (bound 0)'
          % (np.abs(x).max(), constants[0], got['n_over'], int((got['out'] != x).sum())))
    assert np.abs(x).max() < constants[0]
    assert got['n_over'] == 0 and got['max_reduction'] == 0.0 and np.all(got['q'] == 0.0) and np.array_equal(got['out'], x)
    y = run(x.astype(np.float32), constants, makeup=2.0, pre_gain=1.5)
    assert np.array_equal(y['out'], x.astype(np.float32).astype(np.float64) * 1.5 * 2.0)


def test_alternating_sine_is_levelled(constants):
    t = np.arange(4 * SR)
    level = np.where((t // SR) % 2 == 0, 10.0 ** (-10.0 / 20.0), 10.0 ** (-30.0 / 20.0))
    x = level * np.sin(2.0 * np.pi * 1000.0 * t / SR)
    got = run(x, constants)
    q = got['q']
    loud = np.concatenate([q[SR // 2: SR], q[2 * SR + SR // 2: 3 * SR]])
    quiet_end = max(q[2 * SR - 1], q[4 * SR - 1])
    print('loud sections, second half: q in [%.4f, %.4f] dB (want 10.5 within 0.1); q at the end of the quiet sections %.3g dB'
          % (loud.min(), loud.max(), quiet_end))
    # c at a peak = 0.75 (-10 + 24) = 10.5 dB; between the rectified peaks, 22 samples apart, p droops by 1 - aR^22 = 0.5 %
    # = 0.05 dB, and the sampled peak of a 1 kHz sine at 44.1 kHz is within cos(pi / 44.1) = 0.25 % = 0.02 dB of the true one
    assert loud.max() <= 10.5 and loud.min() >= 10.4
    # the quiet sections peak at -30 dBFS, under the knee's start at -27: c = 0, q decays by e^-10 per second of 100 ms release
    assert np.all(got['c'][SR + 1: 2 * SR] == 0.0)
    assert quiet_end < 10.5 * math.exp(-10.0) * 2.0
    gain_db = 20.0 * np.log10(np.abs(got['out'][2 * SR - 12: 2 * SR, 0]).max() / np.abs(x[2 * SR - 12: 2 * SR]).max())
    assert abs(gain_db) < 1e-3


def test_curve_properties(constants):
    knee_start = constants[0]
    lo, hi = 10.0 ** ((T - W / 2) / 20.0), 10.0 ** ((T + W / 2) / 20.0)
    # continuous at the knee's start (c -> 0) and at its end (c -> slope W / 2, the hard curve there)
    just_over = np.nextafter(knee_start, 1.0)
    ends = ref.curve(np.array([knee_start, just_over, hi * (1 - 1e-12), hi * (1 + 1e-12)]), T, R, W, knee_start)
    print('curve at the knee ends: %r' % (ends.tolist(),))
    assert ends[0] == 0.0 and 0.0 <= ends[1] < 1e-12
    assert abs(ends[2] - 0.75 * 3.0) < 1e-9 and abs(ends[3] - 0.75 * 3.0) < 1e-9 and abs(lo - knee_start) < 1e-17
    # c >= 0 everywhere, monotone, directly above knee_start included
    d = np.concatenate([knee_start * (1.0 + np.arange(1, 2000) * 2.0 ** -52), np.geomspace(1e-6, 4.0, 20001)])
    c = ref.curve(d, T, R, W, knee_start)
    assert np.all(c >= 0.0) and np.all(np.diff(c[1999:]) >= -1e-13)
    # W = 0 is the hard knee: 0 up to the threshold, slope (level - T) above
    ks0 = 10.0 ** (T / 20.0)
    d = np.array([ks0 * 0.5, ks0, ks0 * 2.0, 1.0])
    c0 = ref.curve(d, T, R, 0.0, ks0)
    assert c0[0] == 0.0 and c0[1] == 0.0 and abs(c0[2] - 0.75 * 20.0 * math.log10(2.0)) < 1e-12 and abs(c0[3] - 18.0) < 1e-12
    # R = inf: slope 1, the output level stays at the threshold
    ci = ref.curve(np.array([1.0]), T, float('inf'), 0.0, ks0)
    assert ci[0] == 24.0


@pytest.mark.parametrize('K', [64, 256, 1024])
def test_chunked_form_against_sequential(constants, K):
    knee_start, a_att, a_rel = constants
    n = 40000
    worst = 0.0
    for name, x in (('am noise', ref.am_noise(n, 1, seed=1)),
                    ('bursts', ref.bursts_on_a_bed(n, 1, seed=2, boundaries=[K, 2 * K, 3 * K, 10 * K, 20000, 20001]))):
        c = ref.curve(np.abs(x[:, 0]), T, R, W, knee_start)
        p, q = ref.ballistics(c, a_att, a_rel)
        pc, qc = ref.ballistics_chunked(c, a_att, a_rel, K)
        tol = ref.tol_q(ATTACK_MS * 1e-3 * SR, RELEASE_MS * 1e-3 * SR, c.max())
        dq, dp = np.abs(q - qc).max(), np.abs(p - pc).max()
        over = float((np.abs(x[:, 0]) > knee_start).mean())
        print('K %d, %s: max |dq| %.3g dB, max |dp| %.3g dB (bound %.3g); %.0f %% of the samples over the knee start, max c %.2f dB'
              % (K, name, dq, dp, tol, 100 * over, c.max()))
        assert c.max() > 5.0 and dq <= tol and dp <= tol
        worst = max(worst, dq / tol)
    assert worst < 1.0
