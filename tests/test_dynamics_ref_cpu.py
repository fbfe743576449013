"""CPU: the numpy definition of the time-resolved loudness readings (tests/_dynamics_ref.py) against a brute-force form --
every window summed directly from y^2, percentiles from np.sort -- against the four minimum-requirement signals of EBU Tech
3342 and against a steady sine, whose momentary and short-term loudness must read what the integrated meter reads."""
import numpy as np
import pytest

import _dynamics_ref as ref
from oracle import loudness_ref


def brute_force_power(y, h, w):
    """p_i = sum_c G_c sum(y_c^2 over the w hops from hop i) / (w h)."""
    H = y.shape[0] // h
    return np.array([sum(ref.G[c] * np.sum(np.square(y[i * h:(i + w) * h, c])) for c in range(y.shape[1])) / (w * h)
                     for i in range(H - w + 1)])


def brute_force_lra(p):
    l = ref.lufs(p)
    kept = p[l >= -70.0]
    kept = kept[ref.lufs(kept) >= ref.lufs(kept.mean()) - 20.0]
    q = np.sort(ref.lufs(kept))
    n = len(q)
    return q[int(round((n - 1) * 0.95))] - q[int(round((n - 1) * 0.10))], n


@pytest.mark.parametrize('rate,ch', [(48000, 2), (22050, 1), (44100, 5)])
def test_windows_and_lra_against_brute_force(rate, ch):
    rng = np.random.default_rng(rate + ch)
    n = 7 * rate + 123                                                 # not a multiple of the hop
    x = rng.standard_normal((n, ch)) * np.exp(-np.arange(n) / (1.2 * rate))[:, None] * 0.3
    d = ref.dynamics(x, rate)
    y = ref.kweighted(x, rate)
    h = ref.hop_length(rate)
    assert d['hop_energies'].shape == (ch, n // h) and d['short_term'].shape == (n // h - 29,)
    for w, key in ((4, 'momentary'), (30, 'short_term')):
        want = brute_force_power(y, h, w)
        err = np.max(np.abs(10.0 ** ((d[key] + 0.691) / 10.0) / want - 1.0))
        print('%s power, rate %d, %d ch: max rel diff %.3g (bound 1e-12)' % (key, rate, ch, err))
        assert err < 1e-12
    lra, kept = brute_force_lra(d['short_term_power'])
    print('LRA %.9f LU (brute force %.9f), %d windows kept' % (d['lra'], lra, kept))
    assert kept == d['stats'][4] and abs(d['lra'] - lra) < 1e-9 and d['lra'] > 1.0
    assert d['short_term_max'] == d['short_term'].max() and d['momentary_max'] == d['momentary'].max()


def test_percentile_index_is_rounded_rank():
    for n in range(1, 400):
        for P in (10, 95):
            assert ((n - 1) * P + 50) // 100 == int(np.floor((n - 1) * P / 100.0 + 0.5))
    # n = 5 -> 6 moves the 95 % index from the last value to ... still the last; the 10 % index moves at n = 6
    assert [((n - 1) * 10 + 50) // 100 for n in (5, 6)] == [0, 1] and [((n - 1) * 95 + 50) // 100 for n in (5, 6)] == [4, 5]


def test_curve_stats_edge_cases():
    s = ref.curve_stats(np.full(7, 1e-3))
    assert s[0] == 0.0 and s[1] == s[2] == s[5] and s[4] == 7
    s = ref.curve_stats(np.zeros(4))
    assert s[0] == 0.0 and np.isnan(s[1]) and np.isnan(s[2]) and np.isnan(s[3]) and s[4] == 0 and s[5] == -np.inf
    s = ref.curve_stats(np.full(3, ref.P_ABS * 0.5))                    # entirely under the absolute gate
    assert s[4] == 0 and np.isnan(s[3]) and np.isfinite(s[5])
    s = ref.curve_stats(np.array([1.0] + [1e-4] * 40))                  # gate 0.01 * 0.0245: the relative gate leaves the 1.0
    assert s[4] == 1 and s[0] == 0.0 and s[1] == s[2] == ref.lufs(1.0)
    assert ref.lufs(ref.P_ABS) == -70.0


@pytest.mark.parametrize('case', range(4))
def test_tech3342_minimum_requirements(case):
    levels, want = ref.TECH3342[case]
    d = ref.dynamics(ref.tech3342_signal(levels), 44100)
    margin = ref.gate_margin(d['short_term_power'])
    print('Tech 3342 signal %d: LRA %.6f LU (required %g +- 1), %d windows kept, gate margin %.3g'
          % (case + 1, d['lra'], want, int(d['stats'][4]), margin))
    assert abs(d['lra'] - want) <= 1.0                                   # the standard's tolerance
    assert abs(d['lra'] - want) < 1e-3 and d['stats'][4] == ref.TECH3342_KEPT[case]
    assert margin > 1e-9


def test_steady_sine_reads_the_integrated_loudness():
    rate = 44100
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(10 * rate) / rate)
    d = ref.dynamics(x, rate)
    integrated = loudness_ref.integrated_loudness(x, rate)
    m, s = d['momentary'][10:], d['short_term'][10:]                    # past the filter's onset
    print('997 Hz full scale: momentary %.4f .. %.4f, short-term %.4f .. %.4f, integrated %.4f LUFS'
          % (m.min(), m.max(), s.min(), s.max(), integrated))
    # a window of T seconds holds a non-integer number of cycles: the mean of sin^2 over it is 1/2 -+ at most 1 / (2 w T)
    ripple = lambda T: 10.0 * np.log10(1.0 + 1.0 / (2.0 * np.pi * 997.0 * T))
    assert np.abs(m - integrated).max() < ripple(0.4) + 1e-4 and np.abs(s - integrated).max() < ripple(3.0) + 1e-4
    assert abs(integrated + 3.0524) < 1e-4 and d['lra'] < 1e-3


def test_profile_error():
    rng = np.random.default_rng(5)
    R = rng.uniform(-40.0, -10.0, (4, 50))
    assert ref.profile_error(R, R) == (0.0, 50)
    assert ref.profile_error(R, R + 3.0)[0] < 1e-13                     # a level offset is no profile change
    C = R.copy()
    C[0] += 4.0                                                          # one stem 4 dB up: |3| + 3 |-1| over 4 stems
    assert abs(ref.profile_error(R, C)[0] - 1.5) < 1e-12
    C[1, :10] = -np.inf
    R2 = R.copy()
    R2[2, 5:20] = -80.0
    assert ref.profile_error(R2, C)[1] == 30
    err, count = ref.profile_error(np.full((4, 3), -90.0), C[:, :3])
    assert np.isnan(err) and count == 0
