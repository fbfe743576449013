"""CPU: the numpy definition of the look-ahead true-peak limiter (tests/_limiter_ref.py) -- the guarantee g <= r, the
regions it must leave untouched, the shape of the gain around one impulse and between two close peaks, and what it buys on
the bed-plus-bursts song (tests/_limiter_inputs.py) against the static clamp.  The figures asserted here come from the
definition, not from the kernel.  Every test prints its largest observed figure beside its bound.

g <= r holds for the exact mean of L+1 values that are each <= r.  The definition's g is that mean in float64: L additions
and one division, each rounded once, so it can exceed the exact mean -- and, where all L+1 terms equal r, r itself -- by a
relative (L+1) * 2^-53 at the most (observed: 1 ulp at L = 2, where (m + m + m) / 3 rounds up).  ``slack`` is that bound;
with it the guarantee reads g <= r * (1 + slack), 5e-15 at L = 40."""
import numpy as np
import pytest

import _limiter_inputs as li
import _limiter_ref as lr
import _truepeak_ref as tpref
from oracle import loudness_ref as ref

CEILING = 10.0 ** (-1.0 / 20.0)
def slack(L):
    return (L + 1) * 2.0 ** -53


REACH = 5                                            # the interpolator's reach: |y_p[i]| is non-zero from 5 samples before a sample


def noisy_with_bursts(n, channels, seed):
    """Noise under the ceiling with a few stretches well over it."""
    rng = np.random.default_rng(seed)
    x = 0.2 * rng.standard_normal((n, channels))
    for start in (0, n // 3, n // 3 + 50, n - 7):
        x[start:start + 6] *= 12.0
    return x


@pytest.mark.parametrize('L,H', [(1, 1), (2, 3), (40, 160)])
def test_gain_never_exceeds_what_a_sample_asks_for(L, H):
    x = noisy_with_bursts(3000, 2, 5)
    o = lr.limit(x, CEILING, L, H)
    worst = float((o['g'] / o['r'] - 1.0).max())
    print('L %d H %d: max (g / r - 1) %.3g (bound %.3g), min gain %.4f, %d of %d limited'
          % (L, H, worst, slack(L), o['min_gain'], o['n_limited'], len(x)))
    assert o['min_gain'] < 0.5 and worst <= slack(L)
    # the hold: g[i] <= r[k] for every k in [i - H, i]
    for k in range(1, H + 1):
        assert (o['g'][k:] <= o['r'][:-k] * (1.0 + slack(L))).all()


@pytest.mark.parametrize('L,H', [(1, 1), (7, 20), (40, 160)])
def test_untouched_regions_are_bitwise(L, H):
    n = 6000
    rng = np.random.default_rng(8)
    x = (0.1 * rng.standard_normal((n, 2))).astype(np.float32)                 # 6 sigma stays under the ceiling
    x[2500:2504] *= 40.0
    o = lr.limit(x, CEILING, L, H, pre_gain=1.25)
    over = np.flatnonzero(o['d'] > CEILING)
    assert len(over) and over.min() > 2400 and over.max() < 2600
    near = np.zeros(n, dtype=bool)                                   # a demand over the ceiling within [i - H - L, i + 2 L]
    for k in over:
        near[max(0, k - 2 * L): k + H + L + 1] = True
    far = ~near
    print('L %d H %d: %d samples far from every demand over the ceiling; %d of them with g != 1 (bound 0)'
          % (L, H, far.sum(), int((o['g'][far] != 1.0).sum())))
    assert far.sum() > n // 2
    assert (o['g'][far] == 1.0).all()
    assert np.array_equal(o['out'][far], o['xs'][far])
    assert o['n_limited'] == int((o['g'] < 1.0).sum()) <= near.sum()


def test_single_impulse():
    L, H, n, i0 = 40, 160, 4000, 1500
    ceiling = 10.0 ** (-6.0 / 20.0)
    x = np.zeros(n)
    x[i0] = 1.0
    o = lr.limit(x, ceiling, L, H)
    g, r = o['g'], o['r']
    print('impulse: r[i0] %.6f, g[i0] %.6f (bound: equal), first g < 1 at %d (bound >= %d), last at %d'
          % (r[i0], g[i0], np.flatnonzero(g < 1.0).min(), i0 - L - REACH - L, np.flatnonzero(g < 1.0).max()))
    assert r[i0] == ceiling and g[i0] == o['min_gain'] and abs(g[i0] / r[i0] - 1.0) <= slack(L)
    assert (g[:i0 - L - REACH - L] == 1.0).all()
    assert (np.diff(g[:i0 + 1]) <= 0.0).all()                        # the attack falls ...
    assert (np.diff(g[i0:]) >= 0.0).all()                            # ... and the release rises, monotonically
    assert g[-1] == 1.0
    assert tpref.true_peak(o['out'])[0] <= ceiling * (1.0 + 1e-12)


def test_gain_does_not_rise_between_two_close_peaks():
    L, H, n = 40, 160, 4000
    x = np.zeros(n)
    x[1500], x[1500 + H - 1] = 2.0, 2.0
    o = lr.limit(x, CEILING, L, H)
    between = o['g'][1500:1500 + H]
    print('two peaks %d apart: gain between them %.6f .. %.6f (bound: constant at r = %.6f)'
          % (H - 1, between.min(), between.max(), o['r'][1500]))
    assert (np.diff(between) <= 0.0).all() and between.max() <= o['r'][1500] * (1.0 + slack(L))
    # further apart than H + L the gain recovers in between, though not fully
    x = np.zeros(n)
    x[1500], x[1500 + H + 3 * L] = 2.0, 2.0
    g = lr.limit(x, CEILING, L, H)['g']
    assert g[1500:1500 + H + 3 * L].max() > g[1500]


def test_bed_plus_bursts_song():
    mix = li.unit_mix(li.burst_song())
    at_target = ref.normalize_loudness(mix.T, ref.integrated_loudness(mix.T, li.SR), -20.0)            # [n, channels]
    peak = tpref.true_peak(at_target).max()
    static = at_target * min(1.0, CEILING / peak)
    L, H = lr.samples(5.0, li.SR), lr.samples(20.0, li.SR)
    o = lr.limit(at_target, CEILING, L, H)
    over_db = tpref.to_db(tpref.true_peak(o['out']).max() / CEILING)
    static_lufs, limited_lufs = ref.integrated_loudness(static, li.SR), ref.integrated_loudness(o['out'], li.SR)
    print('at -20 LUFS the mix is %.3f dB over the ceiling; static clamp %.3f LUFS, limiter (L %d, H %d) %.3f LUFS: %.3f LU '
          'louder (bound 3); limited share %.4f; true peak %.3g dB over the ceiling (bound 1e-3)'
          % (tpref.to_db(peak / CEILING), static_lufs, L, H, limited_lufs, limited_lufs - static_lufs, o['n_limited'] / li.N, over_db))
    assert (L, H) == (40, 160)
    assert over_db <= 1e-3
    assert limited_lufs - static_lufs >= 3.0
    assert (o['g'] <= o['r'] * (1.0 + slack(L))).all()
