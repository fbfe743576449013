"""CPU: the numpy definition of the true-peak meter (tests/_truepeak_ref.py) -- the properties of its interpolator, two
known answers, homogeneity, and the phase form against zero-stuffing + np.convolve -- and the taps the library exports
(dam_true_peak_taps_host is a host function: no GPU needed).  Every test prints its largest observed error."""
import ctypes

import numpy as np

import _truepeak_ref as tp

N = 44100


def test_tap_properties():
    h = tp.taps()
    assert h.shape == (49,) and h.dtype == np.float64
    assert h[24] == 1.0
    for m in range(1, 7):
        assert h[24 + 4 * m] == 0.0 and h[24 - 4 * m] == 0.0
    assert np.array_equal(h, h[::-1])
    # the closed form itself, where it is not pinned: np.sinc leaves ~4e-17 at the integer arguments
    k = np.arange(49)
    formula = np.sinc((k - 24) / 4.0) * 0.5 * (1.0 - np.cos(2.0 * np.pi * k / 48.0))
    print('taps vs the unpinned closed form: max diff %.3g (bound 1e-15)' % np.abs(h - formula).max())
    assert np.abs(h - formula).max() <= 1e-15
    sums = [np.abs(h[24 + p + 4 * np.arange(-6, 6)]).sum() for p in (1, 2, 3)]
    print('sum |h_p| per phase: %s (the GPU tolerance assumes < 2.2)' % sums)
    assert max(sums) < 2.2


def test_known_answers():
    n = np.arange(N)
    for name, x, want_sample_db, want_tp_db in (
            ('fs/4 at 45 degrees', np.sin(2 * np.pi * n / 4 + np.pi / 4), -3.0103, 0.1035),
            ('997 Hz full scale', np.sin(2 * np.pi * 997 * n / 44100.0), 0.0, 0.0051)):
        got_tp, got_sp = tp.to_db(tp.true_peak(x))[0], tp.to_db(tp.sample_peak(x))[0]
        print('%s: sample peak %.6f dBFS, true peak %.6f dBTP (expected %.4f, bound 1e-3 dB)' % (name, got_sp, got_tp, want_tp_db))
        assert abs(got_tp - want_tp_db) <= 1e-3
        assert got_sp == tp.to_db(np.abs(x).max())
        assert abs(got_sp - want_sample_db) < 1e-4


def test_true_peak_is_at_least_the_sample_peak_and_homogeneous():
    rng = np.random.default_rng(5)
    worst = 0.0
    for n in (1, 5, 6, 7, 12, 13, 4097):
        x = rng.standard_normal((n, 2))
        t = tp.true_peak(x)
        assert (t >= tp.sample_peak(x)).all()
        for a in (0.37, 3.0, 1e-3):
            worst = max(worst, np.abs(tp.true_peak(a * x) / (a * t) - 1.0).max())
    print('homogeneity: max relative deviation %.3g (bound 1e-15)' % worst)
    assert worst <= 1e-15
    assert tp.true_peak(np.zeros(100))[0] == 0.0 and tp.to_db(tp.true_peak(np.zeros(100)))[0] == -np.inf


def test_phase_form_equals_zero_stuffing():
    rng = np.random.default_rng(6)
    h = tp.taps()
    worst = 0.0
    for n in (1, 5, 6, 7, 12, 13, 1000):
        x = rng.standard_normal(n)
        up = np.zeros(4 * n)
        up[::4] = x
        full = np.convolve(up, h)[24: 24 + 4 * n].reshape(n, 4)          # output positions 0 .. 4n-1, delay removed
        y = tp.phases(x, h)
        assert np.array_equal(full[:, 0], x)                              # phase 0 is the identity
        worst = max(worst, np.abs(full[:, 1:].T - y).max() / np.abs(x).max())
    # two float64 sums of the same 12 products in different orders: each within 12 * 2^-53 * sum|h_p| * max|x| of the exact value
    print('phase form vs zero-stuffing + convolve: max diff %.3g of max|x| (bound 6e-15)' % worst)
    assert worst <= 2 * 12 * 2.0 ** -53 * 2.2


def test_gain_ramp_and_limiter_restatement():
    x = np.arange(10, dtype=np.float32).reshape(10, 1) + 1
    got = tp.apply_gains(x, [1.0, 2.0, 3.0])                      # hold 10 // 3 = 3 samples, the last gain to the end
    assert got[:, 0].tolist() == [1, 2, 3, 8, 10, 12, 21, 24, 27, 30]
    lim = tp.limit_gains([2.0, 0.1, 5.0], [[0.5, 1.0], [0.5, 1.0], [0.0, 0.0]], 0.5)
    assert lim.tolist() == [0.5, 0.1, 5.0]


def test_library_taps(dam_lib):
    h = (ctypes.c_double * 49)()
    assert dam_lib.dam_true_peak_taps_host(h) == 0
    got = np.array(list(h))
    want = tp.taps()
    print('library taps vs numpy: max diff %.3g (bound 1e-15)' % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-15
    assert got[24] == 1.0 and np.array_equal(got, got[::-1])
    assert all(got[24 + 4 * m] == 0.0 for m in range(-6, 7) if m)
    assert dam_lib.dam_true_peak_taps_host(None) == -1
    assert dam_lib.dam_true_peak_tile_samples() >= 64 and dam_lib.dam_true_peak_max_blocks() >= 1
