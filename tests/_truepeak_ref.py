"""numpy float64 restatement of the true-peak meter (include/dam_hip.h: dam_true_peak_batch, dam_peak_limit_gains) -- the
interpolator, the three interpolated phases, the peak and the gain clamp, written from the definition and nothing else.
The GPU tests compare the kernel with it; tests/test_truepeak_ref_cpu.py checks it against zero-stuffing + np.convolve and
against two known answers.

    h[k] = sinc((k - 24) / 4) * 0.5 * (1 - cos(2 pi k / 48)),  k = 0..48        (h[24] = 1, h[24 +- 4m] = 0)
    y_p[i] = sum_{j=-6..5} x[i - j] * h[24 + p + 4 j],  p = 1, 2, 3,  i in [0, n),  x = 0 outside [0, n)
    TP = max(max |x|, max |y_p|)

y_p[i] is the value 4x oversampling puts p/4 of the way from x[i] to x[i+1]; it reads x[i-5 .. i+6].  Parity with
libebur128 or the ITU conformance table is not claimed: this filter is the project's own."""
import numpy as np

N_TAPS, CENTRE, FACTOR = 49, 24, 4


def taps():
    """The 49 taps in closed form.  sinc of a non-zero integer is set to exactly 0 (np.sinc leaves ~4e-17) and the upper
    half mirrors the lower, so the filter is exactly symmetric."""
    k = np.arange(CENTRE + 1)
    h = np.sinc((k - CENTRE) / 4.0) * 0.5 * (1.0 - np.cos(2.0 * np.pi * k / 48.0))
    h[(CENTRE - k) % FACTOR == 0] = 0.0
    h[CENTRE] = 1.0
    return np.concatenate([h, h[-2::-1]])


def phases(x, h=None):
    """x: float64 [n] -> y [3, n], y[p-1][i] = y_p[i]; the products are added in the order j = -6 .. 5."""
    h = taps() if h is None else np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    xp = np.concatenate([np.zeros(6), x, np.zeros(6)])           # x[i] = xp[i + 6]
    y = np.zeros((3, n))
    for p in (1, 2, 3):
        for j in range(-6, 6):
            y[p - 1] += xp[6 - j: 6 - j + n] * h[CENTRE + p + FACTOR * j]
    return y


def apply_gains(x, gains):
    """x [n, channels] (any float dtype) times the gain ramp of one track: (double)x[n] * gains[min(n // (n_samples //
    n_gains), n_gains - 1)] -- the product the batched loudness meter and dam_gain_ramp_apply form."""
    x = np.asarray(x).astype(np.float64)
    g = np.atleast_1d(np.asarray(gains, dtype=np.float64))
    n = x.shape[0]
    idx = np.minimum(np.arange(n) // (n // len(g)), len(g) - 1)
    return x * g[idx][:, None]


def sample_peak(x):
    """x [n] or [n, channels] -> max |x| per channel, float64 [channels]."""
    x = np.asarray(x).astype(np.float64)
    return np.abs(x.reshape(x.shape[0], -1)).max(axis=0)


def true_peak(x, h=None, gains=None):
    """x [n] or [n, channels] -> linear true peak per channel, float64 [channels]."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    x = apply_gains(x, gains) if gains is not None else x.astype(np.float64)
    return np.array([max(np.abs(x[:, c]).max(), np.abs(phases(x[:, c], h)).max()) for c in range(x.shape[1])])


def to_db(peak):
    """20 log10; silence reads -inf."""
    with np.errstate(divide='ignore'):
        return 20.0 * np.log10(np.asarray(peak, dtype=np.float64))


def limit_gains(gains, peaks, ceiling_lin):
    """dam_peak_limit_gains: min(gains[i], ceiling_lin / max(peaks[i])); a zero peak leaves the gain alone (ceiling / 0 = inf)."""
    gains = np.asarray(gains, dtype=np.float64)
    peaks = np.asarray(peaks, dtype=np.float64).reshape(len(gains), -1)
    with np.errstate(divide='ignore'):
        return np.minimum(gains, ceiling_lin / np.max(peaks, axis=1))
