"""numpy float64 restatement of the time-resolved loudness readings (include/dam_hip.h: dam_loudness_window_power,
dam_loudness_curve_stats, dam_loudness_profile_error), written from the definitions there and nothing else.  The GPU tests
compare the kernels with it; tests/test_dynamics_ref_cpu.py checks it against a brute-force form (direct slices of y^2,
np.sort) and against the four minimum-requirement signals of EBU Tech 3342.

    hop energies   h = round(0.1 rate), H = n // h, e[c][j] = sum(y^2 over [j h, (j+1) h)) / h, y the K-weighted row
    window power   p_i = (sum_c G_c sum_{k<w} e[c][i+k]) / w, k then c ascending; l = -0.691 + 10 log10(p)
    curve stats    absolute gate p >= P_ABS, relative gate p >= 0.01 mean(absolutely gated), 10 % / 95 % order statistics at
                   ((n-1) P + 50) // 100 of the values that pass both
    profile error  mean |(C - mean_s C) - (R - mean_s R)| over the windows where every stem of both is >= -70 LUFS

The K-weighting is the oracle's (oracle.loudness_ref.kweight_coefficients + scipy.signal.lfilter), as in the other loudness
tests.  Sums that the kernels take in a stated order (thread t takes t, t + 256, ..., then a tree) are taken in that order."""
import numpy as np
import scipy.signal

from oracle.loudness_ref import kweight_coefficients

G = (1.0, 1.0, 1.0, 1.41, 1.41)
P_ABS = float.fromhex('0x1.f791ec6e1d5b7p-24')           # 10^((-70 + 0.691) / 10), the header's literal
THREADS = 256


def apply_gains(x, gains):
    """x [n, channels] times the gain ramp of one track: (double)x[n] * gains[min(n // (n_samples // n_gains), n_gains - 1)]
    (tests/_truepeak_ref.apply_gains: the product the batched meter forms as it loads a sample)."""
    x = np.asarray(x).astype(np.float64)
    g = np.atleast_1d(np.asarray(gains, dtype=np.float64))
    n = x.shape[0]
    idx = np.minimum(np.arange(n) // (n // len(g)), len(g) - 1)
    return x * g[idx][:, None]


def kweighted(x, rate, gains=None):
    """x [n] or [n, channels] -> K-weighted float64 [n, channels]."""
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    y = apply_gains(x, gains) if gains is not None else x.astype(np.float64)
    for c in kweight_coefficients(rate):
        y = scipy.signal.lfilter(c[:3], c[3:], y, axis=0)
    return y


def hop_length(rate):
    return int(round(0.1 * rate))


def hop_energies(x, rate, gains=None):
    """-> e [channels, H]."""
    y = kweighted(x, rate, gains)
    h = hop_length(rate)
    H = y.shape[0] // h
    return np.array([[np.sum(np.square(y[j * h:(j + 1) * h, c])) / h for j in range(H)] for c in range(y.shape[1])])


def window_power(e, w):
    """e [channels, H] -> p [H - w + 1]."""
    e = np.asarray(e, dtype=np.float64)
    W = e.shape[1] - w + 1
    p = np.zeros(W)
    for c in range(e.shape[0]):
        s = np.zeros(W)
        for k in range(w):
            s += e[c, k:k + W]
        p += G[c] * s
    return p / float(w)


def lufs(p):
    with np.errstate(divide='ignore', invalid='ignore'):
        return -0.691 + 10.0 * np.log10(np.asarray(p, dtype=np.float64))


def strided_tree_sum(v):
    """Sum of v in the kernels' order: partial t = v[t] + v[t + 256] + ... (ascending), then red[t] += red[t + w] for
    w = 128, 64, ..., 1."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-len(v) // THREADS)
    padded = np.zeros(rows * THREADS)
    padded[:len(v)] = v
    red = np.zeros(THREADS)
    for row in padded.reshape(rows, THREADS):
        red += row
    w = THREADS // 2
    while w >= 1:
        red[:w] += red[w:2 * w]
        w //= 2
    return red[0]


def gates(p):
    """-> (m, kept): the mean of the absolutely gated powers and the boolean mask of those that pass both gates."""
    p = np.asarray(p, dtype=np.float64)
    absolute = p >= P_ABS
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.float64(strided_tree_sum(np.where(absolute, p, 0.0))) / np.float64(absolute.sum())
        kept = absolute & (p >= 0.01 * m)                 # m NaN (empty absolute gate): nothing passes
    return m, kept


def gate_margin(p):
    """Smallest relative distance of any p_i from either gate (inf where there is no gate to be near)."""
    p = np.asarray(p, dtype=np.float64)
    m, _ = gates(p)
    margin = np.min(np.abs(p - P_ABS) / P_ABS)
    if m == m:
        margin = min(margin, np.min(np.abs(p[p >= P_ABS] - 0.01 * m) / (0.01 * m)))
    return margin


def curve_stats(p):
    """p [W] -> float64 [6]: LRA, l(lo), l(hi), Gamma_r, n, max l."""
    p = np.asarray(p, dtype=np.float64)
    m, kept = gates(p)
    q = np.sort(p[kept])
    n = len(q)
    if n:
        lo, hi = q[((n - 1) * 10 + 50) // 100], q[((n - 1) * 95 + 50) // 100]
        l_lo, l_hi = float(lufs(lo)), float(lufs(hi))
        lra = l_hi - l_lo
    else:
        l_lo = l_hi = np.nan
        lra = 0.0
    return np.array([lra, l_lo, l_hi, float(lufs(m)) - 20.0, float(n), float(lufs(p.max()))])


def profile_error(R, C):
    """R, C float64 [S, W] (LUFS) -> (err, active windows)."""
    R, C = np.asarray(R, dtype=np.float64), np.asarray(C, dtype=np.float64)
    S, W = R.shape
    active = np.all(R >= -70.0, axis=0) & np.all(C >= -70.0, axis=0)
    per_window = np.zeros(W)
    for i in np.nonzero(active)[0]:
        mr = mc = 0.0
        for s in range(S):
            mr += R[s, i]
            mc += C[s, i]
        mr, mc = mr / S, mc / S
        a = 0.0
        for s in range(S):
            a += abs((C[s, i] - mc) - (R[s, i] - mr))
        per_window[i] = a
    count = int(active.sum())
    with np.errstate(invalid='ignore'):
        return float(np.float64(strided_tree_sum(per_window)) / np.float64(count * S)), count


def dynamics(x, rate, gains=None):
    """One track [n] or [n, channels] -> dict of the readings Meter.loudness_dynamics_batch returns, plus 'hop_energies',
    'short_term_power' and 'stats' (curve_stats of the short-term power)."""
    e = hop_energies(x, rate, gains)
    pm, ps = window_power(e, 4), window_power(e, 30)
    stats = curve_stats(ps)
    return {'hop_energies': e, 'momentary': lufs(pm), 'short_term': lufs(ps), 'short_term_power': ps, 'stats': stats,
            'momentary_max': float(lufs(pm.max())), 'short_term_max': stats[5], 'lra': stats[0], 'lra_low': stats[1],
            'lra_high': stats[2]}


# EBU Tech 3342, minimum-requirement signals: 1 kHz stereo sine, 20 s per segment at these dBFS levels -> required LRA
TECH3342 = (((-20.0, -30.0), 10.0), ((-20.0, -15.0), 5.0), ((-40.0, -20.0), 20.0), ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0))
TECH3342_KEPT = (371, 371, 371, 627)                      # windows that pass both gates


def tech3342_signal(levels, rate=44100, seconds=20.0):
    n = int(rate * seconds)
    tone = np.sin(2.0 * np.pi * 1000.0 * np.arange(n * len(levels)) / rate)
    amp = np.repeat(10.0 ** (np.asarray(levels) / 20.0), n)
    return np.stack([amp * tone, amp * tone], axis=1)
