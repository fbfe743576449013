"""numpy float64 restatement of the alignment (include/dam_hip.h: dam_align_estimate / dam_align_shift) for the tests: the
mono signal, the direct cross-correlation (no FFT: the known answer), the framed cross-spectrum whose inverse transform is
that correlation, the two weightings, the estimate, the shift -- and the error bound of the device's float32 transforms,
propagated from the project's per-bin FFT bound EPS through the product, the weighting and the inverse transform."""
import math

import numpy as np

MAX_LAG = 4096
MAX_STEMS = 8
PHAT_FLOOR = 1e-2
WEIGHTINGS = {'plain': 0, 'phat': 1}
EPS = 2e-6            # the LDS FFT's bound per bin, relative to the frame's largest bin magnitude (tests/test_features_gpu.py,
                      # tests/test_spectrum_gpu.py hold the same transform to it)


def fft_size(max_lag):
    """N = max(64, 4 * 2^ceil(log2 L))."""
    assert 1 <= max_lag <= MAX_LAG
    p = 1
    while p < max_lag:
        p *= 2
    return max(64, 4 * p)


def mono(x):
    """[n, C] or [n] (float32 / float64) -> the float32 mono signal: (float)(((double)l + (double)r) * 0.5), or (float) of
    the single channel."""
    x = np.asarray(x)
    if x.ndim == 1:
        return x.astype(np.float32)
    if x.shape[1] == 1:
        return x[:, 0].astype(np.float32)
    assert x.shape[1] == 2
    return ((x[:, 0].astype(np.float64) + x[:, 1].astype(np.float64)) * 0.5).astype(np.float32)


def correlation_direct(a, y, L):
    """R[l + L] = sum_p a[p] y[p + l], l in [-L, L], samples outside [0, n) zero: plain float64 dot products."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(a)
    assert len(y) == n
    R = np.zeros(2 * L + 1)
    for l in range(-L, L + 1):
        lo, hi = max(0, -l), min(n, n - l)
        if hi > lo:
            R[l + L] = float(np.dot(a[lo:hi], y[lo + l:hi + l]))
    return R


def frames(a, y, N):
    """-> (fa [T, N], fy [T, N]) float64: frame t of the stem holds a[t H + j] at j < H = N/2 and zeros above, frame t of
    the mix holds y[t H - N/4 + j], j < N; T = ceil(n / H)."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, H, Q = len(a), N // 2, N // 4
    T = -(-n // H)
    ap = np.concatenate([a, np.zeros(T * H - n)])
    yp = np.concatenate([np.zeros(Q), y, np.zeros(T * H + N - Q - n)])
    fa = np.zeros((T, N))
    fa[:, :H] = ap.reshape(T, H)
    fy = np.stack([yp[t * H:t * H + N] for t in range(T)])
    return fa, fy


def cross_spectrum(a, y, N):
    """-> (C [N/2 + 1] complex128 = sum_t conj(A'_t) Y'_t, beta [N/2 + 1]): beta bounds the error of the device's C, whose
    frames go through a float32 FFT good to EPS of the frame's largest bin magnitude pk per bin:
    beta[k] = sum_t EPS (pkA_t |Y_t[k]| + pkY_t |A_t[k]| + EPS pkA_t pkY_t)."""
    fa, fy = frames(a, y, N)
    A, Y = np.fft.rfft(fa, axis=1), np.fft.rfft(fy, axis=1)
    C = (np.conj(A) * Y).sum(axis=0)
    pa, py = np.abs(A).max(axis=1)[:, None], np.abs(Y).max(axis=1)[:, None]
    beta = (EPS * (pa * np.abs(Y) + py * np.abs(A) + EPS * pa * py)).sum(axis=0)
    return C, beta


def _bin_weights(N):
    c = np.full(N // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def weighted(C, weighting):
    """The spectrum whose inverse transform is the curve: C, or C / (|C| + PHAT_FLOOR * mean |C|)."""
    if weighting == 'plain':
        return C
    assert weighting == 'phat'
    mag = np.abs(C)
    return C / (mag + PHAT_FLOOR * mag.mean())


def curve(C, N, L, weighting):
    """c[l + L] = irfft(weighted C)[l + N/4], l in [-L, L]."""
    full = np.fft.irfft(weighted(C, weighting), N)
    return full[N // 4 - L:N // 4 + L + 1].copy()


def curve_bound(C, beta, N, weighting):
    """One number that bounds |device curve - curve| at every lag:
    plain  (1/N) sum_k c_k beta[k] + EPS (1/N) sum_k c_k |C[k]|   (the product's error, then the float32 inverse transform's,
           every output a sum of the N terms c_k |C[k]| / N);
    phat   the same with beta scaled by the weighting's Lipschitz constant 2 / (PHAT_FLOOR mean |C|) and |C| weighted."""
    ck = _bin_weights(N)
    if weighting == 'plain':
        return float((ck * beta).sum() / N + EPS * (ck * np.abs(C)).sum() / N)
    lip = 2.0 / (PHAT_FLOOR * np.abs(C).mean())
    return float(lip * (ck * beta).sum() / N + EPS * (ck * np.abs(weighted(C, 'phat'))).sum() / N)


def pick(c, L):
    """argmax |c| over l in [-L, L]; ties go to the smallest |l|, then to the negative lag -> l*."""
    mag = np.abs(c)
    best = None
    for l in range(-L, L + 1):
        key = (-mag[l + L], abs(l), l)
        if best is None or key < best[0]:
            best = (key, l)
    return best[1]


def parabola(y0, y1, y2):
    den = (y0 - 2.0 * y1) + y2
    return 0.5 * (y0 - y2) / den if den < 0.0 else 0.0


def estimate(c, L, Ea, Ey, weighting, silent=False):
    """-> dict(lag, frac, peak, sign, status, lead): lead = |c[l*]| less the largest |c| elsewhere."""
    if silent or not Ea > 0.0 or not Ey > 0.0:
        return dict(lag=0, frac=0.0, peak=math.nan, sign=0, status=0, lead=0.0)
    l = pick(c, L)
    mag = np.abs(c)
    y1 = mag[l + L]
    frac = parabola(mag[l + L - 1], y1, mag[l + L + 1]) if -L < l < L else 0.0
    others = np.delete(mag, l + L)
    peak = y1 if weighting == 'phat' else y1 / math.sqrt(Ea * Ey)
    return dict(lag=l, frac=frac, peak=peak, sign=1 if c[l + L] > 0.0 else -1, status=1, lead=float(y1 - others.max()))


def analyse(stem, mix, L, weighting, framed=True):
    """stem, mix [n, C] -> dict(curve [2 L + 1], bound, lag, frac, peak, sign, status, lead, Ea, Ey) of one (stem, mix) pair.
    framed=False takes the direct correlation for the plain curve (no FFT at all)."""
    a, y = mono(stem).astype(np.float64), mono(mix).astype(np.float64)
    N = fft_size(L)
    Ea, Ey = math.fsum((a * a).tolist()), math.fsum((y * y).tolist())
    C, beta = cross_spectrum(a, y, N)
    silent = not Ea > 0.0 or not Ey > 0.0 or not np.abs(C).max() > 0.0
    if silent:
        c, bound = np.zeros(2 * L + 1), 0.0
    else:
        c = correlation_direct(a, y, L) if (weighting == 'plain' and not framed) else curve(C, N, L, weighting)
        bound = curve_bound(C, beta, N, weighting)
    out = estimate(c, L, Ea, Ey, weighting, silent)
    out.update(curve=c, bound=bound, Ea=Ea, Ey=Ey)
    return out


def frac_bound(c, l, L, b):
    """|device frac - frac| where every |c| is off by at most b: numerator y0 - y2 moves by 2 b, denominator by 4 b.
    inf where the denominator could reach 0."""
    if not -L < l < L:
        return 0.0
    mag = np.abs(c)
    y0, y1, y2 = mag[l + L - 1], mag[l + L], mag[l + L + 1]
    num, den = abs(y0 - y2), abs((y0 - 2.0 * y1) + y2)
    if den <= 4.0 * b:
        return math.inf
    return 0.5 * (2.0 * b / (den - 4.0 * b) + num * 4.0 * b / (den * (den - 4.0 * b)))


def shift(x, lag):
    """x [S, n, C], lag [S] ints -> out[s, p] = x[s, p - lag[s]], zero fill: numpy slicing."""
    x = np.asarray(x)
    out = np.zeros_like(x)
    n = x.shape[1]
    for s, d in enumerate(lag):
        d = int(d)
        if d >= n or d <= -n:
            continue
        if d >= 0:
            out[s, d:] = x[s, :n - d]
        else:
            out[s, :n + d] = x[s, -d:]
    return out


def planted(n, delays, C=2, seed=0, dtype=np.float32, invert=()):
    """The tests' planted-delay input: S = len(delays) stems of white noise at 0.1 RMS and
    mix = sum_s g_s * (stem s delayed by delays[s], zero fill) + another stem that is not handed out + noise at 0.01 RMS,
    g_s = 0.7, or -0.7 for s in ``invert`` -> (stems [S, n, C] dtype, mix [n, C] float64)."""
    rng = np.random.default_rng(seed)
    S = len(delays)
    stems = (0.1 * rng.standard_normal((S + 1, n, C))).astype(dtype)
    g = np.array([-0.7 if s in invert else 0.7 for s in range(S)])
    mix = stems[S].astype(np.float64) + 0.01 * rng.standard_normal((n, C))
    delayed = shift(stems[:S].astype(np.float64), delays)
    for s in range(S):
        mix = mix + g[s] * delayed[s]
    return stems[:S], mix
