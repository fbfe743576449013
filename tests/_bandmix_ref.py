"""numpy float64 restatement of the band-gain mixer (include/dam_hip.h: dam_bandmix_render) for the tests.  The frames, the Hann
table and the window of a frame are _bandfit_ref's; the transforms are numpy's float64 rfft / irfft -- or, to MEASURE what the
device's float32 arithmetic costs, float32 frames, scipy's float32 rfft / irfft, a float32 (complex64) mix spectrum and a float32
overlap-add.  The effective gain is rounded to float32 in both: that rounding is part of the definition, not of the arithmetic."""
import numpy as np

import _bandfit_ref as bref


def effective_gains(gains, fill, edges, n_fft, w):
    """gains [B, S, W], fill [S, W], window w -> e [S, n_fft/2 + 1] float64 holding float32 values: in the lowest band that
    holds the bin, gains[b][s][w] if finite, else fill[s][w] if finite, else 0; outside every band fill[s][w] if finite, else 0."""
    gains, fill, edges = np.asarray(gains, dtype=np.float64), np.asarray(fill, dtype=np.float64), np.asarray(edges)
    B, S, _ = gains.shape
    nbins = n_fft // 2 + 1
    f = np.where(np.isfinite(fill[:, w]), fill[:, w], 0.0)
    e = np.repeat(f[:, None], nbins, axis=1)
    taken = np.zeros(nbins, dtype=bool)
    for b in range(B):
        lo, hi = (int(min(max(v, 0), nbins)) for v in edges[b:b + 2])
        own = np.zeros(nbins, dtype=bool)
        own[lo:hi] = True
        own &= ~taken
        taken |= own
        g = np.where(np.isfinite(gains[b, :, w]), gains[b, :, w], f)
        e[:, own] = g[:, None]
    with np.errstate(over='ignore'):
        return e.astype(np.float32).astype(np.float64)


def substituted(gains, fill):
    """The tables the NaN rule stands for: (gains with fill, or 0, where they are not finite; fill with 0 where it is not)."""
    gains, fill = np.asarray(gains, dtype=np.float64), np.asarray(fill, dtype=np.float64)
    f = np.where(np.isfinite(fill), fill, 0.0)
    return np.where(np.isfinite(gains), gains, f[None]), f


def broadcast_fill(fill, S, W):
    return np.broadcast_to(np.asarray(fill, dtype=np.float64).reshape((S, -1) if np.ndim(fill) else (1, 1)), (S, W))


def render(x, gains, fill, edges, n_fft, hop, transform='f64'):
    """x [S, n, C], gains [B, S, W], fill a number, [S], [S, 1] or [S, W] -> out [C, n] float64 (holding float32 values for
    transform 'f32')."""
    x = np.asarray(x)
    S, n, C = x.shape
    gains = np.asarray(gains, dtype=np.float64)
    W = gains.shape[2]
    fill = broadcast_fill(fill, S, W)
    assert 1 <= hop <= n_fft // 2 < n
    first = bref.frame_windows(n, W, hop)
    T, M = first[-1], n_fft // 2
    assert all(first[w + 1] > first[w] for w in range(W))
    real = np.float32 if transform == 'f32' else np.float64
    E = np.empty((T, S, M + 1), dtype=real)
    for w in range(W):
        E[first[w]:first[w + 1]] = effective_gains(gains, fill, edges, n_fft, w).astype(real)[None]
    win = bref.hann(n_fft).astype(real)
    out = np.zeros((C, n))
    for c in range(C):
        Y = np.zeros((T, M + 1), dtype=np.complex64 if transform == 'f32' else np.complex128)
        for s in range(S):                                          # ascending s
            f = bref.frames(x[s, :, c], n_fft, hop, transform)
            if transform == 'f32':
                import scipy.fft
                X = scipy.fft.rfft(f, axis=1)
                assert X.dtype == np.complex64
            else:
                X = np.fft.rfft(f, axis=1)
            X[:, 0] = X[:, 0].real
            X[:, -1] = X[:, -1].real
            Y = Y + E[:, s, :] * X
            assert Y.dtype == (np.complex64 if transform == 'f32' else np.complex128)
        if transform == 'f32':
            import scipy.fft
            y = scipy.fft.irfft(Y, n_fft, axis=1)
            assert y.dtype == np.float32
        else:
            y = np.fft.irfft(Y, n_fft, axis=1)
        v = y * win[None, :]
        acc, env = np.zeros(n, dtype=real), np.zeros(n, dtype=real)
        for t in range(T):                                          # ascending t
            p0 = t * hop - M                                        # frame sample j lands on output sample p0 + j
            j0, j1 = max(0, -p0), min(n_fft, n - p0)
            if j1 > j0:
                acc[p0 + j0:p0 + j1] += v[t, j0:j1]
                env[p0 + j0:p0 + j1] += win[j0:j1] * win[j0:j1]
        assert acc.dtype == real
        ok = env > 1e-11
        out[c, ok] = acc[ok].astype(np.float64) / env[ok].astype(np.float64) if transform != 'f32' else (acc[ok] / env[ok])
    return out


def interior(n, W, n_fft):
    """Boolean [n]: the samples at least n_fft/2 inside their window, with no margin at the two ends of the signal."""
    seg, M = n // W, n_fft // 2
    keep = np.zeros(n, dtype=bool)
    for w in range(W):
        lo = 0 if w == 0 else w * seg + M
        hi = n if w == W - 1 else (w + 1) * seg - M
        if hi > lo:
            keep[lo:hi] = True
    return keep


def residual_share(mix, render_cn):
    """mix [n, C], render [C, n] -> the share of the mix's energy that (mix - render) holds."""
    mix = np.asarray(mix, dtype=np.float64)
    d = mix - np.asarray(render_cn, dtype=np.float64).T
    return float((d * d).sum() / (mix * mix).sum())
