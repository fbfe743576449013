"""numpy float64 restatement of the band gain fit (include/dam_hip.h: dam_bandfit_moments / dam_bandfit_solve_grouped /
dam_bandfit_summary) for the tests.  The frames are the front-end's (the samples times the float32 periodic Hann table)
in float64 and their transform is numpy's float64 rfft -- or, to MEASURE what the device's float32 transform costs, float32
frames and scipy's float32 rfft; the moments are float64 sums; the solve is _gainfit_ref.solve band by band; the summary is the
definition in plain loops."""
import math

import numpy as np
import torch

import _gainfit_ref as gref


def frame_windows(n, W, hop):
    """[first frame of window w], w = 0 .. W (the last entry is T): frame t belongs to w(t) = min(min(t hop, n-1) // (n // W), W-1)."""
    T = 1 + n // hop
    w_of = [min(min(t * hop, n - 1) // (n // W), W - 1) for t in range(T)]
    first = [w_of.index(w) if w in w_of else None for w in range(W)]
    for w in range(W - 1, -1, -1):                      # a window without a frame starts where the next one does
        if first[w] is None:
            first[w] = first[w + 1] if w + 1 < W and first[w + 1] is not None else T
    return first + [T]


def hann(n_fft):
    return torch.hann_window(n_fft, dtype=torch.float32).numpy()


def frames(signal, n_fft, hop, transform='f64'):
    """One channel [n] -> the frames [T, n_fft] of torch.stft(center=True, pad_mode='reflect') with the float32 Hann table.
    'f64': the samples as they are times the table, in float64 (for float32 samples the products are exact).  'f32': what
    the device forms -- the samples rounded to float32, the products rounded to float32."""
    x = np.asarray(signal)
    x = x.astype(np.float32) if transform == 'f32' else x.astype(np.float64)
    n = x.shape[0]
    assert n > n_fft // 2
    padded = np.pad(x, n_fft // 2, mode='reflect')
    T = 1 + n // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    f = padded[idx] * hann(n_fft).astype(x.dtype)[None, :]
    assert f.dtype == x.dtype
    return f


def spectra(x, y, n_fft, hop, transform='f64'):
    """x [S, n, C], y [n, C] -> U [S + 1, C, T, n_fft/2 + 1] complex128: every channel of every signal on its own.
    transform 'f64': numpy's float64 rfft of the float64 frames; 'f32': scipy's float32 rfft of the float32 frames
    (complex64, widened afterwards) -- the same definition in the device's precision."""
    x, y = np.asarray(x), np.asarray(y)
    S, n, C = x.shape
    out = []
    for sig in list(x) + [y]:
        rows = []
        for c in range(C):
            f = frames(sig[:, c], n_fft, hop, transform)
            if transform == 'f32':
                import scipy.fft
                X = scipy.fft.rfft(f, axis=1)
                assert X.dtype == np.complex64
            else:
                X = np.fft.rfft(f, axis=1)
            X = X.astype(np.complex128)
            X[:, 0] = X[:, 0].real
            X[:, -1] = X[:, -1].real
            rows.append(X)
        out.append(rows)
    return np.array(out)


def moments(x, y, W, n_fft, hop, edges, transform='f64'):
    """-> M [B, W, S + 1, S + 1] float64: sum over the window's frames, the band's bins and the channels of c_k Re(conj(U_i) U_j)."""
    U = spectra(x, y, n_fft, hop, transform)
    n = np.asarray(x).shape[1]
    first = frame_windows(n, W, hop)
    edges = np.asarray(edges)
    B, nsig = len(edges) - 1, U.shape[0]
    ck = np.full(n_fft // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    M = np.zeros((B, W, nsig, nsig))
    for b in range(B):
        for w in range(W):
            cell = U[:, :, first[w]:first[w + 1], edges[b]:edges[b + 1]]
            weight = np.broadcast_to(ck[edges[b]:edges[b + 1]], cell.shape[1:]).reshape(-1)
            flat = cell.reshape(nsig, -1)
            G = (flat.real * weight) @ flat.real.T + (flat.imag * weight) @ flat.imag.T
            M[b, w] = 0.5 * (G + G.T)
    return M


def solve_bands(M, pool=0, ridge=0.0):
    """M [B, W, S + 1, S + 1] -> (gains [B, S, W], residual [B, W], target [B, W], status [B, W] int, cond [B, W])."""
    M = np.asarray(M, dtype=np.float64)
    B, W, U, _ = M.shape
    out = [gref.solve(M[b], pool, ridge) for b in range(B)]
    target = np.zeros((B, W))
    for b in range(B):
        for w in range(W):
            v0, v1 = max(0, w - pool), min(W - 1, w + pool)
            Y = M[b, v0, U - 1, U - 1]
            for v in range(v0 + 1, v1 + 1):
                Y = Y + M[b, v, U - 1, U - 1]
            target[b, w] = Y
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), target, np.stack([o[2] for o in out]),
            np.stack([o[3] for o in out]))


def summary(residual, target, status):
    """[B, W] each -> total [W]: sum_b r' Y / sum_b Y in ascending b; r' = residual where status > 0, else 1; Y = 0 adds nothing."""
    residual, target, status = np.asarray(residual, dtype=np.float64), np.asarray(target, dtype=np.float64), np.asarray(status)
    B, W = residual.shape
    total = np.full(W, np.nan)
    for w in range(W):
        num = den = 0.0
        for b in range(B):
            Y = float(target[b, w])
            if not Y > 0.0:
                continue
            rho = float(residual[b, w]) if status[b, w] > 0 else 1.0
            num = num + rho * Y
            den = den + Y
        if den > 0.0:
            total[w] = num / den
    return total


def moment_ratio(got, want):
    """largest |got_ij - want_ij| / sqrt(want_ii want_jj) over all cells; an entry whose scale is 0 must agree exactly."""
    got, want = np.asarray(got), np.asarray(want)
    d = np.sqrt(np.maximum(np.diagonal(want, axis1=-2, axis2=-1), 0.0))
    scale = d[..., :, None] * d[..., None, :]
    err = np.abs(got - want)
    assert np.all(err[scale == 0.0] == 0.0)
    return float((err[scale > 0.0] / scale[scale > 0.0]).max()) if np.any(scale > 0.0) else 0.0


def band_limited_noise(rng, n, sr, f_lo, f_hi, rms=0.1):
    """White noise whose whole-signal FFT is masked to f_lo .. f_hi, at ``rms``."""
    F = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / sr)
    F[(f < f_lo) | (f > f_hi)] = 0.0
    v = np.fft.irfft(F, n)
    return v * (rms / math.sqrt(float(np.mean(v * v))))


def two_band_case(n=6007, sr=44100, S=4, C=2, seed=11):
    """The meaning test's input: every stem is low + high (noise in 400 .. 1300 Hz and in 4500 .. 11000 Hz, 0.1 RMS each),
    stored as float32 with low32 = float32(low) and high32 = x - low32 (exact in float64); the mix gives every stem one gain
    a_s on its low part and another b_s on its high part -> (x float32 [S, n, C], y float64 [n, C], a [S], b [S])."""
    rng = np.random.default_rng(seed)
    low = np.array([[band_limited_noise(rng, n, sr, 400.0, 1300.0) for _ in range(C)] for _ in range(S)]).transpose(0, 2, 1)
    high = np.array([[band_limited_noise(rng, n, sr, 4500.0, 11000.0) for _ in range(C)] for _ in range(S)]).transpose(0, 2, 1)
    a, b = rng.uniform(0.5, 1.5, S), rng.uniform(0.5, 1.5, S)
    x = (low + high).astype(np.float32)
    low32 = low.astype(np.float32).astype(np.float64)
    high32 = x.astype(np.float64) - low32
    y = np.zeros((n, C))
    for s in range(S):
        y = y + a[s] * low32[s] + b[s] * high32[s]
    return x, y, a, b
