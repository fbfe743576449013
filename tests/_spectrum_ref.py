"""Reference for the band spectrum and the spectral-balance error (include/dam_hip.h, "Band spectrum"): the definition
restated in numpy float64, independent of the library -- and the error bounds the GPU tests hold the kernels to.

What is float32 in the definition is float32 here (the mix signal and the windowed frame); the transform and every sum are
float64, so the only thing the device does differently is its float32 FFT.  tests/test_features_gpu.py and
tests/test_istft_gpu.py hold every bin of that FFT within EPS = 2e-6 of its frame's peak magnitude; a bin off by d changes
|X|^2 by at most d (2 |X| + d), which gives ``beta`` below.
"""
import math

import numpy as np
import torch

EPS = 2e-6                                              # the forward STFT's bound: |dX| <= EPS * max_k |X_k| per frame
GATE = float.fromhex('0x1.ad7f29abcaf48p-24')           # DAM_SPECTRUM_GATE: -70 dB as a power


def band_edges(sr, n_fft, fraction=3, f_lo=25.0, f_hi=20000.0):
    """-> (edges int32 [B + 1], centres float64 [B]); see the header / spectrum.band_edges for the rule."""
    lo = int(math.ceil(fraction * math.log2(f_lo / 1000.0) - 1e-9))
    hi = int(math.floor(fraction * math.log2(min(f_hi, sr / 2.0) / 1000.0) + 1e-9))
    f = {j: 1000.0 * 2.0 ** ((2 * j - 1) / (2.0 * fraction)) for j in range(lo, hi + 2)}
    e = {j: min(n_fft // 2 + 1, int(math.ceil(f[j] * n_fft / sr))) for j in f}
    kept = [i for i in range(lo, hi + 1) if e[i + 1] > e[i]]
    edges = sorted({e[i] for i in kept} | {e[i + 1] for i in kept})
    return np.array(edges, dtype=np.int32), np.array([1000.0 * 2.0 ** (i / fraction) for i in kept])


def mix_signal(stems, gains=None):
    """stems [S, n, channels] (float32 / float64), gains None or [S, n_gains] float64 -> xm float32 [n]."""
    stems = np.asarray(stems)
    S, n, ch = stems.shape
    x = stems.astype(np.float64)
    m = (x[:, :, 0] + x[:, :, 1]) * 0.5 if ch == 2 else x[:, :, 0]
    if gains is not None:
        gains = np.asarray(gains, dtype=np.float64).reshape(S, -1)
        n_gains = gains.shape[1]
        idx = np.minimum(np.arange(n) // (n // n_gains), n_gains - 1)
        m = m * gains[:, idx]
    acc = m[0].copy()
    for s in range(1, S):
        acc = acc + m[s]
    return acc.astype(np.float32)


def frames(xm, n_fft, hop, exact=False):
    """The front-end's frames of a float32 signal: float32 [T, n_fft], T = 1 + n // hop, reflect padding, periodic Hann
    (torch's float32 table, the project's).  exact: nothing is rounded -- the signal as given and the closed-form window
    0.5 - 0.5 cos(2 pi j / n_fft), both float64 -- for known-answer checks of this file's own conventions."""
    n = xm.shape[0]
    assert n > n_fft // 2
    p = np.arange(1 + n // hop)[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :]
    p = np.abs(p)
    p = np.where(p >= n, 2 * (n - 1) - p, p)
    if exact:
        return np.asarray(xm, dtype=np.float64)[p] * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))[None, :]
    w = torch.hann_window(n_fft, dtype=torch.float32).numpy()
    return (xm.astype(np.float32)[p] * w[None, :]).astype(np.float32)


def bin_weights(n_fft):
    c = np.full(n_fft // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def frame_band_power(fr, edges, want_beta=False):
    """fr [T, n_fft] frames -> the band powers of every frame, [T, B] (and the per-frame bound terms, [T, B])."""
    n_fft = fr.shape[1]
    X = np.abs(np.fft.rfft(np.asarray(fr, dtype=np.float64), axis=1))                 # [T, n_fft/2 + 1]
    c = bin_weights(n_fft)[None, :]
    edges = np.asarray(edges)
    fold = lambda v: np.stack([v[:, edges[b]:edges[b + 1]].sum(axis=1) for b in range(len(edges) - 1)], axis=1)
    if not want_beta:
        return fold(c * X * X)
    pk = X.max(axis=1, keepdims=True)
    return fold(c * X * X), fold(c * EPS * pk * (2.0 * X + EPS * pk))


def band_power_signal(xm, n_fft, hop, edges):
    """-> (P [B], beta [B]): the band powers of a float32 mix signal (the mean over its frames) and the bound on an
    implementation whose float32 FFT is within EPS of the frame's peak magnitude in every bin:
    beta[b] = (1/T) sum_t sum_{k in b} c_k EPS pk_t (2 |X_kt| + EPS pk_t) + 1e-12 P[b]."""
    pw, db = frame_band_power(frames(xm, n_fft, hop), edges, want_beta=True)
    P = pw.sum(axis=0) / pw.shape[0]
    return P, db.sum(axis=0) / pw.shape[0] + 1e-12 * P


def band_power(stems, gains, n_fft, hop, edges):
    return band_power_signal(mix_signal(stems, gains), n_fft, hop, edges)


def parseval_power(xm, n_fft, hop):
    """The single all-bins band without an FFT: (n_fft / T) sum_t sum_j frame_t[j]^2."""
    fr = frames(xm, n_fft, hop).astype(np.float64)
    return n_fft * (fr * fr).sum() / fr.shape[0]


def relative_levels_db(P):
    P = np.asarray(P, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10.0 * np.log10(P / total(P))


def total(P):
    t = 0.0
    for v in np.asarray(P, dtype=np.float64):
        t = t + v
    return t


def balance_error(ref, cand):
    """ref [B], cand [B] band powers -> (err in dB, n_kept)."""
    ref, cand = np.asarray(ref, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    tr, tc = total(ref), total(cand)
    s, n = 0.0, 0
    with np.errstate(divide='ignore', invalid='ignore'):
        for b in range(len(ref)):
            if ref[b] >= GATE * tr and cand[b] >= GATE * tc:
                s = s + abs(10.0 * np.log10(cand[b] / tc) - 10.0 * np.log10(ref[b] / tr))
                n += 1
    return (s / n if n else float('nan')), n


def gate_margin(P):
    """How far the closest band lies from the gate, as |P[b] / (GATE * total) - 1| (inputs of a gate test must keep this
    well above the relative error of the powers compared, so that no decision can flip)."""
    P = np.asarray(P, dtype=np.float64)
    return float(np.min(np.abs(P / (GATE * total(P)) - 1.0)))


def level_bound(P, beta):
    """|dL[b]| <= (10 / ln 10) (beta[b] / P[b] + beta_tot / P_tot) * 1.05 (first-order expansion of the log, 5 % for the
    rest), for the bands with P > 0."""
    P, beta = np.asarray(P, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (10.0 / math.log(10.0)) * (beta / P + beta.sum() / P.sum()) * 1.05


def balance_error_bound(ref, ref_beta, cand, cand_beta):
    """The bound on |err| that follows: the mean of |dL_ref| + |dL_cand| over the kept bands."""
    ref, cand = np.asarray(ref, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    keep = (ref >= GATE * total(ref)) & (cand >= GATE * total(cand))
    return float((level_bound(ref, ref_beta) + level_bound(cand, cand_beta))[keep].mean())
