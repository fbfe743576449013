"""Reference for the gradient of the spectrogram distance in the gains (include/dam_hip.h, "Spectrogram distance: gradient"):
the definition restated in numpy float64 with explicit np.fft.rfft / irfft, independent of the library -- and the per-entry
error bound the GPU tests hold the kernels to.

What is float32 in the definition and exact to reproduce is float32 here (the mix signal and the windowed frame, both from
tests/_spectrum_ref.py); the transforms, the levels, u, z and every sum are float64.

The bound is propagated to first order from the error model tests/_specdist_ref.py already holds.  With C[t][k] =
rfft(w * m_s[q(t, .)] * [gain_index(q) == j])[k], the windowed spectrum of the stem's segment inside frame t,
    dJ/dg[s][j] = sum_t sum_k Re(u[t][k] conj C[t][k]),      u = (40 / ln 10) d X / p,
so an error du per bin moves the entry by at most sum |du| |C|.  Per bin
    |du| <= (40 / ln 10) (|X| e / p + 3 |d| dX / p),
e = the bound on d (dX = EPS pk_t through both levels, LOG2_DB and ROUND_DB, as _specdist_ref.levels forms it), 3 dX / p the
bound on X / p with p formed from the perturbed X.  A candidate bin whose |X| lies within dX of the floor threshold amin adds
its WHOLE contribution (40 / ln 10) |d| |C| / |X|: the derivative is discontinuous there.  The inverse transform is within EPS
of the peak of y_t in every sample: EPS max_i |y_t[i]| sum_i |w[i] c[i]| per frame.  The float32 roundings of c_k, of u_k = c_k X_k
and of z = w * (0.5 y) are 2^-24 relative each: 3 * 2^-24 (sum |u| |C| + sum_i |z[i] c[i]|).
"""
import math

import numpy as np
import torch

import _specdist_ref as dref
import _spectrum_ref as sref

EPS = sref.EPS
SCALE = 40.0 / math.log(10.0)
ROUND_F32 = 3.0 * 2.0 ** -24


def channel_mean(stems):
    x = np.asarray(stems).astype(np.float64)
    return (x[:, :, 0] + x[:, :, 1]) * 0.5 if x.shape[2] == 2 else x[:, :, 0]


def positions(n, n_fft, hop):
    """q(t, i) = reflect(t hop - n_fft/2 + i), [T, n_fft]."""
    p = np.abs(np.arange(1 + n // hop)[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :])
    return np.where(p >= n, 2 * (n - 1) - p, p)


def gain_index(n, n_gains):
    return np.minimum(np.arange(n) // (n // n_gains), n_gains - 1)


def frames_owned(n, n_gains, n_fft, hop):
    """How many frames begin (first sample clamped into the signal) in every gain segment: [n_gains]."""
    start = np.clip(np.arange(1 + n // hop) * hop - n_fft // 2, 0, n - 1)
    return np.bincount(gain_index(n, n_gains)[start], minlength=n_gains)


def _window(n_fft, exact):
    if exact:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    return torch.hann_window(n_fft, dtype=torch.float32).numpy().astype(np.float64)


def _mix(stems, gains, exact):
    if not exact:
        return sref.mix_signal(stems, gains)
    m = channel_mean(stems)
    if gains is not None:
        g = np.asarray(gains, dtype=np.float64).reshape(m.shape[0], -1)
        m = m * g[:, gain_index(m.shape[1], g.shape[1])]
    return m.sum(axis=0)


def _spectrum(xm, n_fft, hop, exact):
    return np.fft.rfft(sref.frames(xm, n_fft, hop, exact=exact).astype(np.float64), axis=1)


def _level(X, amin):
    return 20.0 * np.log10(np.maximum(np.abs(X), amin))


def _level_error(X, amin):
    """How far a device level may lie from the level of X: _specdist_ref.levels' e."""
    A = np.abs(X)
    delta = EPS * A.max(axis=1, keepdims=True)
    db = lambda m: 20.0 * np.log10(np.maximum(m, amin))
    L = db(A)
    return np.maximum(db(A + delta) - L, L - db(A - delta)) + dref.LOG2_DB + dref.ROUND_DB, delta


def gradient(stems, gains, ref_stems, ref_gains, n_fft, hop, amin=1e-5, exact=False, want_bound=True):
    """One clip.  stems [S, n, C]; gains None / [R, S, G]; ref_stems [S_ref, n, C']; ref_gains None / [S_ref, G'] ->
    dict: value [R, 2] = (S1, S2), grad [R, S, max(G, 1)], value_bound [R, 2], grad_bound [R, S, G], floored [R] (candidate
    bins at the floor), and d [R, T, K].  exact: nothing is rounded to float32 and the window is the closed form (for the
    finite-difference check of the formula)."""
    stems, ref_stems = np.asarray(stems), np.asarray(ref_stems)
    S, n = stems.shape[:2]
    R = 1 if gains is None else np.asarray(gains).shape[0]
    G = 1 if gains is None else np.asarray(gains).shape[2]
    w, q, idx, m = _window(n_fft, exact), positions(n, n_fft, hop), gain_index(n, G), channel_mean(stems)
    Xr = _spectrum(_mix(ref_stems, ref_gains, exact), n_fft, hop, exact)
    Lr = _level(Xr, amin)
    er, _ = _level_error(Xr, amin)
    # c[s][j][t][i] = m_s[q] [idx[q] == j] and its windowed spectrum
    seg = idx[q]
    out = dict(value=np.zeros((R, 2)), grad=np.zeros((R, S, G)), value_bound=np.zeros((R, 2)), grad_bound=np.zeros((R, S, G)),
               floored=np.zeros(R, dtype=np.int64), d=[])
    for r in range(R):
        X = _spectrum(_mix(stems, None if gains is None else np.asarray(gains)[r], exact), n_fft, hop, exact)
        A = np.abs(X)
        floored = A <= amin
        d = _level(X, amin) - Lr
        p = np.where(floored, 1.0, A * A)
        u = np.where(floored, 0.0, SCALE * d[:, :] * X / p)
        v = u.copy()
        v[:, 0], v[:, -1] = 2.0 * u[:, 0], 2.0 * u[:, -1]
        y = 0.5 * n_fft * np.fft.irfft(v, n=n_fft, axis=1)              # half the unnormalised inverse real transform
        z = w[None, :] * y
        out['value'][r] = d.sum(), (d * d).sum()
        out['floored'][r] = int(floored.sum())
        out['d'].append(d)
        for s in range(S):
            out['grad'][r, s] = np.bincount(seg.ravel(), weights=(z * m[s][q]).ravel(), minlength=G)
        if not want_bound:
            continue
        ec, delta = _level_error(X, amin)
        e = ec + er
        out['value_bound'][r] = e.sum(), (2.0 * np.abs(d) * e + e * e).sum()
        du = np.where(floored, 0.0, SCALE * (A * e + 3.0 * np.abs(d) * delta) / p)
        near = np.abs(A - amin) <= delta                                 # the floor decision may fall either way on the device
        whole = np.where(near, SCALE * np.abs(d) / np.maximum(A, 0.5 * amin), 0.0)
        pk_y = np.abs(y).max(axis=1)
        for s in range(S):
            for j in range(G):
                c = m[s][q] * (seg == j)
                C = np.abs(np.fft.rfft(w[None, :] * c, axis=1))
                out['grad_bound'][r, s, j] = ((du + whole) * C).sum() + EPS * (pk_y * np.abs(w[None, :] * c).sum(axis=1)).sum() \
                    + ROUND_F32 * ((np.abs(u) * C).sum() + np.abs(z * c).sum())
    out['d'] = np.stack(out['d'])
    return out


def gradient_clips(stems, gains, ref_stems, ref_gains, n_fft, hop, amin=1e-5):
    """The clip axis in front of everything: stems [clips, S, n, C], gains None / [clips, R, S, G], ... -> the dict of
    gradient() with a leading clip axis on every array."""
    per = [gradient(stems[c], None if gains is None else gains[c], ref_stems[c], None if ref_gains is None else ref_gains[c],
                    n_fft, hop, amin) for c in range(len(stems))]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


# ----------------------------------------------------------------------------- the inputs of the GPU parity sweep
ROW_LEVELS = (2.0, 0.5, 1.5, 0.0, 0.25)           # row 3 of five is the all-zero mix


PULSE = 8.0
OFFSET = 10.0


def noise_case(rng, S, S_ref, n, ch, dtype, ref_dtype, R, n_gains, ref_n_gains, clips, n_fft):
    """_specdist_ref.noise_case with the row levels of this sweep and a clip axis (another noise per clip) -- and a pulse on
    sample 0 of every stem, PULSE times the rms magnitude sqrt(3 n_fft / 8) sigma of a windowed noise bin.  Frame 0 is
    reflect-padded about sample 0, so it is even and its spectrum real up to a sign: a bin of it is a REAL Gaussian, small
    with a probability linear in the threshold, and with a thousand bins some |X| lies within a few dX of zero -- where the
    derivative 1 / |X| makes every bound useless.  The pulse sits at the window's peak and adds the same real constant to every
    bin of that frame; the other frames' bins are complex Gaussians, whose nulls are rare enough for a seed to avoid.  Bins 0
    and n_fft/2 are real in EVERY frame: a constant and an alternating component of OFFSET sigma / sqrt(n_fft) each put
    (n_fft / 2) of that, OFFSET / sqrt(1.5) times a noise bin's rms magnitude, on those two bins."""
    xs, gs, rs, rgs = [], [], [], []
    for _ in range(clips):
        level = rng.uniform(0.05, 0.2, (S, 1, 1))
        x = rng.standard_normal((S, n, ch)) * level
        x[:, :1] += PULSE * math.sqrt(0.375 * n_fft) * level
        x += (OFFSET / math.sqrt(n_fft)) * level * (1.0 + (-1.0) ** np.arange(n))[None, :, None]
        A = rng.uniform(0.5, 1.5, (S_ref, S))
        A = A / A.sum(axis=0, keepdims=True) * rng.uniform(0.95, 1.05, (1, S))
        xref = np.einsum('js,snc->jnc', A, x) * (1.0 / 3.0 if n_gains is None else 1.0)
        if ch == 2 and S_ref % 2 == 0:
            xref = xref[:, :, :1] * 0.5 + xref[:, :, 1:] * 0.5          # (a mono reference against stereo stems)
        xs.append(x.astype(dtype))
        rs.append(xref.astype(ref_dtype))
        if n_gains is not None:
            gs.append(rng.uniform(0.9, 1.1, (R, S, n_gains)) * np.asarray(ROW_LEVELS[:R])[:, None, None])
        if ref_n_gains is not None:
            rgs.append(rng.uniform(0.95, 1.05, (S_ref, ref_n_gains)))
    return np.stack(xs), (np.stack(gs) if gs else None), np.stack(rs), (np.stack(rgs) if rgs else None)


def _case(rng, i, n_fft, hop, n, n_gains=-1):
    ch, S, S_ref = (1, 2)[i % 2], (1, 2, 3, 5)[i % 4], (2, 1, 4)[i % 3]
    dtype, ref_dtype = (np.float32, np.float64)[(i // 2) % 2], (np.float32, np.float64)[(i // 3) % 2]
    if n_gains == -1:
        n_gains = (3, None, 2, 1)[i % 4]
        while n_gains is not None and n_gains > 1 and n // n_gains < n_fft:
            n_gains -= 1                                                 # a frame touches two segments at most
    R = 1 if n_gains is None else (5, 1)[i % 2]
    clips = (1, 3)[(i // 2) % 2]
    stems, gains, ref_stems, ref_gains = noise_case(rng, S, S_ref, n, ch, dtype, ref_dtype, R, n_gains, (None, 1, 3)[(i // 2) % 3],
                                                    clips, n_fft)
    return dict(n_fft=n_fft, hop=hop, T=1 + n // hop, n=n, planar=bool((i // 4) % 2), ref_planar=bool((i // 2) % 2), stems=stems,
                gains=gains, ref_stems=ref_stems, ref_gains=ref_gains, zero_rows=(3,) if R == 5 else ())


# seeds at which no bin of the sweep lies within a few hundred dX of zero (test_specgrad_ref_cpu.py holds every entry's bound
# to 1e-2 of its row's largest entry on these very inputs; about one seed in five does at n_fft 256, T 19, R 5, three clips)
SWEEP_SEEDS = {64: 2064, 256: 2269, 2048: 4048}


def sweep_cases(n_fft):
    """The parity sweep at one n_fft (64, 256, 2048): every value of every axis, the axes turning at different rates."""
    rng = np.random.default_rng(SWEEP_SEEDS[n_fft])
    cases = []
    for hop in (n_fft // 2, 23, n_fft):
        for T in (2, 9, 19):
            lo, hi = max((T - 1) * hop, n_fft // 2 + 1), T * hop         # 1 + n // hop == T and n > n_fft / 2
            if lo >= hi:
                continue
            n = min(hi - 1, lo + hop // 2 + 1)                           # no multiple of the hop
            cases.append(_case(rng, len(cases), n_fft, hop, n))
    return cases


def large_case(n_fft):
    """8192 / 16384: n = 2 n_fft + n_fft / 2 + 37, two gain nodes, hop n_fft -- three frames, the second node owns one."""
    rng = np.random.default_rng(3000 + n_fft)
    return _case(rng, 5, n_fft, n_fft, 2 * n_fft + n_fft // 2 + 37, n_gains=2)
