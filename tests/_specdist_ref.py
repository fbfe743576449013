"""Reference for the spectrogram distance (include/dam_hip.h, "Spectrogram distance"): the definition restated in numpy
float64, independent of the library -- and the error bounds the GPU tests hold the kernels to.

What is float32 in the definition and exact to reproduce is float32 here (the mix signal and the windowed frame, both from
tests/_spectrum_ref.py); the transform, the levels and every sum are float64.  The device differs by its float32 FFT, its
float32 log2 and the float32 rounding of a level; each has a figure the project already holds:
  * the forward FFT is within EPS = 2e-6 of the frame's peak magnitude in every bin (_spectrum_ref.EPS), so with
    delta = EPS pk_t a device level lies in [dB(max(|X| - delta, amin)), dB(max(|X| + delta, amin))];
  * 1e-5 dB for the float32 log2 (csrc/dam_stft.hip, the comment on power_to_db);
  * one float32 ulp of a level of at most 100 dB (magnitudes 64 .. 128: 2^-17 dB) for the rounding of the product with
    3.0103f, of that constant and of the power re^2 + im^2 (1.5 * 2^-24 relative: 8e-7 dB).
Per bin e = e_cand + e_ref, and then |dS1| <= sum e and |dS2| <= sum (2 |d| e + e^2) over a cell.
"""
import numpy as np

import _spectrum_ref as sref

EPS = sref.EPS
LOG2_DB = 1e-5
ROUND_DB = 2.0 ** -17


def window_of_frames(n, W, hop):
    """w(t) = min(min(t hop, n - 1) // (n // W), W - 1) for t = 0 .. T-1, T = 1 + n // hop."""
    t = np.arange(1 + n // hop)
    return np.minimum(np.minimum(t * hop, n - 1) // (n // W), W - 1)


def levels(xm, n_fft, hop, amin=1e-5):
    """float32 mix signal [n] -> (L [T, n_fft/2 + 1] in dB, e [T, n_fft/2 + 1]: how far a device level may lie from it)."""
    fr = sref.frames(xm, n_fft, hop)
    X = np.abs(np.fft.rfft(fr.astype(np.float64), axis=1))
    delta = EPS * X.max(axis=1, keepdims=True)
    db = lambda m: 20.0 * np.log10(np.maximum(m, amin))
    L, lo, hi = db(X), db(X - delta), db(X + delta)
    return L, np.maximum(hi - L, L - lo) + LOG2_DB + ROUND_DB


def extend_edges(edges, n_fft):
    """One band below and one above where bins are left: the table then covers every bin 0 .. n_fft/2 once."""
    e = [int(v) for v in edges]
    return np.asarray(([0] if e[0] > 0 else []) + e + ([n_fft // 2 + 1] if e[-1] < n_fft // 2 + 1 else []), dtype=np.int32)


def distance(stems, gains, ref_stems, ref_gains, n_fft, hop, edges, W, amin=1e-5):
    """stems [S, n, C], gains None / [R, S, n_gains]; ref_stems [S_ref, n, C'], ref_gains None / [S_ref, n_gains]
    -> (sums [R, B, W, 2], count [B, W], bound [R, B, W, 2]) and the per-bin (d [R, T, K], Lc [R, T, K], Lr [T, K])."""
    stems, ref_stems = np.asarray(stems), np.asarray(ref_stems)
    n = stems.shape[1]
    assert ref_stems.shape[1] == n
    R = 1 if gains is None else np.asarray(gains).shape[0]
    edges = np.asarray(edges)
    B = len(edges) - 1
    Lr, er = levels(sref.mix_signal(ref_stems, ref_gains), n_fft, hop, amin)
    w_of = window_of_frames(n, W, hop)
    sums, bound = np.zeros((R, B, W, 2)), np.zeros((R, B, W, 2))
    count = np.zeros((B, W), dtype=np.int64)
    d_all, lc_all = [], []
    for r in range(R):
        Lc, ec = levels(sref.mix_signal(stems, None if gains is None else np.asarray(gains)[r]), n_fft, hop, amin)
        d, e = Lc - Lr, ec + er
        d_all.append(d)
        lc_all.append(Lc)
        for b in range(B):
            for w in range(W):
                dc, ecell = d[w_of == w, edges[b]:edges[b + 1]], e[w_of == w, edges[b]:edges[b + 1]]
                sums[r, b, w] = dc.sum(), (dc * dc).sum()
                bound[r, b, w] = ecell.sum(), (2.0 * np.abs(dc) * ecell + ecell * ecell).sum()
                count[b, w] = dc.size
    return sums, count, bound, np.stack(d_all), np.stack(lc_all), Lr


def _figures(S1, S2, N):
    with np.errstate(divide='ignore', invalid='ignore'):
        mse, bias = S2 / N, S1 / N
        v = mse - bias * bias
        rms = np.sqrt(np.where(v > 0.0, v, np.where(np.isnan(v), v, 0.0)))
    dead = N <= 0
    return np.stack([np.where(dead, np.nan, mse), np.where(dead, np.nan, bias), np.where(dead, np.nan, rms)], axis=-1)


def summary(sums, count):
    """sums [R, B, W, 2], count [B, W] -> [R, 1 + B + W, 3] = (mse, bias, rms_centred) of the row, of every band, of every
    window; a band adds its cells in ascending window, a window in ascending band, the row its bands' sums in ascending band;
    NaN where the count is 0."""
    sums, count = np.asarray(sums, dtype=np.float64), np.asarray(count)
    R, B, W, _ = sums.shape
    out = np.empty((R, 1 + B + W, 3))
    for r in range(R):
        tot, nt = np.zeros(2), 0
        band, nb = np.zeros((B, 2)), np.zeros(B, dtype=np.int64)
        win, nw = np.zeros((W, 2)), np.zeros(W, dtype=np.int64)
        for b in range(B):
            for w in range(W):
                band[b] = band[b] + sums[r, b, w]
                win[w] = win[w] + sums[r, b, w]
                nb[b], nw[w] = nb[b] + count[b, w], nw[w] + count[b, w]
            tot, nt = tot + band[b], nt + nb[b]
        out[r, 0] = _figures(tot[0], tot[1], np.float64(nt))
        out[r, 1:1 + B] = _figures(band[:, 0], band[:, 1], nb.astype(np.float64))
        out[r, 1 + B:] = _figures(win[:, 0], win[:, 1], nw.astype(np.float64))
    return out


# ----------------------------------------------------------------------------- the inputs of the GPU parity sweep
def edge_tables(n_fft):
    M = n_fft // 2
    every = np.arange(0, M + 2) if M + 1 <= 64 else np.arange(M + 1 - 64, M + 2)      # every bin its own band / the top 64
    return [np.array([0, M + 1]), every, np.array([2, 3, 7, 8, 20, M - 3])]


ROW_LEVELS = (4.0, 0.25, 2.0, 0.0, 0.5)          # row 3 of five is the all-zero mix


def noise_case(rng, S, S_ref, n, ch, dtype, R, n_gains, ref_n_gains):
    """White-noise stems (another level each), a reference whose stems are mixtures of the same noise -- its mix is the
    stems' sum with gains within 0.9 .. 1.1 -- and candidate rows ROW_LEVELS[r] times gains within 0.9 .. 1.1: d is
    20 log10 of the row's level give or take a dB or two in every bin, so no cell's sum d^2 is small beside its bound
    (test_specdist_ref_cpu.py checks that on these very inputs), yet no two gains, rows or stems are alike."""
    x = rng.standard_normal((S, n, ch)) * rng.uniform(0.05, 0.2, (S, 1, 1))
    A = rng.uniform(0.5, 1.5, (S_ref, S))
    A = A / A.sum(axis=0, keepdims=True) * rng.uniform(0.95, 1.05, (1, S))
    xref = np.einsum('js,snc->jnc', A, x) * (1.0 / 3.0 if n_gains is None else 1.0)     # (no gains: the level is the reference's)
    if ch == 2 and S_ref % 2 == 0:
        xref = xref[:, :, :1] * 0.5 + xref[:, :, 1:] * 0.5                      # (a mono reference against stereo stems)
    gains = None if n_gains is None else rng.uniform(0.9, 1.1, (R, S, n_gains)) * np.asarray(ROW_LEVELS[:R])[:, None, None]
    ref_gains = None if ref_n_gains is None else rng.uniform(0.95, 1.05, (S_ref, ref_n_gains))
    return x.astype(dtype), gains, xref.astype(dtype), ref_gains


def sweep_cases(n_fft):
    """The parity sweep at one n_fft: every value of every axis, the axes turning at different rates."""
    rng = np.random.default_rng(1000 + n_fft)
    cases = []
    for hop in (n_fft // 2, 23, n_fft):
        for T in (1, 2, 9, 19):
            lo, hi = max((T - 1) * hop, n_fft // 2 + 1), T * hop                # 1 + n // hop == T and n > n_fft / 2
            if lo >= hi:
                continue
            # the smallest such n, one that is no multiple of hop, and at T = 9 the largest (with W = 5: a last window of one frame)
            for n in sorted({lo, min(hi - 1, lo + hop // 2 + 1)} | ({hi - 1} if T == 9 else set())):
                i = len(cases)
                ch, S, S_ref = (1, 2)[i % 2], (1, 2, 3, 5)[i % 4], (2, 1, 4)[i % 3]
                dtype, ref_dtype = (np.float32, np.float64)[(i // 2) % 2], (np.float32, np.float64)[(i // 3) % 2]
                R = (1, 5)[(i // 3) % 2] if i % 5 else 1                        # (no gains: one row)
                n_gains, ref_n_gains = (None, 1, 3, 7, n)[i % 5], (None, 1, 3)[(i // 2) % 3]
                W = [w for w in (5 if T == 9 and n == hi - 1 else (3, 5, 1)[i % 3], 3, 1) if w <= T and
                     len(set(window_of_frames(n, w, hop).tolist())) == w][0]
                stems, gains, ref_stems, ref_gains = noise_case(rng, S, S_ref, n, ch, dtype, R, n_gains, ref_n_gains)
                cases.append(dict(n_fft=n_fft, hop=hop, T=T, n=n, W=W, edges=edge_tables(n_fft)[(i // 2) % 3],
                                  planar=bool((i // 4) % 2), ref_planar=bool((i // 2) % 2), stems=stems, gains=gains,
                                  ref_stems=ref_stems.astype(ref_dtype), ref_gains=ref_gains,
                                  zero_rows=(3,) if gains is not None and R == 5 else ()))
    return cases
