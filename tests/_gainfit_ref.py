"""numpy float64 restatement of the gain fit (include/dam_hip.h: dam_gainfit_moments / dam_gainfit_solve /
dam_gainfit_gain_error) for the tests.  The moments are exactly rounded (error-free products, math.fsum); the solve follows
the definition step by step, with numpy.linalg.solve on the normalised matrix, and also reports that matrix's condition
number, which the tests' bounds are scaled by; the gain error is the definition in plain loops."""
import math

import numpy as np

MAX_STEMS = 8
GATE = 1e-8
PIVOT = 2.0 ** -40
U_ROUND = 2.0 ** -53


def window_bounds(n, W):
    """[(start, end)] of the W windows of n samples: w(p) = min(p // (n // W), W - 1)."""
    seg = n // W
    return [(w * seg, (w + 1) * seg if w < W - 1 else n) for w in range(W)]


def _two_prod(a, b):
    """a * b = hi + lo exactly (Dekker, with Veltkamp's split; no overflow at audio levels)."""
    hi = a * b
    split = 134217729.0                                # 2^27 + 1
    ca, cb = split * a, split * b
    a1, b1 = ca - (ca - a), cb - (cb - b)
    a2, b2 = a - a1, b - b1
    lo = a2 * b2 - (((hi - a1 * b1) - a2 * b1) - a1 * b2)
    return hi, lo


def moments(x, y, W):
    """x [S, n, C], y [n, C] (float32 or float64 arrays) -> M [W, S + 1, S + 1] float64, every entry the exactly rounded
    sum of the exact products."""
    x, y = np.asarray(x), np.asarray(y)
    S, n, C = x.shape
    assert y.shape == (n, C) and 1 <= S <= MAX_STEMS and 1 <= W <= n
    u = np.concatenate([x.astype(np.float64), y.astype(np.float64)[None]])        # [S + 1, n, C]
    M = np.zeros((W, S + 1, S + 1))
    for w, (a, b) in enumerate(window_bounds(n, W)):
        seg = u[:, a:b].reshape(S + 1, -1)
        for i in range(S + 1):
            for j in range(i, S + 1):
                hi, lo = _two_prod(seg[i], seg[j])
                M[w, i, j] = M[w, j, i] = math.fsum(np.concatenate([hi, lo]).tolist())
    return M


def addends(n, W, C):
    """Addends of one entry of M in the longest window (the last)."""
    a, b = window_bounds(n, W)[-1]
    return (b - a) * C


def solve(M, pool=0, ridge=0.0):
    """M [W, S + 1, S + 1] -> (gains [S, W], residual [W], status [W] int, cond [W]); cond is numpy.linalg.cond of the
    normalised matrix R of a window that was solved, NaN elsewhere."""
    M = np.asarray(M, dtype=np.float64)
    W, U, _ = M.shape
    S = U - 1
    gains = np.full((S, W), np.nan)
    residual = np.full(W, np.nan)
    status = np.zeros(W, dtype=np.int64)
    cond = np.full(W, np.nan)
    for w in range(W):
        v0, v1 = max(0, w - pool), min(W - 1, w + pool)
        A = M[v0].copy()
        for v in range(v0 + 1, v1 + 1):
            A = A + M[v]
        G, b, Y = A[:S, :S], A[:S, S], A[S, S]
        active = [s for s in range(S) if G[s, s] > 0.0 and G[s, s] >= GATE * Y]
        if Y == 0.0 or not active:
            continue
        d = np.sqrt(np.array([G[s, s] for s in active]))
        R = G[np.ix_(active, active)] / (d[:, None] * d[None, :]) + ridge * np.eye(len(active))
        if not _cholesky_pivots_ok(R):
            status[w] = -1
            continue
        h = np.linalg.solve(R, b[active] / d)
        cond[w] = np.linalg.cond(R)
        g = np.zeros(S)
        g[active] = h / d
        gains[active, w] = g[active]
        status[w] = len(active)
        residual[w] = max(0.0, (Y - 2.0 * float(b @ g) + float(g @ (G @ g))) / Y)
    return gains, residual, status, cond


def _cholesky_pivots_ok(R):
    n = R.shape[0]
    L = np.zeros_like(R)
    for j in range(n):
        piv = R[j, j]
        for k in range(j):
            piv -= L[j, k] * L[j, k]
        if not piv > PIVOT:
            return False
        L[j, j] = math.sqrt(piv)
        for i in range(j + 1, n):
            v = R[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return True


def gain_error(fit, cand):
    """fit [S, W], cand [V, S, W] or [V, S, 1] -> (err [V], err_stem [V, S], n_kept [V] int)."""
    fit, cand = np.asarray(fit, dtype=np.float64), np.asarray(cand, dtype=np.float64)
    S, W = fit.shape
    V = cand.shape[0]
    assert cand.shape[1] == S and cand.shape[2] in (1, W)
    err, err_stem, n_kept = np.full(V, np.nan), np.full((V, S), np.nan), np.zeros(V, dtype=np.int64)
    for v in range(V):
        total, count = 0.0, 0
        per, per_n = [0.0] * S, [0] * S
        for w in range(W):
            d = {}
            for s in range(S):
                f, c = fit[s, w], cand[v, s, w if cand.shape[2] > 1 else 0]
                if math.isfinite(f) and math.isfinite(c) and f > 0.0 and c > 0.0:
                    d[s] = 20.0 * math.log10(c / f)
            if len(d) < 2:
                continue
            mu = 0.0
            for s in sorted(d):
                mu += d[s]
            mu /= len(d)
            for s in sorted(d):
                a = abs(d[s] - mu)
                total += a
                count += 1
                per[s] += a
                per_n[s] += 1
        n_kept[v] = count
        if count:
            err[v] = total / count
        for s in range(S):
            if per_n[s]:
                err_stem[v, s] = per[s] / per_n[s]
    return err, err_stem, n_kept


def base_input(y_dtype=np.float64, S=4, C=2, n=6007, W=5, seed=7):
    """The tests' base case: S float32 stems of pairwise correlation 0.5 at 0.1 RMS, gains drawn from U(0.5, 1.5) per stem
    and window, y = sum_s g[s, w(p)] x_s[p] formed in float64 and rounded to ``y_dtype`` -> (x [S, n, C], y [n, C], g [S, W])."""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((S, n, C))
    common = rng.standard_normal((n, C))
    x = (0.1 * (math.sqrt(0.5) * noise + math.sqrt(0.5) * common[None])).astype(np.float32)
    g = rng.uniform(0.5, 1.5, (S, W))
    return x, mix(x, g).astype(y_dtype), g


def mix(x, g):
    """sum_s g[s, w(p)] x_s[p] in float64, ascending s: x [S, n, C], g [S, W] -> [n, C]."""
    S, n, C = x.shape
    W = g.shape[1]
    idx = np.minimum(np.arange(n) // (n // W), W - 1)
    y = np.zeros((n, C))
    for s in range(S):
        y = y + x[s].astype(np.float64) * g[s, idx][:, None]
    return y
