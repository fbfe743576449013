"""numpy float64 restatement of the look-ahead true-peak limiter (include/dam_hip.h: dam_limiter_apply), written from the
definition and nothing else, on top of tests/_truepeak_ref.py's interpolated phases.  The GPU tests compare the kernels with
it; tests/test_limiter_ref_cpu.py checks the properties the definition promises.

    xs[c][i] = (double)x[c][i] * s
    d[i]     = max_c max(|xs[c][i]|, |y_1[c][i]|, |y_2[c][i]|, |y_3[c][i]|)         y_p: _truepeak_ref.phases
    r[i]     = min(1, ceil / d[i]);  1 where d[i] = 0 and outside [0, n)
    m[j]     = min_{k in [j-H, j+L]} r[k]
    g[i]     = (sum_{j=i-L..i} m[j], added in the order j = i-L .. i) / (double)(L+1)
    out[c][i] = xs[c][i] * g[i]
    min_gain = min_i g[i];  n_limited = #{i : g[i] < 1}

Rows are [n, channels] here, as in _truepeak_ref."""
import numpy as np

import _truepeak_ref as tpref


def samples(ms, sr):
    """Milliseconds -> samples: max(1, int(ms * sr / 1000 + 0.5))."""
    return max(1, int(ms * sr / 1000.0 + 0.5))


def scaled(x, pre_gain=None):
    """x [n] or [n, channels] of any float dtype -> xs float64 [n, channels]: one rounding."""
    x = np.asarray(x)
    xs = x.reshape(x.shape[0], -1).astype(np.float64)
    return xs if pre_gain is None else xs * np.float64(pre_gain)


def demand(xs, h=None):
    """xs float64 [n, channels] -> d [n]."""
    d = np.zeros(xs.shape[0])
    for c in range(xs.shape[1]):
        d = np.maximum(d, np.maximum(np.abs(xs[:, c]), np.abs(tpref.phases(xs[:, c], h)).max(axis=0)))
    return d


def required_gain(d, ceiling_lin):
    """r [n] = min(1, ceil / d), 1 where d = 0."""
    r = np.ones(len(d))
    nz = d > 0
    r[nz] = np.minimum(1.0, ceiling_lin / d[nz])
    return r


def held_minimum(r, L, H):
    """m[j] = min r[j-H .. j+L] for j in [-L, n): returned as an array whose element u is m[u - L]; r = 1 outside [0, n)."""
    n = len(r)
    rp = np.concatenate([np.ones(L + H), r, np.ones(L)])             # r[k] = rp[k + L + H]
    m = np.full(n + L, np.inf)
    for k in range(L + H + 1):                                       # m[u - L] = min_k rp[u + k]
        m = np.minimum(m, rp[k: k + n + L])
    return m


def gain(r, L, H):
    """g [n]: each g[i] its own sum of L+1 terms of m, in the order j = i-L .. i, divided by (double)(L+1)."""
    n = len(r)
    m = held_minimum(r, L, H)                                        # m[j] = m_arr[j + L]
    acc = np.zeros(n)
    for q in range(L + 1):                                           # j = i - L + q
        acc = acc + m[q: q + n]
    return acc / np.float64(L + 1)


def limit(x, ceiling_lin, L, H, pre_gain=None, h=None):
    """x [n] or [n, channels] -> dict(out float64 [n, channels], xs, d, r, g, min_gain, n_limited)."""
    xs = scaled(x, pre_gain)
    d = demand(xs, h)
    r = required_gain(d, ceiling_lin)
    g = gain(r, L, H)
    return {'out': xs * g[:, None], 'xs': xs, 'd': d, 'r': r, 'g': g, 'min_gain': float(g.min()), 'n_limited': int((g < 1.0).sum())}
