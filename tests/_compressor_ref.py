"""The compressor of include/dam_hip.h (dam_compressor_apply) in numpy float64, twice.

``compress`` is the definition: the static curve per sample, then the two recurrences as plain sequential loops over Python
floats (IEEE doubles, no fused operations: q = aA * q + (1 - aA) * p has one rounding more than the kernel's fma, which the
bound of tests/test_compressor_gpu.py covers).  About 0.4 s per million samples.

``ballistics_chunked`` restates the kernel's parallel form on the host: chunks of K samples from a zero state, a
left-to-right walk over the chunk summaries, the chunks again from their true entry states -- first p, then q on the true
p.  It is mathematically the same function; tests/test_compressor_ref_cpu.py bounds the difference in rounding.

Every constant comes from ops.compressor_constants, which the kernel's callers use too: both sides see the same bits.
"""
import numpy as np

LN10_20 = 0.11512925464970228              # ln(10) / 20, the kernel's constant


def curve(d, threshold_db, ratio, knee_db, knee_start):
    """Gain reduction c >= 0 in dB for detector values d (any shape).  0 exactly, no logarithm, where d <= knee_start."""
    d = np.asarray(d, dtype=np.float64)
    slope = 1.0 - 1.0 / float(ratio)
    c = np.zeros(d.shape)
    over = d > knee_start
    o = 20.0 * np.log10(d[over]) - threshold_db
    hard = slope * np.maximum(o, 0.0)
    if knee_db > 0.0:
        t = np.maximum(o + 0.5 * knee_db, 0.0)
        c[over] = np.where(o < 0.5 * knee_db, slope * (t * t) / (2.0 * knee_db), hard)
    else:
        c[over] = hard
    return c


def ballistics(c, a_att, a_rel):
    """p[i] = max(c[i], aR p[i-1]), q[i] = aA q[i-1] + (1 - aA) p[i], both from 0: sequential.  -> (p, q)"""
    one_minus = 1.0 - a_att
    p = q = 0.0
    ps, qs = [], []
    for ci in np.asarray(c, dtype=np.float64).tolist():
        ap = a_rel * p
        p = ci if ci > ap else ap
        q = a_att * q + one_minus * p
        ps.append(p)
        qs.append(q)
    return np.array(ps), np.array(qs)


def ballistics_chunked(c, a_att, a_rel, K):
    """The same two recurrences in the kernel's three passes over chunks of K samples.  -> (p, q)"""
    c = np.asarray(c, dtype=np.float64)
    n = len(c)
    chunks = [c[i:i + K].tolist() for i in range(0, n, K)]
    one_minus = 1.0 - a_att
    # pass 1: every chunk from p = 0 -> its map y -> max(P, a^len y)
    rel = []
    for ch in chunks:
        p, a = 0.0, 1.0
        for ci in ch:
            p = max(ci, a_rel * p)
            a *= a_rel
        rel.append((p, a))
    # the walk over the summaries: the true entry state of every chunk
    entry_p, y = [], 0.0
    for P, a in rel:
        entry_p.append(y)
        y = max(P, a * y)
    # pass 2: p from its entry state, q from 0 -> the map y -> A^len y + B
    att, ps = [], []
    for ch, p in zip(chunks, entry_p):
        q, a = 0.0, 1.0
        for ci in ch:
            p = max(ci, a_rel * p)
            q = a_att * q + one_minus * p
            a *= a_att
            ps.append(p)
        att.append((q, a))
    entry_q, y = [], 0.0
    for B, a in att:
        entry_q.append(y)
        y = a * y + B
    # pass 3: q from its entry state on the true p
    qs, i = [], 0
    for ch, q in zip(chunks, entry_q):
        for _ in ch:
            q = a_att * q + one_minus * ps[i]
            qs.append(q)
            i += 1
    return np.array(ps), np.array(qs)


def tol_q(attack_samples, release_samples, c_max):
    """The bound on |q - q'| in dB between two evaluations of the recurrences that differ in the order of their roundings
    (sequential against chunked, device against host): a contraction with factor alpha accumulates at most a few roundings
    of size u * max c per step over an effective 1 / (1 - alpha) ~ tau steps; 8 is 'a few', and covers the few-ulp
    difference between two libraries' log10 and exp."""
    return 8.0 * 2.0 ** -53 * max(attack_samples, release_samples) * max(1.0, c_max)


def compress(x, threshold_db, ratio, knee_db, knee_start, a_att, a_rel, makeup=1.0, pre_gain=None):
    """x [n, channels] (float32 or float64) -> dict of float64 arrays: xs [n, ch], d, c, p, q, g [n], out [n, ch], and
    'max_reduction' (dB), 'n_over'."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    xs = x.astype(np.float64) * (1.0 if pre_gain is None else float(pre_gain))
    d = np.abs(xs).max(axis=1)
    c = curve(d, threshold_db, ratio, knee_db, knee_start)
    p, q = ballistics(c, a_att, a_rel)
    g = np.exp(-(q * LN10_20)) * makeup
    return {'xs': xs, 'd': d, 'c': c, 'p': p, 'q': q, 'g': g, 'out': xs * g[:, None], 'max_reduction': float(q.max()),
            'n_over': int((d > knee_start).sum())}


# ----------------------------------------------------------------------------- inputs shared by the CPU and the GPU tests
def am_noise(n, channels=1, seed=0):
    """Amplitude-modulated noise (0.02 + 0.3 (0.5 - 0.5 cos 2 pi i / 9000)) randn: crosses a knee at -27 .. -21 dBFS
    continuously (on the host, n = 40000, seed 1: 64 % of the samples over its start)."""
    rng = np.random.default_rng(seed)
    env = 0.02 + 0.3 * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / 9000.0))
    return env[:, None] * rng.standard_normal((n, channels))


def bursts_on_a_bed(n, channels=1, seed=0, boundaries=(), amplitude=0.5):
    """A bed of 0.004 randn (clearly under any knee used here) with samples of +-``amplitude`` at both ends of the row and at
    every boundary b given: b - 1 and b (the seam between two owners) for the boundaries at even positions of the list,
    b + 1 alone (one sample behind the seam) for those at odd positions.  Positions outside the row are dropped."""
    rng = np.random.default_rng(seed)
    x = 0.004 * rng.standard_normal((n, channels))
    places = [0, n - 1]
    for k, b in enumerate(boundaries):
        places += [b - 1, b] if k % 2 == 0 else [b + 1]
    for k, i in enumerate(places):
        if 0 <= i < n:
            x[i, k % channels] = amplitude if k % 3 else -amplitude
    return x
