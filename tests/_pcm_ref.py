"""numpy restatement of the PCM encoder (include/dam_hip.h: dam_pcm_encode) -- quantiser, dither and clip count, written
from the definition and nothing else.  The GPU tests compare the kernel with it byte for byte; tests/test_pcm_ref_cpu.py
checks its dither statistics on the host."""
import numpy as np

BITS = {'PCM_16': 16, 'PCM_24': 24, 'PCM_32': 32}
WIDTH = {'PCM_16': 2, 'PCM_24': 3, 'PCM_32': 4, 'FLOAT': 4}
SEED_MUL = np.uint64(0xD1342543DE82EF95)


def splitmix64(z):
    """The full 64-bit splitmix64 finaliser of uint64 `z` (wrap-around arithmetic)."""
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dither(seed, first, count):
    """d[e] for elements e = first .. first + count - 1: u1 - u2 of the high and low 32 bits of r(seed, e), float64, exact."""
    with np.errstate(over='ignore'):
        base = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) * SEED_MUL
        r = splitmix64(base + (np.uint64(first) + np.arange(count, dtype=np.uint64)))
    u1 = (r >> np.uint64(32)).astype(np.float64) / 4294967296.0
    u2 = (r & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0
    return u1 - u2


def quantize(x, subtype, scale=None, dither_seed=None):
    """x: planar [channels, n] float32 / float64; scale: None, or float64 of 1 or `channels` values.
    -> (codes [n, channels]: int64 for the integer subtypes, float32 for 'FLOAT'; clip_count int64 [channels])."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[None]
    ch, n = x.shape
    v = x.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        if scale is not None:
            s = np.asarray(scale, dtype=np.float64).reshape(-1)
            v = v * (s[0] if s.size == 1 else s[:, None])
        if subtype == 'FLOAT':
            return v.T.astype(np.float32), np.zeros(ch, dtype=np.int64)
        b = BITS[subtype]
        full = float(2 ** (b - 1))
        nan = np.isnan(v)
        w = np.where(nan, 0.0, v) * full
        if dither_seed is not None:
            # element index e = frame * channels + channel
            d = dither(dither_seed, 0, n * ch).reshape(n, ch).T
            w = w + d
        q = np.rint(w)
        lo, hi = q < -full, q > full - 1.0
        q = np.where(nan, 0.0, np.clip(q, -full, full - 1.0))
    clipped = (lo | hi | nan).sum(axis=1).astype(np.int64)
    return q.T.astype(np.int64), clipped


def to_bytes(codes, subtype):
    """codes [n, channels] as quantize() returns them -> the interleaved little-endian bytes, uint8 [n * channels * width]."""
    if subtype == 'FLOAT':
        return np.ascontiguousarray(codes, dtype='<f4').view(np.uint8).reshape(-1)
    if subtype == 'PCM_16':
        return np.ascontiguousarray(codes.astype('<i2')).view(np.uint8).reshape(-1)
    if subtype == 'PCM_32':
        return np.ascontiguousarray(codes.astype('<i4')).view(np.uint8).reshape(-1)
    four = np.ascontiguousarray(codes.astype('<i4')).view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(four[:, :3]).reshape(-1)


def encode(x, subtype, scale=None, dither_seed=None):
    """-> (bytes uint8, clip_count int64 [channels])."""
    codes, clipped = quantize(x, subtype, scale, dither_seed)
    return to_bytes(codes, subtype), clipped


def from_bytes(raw, subtype, channels):
    """The inverse of to_bytes: -> codes [n, channels]."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    if subtype == 'FLOAT':
        return raw.view('<f4').reshape(-1, channels)
    if subtype == 'PCM_16':
        return raw.view('<i2').astype(np.int64).reshape(-1, channels)
    if subtype == 'PCM_32':
        return raw.view('<i4').astype(np.int64).reshape(-1, channels)
    b = raw.reshape(-1, 3).astype(np.int64)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return (v - ((v & 0x800000) << 1)).reshape(-1, channels)
