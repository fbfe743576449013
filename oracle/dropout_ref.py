"""Oracle: the product's dropout mask on the host (test infrastructure).

The reference's nn.Dropout draws from torch's Philox stream; the product draws from a counter-based generator of its own
(csrc/dam_dropout.hip), a pure function of (seed, call offset, element index).  This module restates that function in numpy
from the kernel's header comment and the published splitmix64 constants, so that the float64 oracle can apply the SAME mask
as the device and dropout-on training is compared like everything else:

  base    = seed * 0xD1342543DE82EF95 + offset                (uint64, wrap-around)
  r_i     = high 32 bits of splitmix64_finalise(base + i)     (element i of the flattened, contiguous tensor)
  keep_i  = r_i >= uint32(float32(p) * 2**32)
  y_i     = keep_i ? x_i * (float32(1) / (float32(1) - float32(p))) : 0

`offset` is the device's call counter before the call; every call advances it by its element count, so the calls of one
training step use adjacent, disjoint counter ranges.
"""
import numpy as np

SEED_MUL = 0xD1342543DE82EF95
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
MIX_1 = 0xBF58476D1CE4E5B9
MIX_2 = 0x94D049BB133111EB
_M64 = (1 << 64) - 1


def draws(seed: int, offset: int, n: int) -> np.ndarray:
    """r_i for i in [0, n): uint32[n]."""
    base = (int(seed) * SEED_MUL + int(offset)) & _M64
    with np.errstate(over='ignore'):
        z = np.arange(n, dtype=np.uint64) + np.uint64(base)
        z += np.uint64(GOLDEN_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX_1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX_2)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)).astype(np.uint32)


def threshold(p: float) -> np.uint32:
    """keep iff r >= threshold(p); float32(p) * 2**32 is exact (a power-of-two scaling) and below 2**32 for p < 1."""
    if not 0.0 <= p < 1.0:
        raise ValueError('p = %r is outside [0, 1)' % (p,))
    return np.uint32(int(np.float64(np.float32(p)) * 4294967296.0))


def keep_mask(seed: int, offset: int, n: int, p: float, r: np.ndarray = None) -> np.ndarray:
    """bool[n]; r: draws(seed, offset, n) if the caller already has them (several p over the same counters)."""
    if r is None:
        r = draws(seed, offset, n)
    return r >= threshold(p)


def scale(p: float) -> np.float32:
    return np.float32(1) / (np.float32(1) - np.float32(p))


def apply_ref(x: np.ndarray, seed: int, offset: int, p: float, r: np.ndarray = None) -> np.ndarray:
    """What the kernel writes for a contiguous float32 tensor x (and, with dy for x, what its backward writes)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    keep = keep_mask(seed, offset, x.size, p, r).reshape(x.shape)
    return np.where(keep, x * scale(p), np.float32(0))


def block_keep_masks(seed: int, offset: int, shapes_nhwc, ps):
    """The masks of consecutive calls (the five ConvBlock2d of one forward pass): shapes_nhwc are the tensors the device
    kernel sees ([B, Ho, Wo, C], contiguous).  Returns ([bool NCHW arrays], counter after the last call)."""
    out = []
    for shape, p in zip(shapes_nhwc, ps):
        n = int(np.prod(shape))
        out.append(np.ascontiguousarray(keep_mask(seed, offset, n, p).reshape(shape).transpose(0, 3, 1, 2)))
        offset += n
    return out, offset
