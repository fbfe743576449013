#!/usr/bin/env python3
"""Diagnostic: time of the compressor (dam_compressor_apply, the defaults: -12 dB, 2:1, 6 dB knee, 10 / 100 ms) on 4 stereo
float32 stems of 4 minutes at 44.1 kHz as ONE call of N = 4 (a compressor per stem, float64 out) and on one stereo float64
master, beside the look-ahead limiter (dam_limiter_apply, 5 / 20 ms) and the BS.1770 meter on the same master.  The
compressor's cost does not follow the content except for the log10 of the samples over the knee, so one content is timed:
noise with a slow amplitude modulation that crosses the knee (tests/_compressor_ref.am_noise's shape).
`--trace` runs each call a few times and exits (for a kernel trace taken around this script)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import loudness, ops

HBM_BYTES_PER_S = 6.3e12          # achievable, MI355X

dev = torch.device('cuda', 0)
rate, n, ch = 44100, 44100 * 240, 2
g = torch.Generator(device=dev).manual_seed(1)
envelope = 0.02 + 0.3 * (0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(n, device=dev, dtype=torch.float64) / 9000.0))
stems = (envelope * torch.randn((4, ch, n), generator=g, device=dev, dtype=torch.float64)).float()
master = stems.double().sum(0, keepdim=True) * 0.5
constants = ops.compressor_constants(-12.0, 6.0, 10.0, 100.0, rate)
args = (-12.0, 2.0, 6.0) + constants
K, tile, _ = ops.compressor_geometry()


def buffers(N):
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(out=torch.empty((N, ch, n), **f64), max_reduction_out=torch.empty(N, **f64),
                n_over_out=torch.empty(N, dtype=torch.int64, device=dev),
                workspace=torch.empty(ops._lib.lib().dam_compressor_workspace_bytes(N, n) // 8, **f64))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    if '--trace' in sys.argv:
        return float('nan')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def traffic(N, in_bytes):
    """Bytes the six launches move: x read twice, c written once and read twice, out written, four doubles per chunk written
    and read once each."""
    return N * n * (2 * ch * in_bytes + 3 * 8 + ch * 8 + 2 * 4 * 8 / K)


b4, b1 = buffers(4), buffers(1)
t4 = timed(lambda: ops.compressor_apply(stems.transpose(1, 2), *args, **b4), 20)
t1 = timed(lambda: ops.compressor_apply(master.transpose(1, 2), *args, **b1), 20)
L, H = ops.limiter_samples(5.0, rate), ops.limiter_samples(20.0, rate)
lim = dict(out=torch.empty((1, ch, n), dtype=torch.float64, device=dev), min_gain_out=torch.empty(1, dtype=torch.float64, device=dev),
           n_limited_out=torch.empty(1, dtype=torch.int64, device=dev),
           workspace=torch.empty(ops._lib.lib().dam_limiter_workspace_bytes(1, n) // 8, dtype=torch.float64, device=dev))
t_lim = timed(lambda: ops.limiter_apply(master.transpose(1, 2), -1.0, L, H, **lim), 20)
meter, lufs = loudness.Meter(rate), torch.empty(1, dtype=torch.float64, device=dev)
t_meter = timed(lambda: meter.integrated_loudness_batch(master.transpose(1, 2), out=lufs), 20)
print('compressor, 4 stereo float32 stems in one call: %.4f ms (%.1f MB: %.4f ms at 6.3 TB/s); max reduction %s dB, over share %s'
      % (t4, traffic(4, 4) / 1e6, traffic(4, 4) / HBM_BYTES_PER_S * 1e3, [round(v, 3) for v in b4['max_reduction_out'].tolist()],
         [round(v / n, 3) for v in b4['n_over_out'].tolist()]))
print('compressor, one stereo float64 master: %.4f ms (%.1f MB: %.4f ms at 6.3 TB/s); limiter on the same master %.4f ms, '
      'BS.1770 meter %.4f ms' % (t1, traffic(1, 8) / 1e6, traffic(1, 8) / HBM_BYTES_PER_S * 1e3, t_lim, t_meter))
print('chunk %d samples, tile %d: %d tiles per row, %d passes of the tile scan' % (K, tile, -(-n // tile), -(-(-(-n // tile)) // 256)))
