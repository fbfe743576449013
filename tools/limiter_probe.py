#!/usr/bin/env python3
"""Diagnostic: time of the look-ahead true-peak limiter (dam_limiter_apply, 5 ms look-ahead, 20 ms hold) on one stereo
float64 master of 4 minutes at 44.1 kHz, beside the true-peak meter (dam_true_peak_batch) on the same buffer -- the meter
kernel reads the same samples and does the same 36 products per sample; the limiter also writes r and the output and adds
L + 1 values of LDS per sample where a tile is touched at all.  Three contents, because a tile whose required gains are all 1
skips the min-table and the sums: 'quiet' (nothing over the ceiling), 'sparse' (a burst every 0.75 s: a few per cent of the
samples limited) and 'dense' (a burst every 1000 samples: every tile does the full work).
`--trace` runs each call a few times and exits (for a kernel trace taken around this script)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import ops

HBM_BYTES_PER_S = 6.3e12          # achievable, MI355X
FP64_OPS_PER_S = 78.6e12 / 2      # vector float64 peak, one FMA = 2 FLOP; an add takes the same slot

dev = torch.device('cuda', 0)
rate, n, ch = 44100, 44100 * 240, 2
L, H = ops.limiter_samples(5.0, rate), ops.limiter_samples(20.0, rate)
g = torch.Generator(device=dev).manual_seed(1)
bed = 0.1 * torch.randn((1, ch, n), generator=g, device=dev, dtype=torch.float64)
burst = 2.0 * torch.sin(2 * torch.pi * torch.arange(4, device=dev, dtype=torch.float64) / 4 + torch.pi / 4)


def content(period):
    x = bed.clone()
    if period:
        for k in range(4):
            x[0, :, 2000 + k::period] = burst[k]
    return x


out = torch.empty((1, ch, n), dtype=torch.float64, device=dev)
mg, nl = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
ws = torch.empty(ops._lib.lib().dam_limiter_workspace_bytes(1, n) // 8, dtype=torch.float64, device=dev)
tp, sp = torch.empty((1, ch), dtype=torch.float64, device=dev), torch.empty((1, ch), dtype=torch.float64, device=dev)


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


for name, period in (('quiet', 0), ('sparse', int(0.75 * rate)), ('dense', 1000)):
    x = content(period).transpose(1, 2)
    t_meter = timed(lambda: ops.true_peak_batch(x, out=tp, sample_peak_out=sp), 50)
    t_lim = timed(lambda: ops.limiter_apply(x, -1.0, L, H, out=out, min_gain_out=mg, n_limited_out=nl, workspace=ws), 50)
    after = ops.true_peak_batch(out.transpose(1, 2))
    print('%s: limiter %.4f ms per call (three launches), meter %.4f ms (two launches), ratio %.2f; min gain %.4f, limited '
          'share %.4f, true peak %.3f -> %.6f dBTP'
          % (name, t_lim, t_meter, t_lim / t_meter, mg.item(), nl.item() / n, 20 * torch.log10(tp.max()).item(),
             20 * torch.log10(after.max()).item()))
traffic = ch * n * 8 * 3 + n * 8 * 2             # x read twice, out written once; r written and read
fmas, adds = ch * n * 36, n * (L + 1)
print('L %d, H %d; %.1f MB of traffic at 6.3 TB/s: %.4f ms; %.2f G float64 FMAs + %.2f G adds (dense) at %.1f T/s: %.4f ms'
      % (L, H, traffic / 1e6, traffic / HBM_BYTES_PER_S * 1e3, fmas / 1e9, adds / 1e9, FP64_OPS_PER_S / 1e12,
         (fmas + adds) / FP64_OPS_PER_S * 1e3))
