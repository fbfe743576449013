#!/usr/bin/env python3
"""Diagnostic: time of the gain fit's moments pass (dam_gainfit_moments) on the evaluator's shape -- 4 stereo float32 stems
of 4 minutes at 44.1 kHz against a float64 stereo target, 119 windows (2 s chunks) -- beside two meters that read the same
stems once on the same device (the true-peak meter, and the float64 mixdown that forms the fit's target), each with the
bytes it moves, and the solve and gain-error launches that follow it.  `--trace` runs every call a few times and exits (for a
kernel trace taken around this script)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import gainfit, ops

dev = torch.device('cuda', 0)
rate, n, S, ch, W = 44100, 44100 * 240, 4, 2, 119
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
x = pcm.transpose(1, 2)
true = 0.5 + torch.rand((S, W), generator=g, device=dev, dtype=torch.float64)
target = ops.mixdown_peak_normalize(pcm, true, normalize=False)                 # float64 [ch, n]: stems x known gain ramps
y = target.transpose(0, 1)
M = gainfit.moments(x, y, W)
fit, residual, status = gainfit.solve(M)
cand = 0.5 + torch.rand((9, S, W), generator=g, device=dev, dtype=torch.float64)
bytes_moments = (S * 4 + 8) * ch * n
bytes_stems = S * 4 * ch * n

calls = {
    'gain fit moments (4 stems + target)': (lambda: gainfit.moments(x, y, W), bytes_moments),
    'true-peak meter of the 4 stems': (lambda: ops.true_peak_batch(x), bytes_stems),
    'float64 mixdown of the 4 stems': (lambda: ops.mixdown_peak_normalize(pcm, true, normalize=False), bytes_stems + 8 * ch * n),
    'gain fit solve, 119 windows': (lambda: gainfit.solve(M), 0),
    'gain error, 9 variants': (lambda: gainfit.gain_error_device(fit, cand), 0),
}
for fn, _ in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
print('%d stereo float32 stems of %d s at %d Hz, float64 target, %d windows of %d samples' % (S, n // rate, rate, W, n // W))
print('  recovered gains: largest |fit - true| = %.3g, largest residual %.3g, status %s'
      % (float((fit - true).abs().max()), float(residual.max()), sorted(set(status.tolist()))))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for name, (fn, nbytes) in calls.items():
    reps = 50
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    rate_txt = ', %.1f MB = %.2f TB/s' % (nbytes / 1e6, nbytes / ms / 1e9) if nbytes else ''
    print('  %-38s %.4f ms per call (events over %d calls, every launch and allocation of the call)%s' % (name, ms, reps, rate_txt))
