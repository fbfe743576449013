#!/usr/bin/env python3
"""Diagnostic: time of the alignment (dam_align_estimate, dam_align_shift) on the meter shape -- 4 stereo float32 stems and a
float32 stereo mix of 4 minutes at 44.1 kHz, max_lag 4096 (frames of 16384 samples, hop 8192, 1292 frames) -- beside the
band-spectrum meter on the same stems on the same device, which does the same kind of work (LDS FFTs over the same samples):
at the alignment's own frame size and hop (n_fft 16384 / hop 8192: one transform per frame where the alignment makes two per
frame and stem) and at the size the meter was recorded with (8192 / 4096).  Every stem sits in the mix at an offset of its
own; the probe prints the lags that come back.  `--trace` runs every call a few times and exits (for a kernel trace taken
around this script)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import align, ops, spectrum

dev = torch.device('cuda', 0)
rate, n, S, ch, L = 44100, 44100 * 240, 4, 2, 4096
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
x = pcm.transpose(1, 2)
planted = [-4096, -300, 17, 2500]
late = align.shift_tracks(x, torch.tensor(planted, dtype=torch.int32, device=dev))
mix = (late * torch.tensor([0.75, 1.25, 1.5, 0.875], device=dev).view(S, 1, 1)).sum(dim=0)         # float32 [n, ch]
cap, F, N, H = ops.align_geometry(L)
T = -(-n // H)
edges16, _ = spectrum.band_edges(rate, 16384)
edges8, _ = spectrum.band_edges(rate, 8192)
lag = align.estimate_lag(x, mix, L)[0]

calls = {
    'estimate_lag, phat (cross spectrum, reduce, finish)': lambda: align.estimate_lag(x, mix, L),
    'estimate_lag, plain': lambda: align.estimate_lag(x, mix, L, weighting='plain'),
    'shift_tracks': lambda: align.shift_tracks(x, lag),
    'band spectrum R=1 at n_fft 16384 / hop 8192': lambda: spectrum.band_power_mix(x, None, n_fft=16384, hop=8192, edges=edges16),
    'band spectrum R=1 at n_fft 8192 / hop 4096': lambda: spectrum.band_power_mix(x, None, n_fft=8192, hop=4096, edges=edges8),
}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
print('%d stereo float32 stems + mix of %d s at %d Hz, max_lag %d: N %d, hop %d, %d frames, %d workgroups of %d frames per stem'
      % (S, n // rate, rate, L, N, H, T, -(-T // F), F))
est = align.estimate_lag(x, mix, L)
print('  planted %s -> lag %s, peak %s' % (planted, est[0].tolist(), [round(v, 3) for v in est[2].tolist()]))
print('  workspace %.1f MB' % (ops._lib.lib().dam_align_workspace_bytes(S, n, L) / 1e6))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for name, fn in calls.items():
    reps = 20
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print('  %-52s %.4f ms per call (events over %d calls, every launch and allocation of the call)' % (name, e0.elapsed_time(e1) / reps, reps))
print('  sample loads of the cross spectrum: T S channels (N + N/2) 4 B = %.2f GB; of the meter at 16384 / 8192: %.2f GB'
      % (T * S * ch * (N + N // 2) * 4 / 1e9, (1 + n // 8192) * S * ch * 16384 * 4 / 1e9))
