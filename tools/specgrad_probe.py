#!/usr/bin/env python3
"""Diagnostic: time of the fused gradient of the spectrogram distance (ops.specgrad) on the evaluator's shape -- 4 stereo
float32 stems of 4 minutes at 44.1 kHz, R = 9 gain rows of 120 nodes against the stems' own reference mix, n_fft 2048 / hop
1024 -- alternated with (a) the distance alone on the same inputs (ops.specdist_sums, one band, one window: T (1 + R) transforms
against T (1 + 2 R)) and (b) the composition a user had before: the mix formed in torch, torch.stft, float32 levels,
((L - L_ref)^2).sum().backward() into the gains, row by row.  Median of the repeats, events around each call.  `--trace` runs
the two library calls a few times and exits (for a kernel trace taken around this script)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import features, ops

dev = torch.device('cuda', 0)
rate, n, S, ch, W, R, n_fft, hop, amin = 44100, 44100 * 240, 4, 2, 120, 9, 2048, 1024, 1e-5
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
ref_pcm = pcm * torch.tensor([0.75, 1.25, 1.5, 0.875], device=dev).view(S, 1, 1)       # the reference mix as its own stems
gains = 0.5 + torch.rand((R, S, W), generator=g, device=dev, dtype=torch.float64)
x, y = pcm.transpose(1, 2), ref_pcm.transpose(1, 2)
T, nbins = 1 + n // hop, n_fft // 2 + 1
win, tw = features._get_tables(dev, n_fft)
edges = torch.tensor([0, nbins], dtype=torch.int32, device=dev)
node = (torch.arange(n, device=dev) // (n // W)).clamp_max(W - 1)
hann = torch.hann_window(n_fft, dtype=torch.float32, device=dev)


def fused():
    return ops.specgrad(x.unsqueeze(0), gains.unsqueeze(0), y.unsqueeze(0), None, win, tw, n_fft, hop, amin)[1][0]


def distance():
    return ops.specdist_sums(x, gains, y, None, win, tw, n_fft, hop, edges, 1, amin)[0]


def level(mix):
    spec = torch.stft(mix, n_fft, hop_length=hop, window=hann, center=True, pad_mode='reflect', return_complex=True)
    p = spec.real * spec.real + spec.imag * spec.imag
    return 10.0 * torch.log10(p.clamp_min(amin * amin))


def composed():
    mono, leaf = pcm.mean(dim=1), gains.clone().requires_grad_(True)
    with torch.no_grad():
        ref_level = level(ref_pcm.mean(dim=1).sum(dim=0))
    for r in range(R):                                                                   # (row by row: one graph resident at a time)
        mix = (mono * leaf[r].to(torch.float32)[:, node]).sum(dim=0)
        ((level(mix) - ref_level) ** 2).sum().backward()
    return leaf.grad


calls = {'fused': fused, 'distance': distance, 'composed': composed}
for name, fn in calls.items():
    for _ in range(3):
        if name != 'composed' or '--trace' not in sys.argv:
            fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
a, b = fused(), composed()
print('%d stereo float32 stems of %d s at %d Hz, %d rows of %d nodes, %d / %d, %d bins, %d frames'
      % (S, n // rate, rate, R, W, n_fft, hop, nbins, T))
rel = ((a - b).abs() / a.abs()).flatten()
print('  |fused - composed| / |fused| per entry: median %.3g, largest %.3g (float32 levels and sums in the composition; an entry is '
      'dominated by its bins nearest a spectral null, where the derivative goes as 1 / p)' % (float(rel.median()), float(rel.max())))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {name: [] for name in calls}
reps = 15
for _ in range(reps):                                   # alternated: all see the same clock and the same neighbours
    for name, fn in calls.items():
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
med = {name: statistics.median(times[name]) for name in calls}
for name in calls:
    print('  %-8s median %.4f ms over %d alternated calls (min %.4f, max %.4f; events, every launch and allocation of the call)'
          % (name, med[name], reps, min(times[name]), max(times[name])))
print('  fused / distance = %.3f (expected under 2: T (1 + 2 R) transforms against T (1 + R));  composed / fused = %.3f'
      % (med['fused'] / med['distance'], med['composed'] / med['fused']))
print('  records: %.1f MB written and read back' % (ops._lib.lib().dam_specgrad_workspace_bytes(1, R, S, n, n_fft, hop, W) / 1e6))
