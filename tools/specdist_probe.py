#!/usr/bin/env python3
"""Diagnostic: time of the spectrogram distance (spectrum.spectrogram_distance + distance_summary) on the evaluator's shape --
4 stereo float32 stems of 4 minutes at 44.1 kHz, R = 9 gain rows of 120 windows against the stems' own reference mix, n_fft 2048
/ hop 1024, third-octave bands grown to every bin -- alternated with the composition it replaces on the same input: nine rendered
mixes (ops.mixdown_peak_normalize) -> features.stft -> dB, subtract, square and sum in torch.  Median of the repeats, events
around each call.  `--trace` runs both a few times and exits (for a kernel trace taken around this script)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import features, ops, spectrum

dev = torch.device('cuda', 0)
rate, n, S, ch, W, R, n_fft, hop, amin = 44100, 44100 * 240, 4, 2, 120, 9, 2048, 1024, 1e-5
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
ref_pcm = pcm * torch.tensor([0.75, 1.25, 1.5, 0.875], device=dev).view(S, 1, 1)       # the reference mix as its own stems
gains = 0.5 + torch.rand((R, S, W), generator=g, device=dev, dtype=torch.float64)
x, y = pcm.transpose(1, 2), ref_pcm.transpose(1, 2)
edges = spectrum.extend_edges(spectrum.band_edges(rate, n_fft, 3)[0], n_fft)[0]
B, T, nbins = len(edges) - 1, 1 + n // hop, n_fft // 2 + 1
ones = torch.ones((S, 1), dtype=torch.float64, device=dev)


def fused():
    sums, count = spectrum.spectrogram_distance(x, gains, y, None, n_fft=n_fft, hop=hop, edges=edges, n_windows=W, amin=amin)
    return spectrum.distance_summary(sums, count).mse


def level(stem_pcm, row):
    mix = ops.mixdown_peak_normalize(stem_pcm, row, normalize=False).to(torch.float32)            # [channels, n]
    spec = features.stft(mix.transpose(0, 1).unsqueeze(0), n_fft=n_fft, hop=hop)[0]                 # complex64 [bins, T]
    return 20.0 * torch.log10(spec.abs().clamp_min(amin))


def composed():
    ref_level = level(ref_pcm, ones)
    return torch.stack([((level(pcm, gains[r]) - ref_level) ** 2).sum() for r in range(R)]) / (nbins * T)


calls = {'fused': fused, 'composed': composed}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
a, b = fused(), composed()
print('%d stereo float32 stems of %d s at %d Hz, %d rows of %d windows, %d / %d, %d bands over %d bins, %d frames'
      % (S, n // rate, rate, R, W, n_fft, hop, B, nbins, T))
print('  mse of the rows, dB^2: fused %s' % ' '.join('%.4f' % v for v in a.tolist()))
print('                      composed %s   (float32 dB differences summed in float32: largest relative difference %.2e)'
      % (' '.join('%.4f' % v for v in b.tolist()), float(((a - b.double()).abs() / a).max())))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
times = {name: [] for name in calls}
reps = 15
for _ in range(reps):                                   # alternated: both see the same clock and the same neighbours
    for name, fn in calls.items():
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1))
pcm_bytes = S * ch * n * 4
for name in calls:
    ms = statistics.median(times[name])
    print('  %-8s median %.4f ms over %d alternated calls (min %.4f, max %.4f; events, every launch and allocation of the call)'
          % (name, ms, reps, min(times[name]), max(times[name])))
print('  fused bytes: stems %.1f MB read by every row of a frame\'s workgroup (once from HBM, the rows and the overlap from cache), the '
      'reference stems %.1f MB once, records %.1f MB written and read back; composed: %d mixes of %.1f MB and %d spectrograms of '
      '%.1f MB written and read back'
      % (pcm_bytes / 1e6, pcm_bytes / 1e6, ops._lib.lib().dam_specdist_workspace_bytes(R, n, n_fft, hop, B, W) / 1e6, R + 1, ch * n * 4 / 1e6, R + 1,
         nbins * T * 8 / 1e6))
