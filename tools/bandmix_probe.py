#!/usr/bin/env python3
"""Diagnostic: time of the band-gain mixer (gainfit.render_band_gains) on the evaluator's shape -- 4 stereo float32 stems of 4
minutes at 44.1 kHz, n_fft 4096 / hop 2048, third-octave bands, one window per 2-second chunk -- alternated with the composition
a user had before it: features.stft of every stem and channel, a torch multiply by the gain map and sum over the stems,
features.istft.  Median of the repeats with their spread, beside the bytes each path moves and the algorithmic minimum (the
samples read once, the mix written once).  One process, one configuration; `--trace` runs each path a few times and exits (for a
kernel trace taken around this script: rocprofv3 --kernel-trace --stats -- python tools/bandmix_probe.py --trace)."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import features, gainfit, ops, spectrum

dev = torch.device('cuda', 0)
rate, seconds, S, ch, n_fft, hop = 44100, 240, 4, 2, 4096, 2048
n, W = rate * seconds, seconds // 2
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
x = pcm.transpose(1, 2)                                 # [S, n, ch] over planar storage
edges, centres = spectrum.band_edges(rate, n_fft, 3)
B, T, nbins = len(centres), 1 + n // hop, n_fft // 2 + 1
gains = 0.5 + torch.rand((B, S, W), generator=g, device=dev, dtype=torch.float64)
fill = 0.5 + torch.rand((S, W), generator=g, device=dev, dtype=torch.float64)

# the gain map of the composition, built once outside the clock: [S, bins, frames] float32
first = ops.gainfit_band_frame_windows(n, W, hop)
w_of_t = torch.repeat_interleave(torch.arange(W, device=dev), torch.tensor([first[w + 1] - first[w] for w in range(W)], device=dev))
band_of_k = torch.full((nbins,), B, dtype=torch.long, device=dev)
for b in range(B):
    band_of_k[int(edges[b]):int(edges[b + 1])] = b
table = torch.cat([gains, fill.unsqueeze(0)]).to(torch.float32)                  # [B + 1, S, W], the last row: outside every band
gain_map = table[band_of_k][:, :, w_of_t].permute(1, 0, 2).contiguous()          # [S, bins, T]
mono = pcm.reshape(S * ch, n)


def fused():
    return gainfit.render_band_gains(x, gains, n_fft=n_fft, hop=hop, edges=edges, fill=fill)


def composed():
    spec = features.stft(mono, n_fft=n_fft, hop=hop).view(S, ch, nbins, T)
    return features.istft((spec * gain_map.unsqueeze(1)).sum(0), hop=hop, length=n)


calls = {'fused': fused, 'composed': composed}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
a, b = fused(), composed()
print('%d stereo float32 stems of %d s at %d Hz, %d / %d, %d third-octave bands, %d windows, %d frames'
      % (S, seconds, rate, n_fft, hop, B, W, T))
print('  fused against composed: max |difference| %.3g at max |mix| %.3g' % (float((a - b).abs().max()), float(a.abs().max())))
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
pcm_bytes, out_bytes = S * ch * n * 4, ch * n * 4
spec_bytes, frame_bytes = S * ch * T * nbins * 8, ch * T * n_fft * 4
moved = {'fused': pcm_bytes + 2 * frame_bytes + out_bytes,            # samples in, the synthesised frames written and gathered, the mix out
         # the spectra written, read by the multiply with the map, the products written and read by the sum, the mix spectrum written and inverted
         'composed': pcm_bytes + 4 * spec_bytes + S * T * nbins * 4 + 2 * spec_bytes // S + out_bytes}
for name in calls:
    ms = statistics.median(times[name])
    print('  %-8s median %.4f ms over %d alternated calls (min %.4f, max %.4f; events, every launch and allocation of the call), '
          '%.1f MB = %.2f TB/s' % (name, ms, reps, min(times[name]), max(times[name]), moved[name] / 1e6, moved[name] / ms / 1e9))
print('  algorithmic minimum %.1f MB (samples in, mix out); fused workspace %.1f MB; spectra the composition writes %.1f MB'
      % ((pcm_bytes + out_bytes) / 1e6, ops._lib.lib().dam_bandmix_workspace_bytes(n, ch, n_fft, hop) / 1e6, spec_bytes / 1e6))
