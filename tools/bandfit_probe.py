#!/usr/bin/env python3
"""Diagnostic: time of the band gain fit (gainfit.fit_band_gains) on the evaluator's shape -- 4 stereo float32 stems of 4 minutes
at 44.1 kHz and their float32 mix, n_fft 4096 / hop 2048, third-octave bands, 120 windows -- alternated with the time-domain
fit (gainfit.fit_gains) on the same input, median of the repeats, beside the bytes its two stages move; then
LoudnessEvaluator.process_song_tracks(gain_fit=True) on a synthetic song of the same length with and without band_fit=True.
`--trace` runs every call a few times and exits (for a kernel trace taken around this script); `--no-evaluator` skips the
second part."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import gainfit, ops, spectrum

dev = torch.device('cuda', 0)
rate, n, S, ch, W, n_fft, hop = 44100, 44100 * 240, 4, 2, 120, 4096, 2048
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
x = pcm.transpose(1, 2)
true = 0.5 + torch.rand((S, W), generator=g, device=dev, dtype=torch.float64)
y = ops.mixdown_peak_normalize(pcm, true, normalize=False).to(torch.float32).transpose(0, 1)     # float32 [n, ch]
edges, centres = spectrum.band_edges(rate, n_fft, 3)
B, T, nbins = len(centres), 1 + n // hop, n_fft // 2 + 1
calls = {'band': lambda: gainfit.fit_band_gains(x, y, W, n_fft=n_fft, hop=hop, edges=edges),
         'time': lambda: gainfit.fit_gains(x, y, W)}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
gains, residual, target, status = calls['band']()
total = gainfit.band_residual_total(residual, target, status)
print('%d stereo float32 stems of %d s at %d Hz and their float32 mix, %d / %d, %d third-octave bands, %d windows, %d frames'
      % (S, n // rate, rate, n_fft, hop, B, W, T))
print('  recovered band gains: median |fit - true| = %.3g, band total residual <= %.3g, status %s'
      % (float((gains - true.unsqueeze(0)).abs().median()), float(total.max()), sorted(set(status.reshape(-1).tolist()))))
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
pcm_bytes = (S + 1) * ch * n * 4
spec_bytes = (S + 1) * ch * T * nbins * 8
band_bytes = pcm_bytes + 2 * spec_bytes                 # stage 1 reads the samples (the overlap comes from L2) and writes the spectra, stage 2 reads them
for name, nbytes in (('band', band_bytes), ('time', pcm_bytes)):
    ms = statistics.median(times[name])
    print('  %-4s fit: median %.4f ms over %d alternated calls (min %.4f, max %.4f; events, every launch and allocation of the call), '
          '%.1f MB = %.2f TB/s' % (name, ms, reps, min(times[name]), max(times[name]), nbytes / 1e6, nbytes / ms / 1e9))
print('  band fit bytes: samples %.1f MB, spectra %.1f MB written and read back; workspace %.1f MB in slabs of %.0f MiB'
      % (pcm_bytes / 1e6, spec_bytes / 1e6, ops._lib.lib().dam_bandfit_workspace_bytes(W, n, S, ch, n_fft, hop, B, 0) / 1e6, 128))
if '--no-evaluator' in sys.argv:
    sys.exit(0)

from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
from deep_audio_mixer_amd.models.model_resnet import ResNet18
keys = ('bass', 'drums', 'vocals', 'other')
rng = np.random.default_rng(0)
tracks = {k: (0.05 * rng.standard_normal((2, n))).astype(np.float32) for k in keys}
reference = {k: tracks[k] * np.float32(c) for k, c in zip(keys, (0.75, 1.25, 1.5, 0.875))}
torch.manual_seed(3)
model = ResNet18(n_stems=4, input_shape=(1025, 1 + 2 * rate // 1024)).cuda().eval()
d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :rate * 2].T for k, v in tracks.items()}, 'mix': tracks['bass'][:, :rate * 2].T}},
                                       chunk_length=2, sr=rate, tracklist=list(keys) + ['mix'])
ev = LoudnessEvaluator(rate, keys, dataset=d, d_mean_loudness={k: -23.0 for k in keys}, mix_model=model, seed=7)
variants = {'gain_fit=True': dict(gain_fit=True), 'gain_fit=True, band_fit=True': dict(gain_fit=True, band_fit=True)}
wall = {name: [] for name in variants}
for i in range(4):                                      # the first round warms up (graph capture, tables)
    for name, kw in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = ev.process_song_tracks(tracks, reference, 'probe', n_random_samples=5, chunk_length=2, **kw)
        torch.cuda.synchronize()
        if i:
            wall[name].append(time.perf_counter() - t0)
for name in variants:
    print('  process_song_tracks(%s): median %.1f ms of %d alternated calls (host clock around the call, uploads included)'
          % (name, 1e3 * statistics.median(wall[name]), len(wall[name])))
print('  oracle_residual <= %.3g, oracle_band_residual_total <= %.3g' % (max(stats['oracle_residual']), max(stats['oracle_band_residual_total'])))
