#!/usr/bin/env python3
"""Diagnostic: time of the band-spectrum meter (dam_spectrum_band_power) on the evaluator's measurement shape -- 4 stereo
float32 stems of 4 minutes at 44.1 kHz, n_fft 8192, hop 4096, the 28 third-octave bands of spectrum.band_edges(44100, 8192)
-- for one mix without gains (R = 1, the reference spectrum) and for nine gain-ramped mixes in one call (R = 9, as many
as the evaluator's variants), beside two yardsticks on the same device: features.stft of the pre-rendered mono sum at the
same n_fft / hop (the same FFT work plus a spectrum store; the meter reads stems x channels times the samples and stores
nothing) and the integrated loudness meter on the same stems.  `--trace` runs every call a few times and exits (for a
kernel trace taken around this script); `--host` also times the float64 numpy / torch composition on the CPU."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import features, loudness, spectrum

dev = torch.device('cuda', 0)
rate, n, S, ch, n_fft, hop = 44100, 44100 * 240, 4, 2, 8192, 4096
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((S, ch, n), generator=g, device=dev)
x = pcm.transpose(1, 2)
edges, centres = spectrum.band_edges(rate, n_fft)
gains9 = 0.5 + torch.rand((9, S, 120), generator=g, device=dev, dtype=torch.float64)      # a gain per 2 s chunk
mono = pcm.mean(dim=1).sum(dim=0, keepdim=True).contiguous()                              # [1, n]: the plain stem sum
meter = loudness.Meter(rate)
T = features.num_frames(n, hop)

calls = {
    'band spectrum R=1, no gains': lambda: spectrum.band_power_mix(x, None, n_fft=n_fft, hop=hop, edges=edges),
    'band spectrum R=9, 120 gains per stem': lambda: spectrum.band_power_mix(x, gains9, n_fft=n_fft, hop=hop, edges=edges),
    'features.stft of the mono sum': lambda: features.stft(mono, n_fft=n_fft, hop=hop),
    'integrated loudness of the 4 stems': lambda: meter.integrated_loudness_batch(x),
}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
print('%d stereo float32 stems of %d s at %d Hz, n_fft %d, hop %d: %d frames, %d bands' % (S, n // rate, rate, n_fft, hop, T, len(centres)))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for name, fn in calls.items():
    reps = 20
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print('  %-40s %.4f ms per call (events over %d calls, every launch and allocation of the call)' % (name, e0.elapsed_time(e1) / reps, reps))
for R in (1, 9):
    print('  sample loads R=%d: R T S channels n_fft 4 B = %.2f GB' % (R, R * T * S * ch * n_fft * 4 / 1e9))
levels = spectrum.relative_levels_db(spectrum.band_power_mix(x, None, n_fft=n_fft, hop=hop, edges=edges))[0]
print('  LTAS of white-noise stems, dB re total (rises 1 dB per third octave): %s' % levels.cpu().numpy().round(2).tolist())

if '--host' in sys.argv:
    host = pcm.cpu().numpy()
    t0 = time.perf_counter()
    xm = torch.from_numpy(host.astype(np.float64).mean(axis=1).sum(axis=0).astype(np.float32).astype(np.float64))
    X = torch.stft(xm, n_fft, hop, window=torch.hann_window(n_fft, dtype=torch.float32).double(), center=True,
                   pad_mode='reflect', return_complex=True)
    pw = (X.real ** 2 + X.imag ** 2).numpy()
    pw[1:-1] *= 2.0
    P = np.array([pw[edges[b]:edges[b + 1]].sum() for b in range(len(centres))]) / pw.shape[1]
    dt = time.perf_counter() - t0
    print('  host float64 composition (numpy mix, torch.stft, band fold), one mix: %.1f ms on %d threads; largest level '
          'difference to the device %.2e dB' % (dt * 1e3, torch.get_num_threads(),
                                                float(np.abs(spectrum.relative_levels_db(P) - levels.cpu().numpy()).max())))
