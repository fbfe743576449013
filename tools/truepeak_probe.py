#!/usr/bin/env python3
"""Diagnostic: (1) time of the true-peak meter (dam_true_peak_batch) on the loudness meter's measurement shape -- 4 stereo
float32 stems of 4 minutes at 44.1 kHz -- beside the time one read of those bytes takes at the achievable HBM rate and
the time its float64 FMAs take at the vector peak; (2) what the ceiling costs the C5 master graph: SongMixer(kind='master',
normalize='loudness', encode='PCM_16') with ceiling_dbtp=-1.0 against the same mixer without it, alternated over two rounds.
`--trace` runs only the meter a few times (for a kernel trace taken around this script)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import deep_audio_mixer_amd  # noqa: F401
from deep_audio_mixer_amd import inference_utils, ops
from deep_audio_mixer_amd.models.model_resnet import ResNet18

HBM_BYTES_PER_S = 6.3e12          # achievable, MI355X
FP64_FMA_PER_S = 78.6e12 / 2      # vector float64 peak, one FMA = 2 FLOP

dev = torch.device('cuda', 0)
rate, n, stems, ch = 44100, 44100 * 240, 4, 2
g = torch.Generator(device=dev).manual_seed(1)
pcm = 0.1 * torch.randn((stems, ch, n), generator=g, device=dev)
out = torch.empty((stems, ch), dtype=torch.float64, device=dev)
sp = torch.empty((stems, ch), dtype=torch.float64, device=dev)
x = pcm.transpose(1, 2)
for _ in range(3):
    ops.true_peak_batch(x, out=out, sample_peak_out=sp)
torch.cuda.synchronize()
if '--trace' in sys.argv:
    sys.exit(0)
reps = 50
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    ops.true_peak_batch(x, out=out, sample_peak_out=sp)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / reps
nbytes, fmas = stems * ch * n * 4, stems * ch * n * 36
t_hbm, t_fma = nbytes / HBM_BYTES_PER_S * 1e3, fmas / FP64_FMA_PER_S * 1e3
print('true peak, %d stereo float32 stems of %d s: %.4f ms per call (events over %d calls, both launches)' % (stems, n // rate, ms, reps))
print('  one read of %.1f MB at 6.3 TB/s: %.4f ms (%.2f of the call); %.2f G float64 FMAs at %.1f T/s: %.4f ms (%.2f of the call)'
      % (nbytes / 1e6, t_hbm, t_hbm / ms, fmas / 1e9, FP64_FMA_PER_S / 1e12, t_fma, t_fma / ms))
print('  true peaks (dBTP): %s' % (20 * torch.log10(out)).cpu().numpy().round(3).tolist())
del pcm, x

# (2) the C5 master graph with and without the ceiling
S, song, chunk = 8, rate * 180, rate * 3
torch.manual_seed(0)
model = ResNet18(n_stems=S, input_shape=(1025, 1 + chunk // 1024)).to(dev).eval()


def mixer_ms(ceiling, steps=20):
    m = inference_utils.SongMixer(model, S, 2, song, torch.float32, chunk, 'master', 'loudness', sr=rate, encode='PCM_16',
                                  ceiling_dbtp=ceiling)
    m.pcm.copy_(0.1 * torch.randn(m.pcm.shape, generator=torch.Generator(device=dev).manual_seed(1234), device=dev))
    for _ in range(3):
        m.launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.launch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, m.graph is not None


for rnd in range(2):
    for ceiling in (None, -1.0):
        ms, graphed = mixer_ms(ceiling)
        print('round %d: C5 song to PCM_16, normalize=loudness, ceiling_dbtp=%s: %.3f ms per song (hipGraph %s)' % (rnd, ceiling, ms, graphed))
