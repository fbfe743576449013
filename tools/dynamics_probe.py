#!/usr/bin/env python3
"""Diagnostic: the time-resolved loudness readings (Meter.loudness_dynamics_batch) beside the integrated meter on the shape
the meter was measured on -- 4 stereo float32 stems of 4 minutes at 44.1 kHz.  Prints end-to-end times; under
`rocprofv3 --kernel-trace --stats -- python3 tools/dynamics_probe.py` the kernel-stats file gives the per-kernel times quoted
in DESIGN.md section 7 (the dyn_* kernels are the new ones, the kw_* kernels are shared with the integrated meter)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import deep_audio_mixer_amd
from deep_audio_mixer_amd import loudness
rate, n, iters = 44100, 44100 * 240, 5
rng = np.random.RandomState(0)
env = 10.0 ** rng.uniform(-1.5, 0.0, 24).repeat(n // 24)                        # ten-second sections 0 .. 30 dB apart
x = (0.1 * rng.randn(4, n, 2) * env[None, :, None]).astype(np.float32)
xd = torch.from_numpy(x).cuda()
m = loudness.Meter(rate)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out


t_int, lufs = timed(lambda: m.integrated_loudness_batch(xd))
t_dyn, d = timed(lambda: m.loudness_dynamics_batch(xd))
print('integrated: %.3f ms end to end for 4 stems, %s LUFS' % (t_int, np.round(lufs.cpu().numpy(), 3).tolist()))
print('dynamics:   %.3f ms end to end for 4 stems, LRA %s LU, short-term max %s LUFS, %d short-term windows'
      % (t_dyn, np.round(d['lra'].cpu().numpy(), 3).tolist(), np.round(d['short_term_max'].cpu().numpy(), 3).tolist(),
         d['short_term'].shape[1]))
