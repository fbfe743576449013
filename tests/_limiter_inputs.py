"""Inputs the limiter tests share: the bed-plus-bursts song -- the four sine stems of test_master_truepeak_gpu.tone_song()
(8 kHz, 26 s + 77 samples) with the burst train of its click_song() added to stem 1: a 4-sample fs/4 burst at 45 degrees every
6000 samples, the second channel 0.8 of the first three samples later.  The bed carries the loudness, the bursts carry the
peaks: brought to -20 LUFS with unit gains and amplitude 3.0 the mix reads 4.745 dB over a -1 dBTP ceiling (host, oracle
meter), which a static clamp pays for with 4.745 LU and the limiter (5 ms / 20 ms) with 0.658."""
import numpy as np

import test_master_truepeak_gpu as tm
from _inputs import make_audio

SR, N, KEYS = tm.SR, tm.N, tm.KEYS


def burst_song(amplitude=3.0):
    song = {k: v.copy() for k, v in tm.tone_song().items()}
    burst = amplitude * np.sin(2 * np.pi * np.arange(4) / 4 + np.pi / 4)
    train = np.tile(make_audio('impulse', 6000, 0), N // 6000 + 1)[:N]           # one unit impulse at 2000 of every 6000
    x = np.convolve(train, burst)[:N]
    song[KEYS[1]] += np.stack([x, 0.8 * np.roll(x, 3)]).astype(np.float32)
    return song


def unit_mix(song):
    """The float64 stem sum with unit gains, [channels, n]."""
    return np.sum([song[k].astype(np.float64) for k in KEYS], axis=0)
