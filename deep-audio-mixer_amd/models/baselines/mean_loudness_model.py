"""Loudness-normalisation baseline: every stem is brought to the mean loudness of that stem over the training set.
Same surface as the reference's models/baselines/mean_loudness_model.py:6-22; the meter is the HIP BS.1770 meter."""
import torch

from ... import ops
from ...loudness import Meter, normalize_loudness, target_gains_device


class MeanLoudnessModel:
    def __init__(self, d_mean_loudness: dict, sr=44100):
        self.mean_loudness = d_mean_loudness
        self.meter = Meter(sr)
        self.tracklist = ('bass', 'drums', 'vocals', 'other')

    def forward(self, x: dict) -> dict:
        result = {}
        for name in self.tracklist:
            track = x[name]                                  # [channels, samples], as load_tracks_* returns it
            measured = self.meter.integrated_loudness(track.T)
            result[name] = normalize_loudness(track.T, measured, self.mean_loudness[name]).T
        return result

    def device_gains(self, pcm, lufs=None):
        """pcm: CUDA [stems, channels, n] in tracklist order -> the stems' normalisation gains, CUDA float64 [stems]
        (batch meter + dam_loudness_target_gains; no host synchronisation).  lufs: the stems' loudness if already measured."""
        if lufs is None:
            lufs = self.meter.integrated_loudness_batch(pcm.transpose(1, 2))
        return target_gains_device(lufs, [self.mean_loudness[name] for name in self.tracklist])

    def forward_device(self, stems, out_dtype=None) -> dict:
        """forward() for stems that stay on the device: stems {track: CUDA [channels, n]} (or one CUDA tensor
        [stems, channels, n] in tracklist order) -> {track: CUDA [channels, n]}, float64 unless out_dtype says otherwise.
        One batched measurement, gains and product on the device, no host synchronisation and no clip warning."""
        pcm = stems if torch.is_tensor(stems) else torch.stack([stems[name] for name in self.tracklist])
        out = ops.gain_ramp_apply(pcm, self.device_gains(pcm).view(-1, 1), out_dtype=out_dtype)
        return {name: out[i] for i, name in enumerate(self.tracklist)}
