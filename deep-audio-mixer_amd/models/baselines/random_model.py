"""Random-gain baseline: every stem times one gain drawn uniformly from [gain_from, gain_to).  Same class, tracklist and
draw order as the reference's models/baselines/random_model.py:4-14 (one ``np.random.uniform`` per stem, in tracklist
order, from numpy's global generator), so a seeded run draws the reference's gains."""
import numpy as np
import torch

from ... import ops


class RandomModel:
    def __init__(self, gain_from=0.5, gain_to=1.5):
        self.tracklist = ('bass', 'drums', 'vocals', 'other')
        self._gain_from = gain_from
        self._gain_to = gain_to

    def draw(self) -> dict:
        """The gains of one forward(): {track: float}, drawn in tracklist order."""
        return {track: float(np.random.uniform(self._gain_from, self._gain_to)) for track in self.tracklist}

    def forward(self, x: dict) -> dict:
        """x: {track: [channels, n]}.  numpy stems are scaled as the reference scales them (``gain * x[track]``); CUDA
        tensors through ops.gain_ramp_apply with the one gain (float64 result, the numpy product's dtype)."""
        gains = self.draw()
        result = {}
        for track in self.tracklist:
            a = x[track]
            if torch.is_tensor(a):
                g = torch.tensor([gains[track]], dtype=torch.float64, device=a.device)
                result[track] = ops.gain_ramp_apply(a.reshape(1, -1), g).view(a.shape)
            else:
                result[track] = gains[track] * a
        return result
