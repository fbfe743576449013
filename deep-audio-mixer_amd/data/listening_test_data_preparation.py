"""Excerpts for a listening test -- the reference's data/listening_test_data_preparation.py: for every song the stem sum
of the reference mix, of the raw stems and of every model's mix over one time interval, each brought to -20 LUFS and
written as ``{song_name}_{identifier}.wav``.  Same function names and arguments; the sum, the BS.1770 measurement, the
gain and the 16-bit quantisation run on the GPU (evaluation.LoudnessEvaluator.write_sum_to_target), the host writes the
encoded bytes.  ``ceiling_dbtp`` (not in the reference) holds every excerpt's true peak under that many dBTP: an excerpt
whose -20 LUFS rendering would clip is written quieter instead."""
import os

import numpy as np
import torch

from .. import staging
from ..evaluation import LoudnessEvaluator
from ..inference_utils import mix_song_smooth
from .dataset_utils import load_tracks_musdb18

TRACKLIST = ('bass', 'drums', 'vocals', 'other')
_evaluators = {}


def _evaluator(sr):
    if sr not in _evaluators:
        _evaluators[sr] = LoudnessEvaluator(sr, TRACKLIST)
    return _evaluators[sr]


def produce_mixture_and_save(track_dict: dict, song_name, identifier, save_dir, sr=44100, ceiling_dbtp=None):
    """track_dict {name: [channels, n]} (host arrays or CUDA tensors) -> ``save_dir/{song_name}_{identifier}.wav``: the sum
    of the tracks at -20 LUFS.  Returns the clipped-sample count."""
    tracks = list(track_dict.values())
    if all(torch.is_tensor(t) and t.is_cuda for t in tracks):
        pcm = torch.stack(tracks)
    else:
        arrays = [np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in tracks]
        np_dt = np.float32 if all(a.dtype == np.float32 for a in arrays) else np.float64
        dev = torch.device('cuda', torch.cuda.current_device())
        pcm = torch.empty((len(arrays),) + arrays[0].shape, dtype=torch.float32 if np_dt == np.float32 else torch.float64,
                          device=dev)
        pipe = staging.pipe_for(dev)
        for i, a in enumerate(arrays):
            pipe.upload(pcm[i], np.asarray(a, dtype=np_dt))
    if pcm.dim() == 2:
        pcm = pcm.unsqueeze(1)                      # mono stems [n]
    return _evaluator(sr).write_sum_to_target(pcm, None, os.path.join(save_dir, '{}_{}.wav'.format(song_name, identifier)),
                                              ceiling_dbtp=ceiling_dbtp)


def process_song(base_dir: str, song_name: str, time_interval: tuple, models: dict, dataset, save_dir, sr: int = 44100,
                 chunk_length: int = 2, ceiling_dbtp=None):
    """time_interval: (from, to) in seconds.  Writes the 'reference' excerpt (stems of ``base_dir/manual_gain_mixes``),
    the 'sum' excerpt (stems of ``base_dir/test``) and one excerpt per entry of ``models`` under its name: the entry
    called 'mix' is a mixing network applied with mix_song_smooth, every other one a baseline with ``forward(tracks)``."""
    sample_from, sample_to = int(time_interval[0] * sr), int(time_interval[1] * sr)

    def excerpt(sub_dir):
        loaded = load_tracks_musdb18(os.path.join(base_dir, sub_dir), song_name, tracklist=TRACKLIST, sr=sr)
        return {name: np.ascontiguousarray(track[..., sample_from:sample_to]) for name, track in loaded.items()}

    produce_mixture_and_save(excerpt('manual_gain_mixes'), song_name, 'reference', save_dir, sr, ceiling_dbtp)
    loaded_tracks = excerpt('test')
    produce_mixture_and_save(loaded_tracks, song_name, 'sum', save_dir, sr, ceiling_dbtp)
    for model_name, model in models.items():
        if model_name == 'mix':
            mixed_tracks, _, _ = mix_song_smooth(dataset, model, loaded_tracks, chunk_length=chunk_length, sr=sr)
        else:
            mixed_tracks = model.forward(loaded_tracks)
        produce_mixture_and_save(mixed_tracks, song_name, model_name, save_dir, sr, ceiling_dbtp)


def process_songlist(base_dir, songlist, time_intervals, models, dataset, save_dir='./test_data', sr: int = 44100,
                     ceiling_dbtp=None):
    os.makedirs(save_dir, exist_ok=True)
    for i, song_name in enumerate(songlist):
        print('{}/{}: {}'.format(i + 1, len(songlist), song_name))
        process_song(base_dir, song_name, time_intervals[i], models, dataset, save_dir, sr, ceiling_dbtp=ceiling_dbtp)
