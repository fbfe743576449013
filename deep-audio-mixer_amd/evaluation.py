"""Loudness evaluation of a mix against a reference mix -- the reference's evaluation.py:20-145 (``LoudnessEvaluator``):
per-stem BS.1770 loudness relative to the stems' mean, the mean absolute difference of two such profiles (the paper's
"loudness error"), and the whole-song comparison built on them (``process_song`` / ``process_songlist``: plain sum,
loudness-normalisation baseline, the model's mix and random mixes against a reference mix).  Same method names and
argument meaning; the meter is the HIP one (loudness.Meter), stems stay on the device.

The whole-song path uploads a song's stems once and never writes a scaled copy of them: the loudnorm and random variants
are constant gains, the model's mix is a gain ramp, and the batched meter applies either as it loads the samples
(Meter.integrated_loudness_batch(gains=...)); the mix variant is the 'loudness' kind of inference_utils.SongMixer, one
hipGraph from PCM to the four LUFS values.  With ``write_wavs_to_disk`` every variant's stem sum is also rendered on the
device from the same resident PCM by the mixer's own master tail (inference_utils.MasterChain) -- mixdown with the
variant's gains, batched meter, gain to -20 LUFS, PCM encoder with that gain -- and written as
``{song_name}_{identifier}.wav`` (evaluation.py:58-66); with ``ceiling_dbtp`` that gain is first clamped so that the file's
true peak stays under the ceiling (dam_true_peak_batch of the resident sum) instead of being hard-clipped by the encoder.
``limiter`` turns down only the peaks over the ceiling instead (dam_limiter_apply), so the file keeps its loudness;
``compressor`` puts the feed-forward compressor (dam_compressor_apply) in front of either.
The reference's spreadsheet (openpyxl) stays out: ``process_songlist`` returns the rows and the means instead of writing
./stats.xlsx.

``dynamics=True`` adds the time axis a mixer of time-varying gains is judged on: the same comparison per 3 s short-term
window (one every 100 ms; loudness.profile_error_device) -- '*_st_error' beside every '*_error' -- and the loudness range
(EBU Tech 3342) of the reference stems.  Two mixes of equal integrated loudness per stem, one of which is 3 dB hot in the
verses and 3 dB shy in the choruses, read the same '*_error'; their '*_st_error' differ.

``spectral=True`` adds the tonal axis the model is trained on (model_trainer.py:34-35 minimises a spectrogram distance,
the loudness errors only see level): every variant's long-term average spectrum in third-octave bands against the
reference mix's, each relative to its own total (spectrum.band_power_mix / balance_error_device) -- '*_spec_error' beside
every '*_error', in dB -- and 'ltas', the two spectra themselves.  Two mixes of equal loudness error, one of them
bass-heavy, differ here; scaling every stem by a common gain changes neither figure.

``gain_fit=True`` asks the direct question the three axes only circle: what gains did the reference mix use, and how far
are a variant's gains from them?  The reference stems' sum is fitted with the raw stems by windowed least squares over the
windows of the model's own gain ramp (gainfit.fit_gains): 'oracle_gains', 'oracle_residual' (the share of the reference no
gain-only mixer explains) and a '*_gain_error' beside every '*_error' -- the mean distance in dB from the fitted gains,
stem by stem and window by window, relative to each window's mean over the stems (gainfit.gain_error_device).

``band_fit=True`` asks what that residual is made of -- a human mix is mostly gain plus EQ per stem: the same fit per
fractional-octave band of the STFT (gainfit.fit_band_gains): 'oracle_band_gains' (the reference's EQ curve per stem),
'oracle_band_residual_total' (what per-band gains still leave unexplained: its distance in dB from 'oracle_residual' is the
headroom of a band-gain mixer over a gain-only one) and a '*_band_gain_error' beside every '*_gain_error' -- how far a
variant's broadband gains sit from the band-wise optimum.  ``band_render=True`` makes that band-gain mixer audible: the fitted
band gains rendered to audio (gainfit.render_band_gains), 'oracle_band_render_residual' -- what the render leaves of the
reference, measured on the audio -- and, with ``write_wavs_to_disk``, ``{song}_oracle_band.wav`` beside the other variants.

``feature_distance=True`` measures the training criterion itself on the audio a variant renders: the distance between the dB
spectrogram of "stems x the variant's gains" and the reference mix's, frame by frame and bin by bin, in the model's own
features (spectrum.spectrogram_distance) -- '*_feat_mse' (the criterion, dB^2) and '*_feat_error' (its level-free part, the
centred RMS in dB) beside every '*_error'.  '*_spec_error' and '*_st_error' are its two marginals: a mix that is bright in the
verses and dull in the choruses reads fine on both and badly here.
"""
import numbers
import os
from collections import OrderedDict
from statistics import mean

import numpy as np
import torch

from . import align, gainfit, inference_utils, ops, spectrum, staging
from .loudness import Meter, curve_stats_device, normalize_loudness, profile_error_device
from .models.baselines.mean_loudness_model import MeanLoudnessModel
from .models.baselines.random_model import RandomModel


class LoudnessEvaluator:
    def __init__(self, sr=44100, keys=('bass', 'drums', 'vocals', 'other'), *, dataset=None, d_mean_loudness=None,
                 mix_model=None, seed=None):
        """``LoudnessEvaluator(sr, keys)`` measures profiles; the whole-song methods also need what the reference's
        constructor takes (evaluation.py:22-30): the dataset (its tracklist names the stems the model mixes), the training
        set's mean loudness per stem and the mixing model.  ``seed`` seeds numpy's global generator, as there."""
        if seed:
            np.random.seed(seed)
        self.sr = sr
        self.meter = Meter(sr)
        self.keys = tuple(keys)
        self.d = dataset
        self.mix_model = mix_model
        self.mean_loudness_model = MeanLoudnessModel(d_mean_loudness, sr) if d_mean_loudness is not None else None
        self.random_model = RandomModel()

    def evaluate_loudness(self, tracks: dict) -> list:
        """evaluation.py:39-46: loudness of every stem ([channels, samples] each) minus the mean over the stems."""
        per_track_loudness = [self.meter.integrated_loudness(tracks[name].T) for name in self.keys]
        avg_loudness = mean(per_track_loudness)
        return [l - avg_loudness for l in per_track_loudness]

    @staticmethod
    def _calculate_diff_between_loudness_dicts(l_dict1: OrderedDict, l_dict2: OrderedDict):
        """evaluation.py:48-53."""
        a1 = np.array(list(l_dict1.values()))
        a2 = np.array(list(l_dict2.values()))
        return float(np.mean(np.abs(a1 - a2)))

    def sum_tracks_to_target(self, track_dict: dict, target_lufs: float = -20.0):
        """evaluation.py:59-66 without the file write: stem sum, measured, brought to target_lufs."""
        stems = [track_dict[k] for k in track_dict]
        if torch.is_tensor(stems[0]):
            track_sum = torch.stack(stems).sum(dim=0)
        else:
            track_sum = np.sum(np.array(stems), axis=0)
        loudness = self.meter.integrated_loudness(track_sum.T)
        return normalize_loudness(track_sum.T, loudness, target_lufs)

    def _sum_and_evaluate_tracks(self, track_dict, reference_dict):
        """evaluation.py:55-75: (loudness profile, error against reference_dict or None)."""
        loudness_dict = OrderedDict(zip(self.keys, self.evaluate_loudness(track_dict)))
        if reference_dict:
            return loudness_dict, self._calculate_diff_between_loudness_dicts(loudness_dict, reference_dict)
        return loudness_dict, None

    # ---- batched device form and the whole-song comparison (evaluation.py:77-145)
    def evaluate_loudness_batch(self, stems, gains=None) -> list:
        """evaluate_loudness in one batched measurement.  stems: CUDA [stems, channels, n] in ``keys`` order, or
        {name: CUDA [channels, n]} (stacked: one device copy); gains: optional CUDA float64 [stems] or [stems, n_gains],
        the stems are then measured as ``stem * gain ramp`` without that product being written.  The [stems] loudness
        values come to the host in one copy."""
        pcm = stems if torch.is_tensor(stems) else torch.stack([stems[name] for name in self.keys])
        lufs = self.meter.integrated_loudness_batch(pcm.transpose(1, 2), gains=gains)
        return self._profile(lufs.cpu().tolist())

    def evaluate_short_term_batch(self, stems, gains=None):
        """Short-term loudness curve (3 s window, one value per 100 ms) of every stem, measured as ``stem * gain ramp`` where
        gains are given; stems and gains as evaluate_loudness_batch takes them -> CUDA float64 [stems, windows].  Nothing
        comes to the host."""
        pcm = stems if torch.is_tensor(stems) else torch.stack([stems[name] for name in self.keys])
        return self.meter.short_term_loudness_batch(pcm.transpose(1, 2), gains=gains)

    SPECTRAL_DEFAULTS = {'n_fft': 8192, 'hop': None, 'fraction': 3, 'f_lo': 25.0, 'f_hi': 20000.0}     # hop None: n_fft / 2

    def _spectral_args(self, spectral):
        """``spectral`` as the whole-song methods take it (True, or a dict with any of n_fft, hop, fraction, f_lo, f_hi)
        -> (n_fft, hop, edges, centres)."""
        given = {} if spectral is True else dict(spectral)
        unknown = set(given) - set(self.SPECTRAL_DEFAULTS)
        if unknown:
            raise ValueError('spectral: unknown keys %s (expected any of %s)' % (sorted(unknown), sorted(self.SPECTRAL_DEFAULTS)))
        o = dict(self.SPECTRAL_DEFAULTS, **given)
        hop = o['n_fft'] // 2 if o['hop'] is None else o['hop']
        edges, centres = spectrum.band_edges(self.sr, o['n_fft'], o['fraction'], o['f_lo'], o['f_hi'])
        return o['n_fft'], hop, edges, centres

    GAIN_FIT_DEFAULTS = {'pool': 0, 'ridge': 0.0, 'align': None}

    def _gain_fit_args(self, gain_fit):
        """``gain_fit`` as the whole-song methods take it (True, or a dict with any of pool, ridge, align) -> (pool, ridge);
        _gain_fit_align gives its align."""
        given = {} if gain_fit is True else dict(gain_fit)
        unknown = set(given) - set(self.GAIN_FIT_DEFAULTS)
        if unknown:
            raise ValueError('gain_fit: unknown keys %s (expected any of %s)' % (sorted(unknown), sorted(self.GAIN_FIT_DEFAULTS)))
        o = dict(self.GAIN_FIT_DEFAULTS, **given)
        return ops.gainfit_check_solve_args(o['pool'], o['ridge'])

    def _gain_fit_align(self, gain_fit):
        """-> None, or the largest lag in samples the stems are searched for against the reference (the 'align' key)."""
        max_lag = None if gain_fit is True else dict(gain_fit).get('align')
        if max_lag is not None:
            ops.align_check_shapes((1, 1, 1), None, max_lag)
        return max_lag

    BAND_FIT_DEFAULTS = {'n_fft': 4096, 'hop': None, 'fraction': 3, 'f_lo': 25.0, 'f_hi': 20000.0, 'pool': 0, 'ridge': 0.0,
                         'align': None}                    # hop None: n_fft / 2

    def _band_fit_args(self, band_fit):
        """``band_fit`` as the whole-song methods take it (True, or a dict with any of n_fft, hop, fraction, f_lo, f_hi, pool,
        ridge, align) -> a dict of n_fft, hop, edges, centres (spectrum.band_edges at the evaluator's rate), pool, ridge, align."""
        given = {} if band_fit is True else dict(band_fit)
        unknown = set(given) - set(self.BAND_FIT_DEFAULTS)
        if unknown:
            raise ValueError('band_fit: unknown keys %s (expected any of %s)' % (sorted(unknown), sorted(self.BAND_FIT_DEFAULTS)))
        o = dict(self.BAND_FIT_DEFAULTS, **given)
        hop = o['n_fft'] // 2 if o['hop'] is None else o['hop']
        # (the shapes are placeholders: what is checked here is n_fft, hop and the number of bands)
        edges, centres = spectrum.band_edges(self.sr, o['n_fft'], o['fraction'], o['f_lo'], o['f_hi'])
        n_fft, hop = ops.gainfit_band_check_shapes((1, o['n_fft'], 1), (o['n_fft'], 1), 1, o['n_fft'], hop, len(centres))[4:]
        pool, ridge = ops.gainfit_check_solve_args(o['pool'], o['ridge'])
        if o['align'] is not None:
            ops.align_check_shapes((1, 1, 1), None, o['align'])
        return {'n_fft': n_fft, 'hop': hop, 'edges': edges, 'centres': centres, 'pool': pool, 'ridge': ridge, 'align': o['align']}

    @staticmethod
    def _band_render_args(band_render, band_fit):
        """``band_render`` as the whole-song methods take it (False, True, or {'fill': 'broadband' | number}) -> None where it is
        off, else the fill: 'broadband' or a float.  It renders what ``band_fit`` fits: ValueError without it."""
        if not band_render:
            return None
        if not band_fit:
            raise ValueError('band_render renders the gains band_fit fits: it needs band_fit')
        given = {} if band_render is True else dict(band_render)
        unknown = set(given) - {'fill'}
        if unknown:
            raise ValueError("band_render: unknown keys %s (expected 'fill')" % sorted(unknown))
        fill = given.get('fill', 'broadband')
        if isinstance(fill, str):
            if fill != 'broadband':
                raise ValueError("band_render: fill must be 'broadband' or a number, got %r" % fill)
            return fill
        if isinstance(fill, bool) or not isinstance(fill, numbers.Real):
            raise ValueError("band_render: fill must be 'broadband' or a number, got %r" % (fill,))
        return float(fill)

    FEATURE_DISTANCE_DEFAULTS = {'n_fft': 2048, 'hop': 1024, 'fraction': 3}          # the model's own features

    def _feature_distance_args(self, feature_distance):
        """``feature_distance`` as the whole-song methods take it (True, or a dict with any of n_fft, hop, fraction) ->
        (n_fft, hop, edges, centres): the fractional-octave table at the evaluator's rate grown by one band below and one above
        where bins are left (spectrum.extend_edges), so that the cells cover every bin and their total is the criterion; the
        centre of such a band is the mean frequency of its bins."""
        given = {} if feature_distance is True else dict(feature_distance)
        given.pop('sensitivity', None)                      # (a switch, not a parameter of the features: _feature_sensitivity)
        unknown = set(given) - set(self.FEATURE_DISTANCE_DEFAULTS)
        if unknown:
            raise ValueError('feature_distance: unknown keys %s (expected any of %s)'
                             % (sorted(unknown), sorted(self.FEATURE_DISTANCE_DEFAULTS) + ['sensitivity']))
        o = dict(self.FEATURE_DISTANCE_DEFAULTS, **given)
        if 'n_fft' in given and 'hop' not in given:
            o['hop'] = None                                 # (n_fft / 2, as everywhere)
        # (the shapes are placeholders: what is checked here is n_fft and hop)
        n_fft, hop = ops.specdist_check_shapes((1, o['n_fft'], 1), None, (1, o['n_fft'], 1), None, o['n_fft'], o['hop'], 1)[6:8]
        edges, centres = spectrum.band_edges(self.sr, n_fft, o['fraction'])
        edges, low, high = spectrum.extend_edges(edges, n_fft)
        mid = lambda a, b: 0.5 * (int(a) + int(b) - 1) * self.sr / n_fft
        centres = ([mid(edges[0], edges[1])] if low else []) + centres.tolist() + ([mid(edges[-2], edges[-1])] if high else [])
        return n_fft, hop, edges, centres

    @staticmethod
    def _feature_sensitivity(feature_distance):
        """Does ``feature_distance`` ask for the '*_feat_sens' keys ({'sensitivity': True, ...})?"""
        return feature_distance is not True and bool(dict(feature_distance).get('sensitivity', False))

    def evaluate_spectrum_batch(self, stems, gains=None, **spectral):
        """Band powers of the stem sum (long-term average spectrum in fractional-octave bands at the evaluator's rate),
        measured as ``sum of stem * gain ramp`` where gains are given, without that sum being written.  stems as
        evaluate_loudness_batch takes them; gains: None, CUDA float64 [stems] or [stems, n_gains] (one mix), or
        [R, stems, n_gains] (R mixes in one call); keywords n_fft, hop, fraction, f_lo, f_hi (8192, n_fft / 2, 3, 25, 20000)
        -> CUDA float64 [R, bands]; spectrum.relative_levels_db turns a row into dB re its total.  Nothing comes to the
        host."""
        n_fft, hop, edges, _ = self._spectral_args(spectral)
        pcm = stems if torch.is_tensor(stems) else torch.stack([stems[name] for name in self.keys])
        return spectrum.band_power_mix(pcm.transpose(1, 2), gains, n_fft=n_fft, hop=hop, edges=edges)

    @staticmethod
    def _profile(per_track_loudness):
        avg_loudness = mean(per_track_loudness)
        return [l - avg_loudness for l in per_track_loudness]

    def _upload(self, tracks):
        first = np.asarray(tracks[self.keys[0]])
        np_dt = np.float32 if first.dtype == np.float32 else np.float64
        pcm = torch.empty((len(self.keys),) + first.shape, dtype=torch.float32 if np_dt == np.float32 else torch.float64,
                          device=inference_utils.device)
        pipe = staging.pipe_for(pcm.device)
        for i, name in enumerate(self.keys):
            pipe.upload(pcm[i], np.asarray(tracks[name], dtype=np_dt))
        return pcm

    def write_sum_to_target(self, pcm, gains, path, target_lufs: float = -20.0, subtype='PCM_16', ceiling_dbtp=None,
                            limiter=None, compressor=None):
        """evaluation.py:58-66 with its ``sf.write``, for stems resident on the device: pcm CUDA [stems, channels, n],
        gains None, CUDA float64 [stems] (a constant per stem) or [stems, n_gains] (a gain ramp).  The float64 stem sum is
        measured, the gain to ``target_lufs`` stays on the device and is applied inside the encoder; the host receives the
        file's sample bytes.  ceiling_dbtp: the gain is clamped on the device to ``ceiling / true peak of the sum`` first, so
        a sum whose -20 LUFS rendering would exceed the ceiling is written quieter instead of clipped.  limiter (None, True
        or {'lookahead_ms', 'hold_ms'}, as inference_utils.MasterChain takes it): only the peaks over the ceiling (-1 dBTP if
        none is given) are turned down, the rest of the file stays at ``target_lufs``.  compressor (None, True or a dict with keys of
        MasterChain.COMPRESSOR_DEFAULTS): the sum at ``target_lufs`` is compressed and brought to ``target_lufs`` again first.
        Returns the clipped-sample count."""
        from .data.dataset_utils import write_wav_bytes
        n_stems, channels, n = pcm.shape
        if gains is None:
            gains = torch.ones((n_stems, 1), dtype=torch.float64, device=pcm.device)
        # built per call, not cached: excerpt lengths vary
        chain = inference_utils.MasterChain(channels, n, pcm.device, 'loudness', sr=self.sr, target_lufs=target_lufs,
                                            ceiling_dbtp=ceiling_dbtp, encode=subtype, limiter=limiter,
                                            compressor=compressor)
        chain.render(pcm, gains.view(n_stems, -1))
        payload = staging.pipe_for(pcm.device).download(chain.enc)
        clipped = int(chain.clip.sum().item())
        write_wav_bytes(path, payload, self.sr, channels, subtype, n, clipped)
        return clipped

    def process_song_tracks(self, loaded_tracks: dict, reference_tracks: dict, song_name: str, n_random_samples: int = 5,
                            chunk_length: int = 2, write_wavs_to_disk=False, results_dir='./experiment',
                            ceiling_dbtp=None, dynamics=False, limiter=None, spectral=False, gain_fit=False, band_fit=False,
                            band_render=False, feature_distance=False, compressor=None) -> dict:
        """evaluation.py:77-116 on stems already in memory ({name: ndarray [channels, n]} each): the loudness profile of
        ``reference_tracks`` against the profiles of ``loaded_tracks`` summed as they are ('sum_error'), normalised to the
        training set's mean loudness ('loudnorm_error'), mixed by the model ('mix_error') and scaled by random gains
        ('random_error', the mean over n_random_samples draws, drawn in the reference's order).  Returns the reference's
        stats dict plus 'smooth_gains' {name: list}, the gains the mix variant used.  write_wavs_to_disk: every variant's
        stem sum at -20 LUFS goes to ``results_dir/{song_name}_{identifier}.wav`` (reference, sum, loudnorm, mix,
        random_0 ...; 16-bit), each held under ``ceiling_dbtp`` dBTP if that is given, by the look-ahead ``limiter`` if one is
        asked for, behind the ``compressor`` if one is asked for (write_sum_to_target); the stats and the order of the random
        draws depend on none of the four.
        dynamics: the stats gain 'sum_st_error', 'loudnorm_st_error', 'mix_st_error' and
        'random_st_error' -- every variant's error taken per short-term window instead of per song, from the gains the
        variant already passes to the meter -- and 'lra' {name: LU}, the loudness range of each reference stem; the other
        keys, their values and the order of the random draws do not depend on it.  The reference mix and the stems must
        then be of one length.
        spectral (True, or a dict with any of n_fft, hop, fraction, f_lo, f_hi; defaults 8192, n_fft / 2, 3, 25, 20000): the
        stats gain, after any dynamics keys, 'sum_spec_error', 'loudnorm_spec_error', 'mix_spec_error', 'random_spec_error'
        (the mean over the draws) -- the spectral-balance error in dB of every variant's stem sum against the reference
        stems' sum, measured from the gains the variant already passes to the meter (the draws in one call) -- and 'ltas'
        {'centres': [Hz], 'reference': [dB re total], 'mix': [...]}.  Nothing else depends on it; the lengths may differ
        (a long-term AVERAGE spectrum).
        gain_fit (True, or a dict with any of pool, ridge; defaults 0, 0.0 -- gainfit.solve explains them): the stats gain,
        after any dynamics and spectral keys, 'sum_gain_error' (unit gains), 'loudnorm_gain_error', 'mix_gain_error' (the
        model's smoothed gains), 'random_gain_error' (the mean over the draws) -- each variant's distance in dB from the gains
        that best rebuild the float64 sum of the reference stems from ``loaded_tracks``, one per stem and window of the
        model's gain ramp, relative to each window's mean over the stems -- 'oracle_gains' {name: [windows]}, those fitted
        gains (NaN where a stem is silent), and 'oracle_residual' [windows], the share of the reference's energy they leave
        unexplained.  Nothing else depends on it.  The reference mix and the stems must be of one length.
        gain_fit={'align': max_lag_samples} is for a reference that is not aligned with ``loaded_tracks`` (a mix that did not
        come out of this package): every stem's lag against the reference within +-max_lag is estimated on the device
        (align.estimate_lag with the plain weighting: a stem that is a component of the reference peaks at its own offset
        whatever its spectrum, where the PHAT weighting loses a near-sinusoidal stem) and the stems are shifted by it before
        the fit; the stats gain 'oracle_lag' {name: samples, positive where the reference is late} and 'oracle_lag_peak'
        {name: the normalised correlation at that lag, 0 .. 1, NaN for a silent stem}.  Absent (the default), nothing is
        estimated and no key is added.
        band_fit (True, or a dict with any of n_fft, hop, fraction, f_lo, f_hi, pool, ridge, align; BAND_FIT_DEFAULTS): the
        same fit taken per frequency band (gainfit.fit_band_gains on the same target, fractional-octave bands at the
        evaluator's rate).  The stats gain, after any gain_fit keys, 'oracle_band_centres' [bands] in Hz, 'oracle_band_gains'
        {name: [bands][windows]} -- the reference's EQ curve per stem --, 'oracle_band_residual' [bands][windows],
        'oracle_band_residual_total' [windows] -- the share of the reference that per-band gains leave unexplained: its
        distance in dB from 'oracle_residual' is the headroom of a band-gain mixer over a gain-only one -- and
        'sum_band_gain_error', 'loudnorm_band_gain_error', 'mix_band_gain_error', 'random_band_gain_error': each variant's
        broadband gains against the band-wise optimum, the gain error over every (band, window) with the variant's curve
        repeated over the bands.  'align' is gain_fit's; where both ask for the same lag the stems are aligned once.  It needs
        no gain_fit, changes no other key and comes to the host in the same copy.  The lengths must agree.
        band_render (True, or {'fill': 'broadband' | number}; needs band_fit, whose hop must then not exceed n_fft / 2): the
        fitted band gains are rendered to audio on the band fit's stems (gainfit.render_band_gains) -- the best band-gain mix.
        fill is the gain of the bins outside the bands and of the cells that were not fitted: 'broadband' (the default) takes the
        broadband fit's gains (gainfit.fit_gains on the same stems with band_fit's pool and ridge; gain_fit's result where its
        arguments are the same), a number that constant.  The stats gain, after the band_fit keys, 'oracle_band_render_residual'
        [windows]: the share of the fit target's energy that (target - render) holds in every window, from the time-domain
        moments of the two -- the time-domain counterpart of 'oracle_band_residual_total', in the same copy to the host.  With
        write_wavs_to_disk the render goes to ``{song_name}_oracle_band.wav`` as the other variants do (-20 LUFS, the ceiling
        and the limiter).  Off (the default), nothing changes.
        feature_distance (True, or a dict with any of n_fft, hop, fraction; defaults 2048, 1024, 3 -- the model's features):
        the dB-spectrogram distance of every variant's rendered stem sum from the reference stems' sum
        (spectrum.spectrogram_distance over third-octave bands grown to cover every bin and the windows of the model's gain
        ramp; every variant in one call, from the gains it already passes to the meter; one copy to the host).  The stats gain,
        after every other key, 'sum_feat_error', 'loudnorm_feat_error', 'mix_feat_error', 'random_feat_error' (the mean over the
        draws): the centred RMS of the difference in dB, which a common gain does not move; the same four as '*_feat_mse': the
        mean squared difference in dB^2, the criterion as trained; and 'feat_profile' {'centres': [Hz], 'mix_band_rms': [bands],
        'mix_window_rms': [windows]}, the centred RMS of the model's mix per band and per window.  Nothing else depends on it.
        The reference mix and the stems must be of one length.  With 'sensitivity': True in the dict, after those keys,
        'sum_feat_sens', 'loudnorm_feat_sens', 'mix_feat_sens', 'random_feat_sens' (the mean over the draws) [stems][windows]:
        the change of the variant's '*_feat_mse' in dB^2 per dB of that stem in that gain window (one fused
        spectrum.spectrogram_distance_grad call, every variant a row; a window must hold at least n_fft samples)."""
        render_fill = self._band_render_args(band_render, band_fit)
        if self.d is None or self.mix_model is None or self.mean_loudness_model is None:
            raise ValueError('process_song needs the dataset, d_mean_loudness and mix_model constructor arguments')
        stems = [t for t in self.d.get_tracklist() if t != 'mix']
        if tuple(stems) != self.keys or self.keys != self.random_model.tracklist:
            raise ValueError('the dataset tracklist and the evaluator keys must both be %s' % (self.random_model.tracklist,))
        if dynamics and np.asarray(reference_tracks[self.keys[0]]).shape[-1] != np.asarray(loaded_tracks[self.keys[0]]).shape[-1]:
            raise ValueError('dynamics=True compares window by window: the reference mix and the stems differ in length')
        if band_fit:
            band = self._band_fit_args(band_fit)
            if np.asarray(reference_tracks[self.keys[0]]).shape[-1] != np.asarray(loaded_tracks[self.keys[0]]).shape[-1]:
                raise ValueError('band_fit fits frame by frame: the reference mix and the stems differ in length')
            if render_fill is not None and band['hop'] > band['n_fft'] // 2:
                raise ValueError('band_render overlap-adds the frames: hop must not exceed n_fft / 2 (got %d for n_fft %d)'
                                 % (band['hop'], band['n_fft']))
        if gain_fit:
            (fit_pool, fit_ridge), fit_align = self._gain_fit_args(gain_fit), self._gain_fit_align(gain_fit)
            if np.asarray(reference_tracks[self.keys[0]]).shape[-1] != np.asarray(loaded_tracks[self.keys[0]]).shape[-1]:
                raise ValueError('gain_fit fits sample by sample: the reference mix and the stems differ in length')
        if feature_distance:
            feat_n_fft, feat_hop, feat_edges, feat_centres = self._feature_distance_args(feature_distance)
            if np.asarray(reference_tracks[self.keys[0]]).shape[-1] != np.asarray(loaded_tracks[self.keys[0]]).shape[-1]:
                raise ValueError('feature_distance compares frame by frame: the reference mix and the stems differ in length')
        stats = {'song_name': song_name}

        def write(identifier, pcm, gains=None):
            if write_wavs_to_disk:
                os.makedirs(results_dir, exist_ok=True)
                self.write_sum_to_target(pcm, gains, os.path.join(results_dir, '{}_{}.wav'.format(song_name, identifier)),
                                         ceiling_dbtp=ceiling_dbtp, limiter=limiter, compressor=compressor)

        reference_pcm = self._upload(reference_tracks)
        reference = OrderedDict(zip(self.keys, self.evaluate_loudness_batch(reference_pcm)))
        write('reference', reference_pcm)
        if dynamics:
            reference_power, reference_st = self.meter.short_term_batch(reference_pcm.transpose(1, 2))
            reference_lra = curve_stats_device(reference_power)[:, 0]
            candidates_st = []                              # sum, loudnorm, mix, random_0 ...: [stems, windows] each
        if spectral:
            n_fft, hop, edges, centres = self._spectral_args(spectral)

            def band_power(stem_pcm, g=None):               # -> [mixes, bands]; g: None, [stems], [stems, n] or [R, stems, 1]
                return spectrum.band_power_mix(stem_pcm.transpose(1, 2), g, n_fft=n_fft, hop=hop, edges=edges)
            reference_spec = band_power(reference_pcm)
            drawn_gains = []
        if gain_fit or band_fit:                            # the fit's target: the float64 sum of the reference stems, [channels, n]
            fit_target = ops.mixdown_peak_normalize(reference_pcm, torch.ones((len(self.keys), 1), dtype=torch.float64,
                                                                              device=reference_pcm.device), normalize=False)
            candidates_fit = []                             # loudnorm, then the draws: [stems] each
        if feature_distance:                                # the reference stays resident until the distance is taken
            feat_reference, candidates_feat = reference_pcm, []                            # loudnorm, then the draws: [stems] each
        del reference_pcm

        def error(profile):
            return self._calculate_diff_between_loudness_dicts(OrderedDict(zip(self.keys, profile)), reference)

        # mixed by the model: the song is uploaded here, once -- the other variants read the mixer's PCM buffer
        mixer, arrays = inference_utils._mixer(self.mix_model, stems, loaded_tracks, chunk_length, self.sr, 'loudness', False,
                                               torch.float64)
        mix_lufs, gains = mixer.run(arrays)
        pcm = mixer.pcm
        lufs = self.meter.integrated_loudness_batch(pcm.transpose(1, 2))
        stats['sum_error'] = error(self._profile(lufs.cpu().tolist()))
        write('sum', pcm)
        if dynamics:
            candidates_st.append(self.evaluate_short_term_batch(pcm))
        if spectral:
            candidates_spec = [band_power(pcm)]             # sum, loudnorm, mix, then the draws: [1 or draws, bands] each
        # each multitrack is normalized to the mean loudness of the corresponding track from train set
        loudnorm_gains = self.mean_loudness_model.device_gains(pcm, lufs)
        stats['loudnorm_error'] = error(self.evaluate_loudness_batch(pcm, loudnorm_gains))
        write('loudnorm', pcm, loudnorm_gains)
        if dynamics:
            candidates_st.append(self.evaluate_short_term_batch(pcm, loudnorm_gains))
        if spectral:
            candidates_spec.append(band_power(pcm, loudnorm_gains))
        if gain_fit or band_fit:
            candidates_fit.append(loudnorm_gains.reshape(-1))
        if feature_distance:
            candidates_feat.append(loudnorm_gains.reshape(-1))
        stats['mix_error'] = error(self._profile([float(v) for v in mix_lufs]))
        write('mix', pcm, mixer.gains[1])
        if dynamics:
            candidates_st.append(self.evaluate_short_term_batch(pcm, mixer.gains[1]))
        if spectral:
            candidates_spec.append(band_power(pcm, mixer.gains[1]))
        random_errors = []
        for exp_i in range(n_random_samples):
            drawn = self.random_model.draw()
            g = torch.tensor([drawn[name] for name in self.keys], dtype=torch.float64, device=pcm.device)
            random_errors.append(error(self.evaluate_loudness_batch(pcm, g)))
            write('random_{}'.format(exp_i), pcm, g)
            if dynamics:
                candidates_st.append(self.evaluate_short_term_batch(pcm, g))
            if spectral:
                drawn_gains.append(g)
            if gain_fit or band_fit:
                candidates_fit.append(g)
            if feature_distance:
                candidates_feat.append(g)
        stats['random_error'] = mean(random_errors)
        stats['smooth_gains'] = {name: list(gains[1, i]) for i, name in enumerate(self.keys)}
        if dynamics:                                        # one launch for every variant, one copy to the host
            st_errors = profile_error_device(reference_st, torch.stack(candidates_st))[0].cpu().tolist()
            stats['sum_st_error'], stats['loudnorm_st_error'], stats['mix_st_error'] = st_errors[:3]
            stats['random_st_error'] = mean(st_errors[3:])
            stats['lra'] = dict(zip(self.keys, reference_lra.cpu().tolist()))
        if spectral:                                        # the draws in one call, one launch for every variant, one copy
            if drawn_gains:
                candidates_spec.append(band_power(pcm, torch.stack(drawn_gains).unsqueeze(-1)))
            cand = torch.cat(candidates_spec)
            spec_errors = spectrum.balance_error_device(reference_spec[0], cand)[0]
            # (a [1, bands] row each, as evaluate_spectrum_batch returns one: the same reduction, the same bits)
            levels = [spectrum.relative_levels_db(reference_spec), spectrum.relative_levels_db(cand[2:3])]
            host = torch.cat([spec_errors, levels[0][0], levels[1][0]]).cpu().tolist()
            n_var, n_bands = cand.shape[0], len(centres)
            stats['sum_spec_error'], stats['loudnorm_spec_error'], stats['mix_spec_error'] = host[:3]
            stats['random_spec_error'] = mean(host[3:n_var])
            stats['ltas'] = {'centres': centres.tolist(), 'reference': host[n_var:n_var + n_bands],
                             'mix': host[n_var + n_bands:]}
        if gain_fit or band_fit:                            # one launch for every variant and fit, one copy to the host
            n_stems, W = len(self.keys), mixer.n_proc
            raw_stems, target = pcm.transpose(1, 2), fit_target.transpose(0, 1)
            aligned = {}                                    # max_lag -> (shifted stems, lag, peak): a lag asked for twice is estimated once

            def on_reference(max_lag):                      # the raw stems moved onto the reference; the lags stay on the device
                if max_lag not in aligned:
                    lag, _, peak, _, _ = align.estimate_lag(raw_stems, target, max_lag, weighting='plain')
                    aligned[max_lag] = (align.shift_tracks(raw_stems, lag), lag, peak)
                return aligned[max_lag]
            constant = torch.stack(candidates_fit).unsqueeze(-1).expand(-1, -1, W)         # loudnorm, draws: [.., stems, W]
            cand = torch.cat([torch.ones((1, n_stems, W), dtype=torch.float64, device=pcm.device), constant[:1],
                              mixer.gains[1].unsqueeze(0), constant[1:]])
            n_var = cand.shape[0]
            parts = []
            if gain_fit:
                fit_stems = raw_stems
                if fit_align is not None:
                    fit_stems, stem_lag, stem_lag_peak = on_reference(fit_align)
                fitted, residual, _ = gainfit.fit_gains(fit_stems, target, W, pool=fit_pool, ridge=fit_ridge)
                fit_errors = gainfit.gain_error_device(fitted, cand)[0]
                parts += [fit_errors, fitted.reshape(-1), residual]
                if fit_align is not None:
                    parts += [stem_lag.to(torch.float64), stem_lag_peak]
            if band_fit:
                band_stems = raw_stems if band['align'] is None else on_reference(band['align'])[0]
                band_gains, band_residual, band_target, band_status = gainfit.fit_band_gains(
                    band_stems, target, W, n_fft=band['n_fft'], hop=band['hop'], edges=band['edges'], pool=band['pool'],
                    ridge=band['ridge'])
                n_bands = band_gains.shape[0]
                # every (band, window) is a window of the gain error: fitted [S][B W], the candidates' curves repeated over the bands
                band_errors = gainfit.gain_error_device(
                    band_gains.permute(1, 0, 2).reshape(n_stems, n_bands * W),
                    cand.unsqueeze(2).expand(-1, -1, n_bands, -1).reshape(n_var, n_stems, n_bands * W))[0]
                parts += [band_errors, band_gains.reshape(-1), band_residual.reshape(-1),
                          gainfit.band_residual_total(band_residual, band_target, band_status)]
                if render_fill is not None:
                    fill = render_fill
                    if fill == 'broadband':
                        if gain_fit and (fit_pool, fit_ridge, fit_align) == (band['pool'], band['ridge'], band['align']):
                            fill = fitted
                        else:
                            fill = gainfit.fit_gains(band_stems, target, W, pool=band['pool'], ridge=band['ridge'])[0]
                    rendered = gainfit.render_band_gains(band_stems, band_gains, n_fft=band['n_fft'], hop=band['hop'],
                                                         edges=band['edges'], fill=fill)             # float32 [channels, n]
                    # (target - render) against the target, window by window: the moments of the pair
                    m = gainfit.moments(rendered.transpose(0, 1).unsqueeze(0), target, W)
                    parts.append((m[:, 0, 0] - 2.0 * m[:, 0, 1] + m[:, 1, 1]) / m[:, 1, 1])
                    write('oracle_band', rendered.unsqueeze(0))
            host = torch.cat(parts).cpu().tolist()
            at = 0

            def take(count):
                nonlocal at
                at += count
                return host[at - count:at]
            if gain_fit:
                errors = take(n_var)
                stats['sum_gain_error'], stats['loudnorm_gain_error'], stats['mix_gain_error'] = errors[:3]
                stats['random_gain_error'] = mean(errors[3:]) if n_var > 3 else float('nan')
                stats['oracle_gains'] = {name: take(W) for name in self.keys}
                stats['oracle_residual'] = take(W)
                if fit_align is not None:
                    stats['oracle_lag'] = {name: int(v) for name, v in zip(self.keys, take(n_stems))}
                    stats['oracle_lag_peak'] = dict(zip(self.keys, take(n_stems)))
            if band_fit:
                errors = take(n_var)
                stats['sum_band_gain_error'], stats['loudnorm_band_gain_error'], stats['mix_band_gain_error'] = errors[:3]
                stats['random_band_gain_error'] = mean(errors[3:]) if n_var > 3 else float('nan')
                stats['oracle_band_centres'] = np.asarray(band['centres'], dtype=np.float64)
                per_band = [[take(W) for _ in self.keys] for _ in range(n_bands)]
                stats['oracle_band_gains'] = {name: [per_band[b][i] for b in range(n_bands)] for i, name in enumerate(self.keys)}
                stats['oracle_band_residual'] = [take(W) for _ in range(n_bands)]
                stats['oracle_band_residual_total'] = take(W)
                if render_fill is not None:
                    stats['oracle_band_render_residual'] = take(W)
        if feature_distance:                                # every variant in one call, one summary launch, one copy to the host
            n_stems, W = len(self.keys), mixer.n_proc
            constant = torch.stack(candidates_feat).unsqueeze(-1).expand(-1, -1, W)        # loudnorm, draws: [.., stems, W]
            cand = torch.cat([torch.ones((1, n_stems, W), dtype=torch.float64, device=pcm.device), constant[:1],
                              mixer.gains[1].unsqueeze(0), constant[1:]])
            sums, count = spectrum.spectrogram_distance(pcm.transpose(1, 2), cand, feat_reference.transpose(1, 2), None,
                                                        n_fft=feat_n_fft, hop=feat_hop, edges=feat_edges, n_windows=W)
            fig = spectrum.distance_summary(sums, count)
            host = torch.cat([fig.rms_centred, fig.mse, fig.band_rms[2], fig.window_rms[2]]).cpu().tolist()
            n_var = cand.shape[0]
            rms, mse = host[:n_var], host[n_var:2 * n_var]
            stats['sum_feat_error'], stats['loudnorm_feat_error'], stats['mix_feat_error'] = rms[:3]
            stats['random_feat_error'] = mean(rms[3:]) if n_var > 3 else float('nan')
            stats['sum_feat_mse'], stats['loudnorm_feat_mse'], stats['mix_feat_mse'] = mse[:3]
            stats['random_feat_mse'] = mean(mse[3:]) if n_var > 3 else float('nan')
            n_bands = len(feat_centres)
            stats['feat_profile'] = {'centres': feat_centres, 'mix_band_rms': host[2 * n_var:2 * n_var + n_bands],
                                     'mix_window_rms': host[2 * n_var + n_bands:]}
            if self._feature_sensitivity(feature_distance):  # one fused call: every variant a row, the gain windows the nodes
                grad_mse = spectrum.spectrogram_distance_grad(pcm.transpose(1, 2), cand, feat_reference.transpose(1, 2), None,
                                                              n_fft=feat_n_fft, hop=feat_hop)[2]
                sens = spectrum.gain_sensitivity_db(cand, grad_mse).cpu()                   # [variants, stems, W]
                stats['sum_feat_sens'], stats['loudnorm_feat_sens'], stats['mix_feat_sens'] = sens[:3].tolist()
                stats['random_feat_sens'] = (sens[3:].mean(dim=0) if n_var > 3 else
                                             torch.full((n_stems, W), float('nan'), dtype=torch.float64)).tolist()
            del feat_reference
        return stats

    def process_song(self, base_dir: str, song_name: str, n_random_samples: int = 5, chunk_length: int = 2,
                     write_wavs_to_disk=False, results_dir='./experiment', ceiling_dbtp=None, dynamics=False, limiter=None,
                     spectral=False, gain_fit=False, band_fit=False, band_render=False, feature_distance=False,
                     compressor=None) -> dict:
        """evaluation.py:77-116: the reference mix from ``base_dir/manual_gain_mixes``, the stems from ``base_dir/test``."""
        from .data.dataset_utils import load_tracks_musdb18
        self._band_render_args(band_render, band_fit)          # (before a file is read)
        if feature_distance:
            self._feature_distance_args(feature_distance)
        reference_tracks = load_tracks_musdb18(os.path.join(base_dir, 'manual_gain_mixes'), song_name, tracklist=self.keys,
                                               sr=self.sr)
        loaded_tracks = load_tracks_musdb18(os.path.join(base_dir, 'test'), song_name, tracklist=self.keys, sr=self.sr)
        return self.process_song_tracks(loaded_tracks, reference_tracks, song_name, n_random_samples, chunk_length,
                                        write_wavs_to_disk, results_dir, ceiling_dbtp, dynamics, limiter, spectral,
                                        **({'gain_fit': gain_fit} if gain_fit else {}),
                                        **({'band_fit': band_fit} if band_fit else {}),
                                        **({'band_render': band_render} if band_render else {}),
                                        **({'feature_distance': feature_distance} if feature_distance else {}),
                                        **({'compressor': compressor} if compressor else {}))

    def process_songlist(self, base_dir, songlist, n_random_samples: int = 5, chunk_length: int = 2,
                         write_wavs_to_disk=False, results_dir='./experiment', ceiling_dbtp=None, dynamics=False, limiter=None,
                         spectral=False, gain_fit=False, band_fit=False, band_render=False, feature_distance=False,
                         compressor=None):
        """evaluation.py:118-144 without the spreadsheet: (rows, means) -- one stats dict per song and the mean of every
        error over the songs (the sheet's last row); with ``dynamics`` the four '*_st_error' keys too, with ``spectral``
        the four '*_spec_error' keys, with ``gain_fit`` the four '*_gain_error' keys (a song whose figure is NaN -- nothing
        to compare -- is left out of that mean; the mean is NaN if every song's is), with ``band_fit`` the four
        '*_band_gain_error' keys in the same way.  ``band_render`` is passed on to every song (its key is per window: no mean).
        With ``feature_distance`` the four '*_feat_error' and the four '*_feat_mse' keys are averaged as the '*_spec_error' keys
        are."""
        self._band_render_args(band_render, band_fit)
        keys = ['sum_error', 'random_error', 'loudnorm_error', 'mix_error']
        if dynamics:
            keys += ['sum_st_error', 'random_st_error', 'loudnorm_st_error', 'mix_st_error']
        if spectral:
            keys += ['sum_spec_error', 'random_spec_error', 'loudnorm_spec_error', 'mix_spec_error']
        if feature_distance:
            keys += ['sum_feat_error', 'random_feat_error', 'loudnorm_feat_error', 'mix_feat_error',
                     'sum_feat_mse', 'random_feat_mse', 'loudnorm_feat_mse', 'mix_feat_mse']
        fit_keys = ['sum_gain_error', 'random_gain_error', 'loudnorm_gain_error', 'mix_gain_error'] if gain_fit else []
        if band_fit:
            fit_keys += ['sum_band_gain_error', 'random_band_gain_error', 'loudnorm_band_gain_error', 'mix_band_gain_error']
        rows = []
        for i, song_name in enumerate(songlist):
            print('{}/{}: {}'.format(i + 1, len(songlist), song_name))
            # (either keyword only where it is asked for: the call without them is the call of before, argument for argument)
            extra = {} if limiter is None or limiter is False else {'limiter': limiter}
            if spectral:
                extra['spectral'] = spectral
            if gain_fit:
                extra['gain_fit'] = gain_fit
            if band_fit:
                extra['band_fit'] = band_fit
            if band_render:
                extra['band_render'] = band_render
            if feature_distance:
                extra['feature_distance'] = feature_distance
            if compressor:
                extra['compressor'] = compressor
            rows.append(self.process_song(base_dir, song_name, n_random_samples, chunk_length, write_wavs_to_disk,
                                          results_dir, ceiling_dbtp, dynamics, **extra))
        means = {key: mean(row[key] for row in rows) for key in keys}
        for key in fit_keys:
            finite = [row[key] for row in rows if row[key] == row[key]]
            means[key] = mean(finite) if finite else float('nan')
        return rows, means
