"""Full-song inference -- drop-in for the reference's inference_utils.py (interpolate_mask :12-41,
mix_song_smooth :105-145) on the GPU (BASELINE config C5).

mix_song_smooth at the reference HEAD cannot run (it hands [channels, n] slices to torch.stft); this
module implements the intended semantics: features of the channel MEAN, gains applied to the original
multichannel audio.

Everything between the PCM upload and the result download stays on the device and -- for a model in eval mode -- is ONE
hipGraph (``SongMixer``): strided STFT front-end over all chunks of all stems straight out of the planar song
(dam_stft_logmag_strided_f32) -> model forward of the whole chunk batch -> 10 ** (0.5 g) and the Savitzky-Golay
smoothing (dam_gains_smooth) -> sample-rate gain ramp x audio (dam_gain_ramp_apply), or for ``mix_song_to_master`` and
``mix_song_to_wav`` the master tail, ``MasterChain``: the fused stem sum + peak normalisation (dam_mixdown_peak_normalize)
or, with ``normalize='loudness'``, the stem sum brought to a target BS.1770 loudness (optionally held under a true-peak
ceiling, ``ceiling_dbtp``: dam_true_peak_batch of the float64 sum, dam_peak_limit_gains on the loudness gain;
``normalize='true_peak'`` puts the true peak AT the ceiling instead; ``limiter=`` turns down only the peaks over the ceiling,
dam_limiter_apply, so the song keeps its loudness), then the PCM encoder as the graph's last node where a
file is asked for (dam_pcm_encode: the loudness gain is applied inside it, the host receives the file's sample bytes instead
of the float master).  MasterChain is the single place a new output stage goes: the evaluator's WAV export runs the same one.
``mix_song_loudness`` ends in the batched meter instead (the per-stem loudness of the mixed
stems, dam_loudness_block_energy_batch with the gain ramp applied at load: the mixed stems are never written).
``mix_song_spectral`` renders in the spectral domain
instead (experiments.ipynb cells 44-53): the model's predicted dB spectrogram ``masked`` on the phases of the stems' sum
(dam_stft_complex_strided_f32), inverted by dam_istft_f32 -- the same graph with a different tail.  The host sees the
song once on the way in (page-locked double-buffered staging, staging.PinnedPipe) and the result once on the way out.

The model is applied as the reference applies it -- whatever ``model.training`` is, never toggled here:
in eval mode all chunks run as one batch inside the graph; in training mode BatchNorm uses per-call batch statistics
(and updates its running statistics), so chunks run one by one, eagerly, exactly as in the reference loop.
"""
import numpy as np
import torch

from . import features, loudness, ops, staging

device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')      # inference_utils.py:9

SAVGOL_POLYORDER = 2          # inference_utils.py:140


def interpolate_mask(spec_mask: np.array, tgt_len: int) -> np.array:
    """inference_utils.py:12-41: every gain held for int(tgt_len / len) samples, the last one to the end of the track.
    Host version, kept for API parity (mix_song_smooth applies the same ramp inside dam_gain_ramp_apply)."""
    gains = np.asarray(spec_mask, dtype=np.float64)
    assert len(gains) <= tgt_len, "Target mask should be longer than the initial one"
    if len(gains) < 2:
        return np.zeros(tgt_len)          # the reference's loop body never runs for a single gain: the mask stays zero
    hold = tgt_len // len(gains)
    index = np.minimum(np.arange(tgt_len) // hold, len(gains) - 1)
    return gains[index]


def _savgol_window(num_chunks):
    w = int(num_chunks / 4)          # inference_utils.py:136-139
    return w if w % 2 else w + 1


def predict_chunk_gains(model, pcm, n_stems, n_chunks, chunk_samples, window_size=2048, hop_length=1024, feats=None):
    """pcm: CUDA [n_stems, channels, n] -> raw model outputs [n_chunks-1, n_stems] for chunks 0..n_chunks-2
    (the reference loop ``range(1, num_chunks)`` processes exactly those, inference_utils.py:111-113)."""
    n_proc = n_chunks - 1
    feats = features.stft_logmag_song_chunks(pcm, n_proc, chunk_samples, window_size, hop_length, out=feats)
    feats = feats.view(n_proc, n_stems, feats.shape[1], feats.shape[2])
    if model.training:
        return torch.cat([model.predict_gains(feats[i:i + 1]) for i in range(n_proc)], 0)
    return model.predict_gains(feats)


class MasterChain:
    """The master tail, the ONE implementation of it (SongMixer kind 'master' captures it into the song's graph,
    evaluation.LoudnessEvaluator.write_sum_to_target runs it eagerly; a new output stage goes here): stem sum -> BS.1770
    measurement -> target gain -> (compressor -> measurement -> target gain) -> look-ahead limiter -> true-peak clamp -> gain
    apply or PCM encode.  It owns every buffer
    those steps need, allocated once and only where the configuration uses it, so a captured ``render`` holds stable pointers.

    normalize: True / False -- the sum, peak-normalised per channel or not (the callers' librosa.util.normalize);
    'loudness' -- the float64 sum brought to ``target_lufs`` (evaluation.py:59-66); 'true_peak' -- the sum scaled so that its
    true peak (dBTP) sits at ``ceiling_dbtp`` (default -1.0).  ceiling_dbtp (with 'loudness'): the gain to the target is
    clamped to ``ceiling / true peak of the sum``, one static gain for all channels.  encode: None (``out``
    holds the master as ``out_dtype``) or a WAV subtype of ops.PCM_FORMATS (``enc`` holds the file's sample bytes, ``clip``
    the clamped-sample count per channel; TPDF dither if ``dither_seed`` is given).  limiter (with 'loudness'; None / False:
    none, True: the defaults, or {'lookahead_ms': 5.0, 'hold_ms': 20.0}): the sum at the target gain goes through the
    look-ahead true-peak limiter (dam_limiter_apply, ceiling -1.0 dBTP unless ``ceiling_dbtp`` says otherwise) into a float64
    limited master; the true-peak clamp then measures THAT and is the residual trim, a few 1e-5 dB, that makes the ceiling
    exact.  compressor (with 'loudness'; None / False: none, True: COMPRESSOR_DEFAULTS, or a dict with some of its keys): the
    sum at the target gain goes through the feed-forward compressor (dam_compressor_apply, the target gain as its
    ``pre_gain``: the threshold is in dBFS of the song AT ``target_lufs`` and means the same for a quiet and a loud song) into
    a float64 buffer of its own, which is measured and brought to ``target_lufs`` again -- the make-up gain is that second
    measurement, not a parameter.  The limiter, the clamp and the encoder then see the compressed signal where they saw the
    sum."""

    LIMITER_DEFAULTS = {'lookahead_ms': 5.0, 'hold_ms': 20.0}
    COMPRESSOR_DEFAULTS = {'threshold_db': -12.0, 'ratio': 2.0, 'knee_db': 6.0, 'attack_ms': 10.0, 'release_ms': 100.0}

    @staticmethod
    def rules(normalize, ceiling_dbtp, encode):
        """What the three arguments may be -> (normalize, ceiling); ValueError otherwise."""
        if encode is not None and encode not in ops.PCM_FORMATS:
            raise ValueError('encode must be one of %s, got %r' % (sorted(ops.PCM_FORMATS), encode))
        if normalize not in (True, False, 'loudness', 'true_peak'):
            raise ValueError("normalize must be True, False, 'loudness' or 'true_peak'")
        if normalize == 'true_peak' and ceiling_dbtp is None:
            ceiling_dbtp = -1.0
        if ceiling_dbtp is not None and normalize not in ('loudness', 'true_peak'):
            raise ValueError("ceiling_dbtp needs normalize 'loudness' or 'true_peak'")
        return normalize, None if ceiling_dbtp is None else float(ceiling_dbtp)

    @staticmethod
    def limiter_rules(limiter, normalize, ceiling):
        """What ``limiter`` may be, given what ``rules`` returned -> (None or (lookahead_ms, hold_ms), ceiling); ValueError
        otherwise.  A limiter without a ceiling takes -1.0 dBTP."""
        if limiter is None or limiter is False:
            return None, ceiling
        if limiter is True:
            limiter = {}
        if not isinstance(limiter, dict) or set(limiter) - set(MasterChain.LIMITER_DEFAULTS):
            raise ValueError('limiter must be None, a bool or a dict with keys of %s, got %r'
                             % (sorted(MasterChain.LIMITER_DEFAULTS), limiter))
        if normalize != 'loudness':
            raise ValueError("limiter needs normalize 'loudness'")
        times = tuple(float(limiter.get(k, v)) for k, v in MasterChain.LIMITER_DEFAULTS.items())
        if not all(t > 0.0 for t in times):
            raise ValueError('limiter times must be positive, got %r' % (limiter,))
        return times, -1.0 if ceiling is None else ceiling

    @staticmethod
    def compressor_rules(compressor, normalize):
        """What ``compressor`` may be, given what ``rules`` returned -> None or (threshold_db, ratio, knee_db, attack_ms,
        release_ms); ValueError otherwise."""
        if compressor is None or compressor is False:
            return None
        if compressor is True:
            compressor = {}
        if not isinstance(compressor, dict) or set(compressor) - set(MasterChain.COMPRESSOR_DEFAULTS):
            raise ValueError('compressor must be None, a bool or a dict with keys of %s, got %r'
                             % (sorted(MasterChain.COMPRESSOR_DEFAULTS), compressor))
        if normalize != 'loudness':
            raise ValueError("compressor needs normalize 'loudness'")
        shape = tuple(float(compressor.get(k, v)) for k, v in MasterChain.COMPRESSOR_DEFAULTS.items())
        _, ratio, knee, attack, release = shape
        if not (ratio >= 1.0 and knee >= 0.0 and attack > 0.0 and release > 0.0 and all(v == v for v in shape)):
            raise ValueError('compressor needs ratio >= 1, knee_db >= 0 and positive times, got %r' % (compressor,))
        return shape

    def __init__(self, channels, n_samples, device, normalize=True, out_dtype=torch.float64, sr=44100, target_lufs=-20.0,
                 ceiling_dbtp=None, encode=None, dither_seed=None, limiter=None, compressor=None):
        self.normalize, self.ceiling = self.rules(normalize, ceiling_dbtp, encode)
        self.limiter, self.ceiling = self.limiter_rules(limiter, self.normalize, self.ceiling)
        self.compressor = self.compressor_rules(compressor, self.normalize)
        self.encode, self.dither_seed = encode, dither_seed
        scaled = self.normalize in ('loudness', 'true_peak')             # the float64 sum times one measured gain
        f64 = dict(dtype=torch.float64, device=device)
        self.out = self.enc = self.clip = self.master_gain = None
        if encode is None or not scaled:                       # (the encoder reads the float64 sum and scales it itself)
            self.out = torch.empty((channels, n_samples), dtype=out_dtype, device=device)
        if encode is not None:
            self.enc = torch.empty(n_samples * channels * ops.PCM_FORMATS[encode][1], dtype=torch.uint8, device=device)
            self.clip = torch.empty(channels, dtype=torch.int64, device=device)
        if scaled:
            # evaluation.py:59-66: the float64 stem sum is measured and scaled; only the result takes out_dtype
            self.mix = torch.empty((channels, n_samples), **f64)
            self.master_gain = torch.empty(1, **f64)
        if self.normalize == 'loudness':
            self.meter = loudness.Meter(sr)
            self.target = torch.full((1,), float(target_lufs), **f64)
            self.lufs = torch.empty(1, **f64)
        if self.ceiling is not None:
            # the gain before the clamp (written by every render; 'true_peak' asks for none: +inf), the true and sample
            # peaks of the sum
            self.free_gain = torch.empty(1, **f64) if self.normalize == 'loudness' else torch.full((1,), float('inf'), **f64)
            self.tp = torch.empty((1, channels), **f64)
            self.sp = torch.empty((1, channels), **f64)
        if self.limiter is not None:
            # look-ahead and hold in samples (ValueError beyond the kernel's caps), the limited master, its statistics, its
            # loudness and the kernel's workspace
            self.lookahead, self.hold = (ops.limiter_samples(ms, sr) for ms in self.limiter)
            _, max_lookahead, max_hold = ops.limiter_geometry()
            if self.lookahead > max_lookahead or self.hold > max_hold:
                raise ValueError('limiter: %d / %d samples of look-ahead / hold at %d Hz exceed the caps %d / %d'
                                 % (self.lookahead, self.hold, sr, max_lookahead, max_hold))
            self.limited = torch.empty((channels, n_samples), **f64)
            self.min_gain = torch.empty(1, **f64)
            self.n_limited = torch.empty(1, dtype=torch.int64, device=device)
            self.limited_lufs = torch.empty(1, **f64)
            self.limiter_ws = torch.empty(ops._lib.lib().dam_limiter_workspace_bytes(1, n_samples) // 8, **f64)
        if self.compressor is not None:
            # the curve and the constants the kernel takes (ValueError beyond its caps), the gain to the target the compressor
            # works at, the compressed sum, its statistics, its loudness and the kernel's workspace
            threshold, ratio, knee, attack, release = self.compressor
            self.comp_args = (threshold, ratio, knee) + ops.compressor_constants(threshold, knee, attack, release, sr)
            longest = ops.compressor_geometry()[2]
            if max(attack, release) * 1e-3 * sr > longest:
                raise ValueError('compressor: %g / %g ms of attack / release at %d Hz exceed the cap of %d samples'
                                 % (attack, release, sr, longest))
            self.comp_gain = torch.empty(1, **f64)
            self.compressed = torch.empty((channels, n_samples), **f64)
            self.comp_max = torch.empty(1, **f64)
            self.comp_over = torch.empty(1, dtype=torch.int64, device=device)
            self.compressed_lufs = torch.empty(1, **f64)
            self.comp_ws = torch.empty(ops._lib.lib().dam_compressor_workspace_bytes(1, n_samples) // 8, **f64)
        self.sum = self.mix if scaled else self.out
        self.ws = torch.empty(ops._lib.lib().dam_mixdown_workspace_elems(channels), dtype=self.sum.dtype, device=device)

    def render(self, pcm, gains):
        """pcm CUDA [stems, channels, n], gains CUDA float64 [stems, n_gains] -> ``out`` or ``enc`` / ``clip``.  No host
        synchronisation and no branch on a tensor's value: capturable."""
        scaled = self.master_gain is not None
        ops.mixdown_peak_normalize(pcm, gains, normalize=not scaled and self.normalize, out=self.sum, workspace=self.ws)
        source = self.sum                          # what master_gain scales
        if self.normalize == 'loudness':
            self.meter.integrated_loudness_batch(self.mix.t().unsqueeze(0), out=self.lufs)
            lufs = self.lufs
            if self.compressor is not None:
                # the sum at the target gain, compressed; what follows measures and scales THAT: the second target gain is
                # the make-up
                loudness.target_gains_device(self.lufs, self.target, out=self.comp_gain)
                ops.compressor_apply(self.mix.t().unsqueeze(0), *self.comp_args, pre_gain=self.comp_gain, out=self.compressed,
                                     max_reduction_out=self.comp_max, n_over_out=self.comp_over, workspace=self.comp_ws)
                source, lufs = self.compressed, self.compressed_lufs
                self.meter.integrated_loudness_batch(source.t().unsqueeze(0), out=lufs)
            loudness.target_gains_device(lufs, self.target, out=self.master_gain if self.ceiling is None else self.free_gain)
        if self.limiter is not None:
            # the sum at the target gain, its peaks turned down; the clamp below measures the result: master_gain is the trim
            ops.limiter_apply(source.t().unsqueeze(0), self.ceiling, self.lookahead, self.hold, pre_gain=self.free_gain,
                              out=self.limited, min_gain_out=self.min_gain, n_limited_out=self.n_limited,
                              workspace=self.limiter_ws)
            source = self.limited
            self.master_gain.fill_(1.0)
        elif self.ceiling is not None:
            self.master_gain.copy_(self.free_gain)
        if self.ceiling is not None:
            ops.true_peak_batch(source.t().unsqueeze(0), out=self.tp, sample_peak_out=self.sp)
            ops.peak_limit_gains(self.master_gain, self.tp, self.ceiling)          # the maximum over the channels
        if self.encode is not None:                # mix * gain is rounded once to float64 either way: the same samples
            ops.pcm_encode(source, self.encode, scale=self.master_gain, dither_seed=self.dither_seed, out=self.enc,
                           clip_count=self.clip)
        elif scaled:
            ops.gain_ramp_apply(source, self.master_gain, out=self.out)
        if self.limiter is not None:               # the loudness of the limited master; peaks() adds the trim
            self.meter.integrated_loudness_batch(self.limited.t().unsqueeze(0), out=self.limited_lufs)

    def peaks(self):
        """The peak measurement of the last render of a chain with a ceiling, from the device tensors the graph wrote:
        {'true_peak_db': [per channel], 'sample_peak_db': [per channel]} of the master as rendered (the measured sum times
        the gain that was applied, before any quantisation), 'limited': whether the ceiling, not the loudness target, set
        that gain (always so for normalize='true_peak' unless the sum is silent), and 'gain', the gain itself.  With a
        limiter the same keys describe the limited master ('gain': the target gain times the trim; 'limited': the limiter
        reduced a sample or the trim is below 1) and four more say what the limiter did: 'max_reduction_db' (20 log10 of its
        smallest gain, 0.0: untouched), 'limited_share' (the share of samples with a gain below 1), 'trim_db' (the residual
        static gain that makes the ceiling exact) and 'loudness_lufs' (BS.1770, of the master as rendered)."""
        if self.ceiling is None:
            raise ValueError('this master chain was built without ceiling_dbtp')
        tp, sp = self.tp.cpu().numpy()[0], self.sp.cpu().numpy()[0]
        gain, free = float(self.master_gain.cpu()[0]), float(self.free_gain.cpu()[0])
        with np.errstate(divide='ignore', invalid='ignore'):
            out = {'true_peak_db': [float(v) for v in 20.0 * np.log10(tp * gain)],
                   'sample_peak_db': [float(v) for v in 20.0 * np.log10(sp * gain)],
                   'limited': bool(gain < free), 'gain': gain}
            if self.limiter is not None:
                min_gain, trim_db = float(self.min_gain.cpu()[0]), float(20.0 * np.log10(gain))
                out.update({'limited': bool(min_gain < 1.0 or gain < 1.0), 'gain': free * gain,
                            'max_reduction_db': float(20.0 * np.log10(min_gain)),
                            'limited_share': int(self.n_limited.cpu()[0]) / self.limited.shape[1], 'trim_db': trim_db,
                            'loudness_lufs': float(self.limited_lufs.cpu()[0]) + trim_db})
        return out

    def compression(self):
        """What the compressor did in the last render of a chain with one, from the device scalars the graph wrote:
        {'max_reduction_db': the largest gain reduction (0.0: untouched), 'over_share': the share of samples above the knee's
        start, 'makeup_db': the gain that brought the compressed signal back to the target, 'loudness_lufs': BS.1770 of the
        compressed signal at that gain (before any limiter or ceiling: peaks() tells what those did)}."""
        if self.compressor is None:
            raise ValueError('this master chain was built without a compressor')
        gain = float((self.master_gain if self.ceiling is None else self.free_gain).cpu()[0])
        with np.errstate(divide='ignore', invalid='ignore'):
            makeup_db = float(20.0 * np.log10(gain))
        return {'max_reduction_db': float(self.comp_max.cpu()[0]),
                'over_share': int(self.comp_over.cpu()[0]) / self.compressed.shape[1], 'makeup_db': makeup_db,
                'loudness_lufs': float(self.compressed_lufs.cpu()[0]) + makeup_db}


class SongMixer:
    """Static device buffers and the captured hipGraph of one song geometry: (model, stems, channels, samples, dtype,
    chunk length, output kind).  ``run(tracks)`` uploads, replays, downloads."""

    def __init__(self, model, n_stems, channels, n_samples, dtype, chunk_samples, kind, normalize=True,
                 out_dtype=torch.float64, use_graph=True, hop_length=1024, sr=44100, target_lufs=-20.0, encode=None,
                 dither_seed=None, ceiling_dbtp=None, limiter=None, compressor=None):
        """normalize, out_dtype, sr, target_lufs, encode, dither_seed, ceiling_dbtp, limiter, compressor: what MasterChain takes,
        for kind 'master' (the other kinds accept neither ``encode`` nor a ceiling nor a limiter nor a compressor).  With ``encode`` the master is
        quantised by the last node of the same graph and ``run`` returns its sample bytes and the clipped-sample count;
        ``peaks()`` reports the true-peak measurement of the last run."""
        if kind not in ('stems', 'master', 'spectral', 'loudness'):
            raise ValueError(kind)
        self.normalize, self.ceiling = MasterChain.rules(normalize, ceiling_dbtp, encode)
        self.limiter, self.ceiling = MasterChain.limiter_rules(limiter, self.normalize, self.ceiling)
        if kind != 'master' and (encode is not None or self.ceiling is not None or self.limiter is not None):
            raise ValueError("encode, ceiling_dbtp and limiter need kind='master'")
        self.compressor = MasterChain.compressor_rules(compressor, self.normalize)
        if kind != 'master' and self.compressor is not None:
            raise ValueError("compressor needs kind='master'")
        self.encode = encode
        self.model, self.kind = model, kind
        self.dev = next(model.parameters()).device
        self.n_stems, self.channels, self.n, self.chunk = n_stems, channels, n_samples, chunk_samples
        self.num_chunks = int(n_samples / chunk_samples)
        self.n_proc = self.num_chunks - 1
        if self.n_proc < 1:
            raise ValueError('the song must hold at least two chunks')
        self.hop = hop_length
        self.window = _savgol_window(self.num_chunks)
        # (the spectral kind smooths nothing: a song of two chunks is valid there)
        if kind != 'spectral' and (self.window <= SAVGOL_POLYORDER or self.window > self.n_proc):
            # scipy.signal.savgol_filter raises for these at inference_utils.py:140
            raise ValueError('polyorder must be less than window_length and window_length must not exceed the number '
                             'of gains (window %d, %d gains)' % (self.window, self.n_proc))
        dev = self.dev
        self.pcm = torch.empty((n_stems, channels, n_samples), dtype=dtype, device=dev)
        t = features.num_frames(chunk_samples, hop_length)
        self.feats = torch.empty((self.n_proc * n_stems, 1025, t), dtype=torch.float32, device=dev)
        if kind == 'spectral':
            self.spec = torch.empty((self.n_proc, 1025, t), dtype=torch.complex64, device=dev)     # phase source
            self.masked = None                                                                       # set by every launch
            self.out = torch.empty((self.n_proc, chunk_samples), dtype=torch.float32, device=dev)
        elif kind == 'stems':
            self.out = torch.empty((n_stems, channels, n_samples), dtype=out_dtype, device=dev)
        elif kind == 'loudness':
            self.meter = loudness.Meter(sr)
            self.out = torch.empty(n_stems, dtype=torch.float64, device=dev)                       # LUFS of every mixed stem
        else:
            self.chain = MasterChain(channels, n_samples, dev, self.normalize, out_dtype, sr, target_lufs, self.ceiling, encode,
                                     dither_seed, limiter, compressor)
            if encode is not None:
                self.enc, self.clip = self.chain.enc, self.chain.clip
            if self.chain.out is not None:                     # (no float master is kept beside an encoded, gain-scaled one)
                self.out = self.chain.out
        self.gains = torch.empty((2, n_stems, self.n_proc), dtype=torch.float64, device=dev)     # [raw amplitude, smoothed]
        self.graph = None
        self.use_graph = use_graph
        self._key = None

    def _body_spectral(self):
        """experiments.ipynb cells 44-53 for every chunk: masked = model(dB features of the stems)[0], the phases of the STFT
        of the stems' sum, istft(db_to_amplitude(masked) * phases).  Each chunk is its own centred STFT, so the chunks are
        independent tracks of one batched launch."""
        feats = features.stft_logmag_song_chunks(self.pcm, self.n_proc, self.chunk, 2048, self.hop, out=self.feats)
        feats = feats.view(self.n_proc, self.n_stems, feats.shape[1], feats.shape[2])
        if self.model.training:
            self.masked = torch.cat([self.model(feats[i:i + 1])[0] for i in range(self.n_proc)], 0)
        else:
            self.masked = self.model(feats)[0]            # (captured: the graph's own static output)
        features.stft_song_chunks_sum(self.pcm, self.n_proc, self.chunk, 2048, self.hop, out=self.spec)
        features.istft(self.spec, self.hop, self.chunk, mag_db=self.masked, out=self.out)

    def _body(self):
        if self.kind == 'spectral':
            return self._body_spectral()
        g = predict_chunk_gains(self.model, self.pcm, self.n_stems, self.num_chunks, self.chunk, hop_length=self.hop,
                                feats=self.feats)
        _, smooth = ops.gains_smooth(g, self.window, SAVGOL_POLYORDER, out=self.gains)
        if self.kind == 'stems':
            ops.gain_ramp_apply(self.pcm, smooth, out=self.out)
        elif self.kind == 'loudness':
            self.meter.integrated_loudness_batch(self.pcm.transpose(1, 2), gains=smooth, out=self.out)
        else:
            self.chain.render(self.pcm, smooth)

    def _model_key(self):
        # the captured forward holds the FOLDED conv + BatchNorm images (layers.FoldedConvBn), computed when it was captured:
        # any change of the parameters or running statistics -- torch-side (version counters) or by this library's own
        # in-place kernels (ops.PARAM_EPOCH) -- needs a new capture, not just a replay
        return (self.model.training, ops.PARAM_EPOCH) + tuple(
            (t.data_ptr(), t._version) for t in self.model.state_dict(keep_vars=True).values())

    def launch(self):
        """Runs the device pipeline on whatever is in self.pcm (graph replay when the model is in eval mode)."""
        if self.model.training or not self.use_graph:
            with torch.no_grad():
                self._body()
            return
        key = self._model_key()
        if self.graph is None or key != self._key:
            with torch.no_grad():
                s = torch.cuda.Stream(device=self.dev)
                s.wait_stream(torch.cuda.current_stream(self.dev))
                with torch.cuda.stream(s):
                    self._body()                   # warm-up: sizes every workspace, builds the weight-packing table
                torch.cuda.current_stream(self.dev).wait_stream(s)
                torch.cuda.synchronize(self.dev)
                self.graph = torch.cuda.CUDAGraph()
                with staging.capture_guard, torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
                    self._body()           # (thread_local: other threads' GPU calls do not invalidate the capture)
            self._key = key
        self.graph.replay()

    def run(self, tracks):
        """tracks: list of n_stems host arrays [channels, n_samples].  Returns (out ndarray, gains ndarray [2, S, n_proc]);
        with ``encode``, out is (sample bytes uint8 ndarray, clipped-sample count)."""
        pipe = staging.pipe_for(self.dev)
        for i, a in enumerate(tracks):
            pipe.upload(self.pcm[i], a)
        self.launch()
        if self.kind == 'loudness':
            return self.out.cpu().numpy(), self.gains.cpu().numpy()
        if self.encode is not None:
            return (pipe.download(self.enc), int(self.clip.sum().item())), self.gains.cpu().numpy()
        out = pipe.download(self.out)
        if self.kind == 'spectral':
            return out.reshape(-1), pipe.download(self.masked)
        return out, self.gains.cpu().numpy()

    def peaks(self):
        """MasterChain.peaks() of the last run."""
        if self.kind != 'master':
            raise ValueError('this mixer was built without ceiling_dbtp')
        return self.chain.peaks()

    def compression(self):
        """MasterChain.compression() of the last run."""
        if self.kind != 'master':
            raise ValueError('this mixer was built without a compressor')
        return self.chain.compression()


_mixers = {}


def _mixer(model, stems, loaded_tracks, chunk_length, sr, kind, normalize, out_dtype, hop_length=1024, target_lufs=-20.0,
           encode=None, dither_seed=None, ceiling_dbtp=None, limiter=None, compressor=None):
    first = np.asarray(loaded_tracks[stems[0]])
    if first.ndim != 2:
        raise ValueError('loaded_tracks[track] must be [channels, n] arrays')
    ch, n = first.shape
    dt = torch.float32 if first.dtype == np.float32 else torch.float64
    if normalize not in ('loudness', 'true_peak'):
        normalize = bool(normalize)            # the callers' ``if normalize:`` (inference.ipynb cells 9/11)
    normalize, ceiling_dbtp = MasterChain.rules(normalize, ceiling_dbtp, encode)
    times, ceiling_dbtp = MasterChain.limiter_rules(limiter, normalize, ceiling_dbtp)
    shape = MasterChain.compressor_rules(compressor, normalize)
    if normalize != 'loudness':
        target_lufs = None                     # (not part of such a mixer: one key whatever the caller passed)
    key = (id(model), len(stems), ch, n, dt, chunk_length * sr, kind, normalize, out_dtype, hop_length, sr, target_lufs,
           encode, dither_seed if encode is not None else None, ceiling_dbtp, times, shape)
    m = _mixers.get(key)
    if m is None:
        _mixers.clear()                        # one geometry at a time: a song's buffers are hundreds of MB
        m = SongMixer(model, len(stems), ch, n, dt, chunk_length * sr, kind, normalize, out_dtype, hop_length=hop_length, sr=sr,
                      target_lufs=-20.0 if target_lufs is None else target_lufs, encode=encode, dither_seed=dither_seed,
                      ceiling_dbtp=ceiling_dbtp, limiter=limiter, compressor=compressor)
        _mixers[key] = m
    np_dt = np.float32 if dt == torch.float32 else np.float64
    return m, [np.asarray(loaded_tracks[t], dtype=np_dt) for t in stems]


def _mix_song(dataset, model, loaded_tracks, chunk_length, sr, kind, normalize, out_dtype, **kw):
    """One song through the cached mixer of its geometry -> (mixer, stems, what ``run`` returned first,
    raw_gains {track: [float]}, smooth_gains {track: list of numpy float64})."""
    stems = [t for t in dataset.get_tracklist() if t != 'mix']
    m, arrays = _mixer(model, stems, loaded_tracks, chunk_length, sr, kind, normalize, out_dtype, **kw)
    out, gains = m.run(arrays)
    raw_gains = {t: [float(v) for v in gains[0, i]] for i, t in enumerate(stems)}
    return m, stems, out, raw_gains, {t: list(gains[1, i]) for i, t in enumerate(stems)}


def mix_song_smooth(dataset, model, loaded_tracks: dict, chunk_length=1, sr=44100):
    """Returns (mixed_tracks {track: ndarray[channels, n] float64}, raw_gains {track: [float]}, smooth_gains {track: list})."""
    _, stems, out, raw_gains, smooth_gains = _mix_song(dataset, model, loaded_tracks, chunk_length, sr, 'stems', False,
                                                       torch.float64)
    return {t: out[i] for i, t in enumerate(stems)}, raw_gains, smooth_gains


def mix_song_loudness(dataset, model, loaded_tracks: dict, chunk_length=1, sr=44100):
    """The loudness of what mix_song_smooth would return, without producing it: the BS.1770 integrated loudness of every
    stem times its smoothed gain ramp (what evaluation.py:102-105 measures of the model's mix), the ramp applied inside
    the meter.  Returns (lufs {track: float}, raw_gains, smooth_gains)."""
    _, stems, lufs, raw_gains, smooth_gains = _mix_song(dataset, model, loaded_tracks, chunk_length, sr, 'loudness', False,
                                                        torch.float64)
    return {t: float(lufs[i]) for i, t in enumerate(stems)}, raw_gains, smooth_gains


def mix_song_to_master(dataset, model, loaded_tracks: dict, chunk_length=1, sr=44100, normalize=True, dtype=np.float64,
                       target_lufs=-20.0, ceiling_dbtp=None, limiter=None, compressor=None):
    """mix_song_smooth followed by what every caller of the reference does next (inference.ipynb cells 9/11,
    evaluation.py:59-66): ``track_sum = np.sum(list(mixed_tracks.values()), axis=0)`` and, if ``normalize``,
    ``librosa.util.normalize(track_sum, axis=1)`` -- fused into one pass over the song on the GPU (the per-stem mixed
    tracks are never materialised).  ``normalize='loudness'`` is evaluation.py:59-66 without the file write instead: the
    sum is measured (BS.1770) and scaled to ``target_lufs``, in the same graph.  ``ceiling_dbtp`` (with 'loudness'): the
    master's true peak is held at or under that many dBTP -- at ``target_lufs`` if its peaks allow, quieter if not (one
    static gain; SongMixer.peaks() of the cached mixer tells which).  ``normalize='true_peak'``: the plain sum scaled so
    that its true peak sits at ``ceiling_dbtp`` (default -1.0), one gain for all channels.  ``limiter`` (with 'loudness';
    True or {'lookahead_ms', 'hold_ms'}): only the peaks over the ceiling (-1.0 dBTP unless given) are turned down, by a gain
    that dips ahead of each and ramps back after it, so the master stays near ``target_lufs``; SongMixer.peaks() reports the
    largest reduction, the share of samples touched and the loudness reached.  ``compressor`` (with 'loudness'; True or a dict
    with keys of MasterChain.COMPRESSOR_DEFAULTS): the sum at ``target_lufs`` is compressed (threshold in dBFS at that
    loudness, one gain for all channels, attack and release) and brought to ``target_lufs`` again before the limiter and the
    ceiling; SongMixer.compression() reports the largest reduction, the share of samples over the knee and the make-up gain.
    Returns (mix ndarray[channels, n], raw_gains, smooth_gains)."""
    out_dt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    _, _, out, raw_gains, smooth_gains = _mix_song(dataset, model, loaded_tracks, chunk_length, sr, 'master', normalize, out_dt,
                                                   target_lufs=target_lufs, ceiling_dbtp=ceiling_dbtp, limiter=limiter,
                                                   compressor=compressor)
    return out, raw_gains, smooth_gains


def mix_song_to_wav(dataset, model, loaded_tracks: dict, path, chunk_length=1, sr=44100, normalize=True, subtype='PCM_16',
                    target_lufs=-20.0, dither_seed=None, ceiling_dbtp=None, limiter=None, compressor=None):
    """mix_song_to_master followed by the callers' ``sf.write(path, master.T, sr)`` (inference.ipynb cells 9/11;
    evaluation.py:59-66 with ``normalize='loudness'``): the float64 master is quantised to ``subtype`` by the last node of
    the song's graph (ops.pcm_encode, TPDF dither if ``dither_seed`` is given), so the host receives the file's sample
    bytes -- a quarter of the float64 master for 'PCM_16' -- and writes them behind a WAV header.  The samples are those
    tests/_pcm_ref.py's quantiser makes of mix_song_to_master(..., dtype=float64).  ``ceiling_dbtp`` / ``normalize='true_peak'``
    ``limiter`` and ``compressor`` as there: with a ceiling below 0 dBTP the encoder has nothing to clip.
    Returns (clipped sample count, raw_gains, smooth_gains); warns (RuntimeWarning) when samples had to be clipped."""
    from .data.dataset_utils import write_wav_bytes
    m, _, (payload, clipped), raw_gains, smooth_gains = _mix_song(
        dataset, model, loaded_tracks, chunk_length, sr, 'master', normalize, torch.float64, target_lufs=target_lufs,
        encode=subtype, dither_seed=dither_seed, ceiling_dbtp=ceiling_dbtp, limiter=limiter, compressor=compressor)
    write_wav_bytes(path, payload, sr, m.channels, subtype, m.n, clipped)
    return clipped, raw_gains, smooth_gains


def mix_song_spectral(dataset, model, loaded_tracks: dict, chunk_length=1, sr=44100, hop_length=1024, dtype=np.float32):
    """Spectral-domain rendering of a whole song, experiments.ipynb cells 44-53 chunk by chunk, chunked exactly as
    mix_song_smooth chunks it (chunks 0 .. num_chunks-2).  Per chunk: dB features of every stem's channel mean ->
    ``masked = model(features)[0]``, the predicted mix spectrogram in dB; the phases are those of the STFT of the sum of
    the stems' channel means over the same chunk; chunk audio = istft(10 ** (masked / 20) * phases, length=chunk samples).
    Returns (audio ndarray [n_proc * chunk_length * sr] mono of ``dtype``, masked_db ndarray [n_proc, 1025, T] float32).
    Nothing is peak-normalised (the cells do not): ``masked`` is unbounded, and so is the output."""
    stems = [t for t in dataset.get_tracklist() if t != 'mix']
    m, arrays = _mixer(model, stems, loaded_tracks, chunk_length, sr, 'spectral', False, torch.float32, hop_length)
    audio, masked = m.run(arrays)
    return audio.astype(dtype, copy=False), masked
