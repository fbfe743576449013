"""Band spectrum of a mix and the spectral-balance error between two mixes -- the tonal counterpart of the loudness
profile evaluation.py compares (include/dam_hip.h: dam_spectrum_band_power / dam_spectrum_balance_error state the
definitions; csrc/dam_spectrum.hip holds the kernels).

The long-term average spectrum (LTAS) of ``sum_s stem_s * gain ramp_s`` is measured in fractional-octave bands straight
from the resident stems: the stems are summed with their gains as a frame is loaded, the frame goes through the front-end's
FFT in LDS and only float64 band powers leave the kernel -- no mix and no spectrogram is written.  Two spectra are compared
by their band levels RELATIVE TO THEIR TOTAL, so the figure does not move when every stem is scaled by a common gain, as
the loudness error does not (evaluation.py:39-53: loudness relative to the stems' mean).

Importable without a GPU (``band_edges`` and ``relative_levels_db`` are host arithmetic); the measuring functions need
CUDA tensors and raise otherwise -- there is no CPU fallback.
"""
import collections
import math
import numbers

import numpy as np
import torch

from . import features, ops

_edge_tables = {}


def band_edges(sr, n_fft, fraction=3, f_lo=25.0, f_hi=20000.0):
    """Fractional-octave bands (``fraction`` per octave, base 2, centred on 1 kHz) as runs of FFT bins -> (edges int32
    [B + 1], centres float64 [B] in Hz): band b is the bins edges[b] .. edges[b+1]-1 of an ``n_fft``-point transform at
    ``sr`` Hz.  Band indices i run from ceil(fraction log2(f_lo / 1000)) to floor(fraction log2(min(f_hi, sr/2) / 1000)),
    each formed with a slack of 1e-9 so that an exact centre is not lost to rounding; centres 1000 * 2^(i / fraction); the
    edge frequencies f_j = 1000 * 2^((2j - 1) / (2 fraction)), j = i_lo .. i_hi + 1, are computed once, so neighbouring
    bands share an edge exactly; edge bins e_j = min(n_fft/2 + 1, ceil(f_j n_fft / sr)).  A band without a bin of its own
    (e_{j+1} == e_j: below the transform's resolution, or above sr/2) is dropped together with its centre."""
    if not isinstance(n_fft, numbers.Integral) or not isinstance(fraction, numbers.Integral):
        raise TypeError('band_edges: n_fft and fraction must be integers')
    n_fft, fraction, sr, f_lo, f_hi = int(n_fft), int(fraction), float(sr), float(f_lo), float(f_hi)
    if n_fft < 2 or fraction < 1 or not sr > 0.0 or not f_lo > 0.0 or not f_hi >= f_lo:
        raise ValueError('band_edges: n_fft >= 2, fraction >= 1, sr > 0 and 0 < f_lo <= f_hi expected')
    i_lo = math.ceil(fraction * math.log2(f_lo / 1000.0) - 1e-9)
    i_hi = math.floor(fraction * math.log2(min(f_hi, sr / 2.0) / 1000.0) + 1e-9)
    top = n_fft // 2 + 1
    e = [min(top, math.ceil(1000.0 * 2.0 ** ((2 * j - 1) / (2.0 * fraction)) * n_fft / sr)) for j in range(i_lo, i_hi + 2)]
    edges, centres = [], []
    for q, i in enumerate(range(i_lo, i_hi + 1)):
        if e[q + 1] > e[q]:
            if not edges:
                edges.append(e[q])
            edges.append(e[q + 1])
            centres.append(1000.0 * 2.0 ** (i / float(fraction)))
    if not centres:
        raise ValueError('band_edges: no band between %g and %g Hz holds a bin at sr = %g, n_fft = %d' % (f_lo, f_hi, sr, n_fft))
    return np.asarray(edges, dtype=np.int32), np.asarray(centres, dtype=np.float64)


def check_edges(edges, n_fft):
    """The host copy of an edge table as the kernel needs it -> contiguous int32 [B + 1]; ValueError / TypeError for
    what dam_spectrum_band_power cannot take (the C entry only sees a device pointer: the content is checked here)."""
    if torch.is_tensor(edges):
        if edges.is_cuda:
            raise TypeError('edges must be a host table (numpy, list or CPU tensor): its content is checked before the upload')
        edges = edges.numpy()
    e = np.asarray(edges)
    if e.ndim != 1 or not np.issubdtype(e.dtype, np.integer):
        raise TypeError('edges must be a one-dimensional integer table')
    e = np.ascontiguousarray(e, dtype=np.int64)
    if e.size < 2:
        raise ValueError('edges: at least one band (two edges) expected')
    if e[0] < 0 or e[-1] > n_fft // 2 + 1 or np.any(np.diff(e) <= 0):
        raise ValueError('edges must ascend strictly within 0 .. n_fft/2 + 1 = %d, got %s' % (n_fft // 2 + 1, e.tolist()))
    return e.astype(np.int32)


def _device_edges(edges, n_fft, device):
    e = check_edges(edges, n_fft)
    _, max_bands = ops.spectrum_geometry()
    if e.size - 1 > max_bands:
        raise ValueError('at most %d bands, got %d' % (max_bands, e.size - 1))
    key = (device.type, device.index, e.tobytes())
    if key not in _edge_tables:                     # uploaded once per table and device: a captured call finds it resident
        _edge_tables[key] = torch.from_numpy(e).to(device)
    return _edge_tables[key]


def _frame_args(n_fft, hop, n, channels):
    if not isinstance(n_fft, numbers.Integral) or (hop is not None and not isinstance(hop, numbers.Integral)):
        raise TypeError('n_fft and hop must be integers')
    n_fft = int(n_fft)
    hop = n_fft // 2 if hop is None else int(hop)
    features._check_n_fft(n_fft, hop, n)
    if channels not in (1, 2):
        raise ValueError('1 or 2 channels expected, got %d' % channels)
    return n_fft, hop


def _measure(data, gains, n_fft, hop, edges):
    if not data.is_cuda:
        raise RuntimeError('deep_audio_mixer_amd kernels run on the GPU only (got a %s tensor); there is no CPU fallback'
                           % data.device)
    if data.dtype not in (torch.float32, torch.float64):
        raise TypeError('float32 or float64 samples expected')
    n_fft, hop = _frame_args(n_fft, hop, data.shape[2], data.shape[3])
    if data.shape[0] < 1 or data.shape[1] < 1 or data.shape[0] > 65535:
        raise ValueError('1..65535 mixes of at least one stem expected')
    if gains is not None:
        if not gains.is_cuda:
            raise RuntimeError('gains must be a CUDA tensor')
        if gains.dtype != torch.float64:
            raise TypeError('gains must be float64')
        if not 1 <= gains.shape[-1] <= data.shape[2]:
            raise ValueError('between one gain and one gain per sample expected')
    dev_edges = _device_edges(edges, n_fft, data.device)      # (checked before anything is launched)
    win, tw = features._get_tables(data.device, n_fft)
    return ops.spectrum_band_power(data, gains, win, tw, n_fft, hop, dev_edges)


def band_power_mix(stems, gains=None, *, n_fft=8192, hop=None, edges):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides (planar [S, channels, n] storage is passed
    as ``pcm.transpose(1, 2)``, no copy).  gains: None (the plain sum), CUDA float64 [S] or [S, n_gains] (one mix) or
    [R, S, n_gains] (R mixes of the same stems in one call).  edges: a host table of bin edges, ``band_edges(...)[0]``
    (strictly ascending within 0 .. n_fft/2 + 1, at most ops.spectrum_geometry()[1] bands).  hop defaults to n_fft / 2.
    -> CUDA float64 [R, B]: the time-averaged power of ``sum_s channel_mean(stem_s) * gain ramp`` in every band
    (frames and window exactly those of features.stft).  A row does not depend on the other rows (bitwise).  No host
    synchronisation once the tables are resident; hipGraph-capturable then."""
    if stems.dim() != 3:
        raise ValueError('stems must be [stems, samples, channels], got shape %s' % (tuple(stems.shape),))
    S = stems.shape[0]
    R = 1
    if gains is not None:
        if gains.dim() == 1:
            gains = gains.view(1, -1, 1)
        elif gains.dim() == 2:
            gains = gains.unsqueeze(0)
        if gains.dim() != 3 or gains.shape[1] != S:
            raise ValueError('gains must be [S], [S, n_gains] or [R, S, n_gains] with S = %d, got shape %s'
                             % (S, tuple(gains.shape)))
        R = gains.shape[0]
    return _measure(stems.unsqueeze(0).expand(R, -1, -1, -1), gains, n_fft, hop, edges)


def band_power_tracks(data, gains=None, *, n_fft=8192, hop=None, edges):
    """data: CUDA float32 / float64 [N, samples, channels] with any strides: N independent tracks.  gains: None or CUDA
    float64 [N] / [N, n_gains].  Otherwise as band_power_mix -> CUDA float64 [N, B]."""
    if data.dim() != 3:
        raise ValueError('data must be [tracks, samples, channels], got shape %s' % (tuple(data.shape),))
    N = data.shape[0]
    if gains is not None:
        if gains.dim() == 1:
            gains = gains.view(-1, 1)
        if gains.dim() != 2 or gains.shape[0] != N:
            raise ValueError('gains must be [N] or [N, n_gains] with N = %d, got shape %s' % (N, tuple(gains.shape)))
        gains = gains.unsqueeze(1)
    return _measure(data.unsqueeze(1), gains, n_fft, hop, edges)


def balance_error_device(ref_power, cand_power):
    """ref_power CUDA float64 [B], cand_power [V, B] (or [B]) -> (err float64 [V] in dB, n_kept int32 [V]): with
    L[b] = 10 log10(P[b] / sum P), the mean of |L_cand[b] - L_ref[b]| over the bands that hold at least -70 dB of the total
    in both spectra; NaN where no band does.  One launch for all candidates, nothing comes to the host."""
    return ops.spectrum_balance_error(ref_power, cand_power)


def relative_levels_db(power):
    """Band powers [..., B] (torch tensor or numpy array, float64) -> 10 log10(P / sum_b P), the band levels in dB relative
    to the spectrum's total; the same kind of array comes back."""
    if torch.is_tensor(power):
        return 10.0 * torch.log10(power / power.sum(dim=-1, keepdim=True))
    power = np.asarray(power, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10.0 * np.log10(power / power.sum(axis=-1, keepdims=True))


DistanceSummary = collections.namedtuple('DistanceSummary', ['mse', 'bias', 'rms_centred', 'band_mse', 'band_bias', 'band_rms',
                                                             'window_mse', 'window_bias', 'window_rms'])


def extend_edges(edges, n_fft):
    """A band table grown by one band below (bins 0 .. edges[0]-1) and one above (edges[-1] .. n_fft/2) where bins are left
    there, so that the cells of spectrogram_distance cover every bin exactly once -> (edges int32, has_low, has_high)."""
    e = check_edges(edges, n_fft).tolist()
    low, high = e[0] > 0, e[-1] < n_fft // 2 + 1
    return np.asarray(([0] if low else []) + e + ([n_fft // 2 + 1] if high else []), dtype=np.int32), low, high


def spectrogram_distance(stems, gains, ref_stems, ref_gains=None, *, n_fft=2048, hop=None, edges=None, n_windows=1, amin=1e-5):
    """The distance between the dB spectrograms of R candidate mixes and of one reference mix -- the training criterion
    (a mean squared error of amplitude_to_DB(|STFT|) features) on the audio that is rendered (include/dam_hip.h:
    dam_specdist_sums states the definition).  stems: CUDA float32 / float64 [S, samples, channels] with any strides (planar
    storage as ``pcm.transpose(1, 2)``, no copy); gains: None (one row, the plain sum) or CUDA float64 [S], [S, n_gains] or
    [R, S, n_gains], as band_power_mix takes them; ref_stems [S_ref, samples, channels] and ref_gains (None, [S_ref] or
    [S_ref, n_gains]): the reference mix as its own stems, of the same length; a finished mix is ``mix.unsqueeze(0)``.
    edges: a host table of bin edges as band_power_mix takes it, None: one band over every bin.  n_windows: W time windows by
    the mixer's gain-index rule (every window must own a frame).  amin: the floor of the levels, the model's 1e-5 (-100 dB).
    -> (sums CUDA float64 [R, B, W, 2] = (sum d, sum d^2) of d = L_cand - L_ref in dB over the cell's frames and bins,
    count CUDA int64 [B, W]).  A cell does not depend on the other rows, bands or windows (bitwise).  No mix and no
    spectrogram is written; no host synchronisation once the tables are resident, hipGraph-capturable then."""
    for t, what in ((stems, 'stems'), (ref_stems, 'ref_stems')):
        if not t.is_cuda:
            raise RuntimeError('deep_audio_mixer_amd kernels run on the GPU only (got a %s tensor); there is no CPU fallback'
                               % t.device)
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError('float32 or float64 samples expected')
        if t.dim() != 3:
            raise ValueError('%s must be [stems, samples, channels], got shape %s' % (what, tuple(t.shape)))
    S, S_ref = stems.shape[0], ref_stems.shape[0]
    if gains is not None:
        if gains.dim() == 1:
            gains = gains.view(1, -1, 1)
        elif gains.dim() == 2:
            gains = gains.unsqueeze(0)
        if gains.dim() != 3 or gains.shape[1] != S:
            raise ValueError('gains must be [S], [S, n_gains] or [R, S, n_gains] with S = %d, got shape %s'
                             % (S, tuple(gains.shape)))
    if ref_gains is not None:
        if ref_gains.dim() == 1:
            ref_gains = ref_gains.view(-1, 1)
        if ref_gains.dim() != 2 or ref_gains.shape[0] != S_ref:
            raise ValueError('ref_gains must be [S_ref] or [S_ref, n_gains] with S_ref = %d, got shape %s'
                             % (S_ref, tuple(ref_gains.shape)))
    for g in (gains, ref_gains):
        if g is not None:
            if not g.is_cuda:
                raise RuntimeError('gains must be a CUDA tensor')
            if g.dtype != torch.float64:
                raise TypeError('gains must be float64')
    R, S, n, ch, S_ref, ch_ref, n_fft, hop, W = ops.specdist_check_shapes(
        stems.shape, None if gains is None else gains.shape, ref_stems.shape, None if ref_gains is None else ref_gains.shape,
        n_fft, hop, n_windows, None, amin)
    if edges is None:
        edges = np.asarray([0, n_fft // 2 + 1], dtype=np.int32)
    dev_edges = _device_edges(edges, n_fft, stems.device)      # (checked before anything is launched)
    win, tw = features._get_tables(stems.device, n_fft)
    return ops.specdist_sums(stems, gains, ref_stems, ref_gains, win, tw, n_fft, hop, dev_edges, W, amin)


def distance_summary(sums, count):
    """sums [R, B, W, 2], count [B, W] of spectrogram_distance -> DistanceSummary of CUDA float64 tensors: mse (dB^2, the
    criterion), bias (dB) and rms_centred = sqrt(max(0, mse - bias^2)) (dB) per row [R], per band [R, B] and per window
    [R, W]; NaN where the count is 0.  One launch, nothing comes to the host."""
    out = ops.specdist_summary(sums, count)
    B, W = count.shape
    tot, band, win = out[:, 0], out[:, 1:1 + B], out[:, 1 + B:]
    return DistanceSummary(tot[:, 0], tot[:, 1], tot[:, 2], band[..., 0], band[..., 1], band[..., 2],
                           win[..., 0], win[..., 1], win[..., 2])


def _grad_args(stems, gains, ref_stems, ref_gains):
    """The tensors of spectrogram_distance_grad with the clip axis in front -> (stems, gains, ref_stems, ref_gains, clipped):
    clipped says whether the caller gave the axis."""
    for t, what in ((stems, 'stems'), (ref_stems, 'ref_stems')):
        if not t.is_cuda:
            raise RuntimeError('deep_audio_mixer_amd kernels run on the GPU only (got a %s tensor); there is no CPU fallback'
                               % t.device)
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError('float32 or float64 samples expected')
    if stems.dim() not in (3, 4) or ref_stems.dim() != stems.dim():
        raise ValueError('stems and ref_stems must both be [S, samples, channels] or [clips, S, samples, channels], got shapes '
                         '%s and %s' % (tuple(stems.shape), tuple(ref_stems.shape)))
    clipped = stems.dim() == 4
    if not clipped:
        stems, ref_stems = stems.unsqueeze(0), ref_stems.unsqueeze(0)
        gains = None if gains is None else gains.unsqueeze(0)
        ref_gains = None if ref_gains is None else ref_gains.unsqueeze(0)
    clips, S, S_ref = stems.shape[0], stems.shape[1], ref_stems.shape[1]
    if gains is not None:
        if gains.dim() == 2:
            gains = gains.view(clips, 1, -1, 1)
        elif gains.dim() == 3:
            gains = gains.unsqueeze(1)
        if gains.dim() != 4 or gains.shape[0] != clips or gains.shape[2] != S:
            raise ValueError('gains must be [S], [S, n_gains] or [R, S, n_gains] with S = %d (behind the clip axis where the stems '
                             'have one), got shape %s' % (S, tuple(gains.shape)))
    if ref_gains is not None:
        if ref_gains.dim() == 2:
            ref_gains = ref_gains.unsqueeze(-1)
        if ref_gains.dim() != 3 or ref_gains.shape[0] != clips or ref_gains.shape[1] != S_ref:
            raise ValueError('ref_gains must be [S_ref] or [S_ref, n_gains] with S_ref = %d (behind the clip axis where the stems '
                             'have one), got shape %s' % (S_ref, tuple(ref_gains.shape)))
    for g in (gains, ref_gains):
        if g is not None:
            if not g.is_cuda:
                raise RuntimeError('gains must be a CUDA tensor')
            if g.dtype != torch.float64:
                raise TypeError('gains must be float64')
    return stems, gains, ref_stems, ref_gains, clipped


def spectrogram_distance_grad(stems, gains, ref_stems, ref_gains=None, *, n_fft=2048, hop=None, amin=1e-5):
    """The criterion of spectrogram_distance over every bin and frame, and its gradient in the gains, in one fused device pass
    (include/dam_hip.h: dam_specgrad states the definition).  stems: CUDA float32 / float64 [S, samples, channels] or
    [clips, S, samples, channels] with any strides; gains: None (one row, every gain 1), CUDA float64 [S], [S, n_gains] or
    [R, S, n_gains], behind a clip axis where the stems have one; ref_stems and ref_gains as spectrogram_distance takes them,
    with the same clip axis.  n_gains == 1 or samples // n_gains >= n_fft (a frame may touch two gain segments at most).
    -> (mse [clips?, R] in dB^2, bias [clips?, R] in dB, grad_mse [clips?, R, S, n_gains] in dB^2 per unit of linear gain), CUDA
    float64: mse = S2 / N, bias = S1 / N, grad_mse = grad / N, N = frames * (n_fft / 2 + 1).  A row does not depend on the other
    rows or clips (bitwise).  No host synchronisation once the tables are resident, hipGraph-capturable then."""
    stems, gains, ref_stems, ref_gains, clipped = _grad_args(stems, gains, ref_stems, ref_gains)
    n_fft, hop = ops.specgrad_check_shapes(stems.shape, None if gains is None else gains.shape, ref_stems.shape,
                                           None if ref_gains is None else ref_gains.shape, n_fft, hop, amin)[7:9]
    win, tw = features._get_tables(stems.device, n_fft)
    value, grad = ops.specgrad(stems, gains, ref_stems, ref_gains, win, tw, n_fft, hop, amin)
    n_pairs = float((1 + stems.shape[2] // hop) * (n_fft // 2 + 1))
    mse, bias, grad_mse = value[..., 1] / n_pairs, value[..., 0] / n_pairs, grad / n_pairs
    return (mse, bias, grad_mse) if clipped else (mse[0], bias[0], grad_mse[0])


class _RenderedSpectrogramMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gains, stems, ref_stems, ref_gains, kw):
        mse, _, grad_mse = spectrogram_distance_grad(stems, gains, ref_stems, ref_gains, **kw)
        ctx.save_for_backward(grad_mse.reshape(mse.shape + (stems.shape[-3], -1)))
        ctx.gains_shape = gains.shape
        return mse

    @staticmethod
    def backward(ctx, grad_out):
        grad_mse, = ctx.saved_tensors
        return (grad_out[..., None, None] * grad_mse).reshape(ctx.gains_shape), None, None, None, None


def rendered_spectrogram_mse(stems, gains, ref_stems, ref_gains=None, **kw):
    """The training criterion on the rendered audio as a differentiable loss: spectrogram_distance_grad's mse [clips?, R], with
    a backward that hands ``grad_out[..., None, None] * grad_mse`` to ``gains`` (nothing flows to the stems or the reference).
    gains: CUDA float64, as spectrogram_distance_grad takes them and not None; from a model's dB output through
    ``(10 ** (db / 20)).double()``.  Keywords n_fft, hop, amin.  The levels are float32: torch.autograd.gradcheck's finite
    differences are not meaningful on it."""
    if gains is None:
        raise ValueError('rendered_spectrogram_mse: gains expected (there is nothing to differentiate without them)')
    if not gains.is_cuda:
        raise RuntimeError('gains must be a CUDA tensor')
    if gains.dtype != torch.float64:
        raise TypeError('gains must be float64')
    return _RenderedSpectrogramMSE.apply(gains, stems, ref_stems, ref_gains, kw)


def gain_sensitivity_db(gains, grad_mse):
    """gains and grad_mse (spectrogram_distance_grad) of one shape -> g * grad_mse * ln 10 / 20: the change of the criterion in
    dB^2 per dB of that stem in that window (d mse / d (20 log10 g)); the same kind of array comes back."""
    return gains * grad_mse * (math.log(10.0) / 20.0)
