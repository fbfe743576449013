"""BS.1770 integrated loudness on the device -- the part of the third-party ``pyloudnorm`` package the reference uses
(``pyln.Meter(sr).integrated_loudness(data)`` at data/dataset.py:118-126, evaluation.py:33,40,64,
models/baselines/mean_loudness_model.py:8,16 and ``pyln.normalize.loudness`` at evaluation.py:65,
mean_loudness_model.py:17), with the same names, argument meaning and error behaviour:

    meter = Meter(44100)                       # K-weighting, 400 ms blocks
    lufs = meter.integrated_loudness(data)     # data: [samples] or [samples, channels], numpy or torch
    out = normalize_loudness(data, lufs, -20.0)

The samples are filtered and block-averaged by ``dam_loudness_block_energy`` (HIP, float64; csrc/dam_loudness.hip); the
gating over the few thousand block energies is the host logic below, a restatement of pyloudnorm 0.1.x ``meter.py``.
There is no CPU path: without the HIP library this raises.

Batched device form, for callers that measure many tracks (evaluation.py:77-116) or sit inside a captured pipeline:

    lufs = meter.integrated_loudness_batch(pcm.transpose(1, 2))          # [N, samples, channels] -> CUDA float64 [N]
    lufs = meter.integrated_loudness_batch(stems, gains=smooth)          # loudness of stems * gain ramp, nothing written
    out = normalize_loudness_device(stems, lufs, -20.0)

filter, block energies, gating (``dam_loudness_gate``) and the normalisation gain (``dam_loudness_target_gains``) all
run on the device: no host synchronisation, hipGraph-capturable.

Peaks -- ``pyln.normalize.peak`` and the true peak (BS.1770 Annex 2 / EBU R128: the 4x oversampled signal) it lacks:

    out = normalize_peak(data, -1.0)                     # pyloudnorm: the SAMPLE peak at -1 dBFS
    out = normalize_peak(data, -1.0, true_peak=True)     # the reconstructed waveform's peak at -1 dBTP
    dbtp = true_peak(data)                               # per channel, numpy
    tp = true_peak_batch(pcm.transpose(1, 2))            # [N, channels] linear, CUDA float64, no synchronisation
    limit_gains_device(gain, tp, -1.0)                   # gain = min(gain, ceiling / max over channels), on the device
    out, info = limit_true_peak(data, 44100, -1.0)       # look-ahead limiter: only the peaks are turned down
    out, info = compress(data, 44100, -12.0, ratio=2.0)  # compressor with attack and release: the dynamics are changed

The interpolator is this package's own 49-tap windowed sinc (include/dam_hip.h); parity with libebur128 is not claimed.

Loudness over time -- the other three readings of an EBU R128 meter, which pyloudnorm lacks: one value per 100 ms hop of
the 400 ms (momentary) and 3 s (short-term) windows, and the loudness range of EBU Tech 3342 over the short-term curve:

    d = meter.loudness_dynamics_batch(pcm.transpose(1, 2), gains=smooth)     # curves, their maxima, LRA: one filter pass
    lra = meter.loudness_range_batch(pcm.transpose(1, 2))                    # CUDA float64 [N] LU
    lu = loudness_range(data, 44100)                                         # one array, a float

all on the device without synchronisation (dam_loudness_window_power, dam_loudness_curve_stats); profile_error_device
compares the short-term curves of two mixes window by window (evaluation.LoudnessEvaluator, ``dynamics=True``).
"""
import ctypes
import warnings

import numpy as np
import torch

from . import _lib

_CHANNEL_GAINS = (1.0, 1.0, 1.0, 1.41, 1.41)      # L, R, C, Ls, Rs (pyloudnorm meter.py: G)


def _as_device_2d(data):
    """[samples] or [samples, channels] (numpy or torch) -> CUDA tensor [samples, channels] of float32/float64."""
    if isinstance(data, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(data))
    elif torch.is_tensor(data):
        t = data
    else:
        raise ValueError('Data must be of type numpy.ndarray or torch.Tensor.')
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError('Data must be floating point.')
    if t.dim() == 1:
        t = t.reshape(-1, 1)
    elif t.dim() != 2:
        raise ValueError('Audio must be [samples] or [samples, channels].')
    if t.shape[1] > 5:
        raise ValueError('Audio must have five channels or less.')
    if not t.is_cuda:
        t = t.cuda()
    return t


class Meter:
    """Same constructor surface as ``pyloudnorm.Meter`` for what the reference uses: ``Meter(rate)``."""

    def __init__(self, rate, filter_class='K-weighting', block_size=0.400):
        if filter_class != 'K-weighting':
            raise ValueError('only the K-weighting filter class is provided')
        self.rate = rate
        self.block_size = block_size
        coef = (ctypes.c_double * 12)()
        _lib.check(_lib.lib().dam_loudness_kweight_coeffs(float(rate), coef), 'dam_loudness_kweight_coeffs')
        self._coef = coef
        self.coefficients = np.array(list(coef)).reshape(2, 6)          # [stage][b0 b1 b2 a0 a1 a2]
        self._bounds = {}                                               # _block_bounds' cache
        self._hops = {}                                                 # _hop_bounds' cache

    # ---- device part: block mean squares z[channel][block]
    def block_energies(self, data):
        x = _as_device_2d(data)
        n, ch = x.shape
        T_g = self.block_size
        if n < T_g * self.rate:
            raise ValueError('Audio must have length greater than the block size.')
        dev = x.device
        lo_d, hi_d = self._block_bounds(n, dev)
        num_blocks = lo_d.numel()
        z = torch.empty((ch, num_blocks), dtype=torch.float64, device=dev)
        L = _lib.lib()
        ws = torch.empty(L.dam_loudness_workspace_bytes(n, ch), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.dam_loudness_block_energy(_lib.ptr(x), 1 if x.dtype == torch.float64 else 0, n, ch, x.stride(0),
                                                   x.stride(1), self._coef, _lib.ptr(lo_d), _lib.ptr(hi_d), num_blocks,
                                                   float(T_g * self.rate), _lib.ptr(z), _lib.ptr(ws), _lib.stream()),
                       'dam_loudness_block_energy')
        return z.cpu().numpy()

    # ---- host part: two-stage gating (pyloudnorm meter.py integrated_loudness)
    def integrated_loudness(self, data):
        z = self.block_energies(data)
        return gated_loudness(z)


    # ---- batched device form: nothing below synchronises with the host
    def _block_bounds(self, n, dev):
        """Device block bounds of an n-sample track, cached per (device, n, rate, block size) so that a captured call
        holds stable pointers."""
        key = (dev, n, self.rate, self.block_size)
        if key not in self._bounds:
            T_g, step = self.block_size, 0.25                                # 75 % overlap
            num_blocks = int(np.round(((n / self.rate - T_g) / (T_g * step))) + 1)
            j = np.arange(0, num_blocks)
            # meter.py: l = int(T_g * (j * step) * rate), u = int(T_g * (j * step + 1) * rate) -- the same float64 operations
            # in the same order, element-wise (int() and astype both truncate)
            lo = (T_g * (j * step) * self.rate).astype(np.int64)
            hi = (T_g * (j * step + 1) * self.rate).astype(np.int64)
            self._bounds[key] = (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))
        return self._bounds[key]

    def _energies_batch(self, data, gains, lo_d, hi_d, length, out=None):
        """Sum of squares of the K-weighted ``data * gain ramp`` over the samples [lo_d[k], hi_d[k]) of every track and
        channel, divided by ``length`` -> [N, channels, K] float64: the one call of dam_loudness_block_energy_batch.  data
        is a CUDA [N, samples, channels] tensor here (the public methods have checked that much)."""
        from . import ops
        if data.dtype not in (torch.float32, torch.float64):
            raise ValueError('Data must be floating point.')
        N, n, ch = data.shape
        if ch > 5:
            raise ValueError('Audio must have five channels or less.')
        dev = data.device
        gains, n_gains = ops.gain_ramp_arg(gains, N, n)
        K = lo_d.numel()
        if out is None:
            out = torch.empty((N, ch, K), dtype=torch.float64, device=dev)
        elif tuple(out.shape) != (N, ch, K) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError('bad out tensor')
        L = _lib.lib()
        ws = torch.empty(L.dam_loudness_batch_workspace_bytes(N, n, ch, K) // 8 + 1, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.dam_loudness_block_energy_batch(
                _lib.ptr(data), 1 if data.dtype == torch.float64 else 0, N, n, ch, data.stride(0), data.stride(1),
                data.stride(2), _lib.ptr(gains), n_gains, self._coef, _lib.ptr(lo_d), _lib.ptr(hi_d), K, float(length),
                _lib.ptr(out), _lib.ptr(ws), _lib.stream()), 'dam_loudness_block_energy_batch')
        return out

    def block_energies_batch(self, data, gains=None, out=None):
        """data: CUDA float32/float64 [N, samples, channels] with any strides (planar [N, channels, n] storage is passed
        as ``pcm.transpose(1, 2)``, no copy).  gains: optional CUDA float64 [N, n_gains] (or [N]): every track is
        measured as ``data[t] * interpolate_mask(gains[t])`` -- the float64 product ops.gain_ramp_apply would store --
        without that product being written.  Returns z [N, channels, blocks] float64 on the device."""
        if not torch.is_tensor(data):
            raise ValueError('Data must be of type torch.Tensor.')
        _lib.require_cuda(data, gains, out)
        if data.dim() != 3:
            raise ValueError('Audio must be [tracks, samples, channels].')
        if data.shape[1] < self.block_size * self.rate:
            raise ValueError('Audio must have length greater than the block size.')
        lo_d, hi_d = self._block_bounds(data.shape[1], data.device)
        return self._energies_batch(data, gains, lo_d, hi_d, self.block_size * self.rate, out)

    def integrated_loudness_batch(self, data, gains=None, out=None):
        """Integrated loudness of every track of ``data`` (see block_energies_batch) -> CUDA float64 [N]; a track the gates
        empty reads -inf.  No host synchronisation."""
        return gate_loudness_device(self.block_energies_batch(data, gains), out=out)

    # ---- loudness over time (EBU R128 momentary / short-term, Tech 3342 loudness range); device only, no synchronisation
    def _hop_bounds(self, n, dev):
        """Device bounds of the 100 ms hops of an n-sample track, cached per (device, n, rate) like _block_bounds."""
        key = (dev, n, self.rate)
        if key not in self._hops:
            h = int(round(0.1 * self.rate))
            lo = np.arange(n // h, dtype=np.int64) * h
            self._hops[key] = (torch.from_numpy(lo).to(dev), torch.from_numpy(lo + h).to(dev), h)
        return self._hops[key]

    def hop_energies_batch(self, data, gains=None):
        """Mean square of the K-weighted signal over every 100 ms hop: data and gains as block_energies_batch takes them
        -> CUDA float64 [N, channels, H], H = samples // round(0.1 * rate) (a shorter tail is dropped).  The same filter
        passes as the integrated meter (dam_loudness_block_energy_batch) with hop bounds in place of gating blocks."""
        if not torch.is_tensor(data):
            raise ValueError('Data must be of type torch.Tensor.')
        if not data.is_cuda or (gains is not None and not gains.is_cuda):
            raise ValueError('Data and gains must be CUDA tensors: the meter runs on the GPU only, there is no CPU fallback.')
        if data.dim() != 3:
            raise ValueError('Audio must be [tracks, samples, channels].')
        lo_d, hi_d, h = self._hop_bounds(data.shape[1], data.device)
        if lo_d.numel() < 1:
            raise ValueError('Audio must have length greater than one 100 ms hop.')
        return self._energies_batch(data, gains, lo_d, hi_d, h)

    def _curves(self, data, gains, hops, what):
        e = self.hop_energies_batch(data, gains)
        if e.shape[2] < hops:
            raise ValueError('Audio must be at least %d hops of 100 ms long for %s loudness.' % (hops, what))
        return e

    def momentary_loudness_batch(self, data, gains=None):
        """Momentary loudness (EBU R128: 400 ms window, one value per 100 ms hop) of every track -> CUDA float64
        [N, H - 3] LUFS; silence reads -inf.  The window is R128's whatever ``block_size`` this Meter was built with."""
        return window_loudness_device(self._curves(data, gains, 4, 'momentary'), 4)[1]

    def short_term_batch(self, data, gains=None, want_lufs=True):
        """The short-term windows (EBU R128: 3 s, one per 100 ms hop) of every track -> (power, LUFS or None), CUDA
        float64 [N, H - 29] each: what curve_stats_device and profile_error_device take."""
        return window_loudness_device(self._curves(data, gains, 30, 'short-term'), 30, want_lufs)

    def short_term_loudness_batch(self, data, gains=None):
        """Short-term loudness (EBU R128: 3 s window, one value per 100 ms hop) of every track -> CUDA float64
        [N, H - 29] LUFS; silence reads -inf.  The window is R128's whatever ``block_size`` this Meter was built with."""
        return self.short_term_batch(data, gains)[1]

    def loudness_range_batch(self, data, gains=None):
        """Loudness range (EBU Tech 3342: the 10th to 95th percentile of the short-term loudness gated at -70 LUFS and at
        -20 LU under the gated mean) of every track -> CUDA float64 [N] LU; a track the gates empty reads 0."""
        return curve_stats_device(self.short_term_batch(data, gains, want_lufs=False)[0])[:, 0]

    def loudness_dynamics_batch(self, data, gains=None):
        """Every time-resolved reading from one pass of the filter: {'momentary' [N, H - 3], 'short_term' [N, H - 29]
        (LUFS curves), 'momentary_max', 'short_term_max', 'lra', 'lra_low', 'lra_high' ([N]; LU and the two percentile
        levels in LUFS)}, all CUDA float64.  The windows are R128's 0.4 s and 3 s, one value per 100 ms, whatever
        ``block_size`` this Meter was built with (that argument shapes the integrated measurement only)."""
        e = self._curves(data, gains, 30, 'short-term')
        m_power, m_lufs = window_loudness_device(e, 4)
        s_power, s_lufs = window_loudness_device(e, 30)
        m_stats, s_stats = curve_stats_device(m_power), curve_stats_device(s_power)
        return {'momentary': m_lufs, 'short_term': s_lufs, 'momentary_max': m_stats[:, 5], 'short_term_max': s_stats[:, 5],
                'lra': s_stats[:, 0], 'lra_low': s_stats[:, 1], 'lra_high': s_stats[:, 2]}


def window_loudness_device(e, w, want_lufs=True):
    """Sliding-window loudness of hop energies e CUDA float64 [N, channels, H]: windows of w hops, one per hop ->
    (power [N, H - w + 1], LUFS of the same shape or None) (dam_loudness_window_power)."""
    _lib.require_cuda(e)
    if e.dtype != torch.float64 or e.dim() != 3:
        raise ValueError('e must be float64 [tracks, channels, hops]')
    e = e.contiguous()
    N, ch, H = e.shape
    if ch > 5:
        raise ValueError('Audio must have five channels or less.')
    if not 1 <= w <= H:
        raise ValueError('a window of 1 to %d hops expected' % H)
    power = torch.empty((N, H - w + 1), dtype=torch.float64, device=e.device)
    lufs = torch.empty_like(power) if want_lufs else None
    with torch.cuda.device(e.device):
        _lib.check(_lib.lib().dam_loudness_window_power(_lib.ptr(e), N, ch, H, w, _lib.ptr(power), _lib.ptr(lufs),
                                                        _lib.stream()), 'dam_loudness_window_power')
    return power, lufs


def curve_stats_device(power):
    """Gated statistics of power curves: power CUDA float64 [N, W] (window_loudness_device) -> [N, 6] =
    (LRA, low percentile LUFS, high percentile LUFS, relative gate LUFS, values kept, maximum LUFS) as
    include/dam_hip.h defines them for dam_loudness_curve_stats.  Exact order statistics at any W."""
    _lib.require_cuda(power)
    if power.dtype != torch.float64 or power.dim() != 2 or power.shape[1] < 1:
        raise ValueError('power must be float64 [tracks, windows]')
    power = power.contiguous()
    N, W = power.shape
    out = torch.empty((N, 6), dtype=torch.float64, device=power.device)
    with torch.cuda.device(power.device):
        _lib.check(_lib.lib().dam_loudness_curve_stats(_lib.ptr(power), N, W, _lib.ptr(out), _lib.stream()),
                   'dam_loudness_curve_stats')
    return out


def profile_error_device(ref_lufs, cand_lufs):
    """Time-resolved loudness error: ref_lufs CUDA float64 [S, W], cand_lufs [V, S, W] (or [S, W]: one variant), short-term
    curves of the S stems of a reference mix and of V candidates -> (err [V], active [V]): over the windows in which every
    stem of both is at or above -70 LUFS, the mean |(C - mean_s C) - (R - mean_s R)|, and how many such windows there
    were; NaN where there were none (dam_loudness_profile_error)."""
    _lib.require_cuda(ref_lufs, cand_lufs)
    if cand_lufs.dim() == 2:
        cand_lufs = cand_lufs.unsqueeze(0)
    if ref_lufs.dtype != torch.float64 or cand_lufs.dtype != torch.float64 or ref_lufs.dim() != 2 or cand_lufs.dim() != 3:
        raise ValueError('float64 [stems, windows] and [variants, stems, windows] expected')
    if tuple(cand_lufs.shape[1:]) != tuple(ref_lufs.shape):
        raise ValueError('reference and candidate curves differ in shape: %s and %s'
                         % (tuple(ref_lufs.shape), tuple(cand_lufs.shape[1:])))
    ref_lufs, cand_lufs = ref_lufs.contiguous(), cand_lufs.contiguous()
    V, S, W = cand_lufs.shape
    if V < 1 or S < 1 or W < 1:
        raise ValueError('at least one variant, stem and window expected')
    err = torch.empty(V, dtype=torch.float64, device=ref_lufs.device)
    active = torch.empty_like(err)
    with torch.cuda.device(ref_lufs.device):
        _lib.check(_lib.lib().dam_loudness_profile_error(_lib.ptr(ref_lufs), _lib.ptr(cand_lufs), V, S, W, _lib.ptr(err),
                                                         _lib.ptr(active), _lib.stream()), 'dam_loudness_profile_error')
    return err, active


def loudness_range(data, rate):
    """Loudness range in LU (EBU Tech 3342) of one [samples] or [samples, channels] array (numpy or torch) at ``rate`` Hz
    -> float; the host convenience beside Meter.loudness_range_batch, as true_peak is beside true_peak_batch."""
    x = _as_device_2d(data)
    return float(Meter(rate).loudness_range_batch(x.unsqueeze(0)).item())


def gate_loudness_device(z, out=None):
    """gated_loudness on the device: z CUDA float64 [N, channels, blocks] -> LUFS [N] (dam_loudness_gate)."""
    _lib.require_cuda(z, out)
    if z.dtype != torch.float64 or z.dim() != 3:
        raise ValueError('z must be float64 [tracks, channels, blocks]')
    z = z.contiguous()
    N, ch, nb = z.shape
    if ch > 5:
        raise ValueError('Audio must have five channels or less.')
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=z.device)
    elif tuple(out.shape) != (N,) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('bad out tensor')
    with torch.cuda.device(z.device):
        _lib.check(_lib.lib().dam_loudness_gate(_lib.ptr(z), N, ch, nb, _lib.ptr(out), _lib.stream()), 'dam_loudness_gate')
    return out


def target_gains_device(lufs_dev, target, out=None):
    """10 ** ((target - lufs) / 20) per track on the device (dam_loudness_target_gains).  lufs_dev: CUDA float64 [N];
    target: a float, a sequence of N floats or a CUDA float64 [N] tensor (pass a tensor inside a graph capture: a host
    value is uploaded).  A silent track (lufs -inf) gets the gain +inf, as ``np.power`` gives in normalize_loudness."""
    _lib.require_cuda(lufs_dev, out)
    if lufs_dev.dtype != torch.float64:
        raise TypeError('lufs must be float64')
    lufs_dev = lufs_dev.contiguous().view(-1)
    N = lufs_dev.numel()
    if torch.is_tensor(target):
        _lib.require_cuda(target)
        tgt = target.to(torch.float64).contiguous().view(-1)
    else:
        t = np.asarray(target, dtype=np.float64)
        tgt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(t, (N,)) if t.ndim == 0 else t)).to(lufs_dev.device)
    if tgt.numel() != N:
        raise ValueError('one target per track expected')
    if out is None:
        out = torch.empty(N, dtype=torch.float64, device=lufs_dev.device)
    elif out.numel() != N or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('bad out tensor')
    with torch.cuda.device(lufs_dev.device):
        _lib.check(_lib.lib().dam_loudness_target_gains(_lib.ptr(lufs_dev), _lib.ptr(tgt), N, _lib.ptr(out), _lib.stream()),
                   'dam_loudness_target_gains')
    return out


def normalize_loudness_device(data, lufs_dev, target, out_dtype=None):
    """normalize_loudness for a batch that stays on the device: data CUDA [N, ...] (every track one leading index, any
    layout behind it), lufs_dev CUDA float64 [N] (integrated_loudness_batch), target a float or per-track targets.
    The gain comes from dam_loudness_target_gains, the product is ops.gain_ramp_apply with one gain per track; the result
    is float64 unless out_dtype says otherwise (the float32-track * float64-gain product).  Unlike normalize_loudness
    this issues NO 'Possible clipped samples' warning: looking at the peak would need a host synchronisation."""
    from . import ops
    _lib.require_cuda(data)
    N = data.shape[0]
    g = target_gains_device(lufs_dev, target)
    # a dense tensor stored as [N, channels, n] and viewed as [N, n, channels] is scaled in place of its storage order
    if data.dim() == 3 and not data.is_contiguous() and data.transpose(1, 2).is_contiguous():
        return ops.gain_ramp_apply(data.transpose(1, 2), g.view(N, 1), out_dtype=out_dtype).transpose(1, 2)
    flat = data.contiguous().view(N, 1, -1)
    return ops.gain_ramp_apply(flat, g.view(N, 1), out_dtype=out_dtype).view(data.shape)


def true_peak_batch(data, gains=None, out=None):
    """Linear true peak of every track and channel: data CUDA float32/float64 [N, samples, channels] with any strides, as
    integrated_loudness_batch takes it; gains as there.  Returns CUDA float64 [N, channels] (dam_true_peak_batch); a
    silent row reads exactly 0.0.  No host synchronisation."""
    from . import ops
    if not torch.is_tensor(data):
        raise ValueError('Data must be of type torch.Tensor.')
    _lib.require_cuda(data, gains, out)
    if data.dtype not in (torch.float32, torch.float64):
        raise ValueError('Data must be floating point.')
    if data.dim() != 3:
        raise ValueError('Audio must be [tracks, samples, channels].')
    return ops.true_peak_batch(data, gains=gains, out=out)


def true_peak(data):
    """dBTP per channel of one [samples] or [samples, channels] array (numpy or torch) -> numpy float64 [channels];
    silence reads -inf."""
    x = _as_device_2d(data)
    tp = true_peak_batch(x.unsqueeze(0))[0].cpu().numpy()
    with np.errstate(divide='ignore'):
        return 20.0 * np.log10(tp)


def normalize_peak(data, target_db, true_peak=False):
    """``pyloudnorm.normalize.peak``: constant gain so that the largest |sample| over all channels sits at ``target_db``
    dBFS.  true_peak=True takes the same gain from the true peak instead (dBTP): the reconstructed waveform, not just
    its samples, then stays at or under the target."""
    if true_peak:
        current_peak = float(true_peak_batch(_as_device_2d(data).unsqueeze(0)).max().item())
    else:
        current_peak = float(data.abs().max()) if torch.is_tensor(data) else float(np.max(np.abs(data)))
    gain = np.power(10.0, target_db / 20.0) / current_peak
    output = gain * data
    peak = float(output.abs().max()) if torch.is_tensor(output) else float(np.max(np.abs(output)))
    if peak >= 1.0:
        warnings.warn('Possible clipped samples in output.')
    return output


def limit_gains_device(gains, peaks, ceiling_db):
    """Clamps device gains (CUDA float64 [G], in place) so that ``gain * max(peaks[g])`` stays at or under ``ceiling_db``:
    peaks CUDA float64 [G, k] linear (true_peak_batch of what the gain will scale: the maximum is taken over the k
    channels).  A zero peak leaves the gain alone.  Returns gains; no host synchronisation (dam_peak_limit_gains)."""
    from . import ops
    return ops.peak_limit_gains(gains, peaks, ceiling_db)


def limit_true_peak_device(data, rate, ceiling_dbtp=-1.0, lookahead_ms=5.0, hold_ms=20.0, pre_gain=None, out_dtype=None):
    """Look-ahead true-peak limiter on the device: data CUDA float32/float64 [N, samples, channels] with any strides (N
    masters, the channels of each limited together), pre_gain an optional CUDA float64 [N] applied first.  Returns
    (limited planar [N, channels, samples], float64 unless out_dtype is given; min_gain CUDA float64 [N]; n_limited CUDA
    int64 [N]).  The gain dips ``lookahead_ms`` before a peak that would pass ``ceiling_dbtp``, holds ``hold_ms`` behind it
    and ramps back linearly (dam_limiter_apply); where nothing comes near the ceiling the samples pass bit for bit.  The true
    peak of the result can exceed the ceiling by a few 1e-5 dB.  No host synchronisation."""
    from . import ops
    if not torch.is_tensor(data):
        raise ValueError('Data must be of type torch.Tensor.')
    _lib.require_cuda(data, pre_gain)
    if data.dtype not in (torch.float32, torch.float64):
        raise ValueError('Data must be floating point.')
    if data.dim() != 3:
        raise ValueError('Audio must be [tracks, samples, channels].')
    return ops.limiter_apply(data, ceiling_dbtp, ops.limiter_samples(lookahead_ms, rate), ops.limiter_samples(hold_ms, rate),
                             pre_gain=pre_gain, out_dtype=out_dtype)


def limit_true_peak(data, rate, ceiling_dbtp=-1.0, lookahead_ms=5.0, hold_ms=20.0):
    """One [samples] or [samples, channels] array (numpy or torch) through the look-ahead true-peak limiter, in the style of
    normalize_peak: returns (limited, info) with ``limited`` a numpy array of data's shape and dtype and info =
    {'max_reduction_db': 20 log10 of the smallest gain (0.0: untouched), 'limited_share': the share of samples whose gain is
    below 1, 'lookahead_samples', 'hold_samples'}."""
    from . import ops
    x = _as_device_2d(data)
    L, H = ops.limiter_samples(lookahead_ms, rate), ops.limiter_samples(hold_ms, rate)
    out, min_gain, n_limited = ops.limiter_apply(x.unsqueeze(0), ceiling_dbtp, L, H, out_dtype=x.dtype)
    limited = out[0].t().cpu().numpy().reshape(tuple(data.shape))
    return limited, {'max_reduction_db': float(20.0 * np.log10(min_gain.item())),
                     'limited_share': n_limited.item() / x.shape[0], 'lookahead_samples': L, 'hold_samples': H}


def compress_device(data, rate, threshold_db=-12.0, ratio=2.0, knee_db=6.0, attack_ms=10.0, release_ms=100.0, makeup_db=0.0,
                    pre_gain=None, out_dtype=None, reduction_out=None):
    """Feed-forward compressor on the device: data CUDA float32/float64 [N, samples, channels] with any strides (N tracks,
    the channels of each compressed with one gain), pre_gain an optional CUDA float64 [N] applied first -- the threshold is
    in dBFS of ``data * pre_gain``.  Above ``threshold_db`` the level rises by 1/``ratio`` dB per dB (``float('inf')``: not
    at all), through a quadratic knee ``knee_db`` wide; the reduction follows the curve with ``attack_ms`` and decays with
    ``release_ms`` (dam_compressor_apply: include/dam_hip.h states the definition).  Returns (compressed planar [N,
    channels, samples], float64 unless out_dtype is given; max_reduction CUDA float64 [N] in dB; n_over CUDA int64 [N], the
    samples above the knee's start).  reduction_out: optional CUDA float64 [N, samples] for the gain-reduction curve in dB.
    Where nothing has reached the knee yet the samples pass bit for bit (times the make-up).  No host synchronisation."""
    from . import ops
    if not torch.is_tensor(data):
        raise ValueError('Data must be of type torch.Tensor.')
    _lib.require_cuda(data, pre_gain)
    if data.dtype not in (torch.float32, torch.float64):
        raise ValueError('Data must be floating point.')
    if data.dim() != 3:
        raise ValueError('Audio must be [tracks, samples, channels].')
    constants = ops.compressor_constants(threshold_db, knee_db, attack_ms, release_ms, rate, makeup_db)
    return ops.compressor_apply(data, threshold_db, ratio, knee_db, *constants, pre_gain=pre_gain, out_dtype=out_dtype,
                                reduction_out=reduction_out)


def compress(data, rate, threshold_db=-12.0, ratio=2.0, knee_db=6.0, attack_ms=10.0, release_ms=100.0, makeup_db=0.0):
    """One [samples] or [samples, channels] array (numpy or torch) through the compressor, in the style of limit_true_peak:
    returns (compressed, info) with ``compressed`` a numpy array of data's shape and dtype and info = {'max_reduction_db':
    the largest gain reduction in dB (0.0: untouched), 'over_share': the share of samples above the knee's start,
    'reduction_db': the gain-reduction curve, numpy float64 [samples]}."""
    x = _as_device_2d(data)
    reduction = torch.empty((1, x.shape[0]), dtype=torch.float64, device=x.device)
    out, max_reduction, n_over = compress_device(x.unsqueeze(0), rate, threshold_db, ratio, knee_db, attack_ms, release_ms,
                                                 makeup_db, out_dtype=x.dtype, reduction_out=reduction)
    compressed = out[0].t().cpu().numpy().reshape(tuple(data.shape))
    return compressed, {'max_reduction_db': float(max_reduction.item()), 'over_share': n_over.item() / x.shape[0],
                        'reduction_db': reduction[0].cpu().numpy()}


def gated_loudness(z):
    """LUFS from block mean squares z[channel][block]: absolute gate -70, relative gate -10 LU (BS.1770-4)."""
    num_channels, num_blocks = z.shape
    G = np.array(_CHANNEL_GAINS[:num_channels])
    Gamma_a = -70.0
    with np.errstate(divide='ignore', invalid='ignore'):
        l = -0.691 + 10.0 * np.log10(np.sum(G[:, None] * z, axis=0))
        J_g = [j for j, l_j in enumerate(l) if l_j >= Gamma_a]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', category=RuntimeWarning)
            z_avg_gated = [np.mean([z[i, j] for j in J_g]) for i in range(num_channels)]
        Gamma_r = -0.691 + 10.0 * np.log10(np.sum([G[i] * z_avg_gated[i] for i in range(num_channels)])) - 10.0
        J_g = [j for j, l_j in enumerate(l) if (l_j > Gamma_r and l_j > Gamma_a)]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', category=RuntimeWarning)
            z_avg_gated = np.nan_to_num(np.array([np.mean([z[i, j] for j in J_g]) for i in range(num_channels)]))
        LUFS = -0.691 + 10.0 * np.log10(np.sum([G[i] * z_avg_gated[i] for i in range(num_channels)]))
    return float(LUFS)


def normalize_loudness(data, input_loudness, target_loudness):
    """``pyloudnorm.normalize.loudness``: constant gain so that a signal measured at input_loudness reads target_loudness."""
    delta_loudness = target_loudness - input_loudness
    gain = np.power(10.0, delta_loudness / 20.0)
    output = gain * data
    peak = float(output.abs().max()) if torch.is_tensor(output) else float(np.max(np.abs(output)))
    if peak >= 1.0:
        warnings.warn('Possible clipped samples in output.')
    return output
