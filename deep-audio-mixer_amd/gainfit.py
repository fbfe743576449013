"""The gains a reference mix used, fitted on the device, and the distance of a gain curve from them -- the direct
counterpart of the loudness, short-term and spectral errors evaluation.py reports (include/dam_hip.h: dam_gainfit_moments /
dam_gainfit_solve / dam_gainfit_gain_error state the definitions; csrc/dam_gainfit.hip holds the kernels).

The model predicts one gain per stem and window.  A windowed least-squares fit of ``sum_s stem_s * g[s, w] ~ mix`` over the
same windows (the gain index of the mixer's ramp) gives the gains the reference mix used, the share of the reference no
gain-only mixer can explain (the residual: the ceiling of any model of this family) and, for any candidate gain curve, its
distance from the fitted one in dB, stem by stem and window by window.  The distance is taken RELATIVE TO THE WINDOW'S
MEAN over the stems: a common gain on all stems is a master fader, not a balance decision -- as the loudness error is
relative to the stems' mean (evaluation.py:39-53).

Importable without a GPU (``residual_db`` and the argument checks are host arithmetic); the measuring functions need
CUDA tensors and raise otherwise -- there is no CPU fallback.
"""
import numpy as np
import torch

from . import features, ops, spectrum


def moments(stems, mix, n_windows):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides (planar [S, channels, n] storage is passed
    as ``pcm.transpose(1, 2)``, no copy), 1 <= S <= 8, 1 or 2 channels.  mix: CUDA float32 / float64 [samples, channels]
    with any strides; its dtype need not be the stems'.  -> CUDA float64 [W, S + 1, S + 1]: for every window the sums of
    products of the S + 1 signals (stems, then the mix) over the window's samples and channels, exactly symmetric.  Window w
    holds the samples whose gain index in the mixer's ramp is w.  A window's matrix does not depend on the other windows
    (bitwise: the same samples as a call of their own with one window give the same bits).  No host synchronisation."""
    ops.gainfit_check_shapes(tuple(stems.shape), tuple(mix.shape), n_windows)
    return ops.gainfit_moments(stems, mix, n_windows)


def solve(moment_matrices, *, pool=0, ridge=0.0):
    """moments [W, S + 1, S + 1] -> (gains float64 [S, W], residual float64 [W], status int32 [W]), all on the device.
    pool: windows w - pool .. w + pool are fitted together (their moments added) for the gains of window w.  ridge: added
    to the diagonal of the unit-diagonal normal matrix; 0 is plain least squares.  A stem more than 80 dB under the mix in a
    window is not fitted there: its gain is NaN.  status: the number of fitted stems; 0 where the mix is silent (all NaN);
    -1 where the fitted stems are linearly dependent (all NaN; a ridge resolves it).  residual: the share of the mix's
    energy the fitted gains leave unexplained, 0 .. 1 (``residual_db`` turns it into dB)."""
    pool, ridge = ops.gainfit_check_solve_args(pool, ridge)
    return ops.gainfit_solve(moment_matrices, pool, ridge)


def fit_gains(stems, mix, n_windows, *, pool=0, ridge=0.0, align=None, align_weighting='phat'):
    """``solve(moments(stems, mix, n_windows), pool=pool, ridge=ridge)`` -> (gains [S, W], residual [W], status [W]): the
    gains the mix used, in the mixer's layout.  Nothing comes to the host; hipGraph-capturable.
    align: None (the stems and the mix are taken as aligned), or ``max_lag`` in samples: the lag of every stem against the
    mix is estimated within +-max_lag (align.estimate_lag with ``align_weighting``: 'phat', or 'plain' for near-sinusoidal
    stems, which PHAT loses), the stems are shifted by it on the device and the shifted stems are fitted -- for a mix that
    is not the sum of these very arrays.  The lags themselves are ``align.estimate_lag``'s to report."""
    ops.gainfit_check_shapes(tuple(stems.shape), tuple(mix.shape), n_windows)
    pool, ridge = ops.gainfit_check_solve_args(pool, ridge)
    if align is not None:
        ops.align_check_shapes(tuple(stems.shape), tuple(mix.shape), align, align_weighting)
        stems = ops.align_shift(stems, ops.align_estimate(stems, mix, align, align_weighting)[0])
    return ops.gainfit_solve(ops.gainfit_moments(stems, mix, n_windows), pool, ridge)


def gain_error_device(fit, cand):
    """fit CUDA float64 [S, W]; cand [V, S, W], [V, S, 1] (constant gains) or one variant [S, W] / [S, 1] -> (err float64
    [V] in dB, err_stem float64 [V, S], n_kept int32 [V]): with d = 20 log10(cand / fit) where both are finite and
    positive, the mean of |d - the window's mean d| over the windows that keep at least two stems; NaN where none does.
    One launch for all candidates, nothing comes to the host."""
    return ops.gainfit_gain_error(fit, cand)


def _band_args(stems, mix, n_windows, n_fft, hop, edges):
    """Everything band_moments checks on the host, before anything is launched -> (n_fft, hop, host edge table)."""
    n_fft, hop = ops.gainfit_band_check_shapes(tuple(stems.shape), tuple(mix.shape), n_windows, n_fft, hop)[4:]
    table = spectrum.check_edges(edges, n_fft)
    ops.gainfit_band_check_shapes(tuple(stems.shape), tuple(mix.shape), n_windows, n_fft, hop, table.size - 1)
    return n_fft, hop, table


def _band_moments(stems, mix, n_windows, n_fft, hop, table):
    ops._lib.require_cuda(stems, mix)
    dev_edges = spectrum._device_edges(table, n_fft, stems.device)      # resident after the first call, as the tables below
    win, tw = features._get_tables(stems.device, n_fft)
    return ops.gainfit_band_moments(stems, mix, n_windows, win, tw, n_fft, hop, dev_edges)


def band_moments(stems, mix, n_windows, *, n_fft=4096, hop=None, edges):
    """stems, mix, n_windows as ``moments`` takes them; edges: a host table of bin edges, ``spectrum.band_edges(...)[0]``
    (strictly ascending within 0 .. n_fft/2 + 1, at most ops.GAINFIT_BAND_MAX_BANDS bands); hop defaults to n_fft / 2.
    -> CUDA float64 [B, W, S + 1, S + 1]: for every band and window the sums, over the band's bins, the window's frames and
    the channels, of Re(conj(U_i) U_j) of the S + 1 signals' STFTs (frames and window exactly those of features.stft, every
    channel transformed on its own), exactly symmetric.  Window w holds the frames whose centre sample has gain index w in
    the mixer's ramp; every window must own a frame.  Frames reach n_fft / 2 samples over a window's borders: a gain step in
    the mix is smeared over one frame.  A cell depends on its own band, frames and signals only (bitwise).  No host
    synchronisation once the tables are resident; hipGraph-capturable then."""
    n_fft, hop, table = _band_args(stems, mix, n_windows, n_fft, hop, edges)
    return _band_moments(stems, mix, n_windows, n_fft, hop, table)


def solve_bands(moment_matrices, *, pool=0, ridge=0.0):
    """moments [B, W, S + 1, S + 1] -> (gains float64 [B, S, W], residual float64 [B, W], target float64 [B, W], status int32
    [B, W]), all on the device: ``solve`` on every band of its own (windows are pooled within a band), and ``target``, the
    mix's energy in the band and (pooled) window -- what ``band_residual_total`` weighs the residuals by."""
    pool, ridge = ops.gainfit_check_solve_args(pool, ridge)
    ops.gainfit_check_grouped_shape(tuple(moment_matrices.shape))
    return ops.gainfit_solve_grouped(moment_matrices, pool, ridge)


def fit_band_gains(stems, mix, n_windows, *, n_fft=4096, hop=None, edges, pool=0, ridge=0.0, align=None, align_weighting='phat'):
    """``solve_bands(band_moments(stems, mix, n_windows, ...), pool=pool, ridge=ridge)`` -> (gains [B, S, W], residual [B, W],
    target [B, W], status [B, W]): the gain every stem had in every band and window of the mix -- its EQ curve per stem.
    align: as ``fit_gains`` takes it; the stems are shifted by the estimated lags first, exactly as there."""
    n_fft, hop, table = _band_args(stems, mix, n_windows, n_fft, hop, edges)
    pool, ridge = ops.gainfit_check_solve_args(pool, ridge)
    if align is not None:
        ops.align_check_shapes(tuple(stems.shape), tuple(mix.shape), align, align_weighting)
        stems = ops.align_shift(stems, ops.align_estimate(stems, mix, align, align_weighting)[0])
    return ops.gainfit_solve_grouped(_band_moments(stems, mix, n_windows, n_fft, hop, table), pool, ridge)


def band_residual_total(residual, target, status):
    """residual, target, status [B, W] of ``solve_bands`` -> CUDA float64 [W]: the share of the mix's energy the band-wise
    gains leave unexplained in every window (a band that could not be fitted counts as unexplained, a silent band adds
    nothing; NaN where the mix is silent in every band) -- the counterpart of ``solve``'s broadband residual; the difference
    of the two in dB is what per-band gains explain beyond scalar gains."""
    return ops.gainfit_band_summary(residual, target, status)


def render_band_gains(stems, band_gains, *, n_fft=4096, hop=None, edges, fill=1.0, out=None):
    """The audio of per-band gains: stems as ``band_moments`` takes them; band_gains CUDA float64 [B, S, W], the layout
    ``fit_band_gains`` returns; edges the host table the gains were fitted on; hop defaults to n_fft / 2 and must not exceed it.
    -> CUDA float32 [channels, n]: every stem's STFT (frames and window those of the fit) scaled bin by bin with the gain of the
    bin's band and the frame's window, summed over the stems, inverted and overlap-added (include/dam_hip.h: dam_bandmix_render)
    in one fused pass -- no spectrum is written to memory.  fill: the gain of the bins outside every band and of the cells whose
    fitted gain is NaN (a silent or unfitted stem): a number, or a CUDA float64 [S], [S, 1] or [S, W] tensor such as
    ``fit_gains``' broadband gains; where that is NaN too the gain is 0.  Unit gains and unit fill give back the stems' sum;
    a sample at least n_fft / 2 inside its window does not depend on the other windows' gains.  NOT the inverse of the fit:
    band-wise constant gains are a filter the synthesis window truncates.  The workspace (the synthesised frames,
    4 * channels * frames * n_fft bytes) comes from torch's caching allocator, which keeps it per device and size.  No host
    synchronisation once the tables are resident; hipGraph-capturable then."""
    if not torch.is_tensor(band_gains):
        raise TypeError('render_band_gains: band_gains must be a tensor [bands, stems, windows]')
    if torch.is_tensor(fill):
        fill_shape = tuple(fill.shape)
    elif isinstance(fill, (int, float)) and not isinstance(fill, bool):
        fill_shape = ()
    else:
        raise TypeError('render_band_gains: fill must be a number or a tensor')
    S, n, ch, B, W, n_fft, hop = ops.bandmix_check_shapes(tuple(stems.shape), tuple(band_gains.shape), fill_shape, n_fft, hop)
    table = spectrum.check_edges(edges, n_fft)
    if table.size - 1 != B:
        raise ValueError('render_band_gains: %d bands of gains for a table of %d bands' % (B, table.size - 1))
    ops._lib.require_cuda(stems, band_gains, fill if torch.is_tensor(fill) else None, out)
    if torch.is_tensor(fill):
        if fill.dtype != torch.float64:
            raise TypeError('render_band_gains: a fill tensor must be float64')
        fill = fill.reshape(S, -1).expand(S, W)
    else:
        fill = torch.full((S, W), float(fill), dtype=torch.float64, device=stems.device)
    dev_edges = spectrum._device_edges(table, n_fft, stems.device)
    win, tw = features._get_tables(stems.device, n_fft)
    return ops.bandmix_render(stems, band_gains, fill, dev_edges, win, tw, n_fft, hop, out=out)


def residual_db(residual):
    """The residual of ``solve`` (torch tensor, numpy array or number) in dB: 10 log10, -inf at 0; the same kind of array
    comes back."""
    if torch.is_tensor(residual):
        return 10.0 * torch.log10(residual)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10.0 * np.log10(np.asarray(residual, dtype=np.float64))
