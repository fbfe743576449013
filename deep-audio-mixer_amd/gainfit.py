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

from . import ops


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


def residual_db(residual):
    """The residual of ``solve`` (torch tensor, numpy array or number) in dB: 10 log10, -inf at 0; the same kind of array
    comes back."""
    if torch.is_tensor(residual):
        return 10.0 * torch.log10(residual)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10.0 * np.log10(np.asarray(residual, dtype=np.float64))
