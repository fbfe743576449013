"""The time offset of stems against a mix, measured on the device, and the sample shift that removes it (include/dam_hip.h:
dam_align_estimate / dam_align_shift state the definitions; csrc/dam_align.hip holds the kernels).

The gain fit (gainfit.py) compares sample by sample, so it can only be trusted when the mix is aligned with the stems.  A
mix that is the float64 sum of the same arrays is; a dataset's own mix file, a bounce with plug-in delay or a file trimmed
by hand is not, and an offset of a handful of samples already rotates the phase of everything above a few kHz: the fit
then returns shrunken gains and a residual that blames the mixer.  ``estimate_lag`` finds the offset of every stem within
+-max_lag samples as the peak of its cross-correlation with the mix -- plain, or PHAT-weighted (every bin of the
cross-spectrum divided by its magnitude plus a smooth floor), which turns the broad, bass-dominated hump real music gives
into a sharp peak -- and ``shift_tracks`` moves the stems by it, reading the lags from device memory: estimate -> shift ->
fit is one sequence without a host round trip (``gainfit.fit_gains(..., align=max_lag)``).

PHAT needs a stem with some bandwidth: a near-sinusoidal stem (a sustained bass note, a test tone) has one live bin, the
whitening then weighs the leakage of the unwindowed frames as much as the tone, and the peak moves to the ends of the lag
range (tests/test_align_gainfit_gpu.py's 80 Hz and 400 + 800 Hz stems: +-max_lag in the float64 reference as well).  The
plain weighting finds those: a stem that is a component of the mix peaks at its own offset whatever its spectrum, which
is why the evaluator and the track loaders use it.

A positive lag means the mix is late; shifting a stem by +lag makes it as late as the mix is.  Offsets beyond
``dam_align_max_lag()`` samples, drift / varispeed and sub-sample shifting are not covered (``frac`` is reported, not
applied).

Importable without a GPU (``lag_from_ms`` and the argument checks are host arithmetic); the measuring functions need CUDA
tensors and raise otherwise -- there is no CPU fallback.
"""
import math
import numbers

import torch

from . import ops

WEIGHTINGS = tuple(sorted(ops.ALIGN_WEIGHTINGS))


def lag_from_ms(ms, sr):
    """A time in milliseconds as a whole number of samples at ``sr`` Hz, rounded up and at least 1: a ``max_lag``."""
    if not isinstance(ms, numbers.Real) or not isinstance(sr, numbers.Real) or isinstance(ms, bool) or isinstance(sr, bool):
        raise TypeError('lag_from_ms: numbers expected')
    if not ms > 0 or not sr > 0:
        raise ValueError('lag_from_ms: a positive time and rate expected, got %r ms at %r Hz' % (ms, sr))
    return max(1, int(math.ceil(float(ms) * float(sr) / 1000.0)))


def cross_correlation(stems, mix, max_lag, *, weighting='plain'):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides (planar [S, channels, n] storage is passed as
    ``pcm.transpose(1, 2)``, no copy), 1 <= S <= 8, 1 or 2 channels; mix: CUDA float32 / float64 [samples, channels] with any
    strides, its dtype independent of the stems' -> CUDA float64 [S, 2 max_lag + 1]: c[s, l + max_lag] = sum_p a_s[p]
    y[p + l] of the mono signals (``weighting='plain'``) or its PHAT-weighted form.  A row does not depend on the other
    stems (bitwise).  No host synchronisation."""
    ops.align_check_shapes(tuple(stems.shape), tuple(mix.shape), max_lag, weighting)
    return ops.align_estimate(stems, mix, max_lag, weighting, want_curve=True)[5]


def estimate_lag(stems, mix, max_lag, *, weighting='phat'):
    """-> (lag int32 [S], frac float64 [S], peak float64 [S], sign int32 [S], status int32 [S]) on the device.  lag: where
    |c| is largest within +-max_lag (ties: the smallest |lag|, then the negative one); frac: the parabola's sub-sample
    correction in [-0.5, 0.5], 0 at the ends of the range; peak: |c[lag]| / sqrt(E_stem E_mix) for 'plain' (1 for a pure
    delay), |c[lag]| for 'phat'; sign: -1 for inverted polarity; status: 1, or 0 for a silent stem or mix (lag 0, frac 0,
    sign 0, peak NaN).  Nothing comes to the host; hipGraph-capturable after a first call for this max_lag."""
    ops.align_check_shapes(tuple(stems.shape), tuple(mix.shape), max_lag, weighting)
    return ops.align_estimate(stems, mix, max_lag, weighting)[:5]


def shift_tracks(stems, lag):
    """out[s, p] = stems[s, p - lag[s]], zeros shifted in.  lag: a CUDA int32 [S] tensor (what ``estimate_lag`` returned:
    read on the device, no synchronisation) or one Python int for every stem.  -> a new tensor of the stems' dtype."""
    if isinstance(lag, numbers.Integral) and not isinstance(lag, bool):
        if not -2 ** 31 < lag < 2 ** 31:
            raise ValueError('shift_tracks: the lag must fit 32 bits')
        ops._lib.require_cuda(stems)
        lag = torch.full((stems.shape[0],), int(lag), dtype=torch.int32, device=stems.device)
    elif not torch.is_tensor(lag):
        raise TypeError('shift_tracks: lag must be an int32 tensor [S] or an integer')
    return ops.align_shift(stems, lag)
