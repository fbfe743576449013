"""CPU: the numpy reference of the band spectrum (tests/_spectrum_ref.py) against known answers, and the product's
``band_edges`` against the reference's copy and the pinned third-octave tables -- so that the GPU tests compare the kernels
with something that has itself been checked."""
import math

import numpy as np
import pytest

import _spectrum_ref as ref

# (sr, n_fft) -> bands, first centre, last centre, first band, {centre: band}
TABLES = [
    (44100, 8192, 28, 31.25, 16000.0, (6, 7), {1000.0: (166, 209), 16000.0: (2648, 3337)}),
    (44100, 2048, 26, 1000.0 * 2.0 ** (-14 / 3.0), 16000.0, (2, 3), {}),
    (8000, 1024, 22, 31.25, 4000.0, (4, 5), {4000.0: (457, 513)}),
]


def both_band_edges():
    from deep_audio_mixer_amd import spectrum
    return [('product', spectrum.band_edges), ('reference', ref.band_edges)]


@pytest.mark.parametrize('sr,n_fft,n_bands,first,last,first_band,named', TABLES)
def test_band_edges_pinned_values(sr, n_fft, n_bands, first, last, first_band, named):
    for who, fn in both_band_edges():
        edges, centres = fn(sr, n_fft)
        assert edges.dtype == np.int32 and centres.dtype == np.float64, who
        assert len(centres) == n_bands and len(edges) == n_bands + 1, who
        assert abs(centres[0] - first) < 1e-9 and abs(centres[-1] - last) < 1e-9, who
        assert (edges[0], edges[1]) == first_band, who
        for centre, band in named.items():
            b = int(np.argmin(np.abs(centres - centre)))
            assert abs(centres[b] - centre) < 1e-9 and (edges[b], edges[b + 1]) == band, (who, centre)
    assert abs(TABLES[1][3] - 39.37) < 0.005


@pytest.mark.parametrize('fraction', [1, 3, 6])
def test_band_edges_ascend(fraction):
    for sr, n_fft in ((44100, 8192), (44100, 2048), (8000, 1024), (48000, 64), (22050, 16384)):
        got = [fn(sr, n_fft, fraction) for _, fn in both_band_edges()]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        edges, centres = got[0]
        assert len(edges) == len(centres) + 1 >= 2
        assert np.all(np.diff(edges) > 0) and edges[0] >= 0 and edges[-1] <= n_fft // 2 + 1
        # every centre lies in its band, up to the rounding of the edges to whole bins
        f_lo, f_hi = (edges[:-1] - 1) * sr / n_fft, edges[1:] * sr / n_fft
        assert np.all(centres >= f_lo) and np.all(centres <= f_hi)


@pytest.mark.parametrize('n_fft,hop,n', [(64, 23, 407), (256, 77, 1500)])
def test_parseval_single_band(n_fft, hop, n):
    rng = np.random.default_rng(n_fft)
    stems = (0.2 * rng.standard_normal((3, n, 2))).astype(np.float32)
    gains = rng.uniform(0.5, 1.5, (3, 5))
    xm = ref.mix_signal(stems, gains)
    P, beta = ref.band_power_signal(xm, n_fft, hop, [0, n_fft // 2 + 1])
    want = ref.parseval_power(xm, n_fft, hop)
    assert P.shape == (1,) and abs(P[0] - want) <= 1e-12 * want and 0.0 < beta[0] < 1e-4 * P[0]
    # ... and bands that tile the bins add up to it
    parts, _ = ref.band_power_signal(xm, n_fft, hop, [0, 1, 7, n_fft // 4, n_fft // 2, n_fft // 2 + 1])
    assert abs(parts.sum() - want) <= 1e-12 * want


def test_bin_centred_sine_known_power():
    n_fft, hop, n, k0, A = 256, 37, 2000, 19, 0.3
    x = A * np.sin(2.0 * np.pi * k0 * np.arange(n) / n_fft + 0.4)
    fr = ref.frames(x, n_fft, hop, exact=True)
    per_frame = ref.frame_band_power(fr, [k0 - 1, k0 + 2])[:, 0]
    t = np.arange(fr.shape[0])
    clean = (t * hop - n_fft // 2 >= 0) & (t * hop + n_fft // 2 <= n)
    assert clean.sum() >= 10 and not clean[0] and not clean[-1]
    want = 3.0 * A * A * n_fft * n_fft / 16.0
    assert np.all(np.abs(per_frame[clean] - want) <= 1e-12 * want)
    # the float32 definition (rounded signal, the float32 window table) stays within its rounding of the same answer
    P32 = ref.frame_band_power(ref.frames(x.astype(np.float32), n_fft, hop), [k0 - 1, k0 + 2])[:, 0]
    assert np.all(np.abs(P32[clean] - want) <= 1e-6 * want)


def test_mix_signal_gain_ramp_convention():
    n = 103
    stems = np.arange(2 * n * 2, dtype=np.float64).reshape(2, n, 2) / 64.0
    gains = np.array([[1.0, 2.0, 4.0], [0.5, 0.25, 0.125]])
    xm = ref.mix_signal(stems, gains)
    seg = n // 3
    for p in (0, seg - 1, seg, 2 * seg, 3 * seg, n - 1):               # 3 * seg = 102: the tail keeps the last gain
        gi = min(p // seg, 2)
        want = sum((stems[s, p, 0] + stems[s, p, 1]) * 0.5 * gains[s, gi] for s in range(2))
        assert xm[p] == np.float32(want)
    assert xm.dtype == np.float32 and np.array_equal(ref.mix_signal(stems), ref.mix_signal(stems, np.ones((2, 1))))


def test_balance_error_known_answers():
    rng = np.random.default_rng(5)
    n_fft, hop, n = 256, 128, 3000
    stems = (0.1 * rng.standard_normal((3, n, 2))).astype(np.float32)
    edges, _ = ref.band_edges(8000, n_fft)
    P, _ = ref.band_power(stems, None, n_fft, hop, edges)
    assert ref.balance_error(P, P) == (0.0, len(P))                     # identical spectra, every band kept
    half, _ = ref.band_power(stems * np.float32(0.5), None, n_fft, hop, edges)
    assert np.array_equal(half, P * 0.25)                               # a common gain scales every power exactly
    assert ref.balance_error(P, half) == (0.0, len(P))
    # another balance: a known shift of one band
    ref_p = np.array([1.0, 1.0, 2.0])
    err, kept = ref.balance_error(ref_p, np.array([1.0, 1.0, 1.0]))
    L = lambda p: 10.0 * np.log10(p / p.sum())
    assert kept == 3 and abs(err - np.abs(L(np.array([1.0, 1.0, 1.0])) - L(ref_p)).mean()) < 1e-13
    # a band under the gate in either spectrum is dropped and counted out
    low = np.array([1.0, 1.0, 0.5 * ref.GATE])
    err, kept = ref.balance_error(low, np.array([1.0, 2.0, 1.0]))
    assert kept == 2 and abs(err - 0.5 * (abs(L(np.array([1.0, 2.0, 1.0]))[0] - L(low)[0]) +
                                          abs(L(np.array([1.0, 2.0, 1.0]))[1] - L(low)[1]))) < 1e-13
    assert ref.balance_error(np.array([1.0, 2.0, 1.0]), low)[1] == 2
    assert ref.balance_error(np.array([1.0, 1.0, 3.0 * ref.GATE]), np.array([1.0, 1.0, 1.0]))[1] == 3
    # no band kept: NaN
    err, kept = ref.balance_error(np.array([1.0, 0.0]), np.array([0.0, 1.0]))
    assert kept == 0 and math.isnan(err)
    assert abs(10.0 * math.log10(ref.GATE) + 70.0) < 1e-12


def test_product_helpers_without_gpu():
    import torch
    from deep_audio_mixer_amd import spectrum
    P = np.array([[1.0, 3.0], [2.0, 2.0]])
    assert np.allclose(spectrum.relative_levels_db(P), ref.relative_levels_db(P[0])[None] * [[1], [0]] +
                       ref.relative_levels_db(P[1])[None] * [[0], [1]], atol=1e-13)
    assert np.allclose(spectrum.relative_levels_db(torch.from_numpy(P)).numpy(), spectrum.relative_levels_db(P), atol=1e-13)
    for bad in ([0, 0, 3], [3, 2], [-1, 4], [0, 40]):
        with pytest.raises(ValueError):
            spectrum.check_edges(np.array(bad), 64)
    with pytest.raises(TypeError):
        spectrum.check_edges(np.array([0.0, 1.0]), 64)
    assert spectrum.check_edges([0, 33], 64).dtype == np.int32
