"""GPU: the spectrogram-distance kernels (csrc/dam_specdist.hip) against the numpy float64 reference (tests/_specdist_ref.py).

Bounds.  Per cell |dS1| <= sum e and |dS2| <= sum (2 |d| e + e^2), e the per-bin level bound of the reference's docstring (the
FFT's 2e-6 of the frame's peak, 1e-5 dB for the float32 log2, one float32 ulp of a 100 dB level) -- figures the project held
before this file; tests/test_specdist_ref_cpu.py checks on the sweep's very inputs that the S2 bound is at most 1e-2 of the
value it guards.  The summary is held to 1e-12 relative against numpy on the device's own sums.  Everything else is bitwise.
Every test prints its largest error as a fraction of the bound before it asserts.  Largest |dS| / bound seen on one MI355X:
parity sweep 0.027 at n_fft 64 (23 cases), 0.036 at 256 (21 cases), 0.049 at 2048 (16 cases); n_fft 8192 0.021, 16384 0.014; the
common-gain bias 1e-4 of its bound; the summary bitwise equal to numpy on the device's sums."""
import numpy as np
import pytest
import torch

import _specdist_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import ops, spectrum
    return ops, spectrum


def upload(stems, planar=False):
    """[S, n, ch] numpy -> a CUDA tensor of that shape: interleaved storage, or planar [S, ch, n] storage transposed."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(stems.transpose(0, 2, 1))).cuda().transpose(1, 2)
    return torch.from_numpy(np.ascontiguousarray(stems)).cuda()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_case(spectrum, c):
    sums, count = spectrum.spectrogram_distance(upload(c['stems'], c['planar']), dev(c['gains']),
                                                upload(c['ref_stems'], c['ref_planar']), dev(c['ref_gains']), n_fft=c['n_fft'],
                                                hop=c['hop'], edges=c['edges'], n_windows=c['W'])
    return sums.cpu().numpy(), count.cpu().numpy()


def check_case(got, got_count, c):
    """-> the largest |dS1| / bound and |dS2| / bound of the case; every cell asserted."""
    sums, count, bound, d, Lc, Lr = ref.distance(c['stems'], c['gains'], c['ref_stems'], c['ref_gains'], c['n_fft'], c['hop'],
                                                 c['edges'], c['W'])
    assert got.shape == sums.shape and got.dtype == np.float64 and got_count.dtype == np.int64
    assert np.array_equal(got_count, count)
    bound = bound.copy()
    for r in c.get('zero_rows', ()):
        # an all-zero row: every device level must be floor_db EXACTLY, d = floor_db - L_ref, so the candidate's share of
        # the bound (log2 and rounding: the FFT term of a zero frame is 0) is taken away
        assert np.all(Lc[r] == -100.0)
        e_c = count * (ref.LOG2_DB + ref.ROUND_DB)
        bound[r, ..., 1] -= 2.0 * np.abs(sums[r, ..., 0]) * (ref.LOG2_DB + ref.ROUND_DB)        # sum 2 |d| e_c, d of one sign
        bound[r, ..., 0] -= e_c
        assert np.all(d[r] <= 0.0) and np.all(bound[r] > 0.0)
    ratio = np.abs(got - sums) / bound
    assert np.all(ratio <= 1.0), (c['n_fft'], c['hop'], c['n'], float(ratio.max()))
    return float(ratio[..., 0].max()), float(ratio[..., 1].max())


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_parity_sweep(env, n_fft):
    ops, spectrum = env
    cases = ref.sweep_cases(n_fft)
    worst = [0.0, 0.0]
    for c in cases:
        got, count = run_case(spectrum, c)
        r1, r2 = check_case(got, count, c)
        worst = [max(worst[0], r1), max(worst[1], r2)]
    print('n_fft %d: %d cases, largest |dS1| / bound = %.4f, |dS2| / bound = %.4f' % (n_fft, len(cases), worst[0], worst[1]))
    assert len(cases) >= 12


@pytest.mark.parametrize('n_fft', [8192, 16384])
def test_large_windows(env, n_fft):
    """The > 64 KB LDS path (PER 16 / 32): extended third-octave bands at 44.1 kHz, stereo planar stems, two rows, W = 2."""
    ops, spectrum = env
    rng = np.random.default_rng(n_fft)
    n = 3 * n_fft + 17
    stems, gains, ref_stems, ref_gains = ref.noise_case(rng, 4, 2, n, 2, np.float32, 2, 3, None)
    edges = spectrum.extend_edges(spectrum.band_edges(44100, n_fft)[0], n_fft)[0]
    c = dict(n_fft=n_fft, hop=n_fft // 2, n=n, W=2, edges=edges, planar=True, ref_planar=False, stems=stems, gains=gains,
             ref_stems=ref_stems, ref_gains=ref_gains)
    got, count = run_case(spectrum, c)
    r1, r2 = check_case(got, count, c)
    assert count.sum() == (1 + n // (n_fft // 2)) * (n_fft // 2 + 1)
    print('n_fft %d, %d bands, T = %d: largest |dS1| / bound = %.4f, |dS2| / bound = %.4f'
          % (n_fft, len(edges) - 1, 1 + n // (n_fft // 2), r1, r2))


def bitwise_inputs(seed=5, n=256 * 9 + 5, S=3, S_ref=2):
    rng = np.random.default_rng(seed)
    stems, gains, ref_stems, ref_gains = ref.noise_case(rng, S, S_ref, n, 2, np.float32, 5, 7, 3)
    return stems, gains, ref_stems, ref_gains


def test_bitwise_properties(env):
    ops, spectrum = env
    n_fft, hop, W = 256, 77, 3
    stems, gains, ref_stems, ref_gains = bitwise_inputs()
    n = stems.shape[1]
    edges = np.array([2, 3, 7, 8, 20, 125])
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    kw = dict(n_fft=n_fft, hop=hop, n_windows=W)
    full, count = spectrum.spectrogram_distance(x, g, y, h, edges=edges, **kw)
    again, _ = spectrum.spectrogram_distance(x, g, y, h, edges=edges, **kw)
    assert torch.equal(full, again)                                                     # two runs
    for r in range(5):                                                                  # a row alone / inside R = 5
        alone, _ = spectrum.spectrogram_distance(x, g[r:r + 1].contiguous(), y, h, edges=edges, **kw)
        assert torch.equal(alone[0], full[r]), r
    for b in range(len(edges) - 1):                                                     # a band alone / inside a table
        alone, c1 = spectrum.spectrogram_distance(x, g, y, h, edges=edges[b:b + 2], **kw)
        assert torch.equal(alone[:, 0], full[:, b]) and torch.equal(c1[0], count[b]), b
    planar, _ = spectrum.spectrogram_distance(upload(stems, True), g, upload(ref_stems, True), h, edges=edges, **kw)
    assert torch.equal(planar, full)                                                    # interleaved / planar
    # window 1 against changes of every sample further than n_fft/2 outside its frames' centres
    first = ops.gainfit_band_frame_windows(n, W, hop)
    lo, hi = first[1] * hop - n_fft // 2, (first[2] - 1) * hop + n_fft // 2
    assert 0 < lo < hi < n
    rng = np.random.default_rng(6)
    s2, r2 = stems.copy(), ref_stems.copy()
    for a in (s2, r2):
        a[:, :lo] = 0.1 * rng.standard_normal(a[:, :lo].shape)
        a[:, hi:] = 0.1 * rng.standard_normal(a[:, hi:].shape)
    moved, _ = spectrum.spectrogram_distance(upload(s2), g, upload(r2), h, edges=edges, **kw)
    assert torch.equal(moved[:, :, 1], full[:, :, 1])
    assert not torch.equal(moved[:, :, 0], full[:, :, 0]) and not torch.equal(moved[:, :, 2], full[:, :, 2])
    # an all-zero candidate against the reference is the reference against silence, negated: the levels of a zero frame
    # are floor_db exactly on either side
    zero = torch.zeros(1, 3, 1, dtype=torch.float64, device='cuda')
    a, _ = spectrum.spectrogram_distance(x, zero, y, h, edges=edges, **kw)
    b, _ = spectrum.spectrogram_distance(y, h, x, zero[0], edges=edges, **kw)
    assert torch.equal(a[..., 0], -b[..., 0]) and torch.equal(a[..., 1], b[..., 1])
    both, _ = spectrum.spectrogram_distance(x, zero, y, torch.zeros(2, dtype=torch.float64, device='cuda'), edges=edges, **kw)
    assert torch.all(both == 0.0)
    print('bitwise: two runs, row alone, band alone, planar, window against far samples, zero frames: all equal')


def test_common_gain_is_a_bias_on_the_device(env):
    ops, spectrum = env
    n_fft, hop, W, c = 256, 128, 3, 0.5
    stems = bitwise_inputs(seed=8)[0]
    edges = spectrum.extend_edges(spectrum.band_edges(44100, n_fft)[0], n_fft)[0]
    gains = np.full((1, 3, 1), c)
    sums, count = spectrum.spectrogram_distance(upload(stems), dev(gains), upload(stems), None, n_fft=n_fft, hop=hop, edges=edges,
                                                n_windows=W)
    fig = spectrum.distance_summary(sums, count)
    _, rcount, bound, d, Lc, Lr = ref.distance(stems, gains, stems, None, n_fft, hop, edges, W)
    assert Lr.min() > -99.0 and Lc.min() > -99.0
    want, tol = 20.0 * np.log10(c), bound[0, ..., 0].sum() / rcount.sum()
    got = fig.bias.item()
    print('common gain %.3g on the device: bias %.9f dB, want %.9f, |difference| / bound = %.4f; centred rms %.3g dB'
          % (c, got, want, abs(got - want) / tol, fig.rms_centred.item()))
    assert abs(got - want) <= tol
    band_tol = bound[0, ..., 0].sum(axis=1) / rcount.sum(axis=1)
    assert np.all(np.abs(fig.band_bias[0].cpu().numpy() - want) <= band_tol)


def test_summary_against_numpy(env):
    ops, spectrum = env
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=9)
    edges = ref.edge_tables(256)[2]
    sums, count = spectrum.spectrogram_distance(upload(stems), dev(gains), upload(ref_stems), dev(ref_gains), n_fft=256, hop=77,
                                                edges=edges, n_windows=5)
    fig = spectrum.distance_summary(sums, count)
    B, W = count.shape
    want = ref.summary(sums.cpu().numpy(), count.cpu().numpy())
    got = ops.specdist_summary(sums, count).cpu().numpy()
    assert got.shape == (5, 1 + B + W, 3) and np.all(np.isfinite(got))
    # mse and bias: quotients of sums added in the same order -> 1e-12 relative; the centred rms is the root of a difference
    # of two such numbers, so it is held through its square, relative to the mse it was taken from
    rel = np.abs(got[..., :2] - want[..., :2]) / np.abs(want[..., :2])
    rel_var = np.abs(got[..., 2] ** 2 - want[..., 2] ** 2) / want[..., 0]
    print('summary against numpy: mse / bias relative %.3g, centred variance relative to the mse %.3g' % (rel.max(), rel_var.max()))
    assert rel.max() <= 1e-12 and rel_var.max() <= 1e-12
    assert np.array_equal(fig.mse.cpu().numpy(), got[:, 0, 0]) and np.array_equal(fig.band_bias.cpu().numpy(), got[:, 1:1 + B, 1])
    assert np.array_equal(fig.window_rms.cpu().numpy(), got[:, 1 + B:, 2]) and tuple(fig.window_mse.shape) == (5, W)
    # zero counts: NaN in the same places as numpy
    holes = count.clone()
    holes[1, :] = 0
    holes[:, 2] = 0
    got = ops.specdist_summary(sums, holes).cpu().numpy()
    want = ref.summary(sums.cpu().numpy(), holes.cpu().numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[:, 2]).all() and np.isnan(got[:, 1 + B + 2]).all()
    ok = ~np.isnan(want)
    assert np.abs(got[ok][..., None] - want[ok][..., None]).max() <= 1e-9 and np.isfinite(got[:, 0]).all()
    assert np.isnan(ops.specdist_summary(sums, torch.zeros_like(count)).cpu().numpy()).all()


def test_graph_capture_and_replay(env):
    ops, spectrum = env
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=10)
    edges = ref.edge_tables(256)[2]
    kw = dict(n_fft=256, hop=77, edges=edges, n_windows=3)
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        spectrum.distance_summary(*spectrum.spectrogram_distance(x, g, y, h, **kw))     # the tables become resident
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sums, count = spectrum.spectrogram_distance(x, g, y, h, **kw)
        fig = spectrum.distance_summary(sums, count)
    x.mul_(0.5)
    y.copy_(y.flip(0))
    g.copy_(g.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    e_sums, e_count = spectrum.spectrogram_distance(x.clone(), g.clone(), y.clone(), h, **kw)
    e_fig = spectrum.distance_summary(e_sums, e_count)
    assert torch.equal(sums, e_sums) and torch.equal(count, e_count)
    for a, b in zip(fig, e_fig):
        assert torch.equal(a, b)
    first, _ = spectrum.spectrogram_distance(upload(stems), dev(gains), upload(ref_stems), dev(ref_gains), **kw)
    assert not torch.equal(first, sums)
    print('graph: captured sums + summary, replayed on rewritten stems, bitwise the eager result')


def test_argument_errors(env, dam_lib):
    ops, spectrum = env
    from deep_audio_mixer_amd import features
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=12)
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    n = x.shape[1]
    good = dict(n_fft=256, hop=77, edges=np.array([0, 5, 129]), n_windows=3)
    spectrum.spectrogram_distance(x, g, y, h, **good)
    for exc, args, change in [
            (ValueError, (x, g, y[:, :-1], h), {}), (ValueError, (x, g, y, h), dict(n_fft=100)),
            (ValueError, (x, g, y, h), dict(hop=0)), (ValueError, (x, g, y, h), dict(n_windows=0)),
            (ValueError, (x, g, y, h), dict(n_windows=n + 1)), (ValueError, (x, g, y, h), dict(n_windows=31, hop=128)),
            (ValueError, (x, g, y, h), dict(amin=0.0)), (ValueError, (x, g, y, h), dict(edges=np.array([0, 5, 130]))),
            (ValueError, (x, g, y, h), dict(edges=np.array([5, 5, 9]))), (ValueError, (x, g, y, h), dict(edges=np.arange(66))),
            (ValueError, (x, g[:, :2], y, h), {}), (ValueError, (x, g, y, h[:1]), {}), (ValueError, (x[0], g, y, h), {}),
            (TypeError, (x, g.float(), y, h), {}), (TypeError, (x.half(), g, y, h), {}), (TypeError, (x, g, y, h), dict(n_fft=256.0)),
            (RuntimeError, (x.cpu(), g, y, h), {}), (RuntimeError, (x, g.cpu(), y, h), {}), (RuntimeError, (x, g, y.cpu(), h), {}),
            (ValueError, (x[:, :128], None, y[:, :128], None), dict(n_windows=1))]:
        with pytest.raises(exc):
            spectrum.spectrogram_distance(*args, **dict(good, **change))
    # the raw C entry: DAM_ERR_BAD_ARG before any launch, nothing written
    win, tw = features._get_tables(x.device, 256)
    edges = torch.tensor([0, 5, 129], dtype=torch.int32, device='cuda')
    sums = torch.full((5, 2, 3, 2), -7.0, dtype=torch.float64, device='cuda')
    count = torch.full((2, 3), -7, dtype=torch.int64, device='cuda')
    ws = torch.full((5 * (1 + n // 77) * 2 * 2,), -7.0, dtype=torch.float64, device='cuda')
    P = lambda t: None if t is None else t.data_ptr()
    base = dict(x=P(x), xk=0, R=5, S=3, ch=2, n=n, ss=x.stride(0), ps=x.stride(1), cs=x.stride(2), g=P(g), ng=7, y=P(y), yk=0,
                Sr=y.shape[0], chr=y.shape[2], rss=y.stride(0), rps=y.stride(1), rcs=y.stride(2), h=P(h), nh=3, win=P(win), tw=P(tw), n_fft=256, hop=77,
                amin=1e-5, edges=P(edges), B=2, W=3, sums=P(sums), count=P(count), ws=P(ws), stream=None)
    call = lambda **kw: dam_lib.dam_specdist_sums(*dict(base, **kw).values())
    assert dam_lib.dam_specdist_workspace_bytes(5, n, 256, 77, 2, 3) == ws.numel() * 8
    bad = [dict(x=None), dict(y=None), dict(win=None), dict(tw=None), dict(edges=None), dict(sums=None), dict(count=None),
           dict(ws=None), dict(R=0), dict(R=65536), dict(S=0), dict(Sr=0), dict(ch=3), dict(chr=0), dict(n_fft=100), dict(n_fft=32),
           dict(n_fft=32768), dict(hop=0), dict(n=128), dict(ng=0), dict(ng=n + 1), dict(nh=0), dict(amin=0.0), dict(amin=-1.0),
           dict(amin=float('nan')), dict(B=0), dict(B=65), dict(W=0), dict(W=n + 1), dict(W=31, hop=128)]
    for change in bad:
        assert call(**change) == -1, change                                  # DAM_ERR_BAD_ARG
        geo = dict(base, **change)
        if any(k in change for k in ('R', 'n', 'n_fft', 'hop', 'B', 'W')):
            assert dam_lib.dam_specdist_workspace_bytes(geo['R'], geo['n'], geo['n_fft'], geo['hop'], geo['B'], geo['W']) == 0
    assert dam_lib.dam_specdist_summary(None, P(count), 5, 2, 3, P(sums), None) == -1
    assert dam_lib.dam_specdist_summary(P(sums), P(count), 5, 65, 3, P(sums), None) == -1
    assert dam_lib.dam_specdist_summary(P(sums), P(count), 0, 2, 3, P(sums), None) == -1
    torch.cuda.synchronize()
    assert torch.all(sums == -7.0) and torch.all(count == -7) and torch.all(ws == -7.0)
    assert call() == 0                                                       # the same arguments unchanged: accepted
    torch.cuda.synchronize()
    want, want_count = spectrum.spectrogram_distance(x, g, y, h, **good)
    assert torch.equal(sums, want) and torch.equal(count, want_count)
