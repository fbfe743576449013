"""GPU: momentary / short-term loudness, loudness range and the per-window profile error (dam_loudness_window_power,
dam_loudness_curve_stats, dam_loudness_profile_error; loudness.Meter.*_batch) against the numpy definition
(tests/_dynamics_ref.py).

Bounds.  Window power: 1e-14 relative -- a sum of at most 150 non-negative terms in the order the definition states;
curves from given energies 1e-12 LU.  Curve statistics: the count exactly, percentiles / LRA / maximum 1e-12 LU (the order
statistic is selected among the exact input doubles, what is left is one log10), the relative gate 1e-9 LU; asserted on
the reference first: no value within relative 1e-9 of either gate.  End to end: hop energies at the batched meter's bound
(1e-9 relative + 1e-18, tests/test_loudness_batch_gpu.py), curves 1e-8 LU where the reference reads -100 LUFS or more, -inf
exactly where the reference has it, LRA 2e-8 LU.  Profile error 1e-12 LU.
Largest observed errors: NOT YET RECORDED -- no GPU could be obtained while this file was written, so these tests have not
run on an MI355X.  What exists is a host rehearsal: the kernel source compiled for the CPU (threads in place of lanes, under
the address and undefined-behaviour sanitizers) gave, on the inputs of the three kernel-alone tests below, the count exactly,
percentiles / LRA / maximum / window power / profile error bitwise and the relative gate within 1.4e-14 LU.
Every test prints its largest observed error before asserting."""
import numpy as np
import pytest
import torch

import _dynamics_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def loudness(dam_lib):
    from deep_audio_mixer_amd import loudness
    return loudness


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_view(x, planar):
    """x numpy [N, n, ch] -> CUDA tensor of that shape, stored interleaved or as a transposed view of planar [N, ch, n]."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
    return cuda(x)


def diff(got, want):
    """Largest |got - want| over the entries where both are finite; NaN and +-inf must sit in the same places."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)]), (got, want)
    assert np.isfinite(got[finite]).all()
    return float(np.abs(got[finite] - want[finite]).max()) if finite.any() else 0.0


def bits(t):
    return t.contiguous().view(torch.int64)


# ---- the window kernel alone
@pytest.mark.parametrize('H,w', [(4, 4), (5, 4), (30, 30), (31, 30), (33, 30), (285, 30), (286, 30), (287, 30)])
def test_window_power(loudness, H, w):
    worst_p = worst_l = 0.0
    for ch in (1, 2, 5):
        for N in (1, 3):
            rng = np.random.default_rng(H * 100 + ch * 10 + N)
            e = rng.uniform(0.1, 1.0, (N, ch, H)) * 10.0 ** rng.uniform(-9.0, 0.0, (N, ch, H))
            e[N - 1, :, :H // 2] = 0.0                                     # leading silence: zero windows where it is w hops long
            if N == 3:
                e[1] = 0.0                                                 # a silent track
            power, lufs = loudness.window_loudness_device(cuda(e), w)
            assert tuple(power.shape) == tuple(lufs.shape) == (N, H - w + 1)
            only_power, none = loudness.window_loudness_device(cuda(e), w, want_lufs=False)
            assert none is None and torch.equal(only_power, power)
            power, lufs = power.cpu().numpy(), lufs.cpu().numpy()
            for t in range(N):
                want = ref.window_power(e[t], w)
                assert np.array_equal(power[t] == 0.0, want == 0.0)
                nz = want > 0.0
                if nz.any():
                    worst_p = max(worst_p, float(np.max(np.abs(power[t][nz] - want[nz]) / want[nz])))
                worst_l = max(worst_l, diff(lufs[t], ref.lufs(want)))
            if N == 3:
                assert (lufs[1] == -np.inf).all() and (power[1] == 0.0).all()
    print('H = %d, w = %d: power max rel err %.3g (bound 1e-14), lufs max err %.3g LU (bound 1e-12)' % (H, w, worst_p, worst_l))
    assert worst_p <= 1e-14 and worst_l <= 1e-12


# ---- the statistics kernel alone
def curves(W):
    """Named power curves of W values."""
    rng = np.random.default_rng(W)
    levels = np.array([3e-7, 2e-5, 2.5e-5, 1e-3, 4e-3])
    c = {
        'random': 10.0 ** rng.uniform(-9.0, -1.0, W),                      # under the absolute gate, under the relative, kept
        'equal': np.full(W, 1.25e-3),
        'duplicates': levels[rng.integers(0, len(levels), W)],             # long runs of equal values across both percentiles
        'zeros': np.where(rng.uniform(size=W) < 0.4, 0.0, 10.0 ** rng.uniform(-5.0, -2.0, W)),
        'under': ref.P_ABS * rng.uniform(0.1, 0.5, W),                      # nothing passes the absolute gate
        'silent': np.zeros(W),
        'one': np.concatenate([[1.0], np.full(W - 1, 2.0 * ref.P_ABS)]),    # the relative gate leaves the first value alone
    }
    rng.shuffle(c['one'])
    return c


def check_stats(got, p):
    """-> (largest error of LRA / percentiles / maximum, error of the relative gate); the count is compared exactly."""
    assert ref.gate_margin(p) > 1e-9
    want = ref.curve_stats(p)
    assert got[4] == want[4], (got, want)
    return diff(got[[0, 1, 2, 5]], want[[0, 1, 2, 5]]), diff(got[3:4], want[3:4])


@pytest.mark.parametrize('W', [1, 2, 5, 6, 10, 11, 255, 256, 257, 3000, 40000])
def test_curve_stats(loudness, W):
    c = curves(W)
    names = list(c)
    batch = loudness.curve_stats_device(cuda(np.stack([c[k] for k in names])))
    assert tuple(batch.shape) == (len(names), 6)
    worst, worst_gate = 0.0, 0.0
    for i, k in enumerate(names):
        alone = loudness.curve_stats_device(cuda(c[k][None]))
        assert torch.equal(bits(alone[0]), bits(batch[i])), k              # bitwise whatever else is in the batch
        a, b = check_stats(alone[0].cpu().numpy(), c[k])
        worst, worst_gate = max(worst, a), max(worst_gate, b)
    got = {k: batch[i].cpu().numpy() for i, k in enumerate(names)}
    print('W = %d: kept %s; max err %.3g LU (bound 1e-12), relative gate %.3g LU (bound 1e-9)'
          % (W, {k: int(v[4]) for k, v in got.items()}, worst, worst_gate))
    assert worst <= 1e-12 and worst_gate <= 1e-9
    assert got['equal'][0] == 0.0 and got['equal'][4] == W
    assert got['under'][4] == 0 and got['under'][0] == 0.0 and np.isnan(got['under'][3]) and np.isfinite(got['under'][5])
    assert got['silent'][4] == 0 and got['silent'][5] == -np.inf
    assert got['one'][4] == 1 and got['one'][0] == 0.0 and got['one'][1] == got['one'][2] == got['one'][5]
    if W >= 255:
        assert 0 < got['random'][4] < W and got['random'][0] > 10.0 and got['duplicates'][0] > 0.0
    three = loudness.curve_stats_device(cuda(np.stack([c['under'], c['random'], c['duplicates']])))
    assert torch.equal(bits(three), bits(batch[[names.index('under'), names.index('random'), names.index('duplicates')]]))


# ---- end to end
def check_tracks(loudness, x, rate, planar=False, gains=None, lra_within=None):
    """x numpy [N, n, ch]: every reading of Meter.loudness_dynamics_batch and hop_energies_batch against the definition.
    Returns the largest errors (hop energies in units of their bound, curves, LRA and the other scalars)."""
    meter = loudness.Meter(rate)
    xd = device_view(x, planar)
    gd = None if gains is None else cuda(np.asarray(gains, dtype=np.float64))
    e = meter.hop_energies_batch(xd, gains=gd).cpu().numpy()
    d = {k: v.cpu().numpy() for k, v in meter.loudness_dynamics_batch(xd, gains=gd).items()}
    assert set(d) == {'momentary', 'short_term', 'momentary_max', 'short_term_max', 'lra', 'lra_low', 'lra_high'}
    worst = np.zeros(3)
    for t in range(x.shape[0]):
        want = ref.dynamics(x[t], rate, None if gains is None else gains[t])
        assert e[t].shape == want['hop_energies'].shape
        worst[0] = max(worst[0], float(np.max(np.abs(e[t] - want['hop_energies']) / (1e-9 * want['hop_energies'] + 1e-18))))
        for key in ('momentary', 'short_term'):
            assert np.array_equal(d[key][t] == -np.inf, want[key] == -np.inf)
            loud = want[key] >= -100.0
            if loud.any():
                worst[1] = max(worst[1], diff(d[key][t][loud], want[key][loud]))
        assert ref.gate_margin(want['short_term_power']) > 1e-9
        for key in ('lra', 'lra_low', 'lra_high', 'momentary_max', 'short_term_max'):
            worst[2] = max(worst[2], diff(d[key][t], want[key]))
        if lra_within is not None:
            assert abs(d['lra'][t] - lra_within[0]) <= lra_within[1]
    return worst, d


def assert_bounds(label, worst):
    print('%s: hop energies %.3g of their bound (1e-9 rel + 1e-18), curves %.3g LU (bound 1e-8), LRA / percentiles / maxima '
          '%.3g LU (bound 2e-8)' % (label, worst[0], worst[1], worst[2]))
    assert worst[0] <= 1.0 and worst[1] <= 1e-8 and worst[2] <= 2e-8


@pytest.mark.parametrize('case', range(4))
def test_tech3342(loudness, case):
    levels, want = ref.TECH3342[case]
    x = ref.tech3342_signal(levels)[None]
    worst, d = check_tracks(loudness, x, 44100, lra_within=(want, 1.0))
    print('Tech 3342 signal %d: LRA %.9f LU (required %g +- 1)' % (case + 1, d['lra'][0], want))
    assert_bounds('Tech 3342 signal %d' % (case + 1), worst)
    assert abs(loudness.loudness_range(x[0], 44100) - d['lra'][0]) == 0.0
    assert loudness.Meter(44100).loudness_range_batch(cuda(x))[0].item() == d['lra'][0]


def burst(rate, ch, dtype, seed, tracks=2):
    """7 s of noise decaying by 36 dB, n not a multiple of the hop; track 1 starts with 1.5 s of digital silence."""
    n = 7 * rate + 123
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal((tracks, n, ch)) * np.exp(-np.arange(n) / (1.2 * rate))[None, :, None]
    x[1:, :int(1.5 * rate)] = 0.0
    return x.astype(dtype)


LAYOUTS = [(1, np.float32, False), (2, np.float64, True), (5, np.float32, True), (2, np.float32, False), (5, np.float64, False)]


@pytest.mark.parametrize('rate', [48000, 22050])
def test_bursts_layouts_and_dtypes(loudness, rate):
    assert (7 * rate + 123) % ref.hop_length(rate)
    total = np.zeros(3)
    for ch, dtype, planar in LAYOUTS:
        worst, d = check_tracks(loudness, burst(rate, ch, dtype, rate + ch), rate, planar)
        assert (d['momentary'][1][:11] == -np.inf).all() and np.isfinite(d['momentary'][0]).all()
        assert (d['lra'] > 5.0).all()
        total = np.maximum(total, worst)
    assert_bounds('bursts at %d Hz' % rate, total)


@pytest.mark.parametrize('n_gains', [1, 7])
def test_gains_at_load(loudness, n_gains):
    rate = 22050
    x = burst(rate, 2, np.float32, 11 + n_gains)
    assert n_gains == 1 or x.shape[1] % n_gains
    gains = np.random.default_rng(n_gains).uniform(0.2, 3.0, (2, n_gains))
    worst, d = check_tracks(loudness, x, rate, True, gains)
    assert_bounds('%d gains' % n_gains, worst)
    plain = loudness.Meter(rate).short_term_loudness_batch(cuda(x)).cpu().numpy()
    assert np.abs(plain[0] - d['short_term'][0]).max() > 1.0                # the gains were applied


def test_exactly_thirty_hops_and_errors(loudness):
    rate = 22050
    h = ref.hop_length(rate)
    meter = loudness.Meter(rate, block_size=0.2)                            # the windows stay R128's
    x = burst(rate, 2, np.float32, 3)[:, :30 * h]
    worst, d = check_tracks(loudness, x, rate)
    assert_bounds('30 hops', worst)
    assert d['short_term'].shape == (2, 1) and d['momentary'].shape == (2, 27) and (d['lra'] == 0.0).all()
    xd = cuda(x)
    assert torch.equal(meter.short_term_loudness_batch(xd), cuda(d['short_term']))
    assert torch.equal(meter.momentary_loudness_batch(xd), cuda(d['momentary']))
    assert tuple(meter.hop_energies_batch(xd[:, :30 * h - 1]).shape) == (2, 2, 29)
    assert tuple(meter.momentary_loudness_batch(xd[:, :30 * h - 1]).shape) == (2, 26)
    for call in (meter.short_term_loudness_batch, meter.loudness_range_batch, meter.loudness_dynamics_batch):
        with pytest.raises(ValueError, match='30 hops'):
            call(xd[:, :30 * h - 1])
    with pytest.raises(ValueError, match='4 hops'):
        meter.momentary_loudness_batch(xd[:, :4 * h - 1])
    assert tuple(meter.momentary_loudness_batch(xd[:, :4 * h]).shape) == (2, 1)
    with pytest.raises(ValueError, match='five channels'):
        meter.short_term_loudness_batch(torch.zeros((1, 30 * h, 6), device='cuda'))
    with pytest.raises(ValueError, match='floating point'):
        meter.short_term_loudness_batch(torch.zeros((1, 30 * h, 2), dtype=torch.int16, device='cuda'))
    with pytest.raises(ValueError, match='CUDA'):
        meter.short_term_loudness_batch(torch.zeros((1, 30 * h, 2)))
    with pytest.raises(ValueError):
        meter.short_term_loudness_batch(torch.zeros((30 * h, 2), device='cuda'))
    with pytest.raises(ValueError):
        loudness.curve_stats_device(torch.zeros((2, 0), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError):
        loudness.profile_error_device(torch.zeros((4, 5), dtype=torch.float64, device='cuda'),
                                      torch.zeros((1, 4, 6), dtype=torch.float64, device='cuda'))


def test_capture_and_replay(loudness):
    """All readings inside one torch.cuda.graph on one stream: capturing proves that nothing synchronises or allocates
    outside the pool; a replay after new data went into the input buffer equals the eager call on that data, bitwise."""
    rate = 22050
    meter = loudness.Meter(rate)
    contents = [cuda(burst(rate, 2, np.float32, seed)) for seed in (20, 21, 22)]
    buf = contents[0].clone()
    gains = cuda(np.random.default_rng(23).uniform(0.3, 1.7, (2, 3)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        meter.loudness_dynamics_batch(buf, gains=gains)                     # (also fills the hop-bounds cache)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = meter.loudness_dynamics_batch(buf, gains=gains)
    for c in contents[1:]:
        buf.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        eager = meter.loudness_dynamics_batch(c, gains=gains.clone())
        for key in eager:
            assert torch.equal(bits(out[key]), bits(eager[key])), key
    assert not torch.equal(out['lra'], meter.loudness_dynamics_batch(contents[1], gains=gains)['lra'])


# ---- the profile-error kernel alone
@pytest.mark.parametrize('W', [1, 31, 300])
@pytest.mark.parametrize('V', [1, 3])
def test_profile_error(loudness, W, V):
    S = 4
    rng = np.random.default_rng(W * 10 + V)
    R = rng.uniform(-45.0, -10.0, (S, W))
    C = R[None] + rng.uniform(-6.0, 6.0, (V, S, W))
    R[1, 0::7] = -80.0                                                       # silenced by the reference only
    R[3, 5::11] = -np.inf
    C[:, 2, 3::5] = -np.inf                                                  # by the candidate only
    C[:, 0, 4::9] = -70.0 - 1e-9
    C[:, 1, 0::14] = -95.0                                                   # by both
    C[0, 3, W // 2] = -70.0                                                  # exactly on the gate: active unless silenced above
    if V == 3:
        C[2, 1] = -100.0                                                     # a variant without any active window
    err, active = loudness.profile_error_device(cuda(R), cuda(C))
    err, active = err.cpu().numpy(), active.cpu().numpy()
    want = [ref.profile_error(R, C[v]) for v in range(V)]
    worst = diff(err, np.array([w[0] for w in want]))
    print('W = %d, V = %d: active %s of %d, max err %.3g LU (bound 1e-12)' % (W, V, active.astype(int).tolist(), W, worst))
    assert np.array_equal(active, np.array([w[1] for w in want], dtype=np.float64))
    assert worst <= 1e-12
    if W >= 31:
        assert 0 < active[0] < W
    if V == 3:
        assert np.isnan(err[2]) and active[2] == 0
    dead, count = loudness.profile_error_device(cuda(np.full((S, W), -71.0)), cuda(C[0]))      # [S, W]: one variant
    assert np.isnan(dead.item()) and count.item() == 0
    same, count = loudness.profile_error_device(cuda(C[0]), cuda(C[0][None]))
    assert (same.item() == 0.0 and count.item() > 0) or (np.isnan(same.item()) and count.item() == 0)
