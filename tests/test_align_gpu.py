"""GPU: the alignment kernels (csrc/dam_align.hip) against the numpy float64 reference (tests/_align_ref.py).

The curve's bound has no constant of its own.  It starts from the project's bound of the LDS FFT, EPS = 2e-6 per bin relative
to the frame's largest bin magnitude (tests/test_features_gpu.py and tests/test_spectrum_gpu.py hold the same transform to
it), and is propagated
  through the product    beta_C[k] = sum_t EPS (pkA_t |Y_t[k]| + pkY_t |A_t[k]| + EPS pkA_t pkY_t),
  through the inverse    |dc| <= (1/N) sum_k c_k beta_C[k] + EPS (1/N) sum_k c_k |C[k]|   (c_k = 1 at k = 0, N/2, else 2),
  for 'phat' through the weighting's Lipschitz constant 2 / (PHAT_FLOOR mean |C|) in front of beta_C, |C| weighted,
all from the reference's float64 frames (_align_ref.cross_spectrum / curve_bound).  The integer lag, sign and status are exact
wherever the REFERENCE's peak leads the runner-up |c| by more than twice that bound -- a condition on the input, computed
before the device's answer is looked at; every planted-delay case of at least one workgroup's length must meet it.  frac and
peak stay within the curve bound propagated through the parabola (_align_ref.frac_bound) or the quotient.
Everything else here (a pair against the same pair in another batch, graph replays, repeated calls, the shift) is bitwise.
Every test prints its largest error as a fraction of its bound before it asserts.
Largest observed (1 x MI355X), curve / frac / peak as fractions of their bounds: N = 64 plain 0.011 / 0.0033 / 0.010, phat
4.6e-5 / 2.3e-5 / 3.8e-5; N = 256 plain 0.012 / 0.0047 / 0.012, phat 4.8e-5 / 1.6e-5 / 4.8e-5; N = 8192 plain 0.0031, phat 5.8e-6;
N = 16384 plain 0.0066, phat 1.2e-5.  Every stem of every case of at least F H samples leads by more than twice the bound
(smallest: 53 bounds); 2 stems of the 129-sample PHAT case do not."""
import math

import numpy as np
import pytest
import torch

import _align_ref as ref

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import align, ops
    cap, F = ops.align_geometry()
    assert cap == ref.MAX_LAG and F >= 1
    return align, ops, int(F)


def up_stems(x, planar):
    """[S, n, C] numpy -> a CUDA tensor of that shape: planar [S, C, n] storage transposed, or contiguous."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def up_mix(y, planar):
    if planar:
        return torch.from_numpy(np.ascontiguousarray(y.T)).cuda().transpose(0, 1)
    return torch.from_numpy(np.ascontiguousarray(y)).cuda()


def bits_equal(a, b):
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    elif a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def lengths(L, F):
    H = ref.fft_size(L) // 2
    return [1, 2, H - 1, H, H + 1, F * H, F * H + 1, 2 * F * H + 3]


# the properties every length is run with, rotated so that each of S in {1, 4, 8}, 1 and 2 channels, the four dtype pairs
# and the two layouts (stems and mix independently) meets short and long signals at both small frame sizes
VARIANTS = [  # S, C, stems dtype, mix dtype, planar stems, planar mix
    (1, 1, F32, F64, True, True), (4, 2, F64, F32, False, False), (8, 1, F32, F32, False, True), (4, 2, F32, F64, True, False),
    (8, 2, F64, F64, True, True), (1, 2, F32, F32, False, False), (4, 1, F64, F32, True, True), (8, 2, F32, F64, False, True),
]
# (max_lag, index into lengths(), variant): every length at N = 64 and N = 256, one case each at 2048 and 4096 (the 128 KB LDS path)
CASES = [(16, i, VARIANTS[i]) for i in range(8)] + [(64, i, VARIANTS[(i + 3) % 8]) for i in range(8)] + \
        [(2048, 6, (2, 2, F32, F64, True, True)), (4096, 7, (2, 2, F32, F32, True, False)), (3000, 4, (1, 1, F64, F64, False, False))]


def planted_case(seed, S, C, n, L, xd, yd):
    rng = np.random.default_rng(seed)
    delays = [int(d) for d in rng.integers(-L, L + 1, S)]
    delays[0] = [-L, L, 0][seed % 3]                                    # the ends of the range and the middle come up
    invert = (S - 1,) if S > 1 else ()
    x, y = ref.planted(n, delays, C=C, seed=seed, dtype=xd, invert=invert)
    return x, y.astype(yd), delays, invert


def check_estimates(tag, est, want, L, weighting, must_lead):
    """est: the device's five tensors; want: the reference's analyses per stem -> (frac / bound, peak / bound, stems whose
    lead was too small for the exact comparison)."""
    lag, frac, peak, sign, status = (t.cpu().numpy() for t in est)
    assert lag.dtype == np.int32 and sign.dtype == np.int32 and status.dtype == np.int32 and frac.dtype == np.float64
    worst_f = worst_p = 0.0
    skipped = 0
    for s, r in enumerate(want):
        b = r['bound']
        if r['status'] == 0:
            assert (lag[s], frac[s], sign[s], status[s]) == (0, 0.0, 0, 0) and math.isnan(peak[s]), (tag, s)
            continue
        if not r['lead'] > 2.0 * b:
            assert not must_lead, '%s stem %d: lead %.3g <= 2 x bound %.3g' % (tag, s, r['lead'], b)
            skipped += 1
            continue
        assert (lag[s], sign[s], status[s]) == (r['lag'], r['sign'], 1), (tag, s, lag[s], r['lag'])
        fb = ref.frac_bound(r['curve'], r['lag'], L, b)
        pb = b if weighting == 'phat' else b / math.sqrt(r['Ea'] * r['Ey']) + 1e-12 * r['peak']
        assert abs(frac[s]) <= 0.5
        if math.isfinite(fb) and fb > 0.0:
            worst_f = max(worst_f, abs(frac[s] - r['frac']) / fb)
        elif fb == 0.0:
            assert frac[s] == 0.0 == r['frac']
        worst_p = max(worst_p, abs(peak[s] - r['peak']) / pb)
    return worst_f, worst_p, skipped


@pytest.mark.parametrize('case', range(len(CASES)))
def test_curve_and_estimates_against_reference(env, case):
    align, ops, F = env
    L, li, (S, C, xd, yd, px, py) = CASES[case]
    n = lengths(L, F)[li]
    x, y, delays, invert = planted_case(500 + case, S, C, n, L, xd, yd)
    dx, dy = up_stems(x, px), up_mix(y, py)
    long_enough = n >= F * (ref.fft_size(L) // 2) and n > 4 * L
    for weighting in ('plain', 'phat'):
        want = [ref.analyse(x[s], y, L, weighting) for s in range(S)]
        got = align.cross_correlation(dx, dy, L, weighting=weighting)
        assert got.dtype == torch.float64 and tuple(got.shape) == (S, 2 * L + 1) and got.is_cuda
        c = got.cpu().numpy()
        worst = 0.0
        for s, r in enumerate(want):
            assert r['status'] == 1 and r['bound'] > 0.0
            worst = max(worst, float(np.abs(c[s] - r['curve']).max()) / r['bound'])
        est = align.estimate_lag(dx, dy, L, weighting=weighting)
        wf, wp, skipped = check_estimates('case %d %s' % (case, weighting), est, want, L, weighting, long_enough)
        print('L %d n %d S %d C %d %s/%s %s: curve %.3g, frac %.3g, peak %.3g of the bound; %d of %d stems without a clear lead'
              % (L, n, S, C, xd.__name__, yd.__name__, weighting, worst, wf, wp, skipped, S))
        assert worst <= 1.0 and wf <= 1.0 and wp <= 1.0
        if long_enough:                                                 # the planted delays themselves
            lag, sign = est[0].tolist(), est[3].tolist()
            assert lag == delays and sign == [-1 if s in invert else 1 for s in range(S)]


def test_silence_and_polarity_on_the_device(env):
    align, ops, F = env
    L, n = 64, 3001
    x, y, delays, _ = planted_case(77, 3, 2, n, L, F32, F64)
    x[1] = 0.0                                                          # a silent stem between two live ones
    dx, dy = up_stems(x, True), up_mix(y, True)
    for weighting in ('plain', 'phat'):
        lag, frac, peak, sign, status = (t.cpu().numpy() for t in align.estimate_lag(dx, dy, L, weighting=weighting))
        assert status.tolist() == [1, 0, 1] and sign.tolist() == [1, 0, -1] and lag.tolist() == [delays[0], 0, delays[2]]
        assert frac[1] == 0.0 and math.isnan(peak[1]) and not math.isnan(peak[0]) and not math.isnan(peak[2])
        c = align.cross_correlation(dx, dy, L, weighting=weighting)
        assert torch.all(c[1] == 0.0) and c[0].abs().max() > 0.0
        # a silent mix: every stem status 0
        out = align.estimate_lag(dx, torch.zeros_like(dy), L, weighting=weighting)
        assert out[4].tolist() == [0, 0, 0] and out[0].tolist() == [0, 0, 0] and torch.isnan(out[2]).all()
    # a pure delay: the plain peak is 1 up to the samples the delay pushes out of the signal
    pure = ref.shift(x[:1].astype(np.float64), [5])[0]
    out = align.estimate_lag(dx[:1], up_mix(pure, False), L, weighting='plain')
    assert out[0].item() == 5 and 0.99 < out[2].item() <= 1.0 + 1e-6


def test_pairs_are_independent_bitwise(env):
    align, ops, F = env
    L = 64
    n = lengths(L, F)[7]                                                # three workgroups per pair: the partial-reduce path
    x, y, _, _ = planted_case(9, 4, 2, n, L, F32, F64)
    dx, dy = up_stems(x, True), up_mix(y, True)
    for weighting in ('plain', 'phat'):
        def run(stems):
            return (align.cross_correlation(stems, dy, L, weighting=weighting),) + align.estimate_lag(stems, dy, L, weighting=weighting)
        full = run(dx)
        again = run(dx)
        assert all(bits_equal(a, b) for a, b in zip(full, again))       # two calls, the same bits
        perm = [2, 0, 3, 1]
        shuffled = run(dx[perm])                                        # the same pair in a permuted batch
        subset = run(dx[1:3])                                           # ... in a subset
        for out, rows in ((shuffled, perm), (subset, [1, 2])):
            for t_full, t_out in zip(full, out):
                for i, s in enumerate(rows):
                    assert bits_equal(t_full[s:s + 1], t_out[i:i + 1]), (weighting, s)
        for s in range(4):                                              # ... and as S calls with one stem each
            single = run(dx[s:s + 1])
            for t_full, t_out in zip(full, single):
                assert bits_equal(t_full[s:s + 1], t_out), (weighting, s)
    print('a pair equals itself in a permuted batch, a subset and a call of its own; two calls give the same bits')


SHIFT_N = 37
SHIFT_LAGS = [0, 1, -1, SHIFT_N - 1, -(SHIFT_N - 1), SHIFT_N, -SHIFT_N, SHIFT_N + 5, -(SHIFT_N + 5)]


@pytest.mark.parametrize('dtype', [F32, F64])
@pytest.mark.parametrize('planar', [True, False])
@pytest.mark.parametrize('C', [1, 2])
def test_shift_is_numpy_slicing(env, dtype, planar, C):
    align, ops, F = env
    rng = np.random.default_rng(12)
    for lags in (SHIFT_LAGS[:5], SHIFT_LAGS[5:]):
        x = rng.standard_normal((len(lags), SHIFT_N, C)).astype(dtype)
        dx = up_stems(x, planar)
        out = align.shift_tracks(dx, torch.tensor(lags, dtype=torch.int32).cuda())
        assert out.dtype == dx.dtype and tuple(out.shape) == tuple(dx.shape)
        assert C == 1 or out.stride() == dx.stride()                    # planar stays planar (one channel: either way)
        assert np.array_equal(out.cpu().numpy(), ref.shift(x, lags)), lags
        for d in lags:                                                  # one Python int for every stem
            assert np.array_equal(align.shift_tracks(dx, d).cpu().numpy(), ref.shift(x, [d] * len(lags))), d
    # more than one workgroup per stem, a strided view that is neither layout, and a given output
    x = rng.standard_normal((3, 700, C)).astype(dtype)
    wide = up_stems(np.concatenate([x, x], axis=1), planar)
    view = wide[:, ::2] if not planar else wide[:, 700:]
    xv = view.cpu().numpy()
    lags = [257, -256, 3]
    dl = torch.tensor(lags, dtype=torch.int32).cuda()
    assert np.array_equal(align.shift_tracks(view, dl).cpu().numpy(), ref.shift(xv, lags))
    out = torch.full((3, 700, C), 9.0, dtype=view.dtype, device='cuda')
    assert ops.align_shift(view, dl, out=out) is out and np.array_equal(out.cpu().numpy(), ref.shift(xv, lags))


def test_capture_and_replay(env):
    from deep_audio_mixer_amd import gainfit
    align, ops, F = env
    L, n, S, W = 64, 2 * F * 128 + 3, 3, 4
    x, y, delays, _ = planted_case(21, S, 2, n, L, F32, F64)
    dx, dy = up_stems(x, True), up_mix(y, True)
    buf, ybuf = dx.clone(), dy.clone()

    def run(xs, ys):
        est = align.estimate_lag(xs, ys, L)
        shifted = align.shift_tracks(xs, est[0])                        # the lags never leave the device
        return est + (shifted, align.cross_correlation(xs, ys, L)) + gainfit.fit_gains(xs, ys, W, align=L)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(buf, ybuf)                                                  # tables resident, LDS limits raised
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(buf, ybuf)
    for k, new_delays in enumerate(([3, -40, 17], [-64, 64, 0])):
        x2, y2 = ref.planted(n, new_delays, C=2, seed=30 + k, dtype=F32)
        buf.copy_(up_stems(x2, True))                                   # stems and mix rewritten in place
        ybuf.copy_(up_mix(y2, True))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(up_stems(x2, True), up_mix(y2, True))
        for got, want in zip(outs, eager):
            assert bits_equal(got, want)
        assert outs[0].tolist() == new_delays
        assert np.array_equal(outs[5].cpu().numpy(), ref.shift(x2, new_delays))
    print('estimate + shift + aligned fit in one graph: two replays on rewritten inputs, bitwise the eager results')


def test_argument_errors(env):
    align, ops, F = env
    L = ops._lib.lib()
    S, n, C, lag_max = 3, 500, 2, 16
    from deep_audio_mixer_amd import features
    x = torch.zeros((S, n, C), dtype=torch.float32, device='cuda')
    y = torch.zeros((n, C), dtype=torch.float64, device='cuda')
    tw = features._get_tables(x.device, ref.fft_size(lag_max))[1]
    ws = torch.zeros(L.dam_align_workspace_bytes(S, n, lag_max) // 8, dtype=torch.float64, device='cuda')
    assert ws.numel() > 0
    sent_i = lambda: torch.full((S,), 77, dtype=torch.int32, device='cuda')
    sent_d = lambda: torch.full((S,), -7.0, dtype=torch.float64, device='cuda')
    lag, sign, status, frac, peak = sent_i(), sent_i(), sent_i(), sent_d(), sent_d()
    curve = torch.full((S, 2 * lag_max + 1), -7.0, dtype=torch.float64, device='cuda')

    def est(x_=x.data_ptr(), y_=y.data_ptr(), S_=S, C_=C, n_=n, L_=lag_max, w_=1, tw_=tw.data_ptr(), lag_=lag.data_ptr(),
            frac_=frac.data_ptr(), peak_=peak.data_ptr(), sign_=sign.data_ptr(), status_=status.data_ptr(), ws_=ws.data_ptr()):
        return L.dam_align_estimate(x_, 0, S_, C_, n_, n * C, C, 1, y_, 1, C, 1, L_, w_, tw_, lag_, frac_, peak_, sign_, status_,
                                    curve.data_ptr(), ws_, None)
    for kw in (dict(x_=None), dict(y_=None), dict(tw_=None), dict(lag_=None), dict(frac_=None), dict(peak_=None), dict(sign_=None),
               dict(status_=None), dict(ws_=None), dict(S_=0), dict(S_=9), dict(C_=0), dict(C_=3), dict(n_=0), dict(n_=-5),
               dict(L_=0), dict(L_=-1), dict(L_=ref.MAX_LAG + 1), dict(w_=2), dict(w_=-1)):
        assert est(**kw) == -1, kw
    torch.cuda.synchronize()
    for t, v in ((lag, 77), (sign, 77), (status, 77), (frac, -7.0), (peak, -7.0), (curve, -7.0)):
        assert torch.all(t == v)                                        # nothing was launched
    assert est() == 0 and est(w_=0) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0] * S and lag.tolist() == [0] * S and torch.all(curve == 0.0) and torch.isnan(peak).all()
    out = torch.full((S, n, C), 9.0, dtype=torch.float32, device='cuda')

    def shf(x_=x.data_ptr(), S_=S, C_=C, n_=n, lag_=lag.data_ptr(), out_=out.data_ptr()):
        return L.dam_align_shift(x_, 0, S_, C_, n_, n * C, C, 1, lag_, out_, n * C, C, 1, None)
    for kw in (dict(x_=None), dict(lag_=None), dict(out_=None), dict(S_=0), dict(S_=9), dict(C_=0), dict(C_=3), dict(n_=0)):
        assert shf(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(out == 9.0)
    assert shf() == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)
    # the Python surface raises for the same, before the library is asked
    for bad in (0, ref.MAX_LAG + 1, -3):
        with pytest.raises(ValueError):
            align.estimate_lag(x, y, bad)
    with pytest.raises(ValueError):
        align.estimate_lag(x, y[:-1], lag_max)
    with pytest.raises(ValueError):
        align.estimate_lag(torch.zeros((9, n, C), dtype=torch.float32, device='cuda'), y, lag_max)
    with pytest.raises(ValueError, match='weighting'):
        align.cross_correlation(x, y, lag_max, weighting='scot')
    with pytest.raises(TypeError):
        align.estimate_lag(x.to(torch.float16), y, lag_max)
    with pytest.raises(TypeError):
        align.estimate_lag(x, y, 16.0)
    with pytest.raises(ValueError):
        align.shift_tracks(x, torch.zeros(S + 1, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        align.shift_tracks(x, torch.zeros(S, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError):
        ops.align_shift(x, lag, out=torch.zeros((S, n, C), dtype=torch.float64, device='cuda'))
    with pytest.raises(RuntimeError, match='GPU only'):
        align.estimate_lag(x.cpu(), y.cpu(), lag_max)
    with pytest.raises(RuntimeError, match='GPU only'):
        align.cross_correlation(x, y.cpu(), lag_max)
    with pytest.raises(RuntimeError, match='GPU only'):
        align.shift_tracks(x.cpu(), lag)
    with pytest.raises(RuntimeError, match='GPU only'):
        align.shift_tracks(x, lag.cpu())
