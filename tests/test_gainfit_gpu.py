"""GPU: the gain-fit kernels (csrc/dam_gainfit.hip) against the numpy float64 reference (tests/_gainfit_ref.py).

Bounds, with u = 2^-53, N the addends of one moment (window length x channels) and kappa the reference's cond(R) of the
window:
  moments    |M_ij - ref_ij| <= 4 N u sqrt(ref_ii ref_jj): recursive summation in any order (N u sum |addends|), Cauchy-Schwarz
             on the addends, margin 4.  The reference is exactly rounded.
  solve      on the same device M: gains within 64 kappa u max|g_ref|, residual within 64 kappa u (1 + sum|g_ref|)^2, status
             equal -- a backward-stable factorisation of an S <= 8 system loses a small multiple of kappa u.
  end to end from samples: the same with N u in place of u (the moments carry N u relative error into the solve).
  gain error 1e-10 dB: values <= 40 dB, log10 good to a few ulp, the rest margin.  n_kept exact.
Everything else here (symmetry, a window against a call of its own, constants against their broadcast, graph replays, the
NaN and status patterns) is bitwise.  Every test prints its largest error as a fraction of its bound before it asserts.
Largest observed (1 x MI355X): moments 0.0004 of the bound; solve on device M 0.016 (gains) and 0.0005 (residual); end to end
1.2e-5 and 2.2e-7, planted gains back to 1.1e-15 (float64 target) and 3.4e-9 (float32 target: its own rounding); pool of three
4.4e-16; identical stems with ridge 1e-6: kappa 2.7e6 .. 2.8e6, gains 0.008 and |g0 - g3| 0.019 of the bound; gain error
8.9e-16 dB; evaluator (W 12, N 34696, kappa <= 1.023): oracle gains 1.2e-6 of the bound, residual 0, the figures equal numpy's."""
import math

import numpy as np
import pytest
import torch

import _gainfit_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U_ROUND
S0, C0, N0, W0 = 4, 2, 6007, 5


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import gainfit, ops
    tile, max_stems = ops.gainfit_geometry()
    assert max_stems == ref.MAX_STEMS and tile >= 256 and tile % 256 == 0
    return gainfit, ops, int(tile)


def up_stems(x, planar):
    """[S, n, C] numpy -> a CUDA tensor of that shape: planar [S, C, n] storage transposed, or contiguous."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def up_mix(y, planar):
    if planar:
        return torch.from_numpy(np.ascontiguousarray(y.T)).cuda().transpose(0, 1)
    return torch.from_numpy(np.ascontiguousarray(y)).cuda()


def random_case(seed, S, C, n, W, x_dtype, y_dtype):
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((S, n, C)) + 0.05 * rng.standard_normal((1, n, C))).astype(x_dtype)
    g = rng.uniform(0.5, 1.5, (S, W))
    y = (ref.mix(x, g) + 0.01 * rng.standard_normal((n, C))).astype(y_dtype)
    return x, y


def moment_ratio(got, want, n, W, C):
    """largest |M_ij - ref_ij| / (4 N u sqrt(ref_ii ref_jj)) over the windows; an entry whose bound is 0 must be exactly 0."""
    worst = 0.0
    for w, (a, b) in enumerate(ref.window_bounds(n, W)):
        dg = np.sqrt(np.diag(want[w]))
        bound = 4.0 * (b - a) * C * U * dg[:, None] * dg[None, :]
        err = np.abs(got[w] - want[w])
        assert np.all(err[bound == 0.0] == 0.0)
        worst = max(worst, float((err[bound > 0.0] / bound[bound > 0.0]).max()))
    return worst


F32, F64 = np.float32, np.float64
MOMENT_CASES = [  # S, C, n, W (None: two windows of 2 tiles + 3), x dtype, y dtype, planar stems, planar mix
    (1, 1, N0, W0, F32, F64, True, True), (1, 2, N0, W0, F64, F32, False, False), (4, 1, N0, W0, F64, F64, True, False),
    (8, 1, N0, W0, F32, F32, False, True), (8, 2, N0, W0, F32, F64, True, True),
    (4, 2, N0, W0, F32, F32, True, True), (4, 2, N0, W0, F32, F64, True, True), (4, 2, N0, W0, F64, F32, True, True),
    (4, 2, N0, W0, F64, F64, True, True), (4, 2, N0, W0, F32, F32, False, False), (4, 2, N0, W0, F32, F64, False, False),
    (4, 2, N0, W0, F64, F32, False, False), (4, 2, N0, W0, F64, F64, False, False),
    (3, 2, None, 2, F32, F64, True, True),
]


@pytest.mark.parametrize('case', range(len(MOMENT_CASES)))
def test_moments_against_reference_and_bitwise(env, case):
    gainfit, ops, tile = env
    S, C, n, W, xd, yd, px, py = MOMENT_CASES[case]
    if n is None:
        n = W * (2 * tile + 3) + 1                                      # windows of 2 tiles + 3 and 2 tiles + 4 samples
    x, y = random_case(100 + case, S, C, n, W, xd, yd)
    dx, dy = up_stems(x, px), up_mix(y, py)
    M = gainfit.moments(dx, dy, W)
    assert M.dtype == torch.float64 and tuple(M.shape) == (W, S + 1, S + 1) and M.is_cuda
    assert torch.equal(M, M.transpose(1, 2))                            # exactly symmetric
    worst = moment_ratio(M.cpu().numpy(), ref.moments(x, y, W), n, W, C)
    print('S %d C %d n %d W %d %s/%s: largest |dM| / bound = %.4f' % (S, C, n, W, xd.__name__, yd.__name__, worst))
    assert worst <= 1.0
    assert torch.equal(gainfit.moments(dx, dy, W), M)                   # reproducible
    bounds = ref.window_bounds(n, W)
    assert bounds[-1][1] - bounds[-1][0] > bounds[0][1] - bounds[0][0]  # the last window is the long one
    for w, (a, b) in enumerate(bounds):                                 # a window == the same samples as a call of their own
        assert torch.equal(gainfit.moments(dx[:, a:b], dy[a:b], 1)[0], M[w]), w


@pytest.fixture(scope='module')
def base(env):
    """The base input with a float64 and a float32 target, its reference moments and solution, and the device moments."""
    gainfit = env[0]
    out = {}
    for name, dt in (('f64', F64), ('f32', F32)):
        x, y, g = ref.base_input(dt)
        Mr = ref.moments(x, y, W0)
        dx, dy = up_stems(x, True), up_mix(y, True)
        out[name] = dict(x=x, y=y, g=g, Mr=Mr, sol=ref.solve(Mr), dx=dx, dy=dy, M=gainfit.moments(dx, dy, W0))
    return out


def solve_ratio(got, want, scale=1.0):
    """(largest gain error / bound, largest residual error / bound) of a device solution against the reference's
    (gains, residual, status, cond) of the same problem; status and the NaN pattern must agree exactly.  scale: N for a
    comparison from samples, 1 on the same moments."""
    gains, residual, status = (t.cpu().numpy() for t in got)
    g_ref, r_ref, s_ref, cond = want
    assert status.dtype == np.int32 and status.tolist() == s_ref.tolist()
    assert np.array_equal(np.isnan(gains), np.isnan(g_ref)) and np.array_equal(np.isnan(residual), np.isnan(r_ref))
    worst_g = worst_r = 0.0
    for w in range(len(s_ref)):
        if s_ref[w] <= 0:
            continue
        act = ~np.isnan(g_ref[:, w])
        bound_g = 64.0 * cond[w] * scale * U * np.abs(g_ref[act, w]).max()
        bound_r = 64.0 * cond[w] * scale * U * (1.0 + np.abs(g_ref[act, w]).sum()) ** 2
        worst_g = max(worst_g, float(np.abs(gains[act, w] - g_ref[act, w]).max() / bound_g))
        worst_r = max(worst_r, abs(residual[w] - r_ref[w]) / bound_r)
        assert residual[w] >= 0.0
    return worst_g, worst_r


@pytest.mark.parametrize('target', ['f64', 'f32'])
@pytest.mark.parametrize('pool,ridge', [(0, 0.0), (1, 0.0), (7, 1e-3)])
def test_solve_against_reference_on_device_moments(env, base, target, pool, ridge):
    gainfit = env[0]
    b = base[target]
    got = gainfit.solve(b['M'], pool=pool, ridge=ridge)
    assert tuple(got[0].shape) == (S0, W0) and got[0].dtype == torch.float64 and got[2].dtype == torch.int32
    wg, wr = solve_ratio(got, ref.solve(b['M'].cpu().numpy(), pool, ridge))
    print('solve on device M (%s target, pool %d, ridge %g): gains %.4f, residual %.4f of the bound' % (target, pool, ridge, wg, wr))
    assert wg <= 1.0 and wr <= 1.0


def test_end_to_end_base_input(env, base):
    gainfit = env[0]
    N = ref.addends(N0, W0, C0)
    for target in ('f64', 'f32'):
        b = base[target]
        got = gainfit.fit_gains(b['dx'], b['dy'], W0)
        assert torch.equal(got[0], gainfit.solve(b['M'])[0])            # fit_gains is moments + solve
        wg, wr = solve_ratio(got, b['sol'], scale=N)
        known = float(np.abs(got[0].cpu().numpy() - b['g']).max())
        print('end to end (%s target): gains %.3g, residual %.3g of the bound; against the planted gains %.3g'
              % (target, wg, wr, known))
        assert wg <= 1.0 and wr <= 1.0
        if target == 'f64':
            assert known <= 1e-9                                        # ~ kappa N u = 1.5e-12 expected; the rest is margin
            assert float(got[1].max()) <= 64.0 * 5.6 * N * U * (1.0 + np.abs(b['g']).sum(axis=0).max()) ** 2


def test_pool_of_three_equals_one_long_window(env):
    gainfit = env[0]
    x, _, g = ref.base_input(F64, W=1)
    y = ref.mix(x, g)                                                   # one gain per stem over the whole track
    dx, dy = up_stems(x, True), up_mix(y, True)
    pooled = gainfit.fit_gains(dx, dy, 3, pool=1)
    single = gainfit.fit_gains(dx, dy, 1)
    want = ref.solve(ref.moments(x, y, 1))
    bound = 64.0 * want[3][0] * (N0 * C0) * U * np.abs(want[0]).max()
    d = float((pooled[0][:, 1] - single[0][:, 0]).abs().max())
    d_ref = float(np.abs(pooled[0][:, 1].cpu().numpy() - want[0][:, 0]).max())
    print('pool 1 of 3 windows against one window: %.3g (reference %.3g), bound %.3g' % (d, d_ref, bound))
    assert d <= bound and d_ref <= bound and pooled[2].tolist() == [S0] * 3 and single[2].tolist() == [S0]


def test_planted_cases(env, base):
    gainfit = env[0]
    x, y, g = base['f64']['x'], base['f64']['y'], base['f64']['g']
    N = ref.addends(N0, W0, C0)
    bounds = ref.window_bounds(N0, W0)

    def fit(xs, ys, **kw):
        return gainfit.fit_gains(up_stems(xs, True), up_mix(ys, True), W0, **kw)
    # a stem silent in one window
    z = x.copy()
    z[1, bounds[1][0]:bounds[1][1]] = 0.0
    yz = ref.mix(z, g)
    got = fit(z, yz)
    assert got[2].tolist() == [4, 3, 4, 4, 4]
    nan = torch.isnan(got[0]).cpu().numpy()
    assert nan.sum() == 1 and nan[1, 1] and not torch.isnan(got[1]).any()
    wg, wr = solve_ratio(got, ref.solve(ref.moments(z, yz, W0)), scale=N)
    assert wg <= 1.0 and wr <= 1.0
    # a silent target in one window
    y0 = y.copy()
    y0[bounds[3][0]:bounds[3][1]] = 0.0
    got = fit(x, y0)
    assert got[2].tolist() == [4, 4, 4, 0, 4]
    assert torch.isnan(got[0]).cpu().numpy().tolist() == [[False, False, False, True, False]] * S0
    assert torch.isnan(got[1]).tolist() == [False, False, False, True, False]
    # identical stems: rank-deficient without a ridge ...
    t = x.copy()
    t[3] = t[0]
    yt = ref.mix(t, g)
    dt, dyt = up_stems(t, True), up_mix(yt, True)
    M = gainfit.moments(dt, dyt, W0)
    assert torch.equal(M[:, 0, :], M[:, 3, :])                          # the same products in the same order
    got = gainfit.solve(M)
    assert got[2].tolist() == [-1] * W0 and torch.isnan(got[0]).all() and torch.isnan(got[1]).all()
    assert ref.solve(M.cpu().numpy())[2].tolist() == [-1] * W0
    # ... and finite, equal gains with one, within the kappa-scaled bound (kappa computed, not assumed)
    got = gainfit.solve(M, ridge=1e-6)
    want = ref.solve(M.cpu().numpy(), ridge=1e-6)
    wg, wr = solve_ratio(got, want)
    kappa = want[3]
    gains = got[0].cpu().numpy()
    equal = np.abs(gains[0] - gains[3]) / (64.0 * kappa * U * np.abs(want[0]).max(axis=0))
    print('identical stems, ridge 1e-6: kappa %.3g .. %.3g, gains %.3g and |g0 - g3| %.3g of the bound'
          % (kappa.min(), kappa.max(), wg, equal.max()))
    assert got[2].tolist() == [4] * W0 and np.all(np.isfinite(gains)) and np.all(kappa > 1e6)
    assert wg <= 1.0 and wr <= 1.0 and np.all(equal <= 1.0)
    # a polarity-flipped stem: a negative gain
    gn = g.copy()
    gn[2] = -gn[2]
    got = fit(x, ref.mix(x, gn))
    gains = got[0].cpu().numpy()
    assert got[2].tolist() == [4] * W0 and np.all(gains[2] < 0.0) and np.all(gains[[0, 1, 3]] > 0.0)
    assert np.abs(gains - gn).max() <= 1e-9


def bits_equal(a, b):
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def test_gain_error_against_reference(env):
    gainfit = env[0]
    rng = np.random.default_rng(31)
    worst = 0.0
    for S, W in ((5, 70), (8, 64), (2, 3), (1, 9)):                     # more than one run of 64 windows; the cap; S = 1 keeps nothing
        fit = rng.uniform(0.3, 3.0, (S, W))
        cand = rng.uniform(0.3, 3.0, (4, S, W))
        if S == 5:                                                      # the planted entries; every other entry is kept
            fit[1, 3] = np.nan
            fit[2, 10] = -0.8
            fit[1:, 20] = np.nan                                        # a window with a single stem left
            cand[1, 0, 65] = np.nan
            cand[1, 4, 66] = -1.0
            cand[2, 3, 0] = 0.0
            cand[2, 3, 69] = np.inf
        cand[3] = fit                                                   # cand == fit: exactly 0
        dfit, dcand = torch.from_numpy(fit).cuda(), torch.from_numpy(cand).cuda()
        err, err_stem, kept = gainfit.gain_error_device(dfit, dcand)
        assert err.dtype == torch.float64 and kept.dtype == torch.int32 and tuple(err_stem.shape) == (4, S)
        e_ref, es_ref, k_ref = ref.gain_error(fit, cand)
        assert kept.tolist() == k_ref.tolist()
        if S == 5:
            assert k_ref[0] == S * W - 1 - 1 - 5 and k_ref[1] == k_ref[0] - 2 and k_ref[2] == k_ref[0] - 2
        e, es = err.cpu().numpy(), err_stem.cpu().numpy()
        assert np.array_equal(np.isnan(e), np.isnan(e_ref)) and np.array_equal(np.isnan(es), np.isnan(es_ref))
        if S == 1:
            assert np.all(np.isnan(e)) and kept.tolist() == [0] * 4
            continue
        worst = max(worst, float(np.abs(e - e_ref).max()), float(np.nanmax(np.abs(es - es_ref))))
        assert e[3] == 0.0 and np.all(es[3] == 0.0)
        twice = gainfit.gain_error_device(dfit, 2.0 * dfit)             # one variant without the leading axis
        assert twice[0].item() <= 1e-12 and twice[2].item() == k_ref[3]
        const = rng.uniform(0.3, 3.0, (3, S, 1))
        a = gainfit.gain_error_device(dfit, torch.from_numpy(const).cuda())
        b = gainfit.gain_error_device(dfit, torch.from_numpy(np.ascontiguousarray(np.broadcast_to(const, (3, S, W)))).cuda())
        assert all(bits_equal(p, q) for p, q in zip(a, b))
        c_ref = ref.gain_error(fit, const)
        worst = max(worst, float(np.abs(a[0].cpu().numpy() - c_ref[0]).max()))
        assert a[2].tolist() == c_ref[2].tolist()
    print('gain error: largest |d| = %.3g dB = %.3g of the 1e-10 bound' % (worst, worst / 1e-10))
    assert worst <= 1e-10


def test_capture_and_replay(env, base):
    gainfit = env[0]
    b = base['f32']
    rng = np.random.default_rng(5)
    buf, ybuf = b['dx'].clone(), b['dy'].clone()
    cand = torch.from_numpy(rng.uniform(0.5, 1.5, (3, S0, W0))).cuda()

    def run(xs, ys):
        M = gainfit.moments(xs, ys, W0)
        g, r, st = gainfit.solve(M, pool=1, ridge=1e-9)
        return (M, g, r, st) + tuple(gainfit.gain_error_device(g, cand))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(buf, ybuf)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(buf, ybuf)
    for scale in (0.5, 1.75):
        new = (b['dx'] * scale).contiguous()
        new[1].mul_(1.5)
        buf.copy_(new)                                                  # the stems rewritten in place
        graph.replay()
        torch.cuda.synchronize()
        eager = run(new.clone(), b['dy'].clone())
        for got, want in zip(outs, eager):
            assert bits_equal(got, want)
        assert not torch.isnan(outs[1]).any() and outs[3].tolist() == [S0] * W0
    print('moments + solve + gain error in one graph: two replays on rewritten stems, bitwise the eager results')


def test_argument_errors(env):
    gainfit, ops, tile = env
    L = ops._lib.lib()
    S, n, C, W = 3, 500, 2, 4
    x = torch.zeros((S, n, C), dtype=torch.float32, device='cuda')
    y = torch.zeros((n, C), dtype=torch.float64, device='cuda')
    sentinel = -7.0
    M = torch.full((W, S + 1, S + 1), sentinel, dtype=torch.float64, device='cuda')
    ws = torch.zeros(L.dam_gainfit_workspace_bytes(W, n, S) // 8, dtype=torch.float64, device='cuda')
    assert ws.numel() == W * 1 * 10

    def mom(x_=x.data_ptr(), y_=y.data_ptr(), S_=S, C_=C, n_=n, W_=W, M_=M.data_ptr(), ws_=ws.data_ptr()):
        return L.dam_gainfit_moments(x_, 0, S_, C_, n_, n * C, C, 1, y_, 1, C, 1, W_, M_, ws_, None)
    for kw in (dict(x_=None), dict(y_=None), dict(M_=None), dict(ws_=None), dict(S_=0), dict(S_=9), dict(C_=0), dict(C_=3),
               dict(n_=0), dict(W_=0), dict(W_=n + 1), dict(W_=-1)):
        assert mom(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(M == sentinel)                                     # nothing was launched
    assert mom() == 0 and torch.all(gainfit.moments(x, y, W) == 0.0)
    torch.cuda.synchronize()
    assert torch.all(M == 0.0)
    g = torch.full((S, W), sentinel, dtype=torch.float64, device='cuda')
    r = torch.full((W,), sentinel, dtype=torch.float64, device='cuda')
    st = torch.full((W,), 77, dtype=torch.int32, device='cuda')

    def sol(M_=M.data_ptr(), W_=W, S_=S, pool=0, ridge=0.0, g_=g.data_ptr(), r_=r.data_ptr(), st_=st.data_ptr()):
        return L.dam_gainfit_solve(M_, W_, S_, pool, ridge, g_, r_, st_, None)
    for kw in (dict(M_=None), dict(g_=None), dict(r_=None), dict(st_=None), dict(W_=0), dict(S_=0), dict(S_=9), dict(pool=-1),
               dict(ridge=-1e-300), dict(ridge=float('nan'))):
        assert sol(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(g == sentinel) and torch.all(r == sentinel) and torch.all(st == 77)
    assert sol(pool=2 ** 31 - 1) == 0                                   # silence: status 0, NaN
    torch.cuda.synchronize()
    assert st.tolist() == [0] * W and torch.isnan(g).all() and torch.isnan(r).all()
    fit = torch.ones((S, W), dtype=torch.float64, device='cuda')
    cand = torch.ones((2, S, W), dtype=torch.float64, device='cuda')
    e = torch.full((2,), sentinel, dtype=torch.float64, device='cuda')
    es = torch.full((2, S), sentinel, dtype=torch.float64, device='cuda')
    k = torch.full((2,), 77, dtype=torch.int32, device='cuda')

    def ge(fit_=fit.data_ptr(), cand_=cand.data_ptr(), V=2, S_=S, W_=W, n_cand=W, e_=e.data_ptr(), es_=es.data_ptr(), k_=k.data_ptr()):
        return L.dam_gainfit_gain_error(fit_, cand_, V, S_, W_, n_cand, e_, es_, k_, None)
    for kw in (dict(fit_=None), dict(cand_=None), dict(e_=None), dict(es_=None), dict(k_=None), dict(V=0), dict(S_=0), dict(S_=9),
               dict(W_=0), dict(n_cand=0), dict(n_cand=2), dict(n_cand=W + 1)):
        assert ge(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(e == sentinel) and torch.all(es == sentinel) and torch.all(k == 77)
    assert ge() == 0 and ge(n_cand=1) == 0
    torch.cuda.synchronize()
    assert e.tolist() == [0.0, 0.0] and k.tolist() == [S * W] * 2
    # the Python surface raises for the same, before the library is asked
    with pytest.raises(ValueError):
        gainfit.moments(x, y, n + 1)
    with pytest.raises(ValueError):
        gainfit.moments(x, y[:-1], W)
    with pytest.raises(ValueError):
        gainfit.moments(torch.zeros((9, n, C), dtype=torch.float32, device='cuda'), y, W)
    with pytest.raises(TypeError):
        gainfit.moments(x.to(torch.float16), y, W)
    with pytest.raises(ValueError):
        gainfit.solve(M, pool=-1)
    with pytest.raises(ValueError):
        gainfit.solve(M, ridge=-1.0)
    with pytest.raises(TypeError):
        gainfit.solve(M.float())
    with pytest.raises(ValueError):
        gainfit.solve(M[:, :, :3])
    with pytest.raises(ValueError):
        gainfit.gain_error_device(fit, cand[:, :, :2])
    with pytest.raises(ValueError):
        gainfit.gain_error_device(fit, cand[:, :2])
    with pytest.raises(TypeError):
        gainfit.gain_error_device(fit.float(), cand)
    with pytest.raises(RuntimeError, match='GPU only'):
        gainfit.fit_gains(x.cpu(), y.cpu(), W)


# ---- the evaluator: LoudnessEvaluator.process_song_tracks(gain_fit=...)
SR, CHUNK_LENGTH = 8000, 2
N_SONG = SR * 26 + 77
KEYS = ('bass', 'drums', 'vocals', 'other')
MEAN_LOUDNESS = {'bass': -25.0, 'drums': -21.0, 'vocals': -19.0, 'other': -23.0}
CONSTANTS = (0.75, 1.25, 1.5, 0.875)
OLD_KEYS = ['song_name', 'sum_error', 'loudnorm_error', 'mix_error', 'random_error', 'smooth_gains']
ST_KEYS = ['sum_st_error', 'loudnorm_st_error', 'mix_st_error', 'random_st_error']
FIT_KEYS = ['sum_gain_error', 'loudnorm_gain_error', 'mix_gain_error', 'random_gain_error', 'oracle_gains', 'oracle_residual']


def song(seed):
    """Four spectrally distinct stereo stems on the 16-bit grid (multiples of 2^-15), so that a stem times a constant of
    three significant bits is exact in float32 and the reference stems' sum is exactly 'stems x constants'."""
    rng = np.random.default_rng(seed)
    t = np.arange(N_SONG) / SR
    tone = lambda f, ph: np.sin(2 * np.pi * f * t[None, :] + np.array([[0.0], [ph]]))
    noise = lambda a: a * rng.standard_normal((2, N_SONG))
    tracks = {'bass': 0.20 * tone(80.0, 0.3) + noise(0.002),
              'drums': noise(0.08),
              'vocals': 0.10 * tone(400.0, 0.5) + 0.06 * tone(800.0, 1.1) + noise(0.002),
              'other': 0.07 * tone(2500.0, 0.7) + noise(0.002)}
    return {k: (np.round(tracks[k] * 32768.0) / 32768.0).astype(np.float32) for k in KEYS}


@pytest.fixture(scope='module')
def evaluator(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.evaluation import LoudnessEvaluator
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(3)
    model = ResNet18(n_stems=4, input_shape=(1025, 16)).cuda().eval()
    a = song(0)
    d = MultitrackAudioDataset.from_arrays({'x': {**{k: v[:, :SR * 2].T for k, v in a.items()}, 'mix': a['bass'][:, :SR * 2].T}},
                                           chunk_length=CHUNK_LENGTH, sr=SR, tracklist=list(KEYS) + ['mix'])
    reference = {k: v * np.float32(c) for (k, v), c in zip(a.items(), CONSTANTS)}
    for k, c in zip(KEYS, CONSTANTS):
        assert reference[k].dtype == np.float32 and np.array_equal(reference[k].astype(np.float64), a[k].astype(np.float64) * c)

    def evaluate(tracks, reference_tracks, **kw):
        ev = LoudnessEvaluator(SR, KEYS, dataset=d, d_mean_loudness=MEAN_LOUDNESS, mix_model=model, seed=7)
        stats = ev.process_song_tracks(tracks, reference_tracks, 'song a', n_random_samples=2, chunk_length=CHUNK_LENGTH, **kw)
        return stats, float(np.random.uniform())                        # the next value of the seeded generator

    runs = {'off': evaluate(a, reference), 'explicit_off': evaluate(a, reference, gain_fit=False),
            'on': evaluate(a, reference, gain_fit=True)}
    yield a, reference, evaluate, runs
    inference_utils._mixers.clear()


def test_evaluator_switch_leaves_todays_stats_alone(evaluator):
    a, reference, evaluate, runs = evaluator
    (off, next_off), (explicit, next_explicit), (on, next_on) = runs['off'], runs['explicit_off'], runs['on']
    assert list(off) == OLD_KEYS and explicit == off and list(on) == OLD_KEYS + FIT_KEYS
    for key in OLD_KEYS:
        assert on[key] == off[key], key                                 # the floats exactly, smooth gains included
    assert next_on == next_off == next_explicit                         # the same number of draws, in the same order
    both, next_both = evaluate(a, reference, dynamics=True, gain_fit={'pool': 0, 'ridge': 0.0})
    assert list(both) == OLD_KEYS + ST_KEYS + ['lra'] + FIT_KEYS and next_both == next_off
    for key in OLD_KEYS:
        assert both[key] == off[key], key
    for key in FIT_KEYS:
        assert both[key] == on[key], key
    with pytest.raises(ValueError, match='unknown'):
        evaluate(a, reference, gain_fit={'pol': 1})
    with pytest.raises(ValueError, match='length'):
        evaluate(a, {k: v[:, :-1] for k, v in reference.items()}, gain_fit=True)


def test_evaluator_oracle_gains_and_errors(env, evaluator):
    gainfit = env[0]
    a, reference, evaluate, runs = evaluator
    stats = runs['on'][0]
    W = len(stats['smooth_gains'][KEYS[0]])
    assert W >= 2 and list(stats['oracle_gains']) == list(KEYS) and len(stats['oracle_residual']) == W
    oracle = np.array([stats['oracle_gains'][k] for k in KEYS])
    assert oracle.shape == (4, W)
    # this song's kappa and N: the moments of what the evaluator fits (float32 stems, the float64 sum of the reference stems)
    x = np.stack([a[k].T for k in KEYS])                                # [S, n, C]
    y = np.zeros((N_SONG, 2))
    for k in KEYS:
        y = y + reference[k].T.astype(np.float64)
    M = gainfit.moments(up_stems(x, True), up_mix(y, True), W)
    g_ref, r_ref, s_ref, kappa = ref.solve(M.cpu().numpy())
    N = ref.addends(N_SONG, W, 2)
    assert s_ref.tolist() == [4] * W
    want = np.array(CONSTANTS)[:, None]
    bound_g = 64.0 * kappa * N * U * max(CONSTANTS)
    bound_r = 64.0 * kappa * N * U * (1.0 + sum(CONSTANTS)) ** 2
    eg = np.abs(oracle - want).max(axis=0) / bound_g
    er = np.array(stats['oracle_residual']) / bound_r
    print('evaluator: W %d, N %d, kappa <= %.3f; oracle gains %.3g and residual %.3g of the end-to-end bounds (%.3g, %.3g)'
          % (W, N, kappa.max(), eg.max(), er.max(), bound_g.max(), bound_r.max()))
    assert np.all(eg <= 1.0) and np.all(er <= 1.0) and np.all(np.array(stats['oracle_residual']) >= 0.0)
    d = -20.0 * np.log10(np.array(CONSTANTS))
    want_sum = float(np.mean(np.abs(d - d.mean())))
    smooth = np.array([stats['smooth_gains'][k] for k in KEYS])
    np.random.seed(7)
    drawn = np.array([[float(np.random.uniform(0.5, 1.5)) for _ in KEYS] for _ in range(2)])
    want_mix = ref.gain_error(oracle, smooth[None])[0][0]
    want_random = float(np.mean(ref.gain_error(oracle, drawn[:, :, None])[0]))
    for key, value in (('sum_gain_error', want_sum), ('mix_gain_error', want_mix), ('random_gain_error', want_random)):
        print('%s: %.12f dB (numpy %.12f, |diff| %.3g)' % (key, stats[key], value, abs(stats[key] - value)))
    for key, value in (('sum_gain_error', want_sum), ('mix_gain_error', want_mix), ('random_gain_error', want_random)):
        assert abs(stats[key] - value) <= 1e-10, key
    assert want_sum > 1.0 and math.isfinite(stats['loudnorm_gain_error']) and stats['loudnorm_gain_error'] > 0.0
    # the reference fitted with itself: unit gains, and the plain sum is then at no distance from them
    same, _ = evaluate(reference, reference, gain_fit=True)
    assert np.abs(np.array([same['oracle_gains'][k] for k in KEYS]) - 1.0).max() <= bound_g.max() / max(CONSTANTS)
    assert same['sum_gain_error'] <= 1e-10
