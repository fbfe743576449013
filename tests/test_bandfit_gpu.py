"""GPU: the band gain fit (csrc/dam_bandfit.hip, the grouped solve of csrc/dam_gainfit.hip) against the numpy float64 reference
(tests/_bandfit_ref.py).

Bounds:
  moments    |M_ij - ref_ij| <= c sqrt(ref_ii ref_jj) per entry of every cell.  The device's transform is float32, the reference's
             float64, so c is not fixed in advance: the test measures what a float32 transform costs -- the same reference
             with float32 frames and scipy's float32 rfft against the float64 one, on the same input -- and allows 8 times the
             largest such ratio (another radix factorisation, the same O(log N) 2^-24 growth).
  solve      on the device's own moments: the condition-scaled bounds of tests/test_gainfit_gpu.py (its helpers, imported).
  summary    finite values to 1e-15 relative, NaN placement equal.
Everything else (two runs, a band against a table of its own, a dropped stem, the triangles, a window against changes in the
other windows, slabs, one group against dam_gainfit_solve, a group against changes in the other groups, graph replays, the
aligned fit against its parts) is bitwise.  Every test prints its figures before it asserts.
Largest observed (1 x MI355X): moments 0.39 of c on the case whose last window owns one frame (c = 3.4e-5: single-bin cells of one
frame), 0.11 .. 0.22 of c on the other eight cases (c = 4.3e-7 .. 3.2e-6, |dM| / sqrt(M_ii M_jj) <= 3.6e-7); grouped solve on the
device's moments 0.021 (gains) and 0.0007 (residual) of the bounds, the target exact; summary exact on 69 finite windows; two-band
case: low gains to 2.6e-4, high gains to 6.6e-5, broadband residual 3.5e-2 against a band total of 9.0e-7, moments 0.19 of c
(4.7e-7) and gains 0.039 of c cond(R) max|g|."""
import numpy as np
import pytest
import torch

import _bandfit_ref as ref
import _gainfit_ref as gref
from test_bandfit_ref_cpu import check_two_band, inside
from test_gainfit_gpu import bits_equal, solve_ratio, up_mix, up_stems

pytestmark = pytest.mark.gpu

SR = 44100
F32, F64 = np.float32, np.float64
WIDE = np.array([0, 3, 40, 129], dtype=np.int32)                        # n_fft 256: DC and Nyquist, a cell of 12 tiles at hop 32


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import gainfit, ops, spectrum
    assert ops.GAINFIT_BAND_MAX_BANDS == dam_lib.dam_spectrum_max_bands()
    assert dam_lib.dam_bandfit_tile_elements() == 2048
    return gainfit, ops, spectrum


def third_octaves(spectrum, n_fft):
    return spectrum.band_edges(SR, n_fft, 3)[0]


def random_case(seed, S, C, n, W, x_dtype, y_dtype):
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((S, n, C)) + 0.05 * rng.standard_normal((1, n, C))).astype(x_dtype)
    g = rng.uniform(0.5, 1.5, (S, W))
    y = (gref.mix(x, g) + 0.01 * rng.standard_normal((n, C))).astype(y_dtype)
    return x, y


MOMENT_CASES = [  # S, C, n, W, n_fft, hop, x dtype, y dtype, planar stems, planar mix, edges (None: third octaves)
    (4, 2, 6007, 5, 256, 128, F32, F64, True, True, None),
    (1, 1, 6007, 3, 64, 32, F64, F32, False, False, None),
    (2, 2, 6007, 5, 256, 77, F32, F32, False, True, None),              # an odd hop
    (8, 1, 6007, 1, 2048, 1024, F32, F64, True, False, None),           # a cell of 4 tiles
    (8, 2, 6007, 3, 256, 128, F64, F64, False, False, None),
    (4, 2, 129, 1, 256, 128, F32, F32, True, True, None),               # n = n_fft / 2 + 1: two frames, all reflection
    (2, 1, 6007, 46, 256, 128, F32, F64, True, True, None),             # the last window owns a single frame
    (4, 2, 6007, 3, 2048, 1024, F64, F32, True, True, None),
    (3, 2, 6007, 1, 256, 32, F32, F64, False, False, WIDE),             # 12 tiles on 4 workgroups; bins 0 and n_fft / 2
]


@pytest.mark.parametrize('case', range(len(MOMENT_CASES)))
def test_moments_against_reference(env, case):
    gainfit, ops, spectrum = env
    S, C, n, W, n_fft, hop, xd, yd, px, py, edges = MOMENT_CASES[case]
    if edges is None:
        edges = third_octaves(spectrum, n_fft)
    x, y = random_case(200 + case, S, C, n, W, xd, yd)
    first = ref.frame_windows(n, W, hop)
    if case == 6:
        assert first[-1] - first[-2] == 1
    M = gainfit.band_moments(up_stems(x, px), up_mix(y, py), W, n_fft=n_fft, hop=hop, edges=edges)
    B = len(edges) - 1
    assert M.dtype == torch.float64 and tuple(M.shape) == (B, W, S + 1, S + 1) and M.is_cuda
    assert torch.equal(M, M.transpose(2, 3))                            # exactly symmetric
    want = ref.moments(x, y, W, n_fft, hop, edges)
    c = 8.0 * ref.moment_ratio(ref.moments(x, y, W, n_fft, hop, edges, transform='f32'), want)
    worst = ref.moment_ratio(M.cpu().numpy(), want)
    print('S %d C %d n %d W %d n_fft %d hop %d %s/%s, %d bands: c = %.3g, largest |dM| / sqrt(M_ii M_jj) = %.3g = %.3f of c'
          % (S, C, n, W, n_fft, hop, xd.__name__, yd.__name__, B, c, worst, worst / c))
    assert c > 0.0 and worst <= c


@pytest.fixture(scope='module')
def base(env):
    gainfit, ops, spectrum = env
    x, y, g = gref.base_input(F64)
    edges = third_octaves(spectrum, 256)
    dx, dy = up_stems(x, True), up_mix(y, True)
    return dict(x=x, y=y, g=g, dx=dx, dy=dy, edges=edges, kw=dict(n_fft=256, hop=128),
                M=gainfit.band_moments(dx, dy, 5, n_fft=256, hop=128, edges=edges))


def test_moments_bitwise_properties(env, base):
    gainfit, ops, spectrum = env
    dx, dy, edges, kw, M = base['dx'], base['dy'], base['edges'], base['kw'], base['M']
    assert bits_equal(gainfit.band_moments(dx, dy, 5, edges=edges, **kw), M)                       # two runs
    assert torch.equal(M, M.transpose(2, 3)) and not torch.isnan(M).any()
    for b in (0, 7, len(edges) - 2):                                    # a table that holds band b alone
        assert bits_equal(gainfit.band_moments(dx, dy, 5, edges=edges[b:b + 2], **kw)[0], M[b]), b
    keep = [0, 1, 3]                                                    # a dropped stem: the sub-matrix
    sub = gainfit.band_moments(dx[keep], dy, 5, edges=edges, **kw)
    idx = torch.tensor(keep + [4], device='cuda')
    assert bits_equal(sub, M.index_select(2, idx).index_select(3, idx))
    # window 2 holds samples 2402 .. 3602, its frames 19 .. 28 reach samples 2304 .. 3711: the rest of the song may change
    assert ref.frame_windows(6007, 5, 128)[2:4] == [19, 29]
    x2, y2 = base['x'].copy(), base['y'].copy()
    x2[:, :2304] *= 0.5
    y2[3712:] = 0.25
    other = gainfit.band_moments(up_stems(x2, True), up_mix(y2, True), 5, edges=edges, **kw)
    assert bits_equal(other[:, 2], M[:, 2]) and not bits_equal(other[:, 1], M[:, 1]) and not bits_equal(other[:, 3], M[:, 3])
    # slabs of one window each: not a bit changes, the workspace shrinks
    from deep_audio_mixer_amd import features
    win, tw = features._get_tables(dx.device, 256)
    dev_edges = spectrum._device_edges(edges, 256, dx.device)
    assert bits_equal(ops.gainfit_band_moments(dx, dy, 5, win, tw, 256, 128, dev_edges, slab_bytes=1), M)
    L = ops._lib.lib()
    sizes = [L.dam_bandfit_workspace_bytes(5, 6007, 4, 2, 256, 128, len(edges) - 1, sb) for sb in (0, 1)]
    assert 0 < sizes[1] < sizes[0]
    # interleaved storage of the same values: the layout is not part of the result
    assert bits_equal(gainfit.band_moments(up_stems(base['x'], False), up_mix(base['y'], False), 5, edges=edges, **kw), M)


def test_solve_grouped(env, base):
    gainfit, ops, spectrum = env
    # one group is dam_gainfit_solve
    Mt = gainfit.moments(base['dx'], base['dy'], 5)
    for pool, ridge in ((0, 0.0), (1, 0.0), (0, 1e-3), (1, 1e-3)):
        one = ops.gainfit_solve_grouped(Mt.unsqueeze(0), pool, ridge)
        plain = gainfit.solve(Mt, pool=pool, ridge=ridge)
        assert bits_equal(one[0][0], plain[0]) and bits_equal(one[1][0], plain[1]) and bits_equal(one[3][0], plain[2])
        assert not torch.isnan(one[2]).any()
    # three groups: pooling stays inside a group, and a group does not see the others
    M3 = base['M'][[3, 9, 15]].contiguous()
    got = gainfit.solve_bands(M3, pool=1, ridge=1e-3)
    assert tuple(got[0].shape) == (3, 4, 5) and got[3].dtype == torch.int32 and tuple(got[2].shape) == (3, 5)
    for g in range(3):
        plain = gainfit.solve(M3[g], pool=1, ridge=1e-3)
        assert bits_equal(got[0][g], plain[0]) and bits_equal(got[1][g], plain[1]) and bits_equal(got[3][g], plain[2]), g
    changed = M3.clone()
    changed[1] *= 3.0
    changed[1, :, 0, 4] *= 0.5
    changed[1, :, 4, 0] *= 0.5
    again = gainfit.solve_bands(changed, pool=1, ridge=1e-3)
    for g in (0, 2):
        assert all(bits_equal(a[g], b[g]) for a, b in zip(got, again)), g
    assert not bits_equal(got[0][1], again[0][1])
    # against the reference on the device's own moments, every band
    worst_g = worst_r = worst_t = 0.0
    for pool, ridge in ((0, 0.0), (1, 1e-3)):
        dev = gainfit.solve_bands(base['M'], pool=pool, ridge=ridge)
        g_ref, r_ref, t_ref, s_ref, cond = ref.solve_bands(base['M'].cpu().numpy(), pool, ridge)
        for b in range(base['M'].shape[0]):
            wg, wr = solve_ratio((dev[0][b], dev[1][b], dev[3][b]), (g_ref[b], r_ref[b], s_ref[b], cond[b]))
            worst_g, worst_r = max(worst_g, wg), max(worst_r, wr)
        worst_t = max(worst_t, float(np.abs(dev[2].cpu().numpy() / t_ref - 1.0).max()))
    print('grouped solve on device M: gains %.4f, residual %.4f of the bound; target to %.3g relative' % (worst_g, worst_r, worst_t))
    assert worst_g <= 1.0 and worst_r <= 1.0 and worst_t <= 1e-15


def test_band_summary_against_reference(env):
    gainfit = env[0]
    rng = np.random.default_rng(17)
    G, W = 5, 70                                                        # more than one run of 64 windows
    status = rng.integers(-1, 5, (G, W)).astype(np.int32)
    target = rng.uniform(0.0, 2.0, (G, W))
    target[rng.uniform(size=(G, W)) < 0.2] = 0.0
    status[target == 0.0] = 0
    target[:, 5] = 0.0                                                  # a window silent in every band: NaN
    status[:, 5] = 0
    status[:, 6] = -1                                                   # nothing fitted anywhere: 1
    target[:, 6] = 1.0
    residual = np.where(status > 0, rng.uniform(0.0, 1.0, (G, W)), np.nan)
    want = ref.summary(residual, target, status)
    got = gainfit.band_residual_total(torch.from_numpy(residual).cuda(), torch.from_numpy(target).cuda(),
                                      torch.from_numpy(status).cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (W,)
    got = got.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[5]) and want[6] == 1.0 and got[6] == 1.0
    ok = ~np.isnan(want)
    rel = float(np.abs(got[ok] / want[ok] - 1.0).max())
    print('band summary: %d finite windows to %.3g relative' % (ok.sum(), rel))
    assert ok.sum() >= 60 and rel <= 1e-15


def test_two_band_case_end_to_end(env):
    gainfit, ops, spectrum = env
    x, y, a, b = ref.two_band_case()
    edges = third_octaves(spectrum, 256)
    assert len(edges) - 1 == 18
    dx, dy = up_stems(x, True), up_mix(y, True)
    gains, residual, target, status = gainfit.fit_band_gains(dx, dy, 1, n_fft=256, hop=128, edges=edges)
    total = float(gainfit.band_residual_total(residual, target, status)[0])
    broadband = float(gainfit.fit_gains(dx, dy, 1)[1][0])
    g = gains.cpu().numpy()[:, :, 0]
    check_two_band(g, residual.cpu().numpy()[:, 0], target.cpu().numpy()[:, 0], status.cpu().numpy()[:, 0], a, b, edges,
                   broadband, total)
    # against the reference's gains: the moment bound (measured as above, over the tested bands) times the reference's cond(R)
    bands = inside(edges, 600.0, 1100.0) + inside(edges, 5500.0, 10000.0)
    want = ref.moments(x, y, 1, 256, 128, edges)
    c = 8.0 * ref.moment_ratio(ref.moments(x, y, 1, 256, 128, edges, transform='f32')[bands], want[bands])
    g_ref, _, _, s_ref, cond = ref.solve_bands(want)
    M = gainfit.band_moments(dx, dy, 1, n_fft=256, hop=128, edges=edges).cpu().numpy()
    worst_m = ref.moment_ratio(M[bands], want[bands])
    worst = max(float(np.abs(g[i] - g_ref[i, :, 0]).max() / (c * cond[i, 0] * np.abs(g_ref[i, :, 0]).max())) for i in bands)
    print('two bands on the device: c = %.3g, moments %.3f of c, gains %.3f of c cond(R) max|g| (cond(R) <= %.2f)'
          % (c, worst_m / c, worst, cond[bands, 0].max()))
    assert worst_m <= c and worst <= 1.0


def test_capture_and_replay(env, base):
    gainfit = env[0]
    edges, kw = base['edges'], base['kw']
    buf, ybuf = base['dx'].clone(), base['dy'].clone()

    def run(xs, ys):
        out = gainfit.fit_band_gains(xs, ys, 5, edges=edges, pool=1, ridge=1e-9, **kw)
        return out + (gainfit.band_residual_total(out[1], out[2], out[3]),)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(buf, ybuf)                                                  # the tables are resident after this call
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(buf, ybuf)
    for scale in (0.5, 1.75):
        new = (base['dx'] * scale).contiguous()
        new[1].mul_(1.5)
        buf.copy_(new)                                                  # the stems rewritten in place
        graph.replay()
        torch.cuda.synchronize()
        eager = run(new.clone(), base['dy'].clone())
        for got, want in zip(outs, eager):
            assert bits_equal(got, want)
        assert not torch.isnan(outs[4]).any() and bool((outs[3] == 4).all())
    print('fit_band_gains + band_residual_total in one graph: two replays on rewritten stems, bitwise the eager results')


def test_aligned_fit_is_its_parts(env):
    gainfit, ops, spectrum = env
    from deep_audio_mixer_amd import align
    rng = np.random.default_rng(43)
    S, n, C, W, d = 3, 6007, 2, 3, 37
    x = (0.1 * rng.standard_normal((S, n, C))).astype(np.float32)
    moved = np.zeros_like(x)
    moved[:, d:] = x[:, :n - d]
    y = gref.mix(moved, rng.uniform(0.5, 1.5, (S, 1)))                  # the mix holds every stem 37 samples late
    dx, dy = up_stems(x, True), up_mix(y, True)
    edges = third_octaves(spectrum, 256)
    lag = align.estimate_lag(dx, dy, 64)[0]
    assert lag.tolist() == [d] * S
    got = gainfit.fit_band_gains(dx, dy, W, n_fft=256, edges=edges, align=64)
    parts = gainfit.fit_band_gains(align.shift_tracks(dx, lag), dy, W, n_fft=256, edges=edges)
    undelayed = gainfit.fit_band_gains(up_stems(moved, True), dy, W, n_fft=256, edges=edges)
    for a, b, c in zip(got, parts, undelayed):
        assert bits_equal(a, b) and bits_equal(a, c)
    assert bool((got[3] == S).all()) and float(got[1].max()) < 1e-6
    assert float(gainfit.fit_band_gains(dx, dy, W, n_fft=256, edges=edges)[1].min()) > 1e-2         # and without: unexplained


def test_argument_errors(env, base):
    gainfit, ops, spectrum = env
    from deep_audio_mixer_amd import features
    L = ops._lib.lib()
    S, n, C, W, n_fft, hop, B = 3, 1000, 2, 3, 256, 128, 4
    x = torch.zeros((S, n, C), dtype=torch.float32, device='cuda')
    y = torch.zeros((n, C), dtype=torch.float64, device='cuda')
    win, tw = features._get_tables(x.device, n_fft)
    edges = torch.tensor([0, 4, 20, 60, 129], dtype=torch.int32, device='cuda')
    sentinel = -7.0
    M = torch.full((B, W, S + 1, S + 1), sentinel, dtype=torch.float64, device='cuda')
    need = L.dam_bandfit_workspace_bytes(W, n, S, C, n_fft, hop, B, 0)
    assert need > 0 and need % 8 == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device='cuda')

    def args(S_=S, C_=C, n_=n, W_=W, n_fft_=n_fft, hop_=hop, B_=B, slab=0):
        return (W_, n_, S_, C_, n_fft_, hop_, B_, slab)

    def mom(x_=x.data_ptr(), y_=y.data_ptr(), win_=win.data_ptr(), tw_=tw.data_ptr(), e_=edges.data_ptr(), M_=M.data_ptr(),
            ws_=ws.data_ptr(), S_=S, C_=C, n_=n, W_=W, n_fft_=n_fft, hop_=hop, B_=B, slab=0):
        return L.dam_bandfit_moments(x_, 0, S_, C_, n_, n * C, C, 1, y_, 1, C, 1, win_, tw_, n_fft_, hop_, e_, B_, W_, slab, M_, ws_,
                                     None)
    bad = (dict(W_=9), dict(W_=0), dict(W_=-1), dict(W_=n + 1), dict(S_=0), dict(S_=9), dict(C_=3), dict(C_=0), dict(n_fft_=100),
           dict(n_fft_=32), dict(n_fft_=32768), dict(hop_=0), dict(n_=128), dict(B_=0), dict(B_=65), dict(slab=-1))
    for kw in bad:                                                      # (W = 9: eight frames, a window without one)
        assert mom(**kw) == -1, kw
        assert L.dam_bandfit_workspace_bytes(*args(**kw)) == 0, kw
    for kw in (dict(x_=None), dict(y_=None), dict(win_=None), dict(tw_=None), dict(e_=None), dict(M_=None), dict(ws_=None)):
        assert mom(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(M == sentinel)                                     # nothing was launched
    assert mom() == 0
    torch.cuda.synchronize()
    assert torch.all(M == 0.0)
    G = 2
    g = torch.full((G, S, W), sentinel, dtype=torch.float64, device='cuda')
    r, t = (torch.full((G, W), sentinel, dtype=torch.float64, device='cuda') for _ in range(2))
    st = torch.full((G, W), 77, dtype=torch.int32, device='cuda')
    tot = torch.full((W,), sentinel, dtype=torch.float64, device='cuda')

    def sol(M_=M.data_ptr(), G_=G, W_=W, S_=S, pool=0, ridge=0.0, g_=g.data_ptr(), r_=r.data_ptr(), t_=t.data_ptr(), st_=st.data_ptr()):
        return L.dam_bandfit_solve_grouped(M_, G_, W_, S_, pool, ridge, g_, r_, t_, st_, None)
    for kw in (dict(M_=None), dict(g_=None), dict(r_=None), dict(t_=None), dict(st_=None), dict(G_=0), dict(W_=0), dict(S_=0),
               dict(S_=9), dict(pool=-1), dict(ridge=-1e-300), dict(ridge=float('nan'))):
        assert sol(**kw) == -1, kw

    def summ(r_=r.data_ptr(), t_=t.data_ptr(), st_=st.data_ptr(), G_=G, W_=W, tot_=tot.data_ptr()):
        return L.dam_bandfit_summary(r_, t_, st_, G_, W_, tot_, None)
    for kw in (dict(r_=None), dict(t_=None), dict(st_=None), dict(tot_=None), dict(G_=0), dict(W_=0)):
        assert summ(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(g == sentinel) and torch.all(r == sentinel) and torch.all(t == sentinel) and torch.all(st == 77)
    assert torch.all(tot == sentinel)
    assert sol() == 0 and summ() == 0                                   # silence: status 0, NaN gains, target 0, total NaN
    torch.cuda.synchronize()
    assert bool((st == 0).all()) and torch.isnan(g).all() and torch.isnan(r).all() and bool((t == 0.0).all()) and torch.isnan(tot).all()
    # the Python surface raises for the same, before the library is asked
    e3 = base['edges']
    for call in (lambda: gainfit.band_moments(x, y, 9, n_fft=256, edges=e3), lambda: gainfit.band_moments(x, y, 0, n_fft=256, edges=e3),
                 lambda: gainfit.band_moments(torch.zeros((9, n, C), dtype=torch.float32, device='cuda'), y, W, n_fft=256, edges=e3),
                 lambda: gainfit.band_moments(torch.zeros((S, n, 3), device='cuda'), torch.zeros((n, 3), device='cuda'), W, n_fft=256, edges=e3),
                 lambda: gainfit.band_moments(x, y, W, n_fft=100, edges=e3), lambda: gainfit.band_moments(x[:, :128], y[:128], 1, n_fft=256, edges=e3),
                 lambda: gainfit.band_moments(x, y, W, n_fft=256, edges=np.arange(66)),
                 lambda: gainfit.solve_bands(M[:, :, :, :3]), lambda: gainfit.solve_bands(M, pool=-1),
                 lambda: gainfit.band_residual_total(r, t[:1], st)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: gainfit.band_moments(x.to(torch.float16), y, W, n_fft=256, edges=e3), lambda: gainfit.solve_bands(M.float()),
                 lambda: gainfit.band_residual_total(r, t, st.long()),
                 lambda: ops.gainfit_band_moments(x, y, W, win, tw, 256, 128, edges.long())):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(RuntimeError, match='GPU only'):
        gainfit.fit_band_gains(x.cpu(), y.cpu(), W, n_fft=256, edges=e3)
