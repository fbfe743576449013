"""GPU: the band-gain mixer (csrc/dam_bandmix.hip, gainfit.render_band_gains) against the numpy float64 reference
(tests/_bandmix_ref.py).

Bound: max |y - ref64| <= c, c = 8 x max |ref32 - ref64| on the same case -- the device's arithmetic is float32, the reference's
float64, so the test measures what float32 costs (the same reference with float32 frames, scipy's float32 rfft / irfft, a
complex64 mix spectrum and a float32 overlap-add) and allows 8 times that, the band-fit tests' allowance for another
factorisation of the FFT.  Everything else (two runs, graph replays, a channel of its own, the storage layout, float64 stems
that hold float32 values, the NaN rule, a window against the other windows' gains) is bitwise.  Every test prints its figures
before it asserts.
Largest observed (1 x MI355X): 0.155 of c on the odd-hop case (c = 8.7e-7), 0.097 .. 0.145 of c on the other seven
(c = 8.0e-7 .. 3.3e-5, max |y - ref64| <= 3.8e-6 at a peak of 2.0); two-band case on the device's own fit and render: 1.4e-6 of the
mix's energy left against a broadband residual of 3.5e-2 (4.0e-5 of it), 6.0e-5 with fill = 0."""
import numpy as np
import pytest
import torch

import _bandfit_ref as bref
import _bandmix_ref as ref
from test_bandmix_ref_cpu import SR, WIDE, stems_of, third_octaves
from test_gainfit_gpu import bits_equal, up_mix, up_stems

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import gainfit, ops
    assert ops.GAINFIT_BAND_MAX_BANDS == dam_lib.dam_spectrum_max_bands()
    return gainfit, ops


def planted(seed, B, S, W):
    """Random gains in 0.5 .. 1.5 with NaNs planted, and a fill [S, W] with one more where there is room."""
    rng = np.random.default_rng(seed)
    gains, fill = rng.uniform(0.5, 1.5, (B, S, W)), rng.uniform(0.5, 1.5, (S, W))
    gains[rng.uniform(size=gains.shape) < 0.1] = np.nan
    gains[B // 2, S - 1, W - 1] = np.nan
    if S * W > 1:
        fill[S - 1, W - 1] = np.nan                                     # under the planted NaN: that cell renders 0
    return gains, fill


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


CASES = [  # S, C, n, n_fft, hop (the six geometries of the CPU test, then S = 8), W, stem dtype, planar, edges (None: third octaves)
    (3, 2, 6007, 256, 128, 5, F32, True, None),
    (2, 1, 6007, 256, 77, 3, F64, False, WIDE),                         # an odd hop; bins outside every band
    (4, 2, 129, 256, 128, 1, F32, False, None),                         # n = n_fft / 2 + 1: two frames, all reflection
    (1, 1, 6007, 64, 32, 5, F32, True, None),
    (2, 2, 6007, 2048, 1024, 3, F64, True, None),                       # four bins a thread
    (1, 1, 20000, 16384, 8192, 3, F32, True, None),                     # 32 bins a thread, 128 KB of LDS, a frame per window
    (8, 2, 6007, 256, 128, 5, F64, False, WIDE),
    (8, 1, 6007, 2048, 1024, 1, F32, True, None),
]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_render_against_reference(env, case):
    gainfit, ops = env
    S, C, n, n_fft, hop, W, xd, planar, edges = CASES[case]
    if edges is None:
        edges = third_octaves(n_fft)
    B = len(edges) - 1
    x = stems_of(400 + case, S, n, C, xd)
    gains, fill = planted(500 + case, B, S, W)
    y = gainfit.render_band_gains(up_stems(x, planar), dev(gains), n_fft=n_fft, hop=hop, edges=edges, fill=dev(fill))
    assert y.dtype == torch.float32 and tuple(y.shape) == (C, n) and y.is_cuda and y.is_contiguous()
    want = ref.render(x, gains, fill, edges, n_fft, hop)
    c = 8.0 * float(np.abs(ref.render(x, gains, fill, edges, n_fft, hop, transform='f32') - want).max())
    worst = float(np.abs(y.cpu().numpy().astype(np.float64) - want).max())
    print('S %d C %d n %d n_fft %d hop %d W %d %s %s, %d bands: c = %.3g, max |y - ref64| = %.3g = %.3f of c (max |ref| %.3g)'
          % (S, C, n, n_fft, hop, W, xd.__name__, 'planar' if planar else 'interleaved', B, c, worst, worst / c,
             np.abs(want).max()))
    assert c > 0.0 and worst <= c


@pytest.fixture(scope='module')
def base(env):
    gainfit, ops = env
    S, C, n, W, n_fft, hop = 4, 2, 6007, 5, 256, 128
    x = stems_of(450, S, n, C)
    edges = third_octaves(n_fft)
    gains, fill = planted(550, len(edges) - 1, S, W)
    kw = dict(n_fft=n_fft, hop=hop, edges=edges)
    dx, dg, df = up_stems(x, True), dev(gains), dev(fill)
    return dict(x=x, gains=gains, fill=fill, edges=edges, kw=kw, dx=dx, dg=dg, df=df, n=n, W=W, n_fft=n_fft,
                y=gainfit.render_band_gains(dx, dg, fill=df, **kw))


def test_bitwise_properties(env, base):
    gainfit, ops = env
    x, gains, fill, kw, dx, dg, df, y = (base[k] for k in ('x', 'gains', 'fill', 'kw', 'dx', 'dg', 'df', 'y'))
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0.1
    assert bits_equal(gainfit.render_band_gains(dx, dg, fill=df, **kw), y)                          # two runs
    out = torch.full_like(y, 7.0)
    assert gainfit.render_band_gains(dx, dg, fill=df, out=out, **kw) is out and bits_equal(out, y)
    mono = gainfit.render_band_gains(dx[:, :, :1], dg, fill=df, **kw)                               # channel 0 on its own
    assert tuple(mono.shape) == (1, base['n']) and bits_equal(mono[0], y[0]) and not bits_equal(mono[0], y[1])
    assert bits_equal(gainfit.render_band_gains(up_stems(x, False), dg, fill=df, **kw), y)          # interleaved storage
    assert bits_equal(gainfit.render_band_gains(up_stems(x.astype(F64), True), dg, fill=df, **kw), y)   # float64 of the same values
    g2, f2 = ref.substituted(gains, fill)                                                           # the NaN rule
    assert np.isnan(gains).sum() >= 3 and np.isnan(fill).sum() == 1
    assert bits_equal(gainfit.render_band_gains(dx, dev(g2), fill=dev(f2), **kw), y)
    # fill as a number, [S] and [S, 1]: the same table spelled out
    col = np.where(np.isfinite(fill[:, :1]), fill[:, :1], 0.0)
    wide = gainfit.render_band_gains(dx, dg, fill=dev(np.repeat(col, base['W'], axis=1)), **kw)
    assert bits_equal(gainfit.render_band_gains(dx, dg, fill=dev(col), **kw), wide)
    assert bits_equal(gainfit.render_band_gains(dx, dg, fill=dev(col[:, 0]), **kw), wide)
    assert bits_equal(gainfit.render_band_gains(dx, dg, fill=0.75, **kw),
                      gainfit.render_band_gains(dx, dg, fill=dev(np.full_like(fill, 0.75)), **kw))


def test_a_window_does_not_see_the_other_windows_gains(env, base):
    gainfit, ops = env
    n, W, n_fft, kw, y = base['n'], base['W'], base['n_fft'], base['kw'], base['y']
    seg = n // W
    for w in (0, 2, W - 1):
        g2, f2 = base['gains'].copy(), base['fill'].copy()
        others = [v for v in range(W) if v != w]
        g2[:, :, others] = g2[:, :, others] * 0.5 + 0.125
        f2[:, others] = f2[:, others] * 2.0
        other = gainfit.render_band_gains(base['dx'], dev(g2), fill=dev(f2), **kw)
        lo = 0 if w == 0 else w * seg + n_fft // 2
        hi = n if w == W - 1 else (w + 1) * seg - n_fft // 2
        assert hi - lo >= seg - n_fft
        assert bits_equal(other[:, lo:hi], y[:, lo:hi]), w
        changed = (other != y).any(0).cpu().numpy()
        # (and the rest of the song did change, but for the less than a hop on either side that no other window's frame reaches)
        assert not changed[lo:hi].any() and changed[np.r_[0:lo, hi:n]].mean() > 0.9, w


def test_capture_and_replay(env, base):
    gainfit = env[0]
    kw = base['kw']
    buf, gbuf, fbuf = base['dx'].clone(), base['dg'].clone(), base['df'].clone()
    out = torch.empty_like(base['y'])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gainfit.render_band_gains(buf, gbuf, fill=fbuf, out=out, **kw)  # the tables are resident after this call
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gainfit.render_band_gains(buf, gbuf, fill=fbuf, out=out, **kw)
    for scale in (0.5, 1.75):
        new = (base['dx'] * scale).contiguous()
        new[1].mul_(1.5)
        buf.copy_(new)                                                  # the stems and the gains rewritten in place
        gbuf.copy_(base['dg'] * scale)
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out, gainfit.render_band_gains(new.clone(), base['dg'] * scale, fill=base['df'], **kw))
    print('render_band_gains in a graph: two replays on rewritten stems and gains, bitwise the eager results')


def test_workspace_and_argument_errors(env, base):
    gainfit, ops = env
    from deep_audio_mixer_amd import features, spectrum
    L = ops._lib.lib()
    for C, n, n_fft, hop in [(g[1], g[2], g[3], g[4]) for g in CASES] + [(2, 44100 * 240, 4096, 2048), (1, 6007, 64, 1)]:
        need = L.dam_bandmix_workspace_bytes(n, C, n_fft, hop)
        assert 0 < need <= 4 * C * (1 + n // hop) * n_fft + 256, (C, n, n_fft, hop)
    S, n, C, W, n_fft, hop, B = 3, 1000, 2, 3, 256, 128, 4
    x = torch.zeros((S, n, C), dtype=torch.float32, device='cuda')
    g = torch.ones((B, S, W), dtype=torch.float64, device='cuda')
    f = torch.ones((S, W), dtype=torch.float64, device='cuda')
    win, tw = features._get_tables(x.device, n_fft)
    edges = torch.tensor([0, 4, 20, 60, 129], dtype=torch.int32, device='cuda')
    sentinel = -7.0
    out = torch.full((C, n), sentinel, dtype=torch.float32, device='cuda')
    need = L.dam_bandmix_workspace_bytes(n, C, n_fft, hop)
    ws = torch.zeros(need // 4, dtype=torch.float32, device='cuda')

    def call(x_=x.data_ptr(), g_=g.data_ptr(), f_=f.data_ptr(), e_=edges.data_ptr(), win_=win.data_ptr(), tw_=tw.data_ptr(),
             out_=out.data_ptr(), ws_=ws.data_ptr(), S_=S, C_=C, n_=n, W_=W, n_fft_=n_fft, hop_=hop, B_=B, bytes_=need):
        return L.dam_bandmix_render(x_, 0, S_, C_, n_, n * C, C, 1, g_, f_, e_, B_, W_, win_, tw_, n_fft_, hop_, out_, ws_, bytes_, None)
    bad = (dict(W_=9), dict(W_=0), dict(W_=-1), dict(W_=n + 1), dict(S_=0), dict(S_=9), dict(C_=3), dict(C_=0), dict(n_fft_=100),
           dict(n_fft_=32), dict(n_fft_=32768), dict(hop_=0), dict(n_=128), dict(B_=0), dict(B_=65), dict(x_=None), dict(g_=None),
           dict(f_=None), dict(e_=None), dict(win_=None), dict(tw_=None), dict(out_=None), dict(ws_=None))
    for kw in bad:                                                      # (W = 9: eight frames, a window without one)
        assert call(**kw) == -1, kw
    for kw in (dict(C_=3), dict(n_fft_=100), dict(hop_=0), dict(n_=128), dict(hop_=129)):
        assert L.dam_bandmix_workspace_bytes(kw.get('n_', n), kw.get('C_', C), kw.get('n_fft_', n_fft), kw.get('hop_', hop)) == 0, kw
    assert call(hop_=129) == -2 and call(hop_=256) == -2                # DAM_ERR_UNSUPPORTED: dam_istft_f32's rule
    assert call(bytes_=need - 1) == -4 and call(bytes_=0) == -4         # DAM_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.all(out == sentinel)                                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)
    # the Python surface raises for the same, before the library is asked
    e3 = third_octaves(256)
    g3 = torch.ones((len(e3) - 1, S, W), dtype=torch.float64, device='cuda')
    dev_e3 = spectrum._device_edges(e3, 256, x.device)
    with pytest.raises(ValueError, match='workspace'):
        ops.bandmix_render(x, g3, f, dev_e3, win, tw, 256, 128, workspace=ws[:-1])
    for call_ in (lambda: gainfit.render_band_gains(x, g3, n_fft=256, hop=129, edges=e3),
                  lambda: gainfit.render_band_gains(x, g3[:, :2], n_fft=256, edges=e3),
                  lambda: gainfit.render_band_gains(x, g3, n_fft=256, edges=e3, fill=f[:, :2]),
                  lambda: gainfit.render_band_gains(x, g3[:, :, :1].expand(-1, -1, 9), n_fft=256, edges=e3),    # a window without a frame
                  lambda: gainfit.render_band_gains(x, g3, n_fft=256, edges=e3, out=out[:1])):
        with pytest.raises(ValueError):
            call_()
    for call_ in (lambda: gainfit.render_band_gains(x, g3.float(), n_fft=256, edges=e3),
                  lambda: gainfit.render_band_gains(x, g3, n_fft=256, edges=e3, fill=f.float()),
                  lambda: gainfit.render_band_gains(x.to(torch.float16), g3, n_fft=256, edges=e3)):
        with pytest.raises(TypeError):
            call_()
    with pytest.raises(RuntimeError, match='GPU only'):
        gainfit.render_band_gains(x.cpu(), g3, n_fft=256, edges=e3)
    with pytest.raises(RuntimeError, match='GPU only'):
        gainfit.render_band_gains(x, g3.cpu(), n_fft=256, edges=e3)


def test_two_band_case_closes_the_loop_on_the_device(env):
    gainfit = env[0]
    x, y, a, b = bref.two_band_case()
    edges = third_octaves(256)
    dx, dy = up_stems(x, True), up_mix(y, True)
    gains = gainfit.fit_band_gains(dx, dy, 1, n_fft=256, hop=128, edges=edges)[0]
    broad_gains, broad_residual, _ = gainfit.fit_gains(dx, dy, 1)
    rendered = gainfit.render_band_gains(dx, gains, n_fft=256, hop=128, edges=edges, fill=broad_gains)
    share, broadband = ref.residual_share(y, rendered.cpu().numpy()), float(broad_residual[0])
    silent = ref.residual_share(y, gainfit.render_band_gains(dx, gains, n_fft=256, hop=128, edges=edges, fill=0.0).cpu().numpy())
    print('two-band case on the device: the render of the fitted band gains leaves %.3g of the mix against a broadband residual '
          'of %.3g (%.3g of it); with fill = 0: %.3g' % (share, broadband, share / broadband, silent))
    assert share <= 1e-3 * broadband
