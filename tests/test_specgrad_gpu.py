"""GPU: the gradient of the spectrogram distance in the gains (csrc/dam_specgrad.hip) against the numpy float64 reference
(tests/_specgrad_ref.py).

Bounds.  Per entry |device - reference| <= the reference's bound: for the gradient the first-order propagation of the FFT's
2e-6 of the frame's peak (forward and inverse), of 1e-5 dB for the float32 log2 and of one float32 ulp of a 100 dB level through
u = (40 / ln 10) d X / p (the reference's docstring); for (S1, S2) the distance's own.  tests/test_specgrad_ref_cpu.py checks on
the sweep's very inputs that every entry's bound is at most 1e-2 of its row's largest entry.  torch.autograd.gradcheck is NOT
used: the levels are float32, so a finite difference of the device's own value is rounding noise.
Every test prints its largest error as a fraction of the bound before it asserts.
Largest |error| / bound seen on one MI355X, gradient | S1 | S2: 0.0016 | 0.0050 | 0.0059 at n_fft 64 (9 cases), 0.0024 | 0.0029 |
0.0034 at 256 (8 cases), 0.0022 | 0.0058 | 0.0066 at 2048 (6 cases), 0.0001 | 0.0004 | 0.0003 at 8192, 0.0004 | 0.0011 | 0.0012 at
16384; S2 against dam_specdist_sums 1.1e-12 of the bound apart, not bitwise equal; the chain rule through 10 ** (db / 20) to
1.5e-16."""
import numpy as np
import pytest
import torch

import _specgrad_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import ops, spectrum
    return ops, spectrum


def upload(stems, planar=False):
    """[clips, S, n, ch] numpy -> a CUDA tensor of that shape: interleaved storage, or planar [.., ch, n] storage transposed."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(np.swapaxes(stems, -1, -2))).cuda().transpose(-1, -2)
    return torch.from_numpy(np.ascontiguousarray(stems)).cuda()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_case(spectrum, c):
    """-> (S1 [clips, R], S2 [clips, R], grad [clips, R, S, G]) of the device, as sums (the divisions by N undone exactly
    enough: the reference's bound is six orders above a float64 ulp)."""
    mse, bias, grad = spectrum.spectrogram_distance_grad(upload(c['stems'], c['planar']), dev(c['gains']),
                                                         upload(c['ref_stems'], c['ref_planar']), dev(c['ref_gains']),
                                                         n_fft=c['n_fft'], hop=c['hop'])
    N = float(c['T'] * (c['n_fft'] // 2 + 1))
    return (bias * N).cpu().numpy(), (mse * N).cpu().numpy(), (grad * N).cpu().numpy()


def check_case(spectrum, c):
    """-> the largest |error| / bound of (grad, S1, S2); every entry asserted; the homogeneity identity on the device's own S1."""
    s1, s2, grad = run_case(spectrum, c)
    want = ref.gradient_clips(c['stems'], c['gains'], c['ref_stems'], c['ref_gains'], c['n_fft'], c['hop'])
    assert grad.shape == want['grad'].shape and grad.dtype == np.float64
    worst = [0.0, 0.0, 0.0]
    for r in range(grad.shape[1]):
        if r in c['zero_rows']:                      # an all-zero mix: every level is floor_db exactly, nothing has a derivative
            assert np.all(grad[:, r] == 0.0) and np.all(want['grad'][:, r] == 0.0)
            # d = floor_db - L_ref: the candidate's share of the bound on d is taken away (the FFT term of a zero frame is 0)
            continue
        gb = want['grad_bound'][:, r]
        ratio = np.abs(grad[:, r] - want['grad'][:, r]) / gb
        assert np.all(ratio <= 1.0), (c['n_fft'], c['hop'], c['n'], r, float(ratio.max()))
        worst[0] = max(worst[0], float(ratio.max()))
        # homogeneity: sum g dJ/dg = (40 / ln 10) S1 where nothing is floored -- against the device's own S1, within the
        # bounds of both sides and the reference's own difference (the float32 rounding of the mix signal and the frame)
        assert want['floored'][:, r].sum() == 0
        g = np.ones_like(grad[:, r]) if c['gains'] is None else c['gains'][:, r]
        lhs, rhs = (g * grad[:, r]).sum(axis=(1, 2)), ref.SCALE * s1[:, r]
        own = np.abs((g * want['grad'][:, r]).sum(axis=(1, 2)) - ref.SCALE * want['value'][:, r, 0])
        tol = (np.abs(g) * gb).sum(axis=(1, 2)) + ref.SCALE * want['value_bound'][:, r, 0] + own
        assert np.all(np.abs(lhs - rhs) <= tol), (c['n_fft'], c['hop'], c['n'], r)
    for i, got in enumerate((s1, s2)):
        ratio = np.abs(got - want['value'][..., i]) / want['value_bound'][..., i]
        assert np.all(ratio <= 1.0), (c['n_fft'], c['hop'], c['n'], i, float(ratio.max()))
        worst[1 + i] = max(worst[1 + i], float(ratio.max()))
    return worst


@pytest.mark.parametrize('n_fft', [64, 256, 2048])
def test_parity_sweep(env, n_fft):
    ops, spectrum = env
    cases = ref.sweep_cases(n_fft)
    worst = [0.0, 0.0, 0.0]
    for c in cases:
        worst = [max(a, b) for a, b in zip(worst, check_case(spectrum, c))]
    print('n_fft %d: %d cases, largest |d grad| / bound = %.4f, |dS1| / bound = %.4f, |dS2| / bound = %.4f'
          % (n_fft, len(cases), worst[0], worst[1], worst[2]))
    assert len(cases) >= 6


@pytest.mark.parametrize('n_fft', [8192, 16384])
def test_large_windows(env, n_fft):
    """The > 64 KB LDS path (PER 16 / 32): n = 2 n_fft + n_fft / 2 + 37, two gain nodes, the second owns exactly one frame."""
    ops, spectrum = env
    c = ref.large_case(n_fft)
    assert ref.frames_owned(c['n'], 2, n_fft, c['hop']).tolist() == [2, 1]
    worst = check_case(spectrum, c)
    print('n_fft %d, T = %d: largest |d grad| / bound = %.4f, |dS1| / bound = %.4f, |dS2| / bound = %.4f'
          % (n_fft, c['T'], worst[0], worst[1], worst[2]))


def bitwise_inputs(seed=5, n=256 * 9 + 5, S=3, S_ref=2, clips=3, n_gains=3):
    rng = np.random.default_rng(seed)
    return ref.noise_case(rng, S, S_ref, n, 2, np.float32, np.float32, 5, n_gains, 3, clips, 256)


def test_agreement_with_the_distance(env):
    """S2 against dam_specdist_sums with one band and one window on the same inputs: equal within the two bounds.  The two
    add the same per-bin d^2 in different orders (bins by lane and frame here, bins by band lane there), so they need not be
    bit for bit equal; the test prints whether they are.  An all-zero row's S2 is held to the same bound."""
    ops, spectrum = env
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=21, clips=1)
    n_fft, hop = 256, 77
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    mse, bias, _ = spectrum.spectrogram_distance_grad(x, g, y, h, n_fft=n_fft, hop=hop)
    sums, count = spectrum.spectrogram_distance(x[0], g[0], y[0], h[0], n_fft=n_fft, hop=hop)
    N = float(count.item())
    assert N == (1 + stems.shape[2] // hop) * (n_fft // 2 + 1)
    want = ref.gradient_clips(stems, gains, ref_stems, ref_gains, n_fft, hop)
    diff = np.abs((mse[0] * N - sums[:, 0, 0, 1]).cpu().numpy())
    diff1 = np.abs((bias[0] * N - sums[:, 0, 0, 0]).cpu().numpy())
    print('S2 against dam_specdist_sums: largest |difference| / bound = %.3g (S1: %.3g); bitwise equal: %s'
          % ((diff / want['value_bound'][0, :, 1]).max(), (diff1 / want['value_bound'][0, :, 0]).max(),
             bool(np.all(diff == 0.0) and np.all(diff1 == 0.0))))
    assert np.all(diff <= 2.0 * want['value_bound'][0, :, 1]) and np.all(diff1 <= 2.0 * want['value_bound'][0, :, 0])
    assert gains[0, 3].max() == 0.0 and want['value'][0, 3, 1] > 0.0                     # the all-zero row


def test_bitwise_properties(env):
    ops, spectrum = env
    n_fft, hop = 256, 77
    stems, gains, ref_stems, ref_gains = bitwise_inputs()
    n = stems.shape[2]
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    kw = dict(n_fft=n_fft, hop=hop)
    full = spectrum.spectrogram_distance_grad(x, g, y, h, **kw)
    again = spectrum.spectrogram_distance_grad(x, g, y, h, **kw)
    assert all(torch.equal(a, b) for a, b in zip(full, again))                          # two runs
    for r in range(5):                                                                  # a row alone / inside R = 5
        alone = spectrum.spectrogram_distance_grad(x, g[:, r:r + 1].contiguous(), y, h, **kw)
        assert all(torch.equal(a[:, 0], b[:, r]) for a, b in zip(alone, full)), r
    for c in range(3):                                                                  # a clip alone / inside 3
        alone = spectrum.spectrogram_distance_grad(x[c:c + 1], g[c:c + 1], y[c:c + 1], h[c:c + 1], **kw)
        assert all(torch.equal(a[0], b[c]) for a, b in zip(alone, full)), c
        plain = spectrum.spectrogram_distance_grad(x[c], g[c], y[c], h[c], **kw)      # (without the clip axis)
        assert all(torch.equal(a, b[c]) for a, b in zip(plain, full)), c
    planar = spectrum.spectrogram_distance_grad(upload(stems, True), g, upload(ref_stems, True), h, **kw)
    assert all(torch.equal(a, b) for a, b in zip(planar, full))                         # interleaved / planar
    # node 0 of 3 against rewritten samples that none of its frames covers.  A frame belongs to node 0 while its FIRST sample
    # lies in segment 0, so its last lies up to n_fft - 1 beyond the segment: everything from there on is rewritten (that is
    # more than n_fft / 2 beyond the segment; samples nearer than n_fft are covered by node 0's own frames and do move it)
    seg = n // 3
    last = max(t for t in range(1 + n // hop) if max(t * hop - n_fft // 2, 0) < seg)
    cut = last * hop + n_fft // 2
    assert seg + n_fft // 2 < cut <= seg + n_fft and cut < 2 * seg
    rng = np.random.default_rng(6)
    s2, r2 = stems.copy(), ref_stems.copy()
    for a in (s2, r2):
        a[:, :, cut:] = 0.1 * rng.standard_normal(a[:, :, cut:].shape)
    moved = spectrum.spectrogram_distance_grad(upload(s2), g, upload(r2), h, **kw)[2]
    assert torch.equal(moved[..., 0], full[2][..., 0])
    live = [r for r in range(5) if r != 3]
    assert not torch.equal(moved[:, live][..., 1], full[2][:, live][..., 1])
    assert not torch.equal(moved[:, live][..., 2], full[2][:, live][..., 2])
    assert torch.all(full[2][:, 3] == 0.0)                                              # the all-zero row
    print('bitwise: two runs, row alone, clip alone, planar, node 0 against far samples: all equal')


def test_graph_capture_and_replay(env):
    ops, spectrum = env
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=10)
    kw = dict(n_fft=256, hop=77)
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        spectrum.spectrogram_distance_grad(x, g, y, h, **kw)                            # the tables become resident
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = spectrum.spectrogram_distance_grad(x, g, y, h, **kw)
    x.mul_(0.5)
    y.copy_(y.flip(1))
    g.copy_(g.flip(1))
    graph.replay()
    torch.cuda.synchronize()
    eager = spectrum.spectrogram_distance_grad(x.clone(), g.clone(), y.clone(), h, **kw)
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    first = spectrum.spectrogram_distance_grad(upload(stems), dev(gains), upload(ref_stems), dev(ref_gains), **kw)
    assert not torch.equal(first[2], out[2])
    print('graph: captured, replayed on rewritten stems, bitwise the eager result')


def test_autograd(env):
    """(No torch.autograd.gradcheck: float32 levels make its finite differences meaningless; the formula is held to finite
    differences in float64 by tests/test_specgrad_ref_cpu.py and the device to the formula by the sweep.)"""
    ops, spectrum = env
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=11, clips=1)
    x, y, h = upload(stems)[0], upload(ref_stems)[0], dev(ref_gains)[0]
    live = gains[0, [0, 1, 2, 4]]
    g = dev(live).requires_grad_(True)
    mse, _, grad_mse = spectrum.spectrogram_distance_grad(x, g.detach(), y, h, n_fft=256, hop=77)
    loss = spectrum.rendered_spectrogram_mse(x, g, y, h, n_fft=256, hop=77)
    assert torch.equal(loss, mse) and loss.requires_grad
    loss.sum().backward()
    assert torch.equal(g.grad, grad_mse)
    # through 10 ** (db / 20): the leaf's gradient is the chain rule on the device's grad_mse, weighted by the upstream gradient
    db = (20.0 * torch.log10(dev(live))).requires_grad_(True)
    weight = torch.tensor([1.0, -2.0, 0.5, 3.0], dtype=torch.float64, device='cuda')
    lin = (10.0 ** (db / 20.0)).double()
    (spectrum.rendered_spectrogram_mse(x, lin, y, h, n_fft=256, hop=77) * weight).sum().backward()
    grad_lin = spectrum.spectrogram_distance_grad(x, lin.detach(), y, h, n_fft=256, hop=77)[2]
    want = weight[:, None, None] * grad_lin * lin.detach() * (np.log(10.0) / 20.0)
    rel = ((db.grad - want).abs().max() / want.abs().max()).item()
    print('autograd through 10 ** (db / 20): largest |leaf gradient - chain rule| = %.3g of the largest entry' % rel)
    assert rel <= 1e-12
    assert torch.allclose(want, weight[:, None, None] * spectrum.gain_sensitivity_db(lin.detach(), grad_lin), rtol=1e-14, atol=0)
    # [S] gains: one row, one node
    g1 = torch.tensor([0.7, 1.1, 0.9], dtype=torch.float64, device='cuda', requires_grad=True)
    one = spectrum.rendered_spectrogram_mse(x, g1, y, h, n_fft=256, hop=77)
    one.sum().backward()
    assert tuple(one.shape) == (1,) and tuple(g1.grad.shape) == (3,)
    assert torch.equal(g1.grad, spectrum.spectrogram_distance_grad(x, g1.detach(), y, h, n_fft=256, hop=77)[2].reshape(3))


def test_argument_errors(env, dam_lib):
    ops, spectrum = env
    from deep_audio_mixer_amd import features
    stems, gains, ref_stems, ref_gains = bitwise_inputs(seed=12)
    x, g, y, h = upload(stems), dev(gains), upload(ref_stems), dev(ref_gains)
    n = x.shape[2]
    good = dict(n_fft=256, hop=77)
    spectrum.spectrogram_distance_grad(x, g, y, h, **good)
    many = torch.ones(3, 5, 3, 10, dtype=torch.float64, device='cuda')                  # n // 10 = 230 < 256
    for exc, args, change in [
            (ValueError, (x, g, y[:, :, :-1], h), {}), (ValueError, (x, g, y, h), dict(n_fft=100)),
            (ValueError, (x, g, y, h), dict(hop=0)), (ValueError, (x, g, y, h), dict(amin=0.0)),
            (ValueError, (x, g[:, :, :2], y, h), {}), (ValueError, (x, g, y, h[:, :1]), {}), (ValueError, (x[0, 0], g, y, h), {}),
            (ValueError, (x, g[:2], y, h), {}), (ValueError, (x, g, y[:2], h), {}), (ValueError, (x, many, y, h), {}),
            (TypeError, (x, g.float(), y, h), {}), (TypeError, (x.half(), g, y, h), {}), (TypeError, (x, g, y, h), dict(n_fft=256.0)),
            (RuntimeError, (x.cpu(), g, y, h), {}), (RuntimeError, (x, g.cpu(), y, h), {}), (RuntimeError, (x, g, y.cpu(), h), {}),
            (ValueError, (x[:, :, :128], None, y[:, :, :128], None), {})]:
        with pytest.raises(exc):
            spectrum.spectrogram_distance_grad(*args, **dict(good, **change))
    # the raw C entry: DAM_ERR_BAD_ARG / DAM_ERR_UNSUPPORTED before any launch, nothing written
    win, tw = features._get_tables(x.device, 256)
    T = 1 + n // 77
    value = torch.full((3, 5, 2), -7.0, dtype=torch.float64, device='cuda')
    grad = torch.full((3, 5, 3, 3), -7.0, dtype=torch.float64, device='cuda')
    ws = torch.full((3 * 5 * T * 4 * 2,), -7.0, dtype=torch.float64, device='cuda')
    P = lambda t: None if t is None else t.data_ptr()
    base = dict(x=P(x), xk=0, clips=3, R=5, S=3, ch=2, n=n, xcs=x.stride(0), ss=x.stride(1), ps=x.stride(2), cs=x.stride(3), g=P(g),
                ng=3, y=P(y), yk=0, Sr=y.shape[1], chr=y.shape[3], rcls=y.stride(0), rss=y.stride(1), rps=y.stride(2),
                rcs=y.stride(3), h=P(h), nh=3, win=P(win), tw=P(tw), n_fft=256, hop=77, amin=1e-5, value=P(value), grad=P(grad),
                ws=P(ws), stream=None)
    call = lambda **kw: dam_lib.dam_specgrad(*dict(base, **kw).values())
    size = lambda geo: dam_lib.dam_specgrad_workspace_bytes(geo['clips'], geo['R'], geo['S'], geo['n'], geo['n_fft'], geo['hop'],
                                                            geo['ng'])
    assert size(base) == ws.numel() * 8
    bad = [dict(x=None), dict(y=None), dict(win=None), dict(tw=None), dict(value=None), dict(grad=None), dict(ws=None),
           dict(clips=0), dict(clips=65536), dict(R=0), dict(R=65536), dict(S=0), dict(Sr=0), dict(ch=3), dict(chr=0),
           dict(n_fft=100), dict(n_fft=32), dict(n_fft=32768), dict(hop=0), dict(n=128), dict(ng=0), dict(ng=n + 1), dict(nh=0),
           dict(amin=0.0), dict(amin=-1.0), dict(amin=float('nan'))]
    for change in bad:
        assert call(**change) == -1, change                                  # DAM_ERR_BAD_ARG
        if any(k in change for k in ('clips', 'R', 'S', 'n', 'n_fft', 'hop')) or change == dict(ng=n + 1):
            assert size(dict(base, **change)) == 0, change
    assert call(ng=10) == -2 and size(dict(base, ng=10)) == 0                # DAM_ERR_UNSUPPORTED: n // 10 = 230 < n_fft
    torch.cuda.synchronize()
    value.fill_(-7.0); grad.fill_(-7.0); ws.fill_(-7.0)
    for change in bad + [dict(ng=10)]:
        call(**change)
    torch.cuda.synchronize()
    assert torch.all(value == -7.0) and torch.all(grad == -7.0) and torch.all(ws == -7.0)
    assert call() == 0                                                       # the same arguments unchanged: accepted
    torch.cuda.synchronize()
    mse, bias, grad_mse = spectrum.spectrogram_distance_grad(x, g, y, h, **good)
    N = float(T * 129)
    assert torch.equal(value[..., 1] / N, mse) and torch.equal(value[..., 0] / N, bias) and torch.equal(grad / N, grad_mse)
