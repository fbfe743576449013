"""GPU: the look-ahead true-peak limiter (dam_limiter_apply) against the numpy definition (tests/_limiter_ref.py) evaluated
with the taps the library exports.

Tolerance.  The meter's own bound is |d_dev - d_ref| <= 1e-13 * max|xs| (tests/test_truepeak_gpu.py).  r = min(1, ceil / d)
moves only where d >= ceil, where |dr| = ceil |dd| / d^2 <= |dd| / ceil; a minimum and a mean of such values move no more,
and the mean's own rounding ((L+1) * 1.1e-16 <= 6e-14 at the cap, relative to g <= 1) is the same on both sides up to the
order of identical additions -- the kernel adds in the reference's order.  So
    |g_dev - g_ref| <= TOL_G = 1e-13 * max(1, max|xs| / ceil),
    |out_dev - out_ref| <= TOL_G * max|xs| + one ulp of the output dtype,   |min_gain_dev - min_gain_ref| <= TOL_G.
n_limited counts g < 1: a sample whose reference g is within TOL_G below 1, or whose window holds a demand within
1e-13 * max|xs| of the ceiling, may fall on either side and is excluded -- at most 0.1 % of a row, asserted (0 on these
inputs: bursts are clearly over the ceiling, the bed clearly under).
Largest observed errors (1 x MI355X, the parity cases): |dout| 0.0041 of its bound, |dmin_gain| 0.00084 of its bound, no
sample excluded.  Each test prints its figures beside the bound before asserting."""
import ctypes

import numpy as np
import pytest
import torch

import _limiter_ref as ref
from test_truepeak_gpu import burst

pytestmark = pytest.mark.gpu

CEILING_DB = -1.0
CEILING = 10.0 ** (CEILING_DB / 20.0)
BAD_ARG = -1                                         # DAM_ERR_BAD_ARG


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import ops
    h = (ctypes.c_double * 49)()
    assert dam_lib.dam_true_peak_taps_host(h) == 0
    taps = np.array(list(h))
    taps.setflags(write=False)
    T, max_l, max_h = (int(v) for v in ops.limiter_geometry())
    assert max_l >= 512 and max_h >= 4096
    return ops, taps, T, max_l, max_h, dam_lib


def device_view(x, planar):
    """x numpy [N, n, ch] -> CUDA tensor of that shape, stored interleaved or as a transposed view of planar [N, ch, n]."""
    if planar:
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(ops, x, L, H, planar=False, out_dtype=torch.float64, pre_gain=None):
    """x numpy [N, n, ch] -> (out numpy [N, n, ch], min_gain [N], n_limited [N])."""
    pg = None if pre_gain is None else torch.from_numpy(np.asarray(pre_gain, dtype=np.float64)).cuda()
    out, mg, nl = ops.limiter_apply(device_view(x, planar), CEILING_DB, L, H, pre_gain=pg, out_dtype=out_dtype)
    assert out.dtype == out_dtype and tuple(out.shape) == (x.shape[0], x.shape[2], x.shape[1])
    assert mg.dtype == torch.float64 and nl.dtype == torch.int64
    return out.transpose(1, 2).cpu().numpy(), mg.cpu().numpy(), nl.cpu().numpy()


def make_input(n, ch, dtype, T, L, H, seed):
    """A bed clearly under the ceiling with bursts clearly over it: at both ends of the row, around the first tile boundary,
    and as pairs H - 1 and H + L + 1 apart that straddle a tile boundary (positions past the row are dropped)."""
    rng = np.random.default_rng(seed)
    x = 0.04 * rng.standard_normal((n, ch))
    b = 2.5 * burst()
    near, far = T - (H - 1) // 2, 2 * T - (H + L + 1) // 2
    centres = [0, n - 1, T - 1, T, T + 6, near, near + H - 1, far, far + H + L + 1]
    if far + H + L + 1 >= n:                         # the wider pair does not fit behind the second boundary: try the first
        far = T - (H + L + 1) // 2
        centres[-2:] = [far, far + H + L + 1]
    for k, centre in enumerate(centres):
        if 0 <= centre < n:
            lo = centre - len(b) // 2
            a, z = max(lo, 0), min(lo + len(b), n)
            x[a:z, k % ch] = b[a - lo: z - lo]        # (set, not added: overlapping bursts must not cancel)
    return x.astype(dtype)


def check(x, got, want, tag=''):
    """Asserts one row set's device results (out [n, ch] of any float dtype, min_gain, n_limited) against the reference dict;
    returns (|dout| beyond the output ulp as a fraction of its bound, |dmin_gain| / TOL_G, the excluded share)."""
    out, min_gain, n_limited = got
    n = x.shape[0]
    peak = np.abs(want['xs']).max()
    tol_g = 1e-13 * max(1.0, peak / CEILING)
    ulp = np.spacing(np.abs(want['out']).astype(out.dtype)).astype(np.float64)
    err = (np.abs(out.astype(np.float64) - want['out']) - ulp).max() / (tol_g * peak)
    g = want['g']
    sure = int((g < 1.0 - tol_g).sum())
    doubtful = (g >= 1.0 - tol_g) & (g < 1.0)
    edge = np.flatnonzero(np.abs(want['d'] - CEILING) <= 1e-13 * peak)
    for k in edge:                                   # every g whose window [i - H - L, i + L] holds such a demand
        doubtful[max(0, k - want['L']): k + want['H'] + want['L'] + 1] = True
    doubtful &= g >= 1.0 - tol_g
    excluded = int(doubtful.sum())
    assert err <= 1.0, (tag, 'out', err)
    assert abs(min_gain - want['min_gain']) <= tol_g, (tag, 'min_gain', min_gain, want['min_gain'])
    assert excluded <= 1e-3 * n, (tag, 'excluded', excluded, n)
    assert sure <= n_limited <= sure + excluded, (tag, 'n_limited', n_limited, sure, excluded)
    return max(err, 0.0), abs(min_gain - want['min_gain']) / tol_g, excluded / n


def reference(x, L, H, taps, pre_gain=None):
    want = ref.limit(x, CEILING, L, H, pre_gain=pre_gain, h=taps)
    want['L'], want['H'] = L, H
    return want


WINDOWS = ['1,1', '2,3', '40,160', 'max']
LENGTHS = ['1', '2', 'L', 'L+1', 'T-1', 'T', 'T+1', '2T+3']


@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('window', WINDOWS)
def test_parity_with_the_definition(env, window, length):
    ops, taps, T, max_l, max_h, _ = env
    L, H = (max_l, max_h) if window == 'max' else (int(v) for v in window.split(','))
    n = {'L': L, 'L+1': L + 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+3': 2 * T + 3}.get(length) or int(length)
    worst = [0.0, 0.0, 0.0]
    limited = 0
    for ch in (1, 2, 3):
        for dtype in (np.float32, np.float64):
            x = make_input(n, ch, dtype, T, L, H, seed=n * 7 + ch)
            want = reference(x, L, H, taps)
            limited = max(limited, want['n_limited'])
            for out_dtype in (torch.float32, torch.float64):
                out, mg, nl = run(ops, x[None], L, H, planar=ch == 2, out_dtype=out_dtype)
                figures = check(x, (out[0], mg[0], int(nl[0])), want, (ch, dtype.__name__, out_dtype))
                worst = [max(a, b) for a, b in zip(worst, figures)]
    print('L %d H %d n %d: |dout| %.3g of its bound, |dmin_gain| %.3g of its bound, excluded share %.3g (bound 1e-3); up to %d '
          'samples limited' % (L, H, n, worst[0], worst[1], worst[2], limited))
    assert limited > 0


def test_row_under_the_ceiling_is_returned_bitwise(env):
    ops, _, T, _, _, _ = env
    n = 2 * T + 3
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal((1, n, 2))).astype(np.float32)
    gain = 1.7
    for out_dtype, np_dtype in ((torch.float64, np.float64), (torch.float32, np.float32)):
        out, mg, nl = run(ops, x, 40, 160, out_dtype=out_dtype, pre_gain=[gain])
        xs = (x.astype(np.float64) * gain).astype(np_dtype)
        print('under the ceiling (%s out): %d samples differ from xs (bound 0), min_gain %r, n_limited %d'
              % (np_dtype.__name__, int((out != xs).sum()), mg[0], nl[0]))
        assert np.array_equal(out, xs) and mg[0] == 1.0 and nl[0] == 0


def test_a_row_set_does_not_depend_on_its_batch(env):
    ops, taps, T, _, _, _ = env
    n, L, H = 2 * T + 3, 40, 160
    sets = np.stack([make_input(n, 2, np.float32, T, L, H, seed=s) * (1.0 + 0.3 * s) for s in range(5)])
    alone = [run(ops, sets[s:s + 1], L, H, planar=True) for s in range(5)]
    order = [3, 0, 4, 1, 2]
    out, mg, nl = run(ops, sets[order], L, H, planar=True)
    differ = sum(int((out[k] != alone[s][0][0]).sum()) for k, s in enumerate(order))
    print('permuted batch of five: %d samples differ from the row sets alone (bound 0); min gains %s' % (differ, mg.tolist()))
    for k, s in enumerate(order):
        assert np.array_equal(out[k], alone[s][0][0]) and mg[k] == alone[s][1][0] and nl[k] == alone[s][2][0]
    assert len(set(mg.tolist())) == 5 and nl.min() > 0               # the sets do differ
    check(sets[3], (out[0], mg[0], int(nl[0])), reference(sets[3], L, H, taps))


def test_pre_gain_is_the_same_as_scaled_input(env):
    ops, _, T, _, _, _ = env
    n, L, H = T + 1, 40, 160
    for dtype in (np.float32, np.float64):
        x = make_input(n, 2, dtype, T, L, H, seed=9)[None]
        a = run(ops, x, L, H, pre_gain=[2.0])
        b = run(ops, (2 * x).astype(dtype), L, H)
        print('%s: pre_gain 2 on x against 2x: %d samples differ (bound 0), min_gain %r / %r'
              % (dtype.__name__, int((a[0] != b[0]).sum()), a[1][0], b[1][0]))
        assert np.array_equal(a[0], b[0]) and a[1][0] == b[1][0] and a[2][0] == b[2][0] and a[2][0] > 0


def test_graph_capture(env):
    ops, _, T, _, _, _ = env
    n, L, H = 2 * T + 3, 40, 160
    contents = [torch.from_numpy(make_input(n, 2, np.float32, T, L, H, seed=s)[None] * (1.0 + s)).cuda() for s in (1, 2)]
    eager = [ops.limiter_apply(c, CEILING_DB, L, H) for c in contents]
    x = torch.empty_like(contents[0])
    gain = torch.ones(1, dtype=torch.float64, device='cuda')
    ws = torch.empty(ops._lib.lib().dam_limiter_workspace_bytes(1, n) // 8, dtype=torch.float64, device='cuda')
    out = torch.empty((1, 2, n), dtype=torch.float64, device='cuda')
    mg, nl = torch.empty(1, dtype=torch.float64, device='cuda'), torch.empty(1, dtype=torch.int64, device='cuda')

    def body():
        ops.limiter_apply(x, CEILING_DB, L, H, pre_gain=gain, out=out, min_gain_out=mg, n_limited_out=nl, workspace=ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for c, (want_out, want_mg, want_nl) in zip(contents, eager):
        x.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        print('replay: %d samples differ from the eager call (bound 0), n_limited %d / %d'
              % (int((out != want_out).sum()), int(nl[0]), int(want_nl[0])))
        assert torch.equal(out, want_out) and torch.equal(mg, want_mg) and torch.equal(nl, want_nl)
    assert int(eager[0][2][0]) > 0 and not torch.equal(eager[0][0], eager[1][0])


def test_argument_errors(env):
    ops, _, T, max_l, max_h, lib = env
    n = 64
    x = torch.zeros((2, n), dtype=torch.float32, device='cuda')
    out = torch.zeros((2, n), dtype=torch.float64, device='cuda')
    ws = torch.zeros(lib.dam_limiter_workspace_bytes(1, n) // 8, dtype=torch.float64, device='cuda')
    mg, nl = torch.zeros(1, dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')

    def call(x_ptr=x.data_ptr(), out_ptr=out.data_ptr(), ws_ptr=ws.data_ptr(), ceiling=CEILING, L=4, H=8, sets=1, samples=n,
             channels=2):
        return lib.dam_limiter_apply(x_ptr, 0, sets, samples, channels, 2 * n, 1, n, None, ceiling, L, H, out_ptr, 1,
                                     mg.data_ptr(), nl.data_ptr(), ws_ptr, None)

    assert call() == 0
    assert lib.dam_limiter_apply(x.data_ptr(), 0, 1, n, 2, 2 * n, 1, n, None, CEILING, 4, 8, out.data_ptr(), 1, None, None,
                                 ws.data_ptr(), None) == 0                       # the statistics are optional
    torch.cuda.synchronize()
    bad = {'L = 0': dict(L=0), 'H = 0': dict(H=0), 'L past the cap': dict(L=max_l + 1), 'H past the cap': dict(H=max_h + 1),
           'NULL x': dict(x_ptr=None), 'NULL out': dict(out_ptr=None), 'NULL workspace': dict(ws_ptr=None),
           'ceiling 0': dict(ceiling=0.0), 'ceiling < 0': dict(ceiling=-0.5), 'ceiling NaN': dict(ceiling=float('nan')),
           'no row set': dict(sets=0), 'no sample': dict(samples=0), 'no channel': dict(channels=0)}
    for name, kw in bad.items():
        got = call(**kw)
        print('%s -> %d (want %d)' % (name, got, BAD_ARG))
        assert got == BAD_ARG
    assert lib.dam_limiter_workspace_bytes(0, n) == 0 and lib.dam_limiter_workspace_bytes(1, 0) == 0
    xd = torch.zeros((1, n, 2), dtype=torch.float32, device='cuda')
    for L, H in ((0, 8), (4, 0), (max_l + 1, 8), (4, max_h + 1)):
        with pytest.raises(ValueError):
            ops.limiter_apply(xd, CEILING_DB, L, H)
    assert T == lib.dam_limiter_tile_samples()
