"""GPU: the compressor (dam_compressor_apply) against the sequential numpy definition (tests/_compressor_ref.py) evaluated with
the constants of ops.compressor_constants, which the kernel receives bit for bit.

Tolerance, derived, not tuned.  A recurrence with contraction factor alpha accumulates at most a few roundings of magnitude
u * max c per step over an effective 1 / (1 - alpha) ~ tau * sr steps; the kernel's chunked order, its fma and the few-ulp
difference between the device's log10 / exp and numpy's are inside the same factor:
    TOL_Q = 8 * 2^-53 * max(tau_A, tau_R) * sr * max(1, max c)   dB                       (ref.tol_q)
    |out_dev - out_ref| <= max|xs| * M * (ln10/20 * TOL_Q + 4 * 2^-53) + one ulp of the output dtype
    |max_reduction_dev - ref| <= TOL_Q;   |q_dev - q_ref| <= TOL_Q;   n_over exactly equal, no sample excluded.
Everything in the second half of the file is bitwise.
Largest observed errors (1 x MI355X, all parity cases and the two rows of 2^20 + 7): |dq| 0.0045 of its bound, |dout| 0.0020 of
its bound, |dmax_reduction| 0.0013 of its bound, n_over equal everywhere; every bitwise test: 0 values differ.  Each test
prints its figures as fractions of the bounds before it asserts."""
import numpy as np
import pytest
import torch

import _compressor_ref as ref
from test_limiter_gpu import device_view

pytestmark = pytest.mark.gpu

SR = 44100
BAD_ARG = -1                                         # DAM_ERR_BAD_ARG
DEFAULTS = dict(threshold_db=-12.0, ratio=2.0, knee_db=6.0, attack_ms=10.0, release_ms=100.0)


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import ops
    K, tile, longest = (int(v) for v in ops.compressor_geometry())
    assert K == dam_lib.dam_compressor_chunk_samples() and tile % (64 * K) == 0 and longest == 2 ** 17
    return ops, K, tile, longest, dam_lib


def params(name, longest):
    """The parameter sets -> dict(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db)."""
    p = dict(DEFAULTS, makeup_db=0.0)
    if name == 'hard knee':
        p.update(threshold_db=-24.0, ratio=4.0, knee_db=0.0, makeup_db=3.0)
    elif name == 'infinite ratio':
        p.update(threshold_db=-24.0, ratio=float('inf'), knee_db=6.0, attack_ms=5.0, release_ms=50.0)
    elif name == 'one sample / cap':
        p.update(threshold_db=-24.0, ratio=4.0, attack_ms=1000.0 / SR, release_ms=1000.0 * longest / SR)
    else:
        assert name == 'defaults'
    return p


PARAMS = ['defaults', 'hard knee', 'infinite ratio', 'one sample / cap']


def curve_args(ops, p):
    """-> the seven positional arguments behind ``data`` / ``x`` of ops.compressor_apply and ref.compress"""
    return (p['threshold_db'], p['ratio'], p['knee_db']) + ops.compressor_constants(
        p['threshold_db'], p['knee_db'], p['attack_ms'], p['release_ms'], SR, p['makeup_db'])


def run(ops, x, args, planar=False, out_dtype=torch.float64, pre_gain=None):
    """x numpy [N, n, ch] -> (out numpy [N, n, ch], q [N, n], max_reduction [N], n_over [N])."""
    pg = None if pre_gain is None else torch.from_numpy(np.asarray(pre_gain, dtype=np.float64)).cuda()
    q = torch.full((x.shape[0], x.shape[1]), -1.0, dtype=torch.float64, device='cuda')
    out, mr, no = ops.compressor_apply(device_view(x, planar), *args, pre_gain=pg, out_dtype=out_dtype, reduction_out=q)
    assert out.dtype == out_dtype and tuple(out.shape) == (x.shape[0], x.shape[2], x.shape[1])
    assert mr.dtype == torch.float64 and no.dtype == torch.int64
    return out.transpose(1, 2).cpu().numpy(), q.cpu().numpy(), mr.cpu().numpy(), no.cpu().numpy()


def boundaries(K, tile):
    """Every seam of the launch geometry a row can cross: chunks, waves of 64 chunks, workgroup tiles and the 256 tiles one
    pass of the tile scan takes.  Even positions get a burst across the seam, odd positions one sample behind it."""
    return [K, 2 * K, 3 * K, 5 * K, 64 * K, 128 * K, tile, tile + K, 2 * tile, 3 * tile, 256 * tile, 256 * tile + K]


def check(got, want, p, tag=''):
    """Asserts one row set's device results (out [n, ch], q [n], max_reduction, n_over) against the reference dict; returns
    (|dout| beyond the output ulp, |dq|, |dmax_reduction|), each as a fraction of its bound."""
    out, q, max_reduction, n_over = got
    tol = ref.tol_q(p['attack_ms'] * 1e-3 * SR, p['release_ms'] * 1e-3 * SR, want['c'].max())
    makeup = 10.0 ** (p['makeup_db'] / 20.0)
    bound = max(np.abs(want['xs']).max(), 1e-300) * makeup * (ref.LN10_20 * tol + 4 * 2.0 ** -53)
    ulp = np.spacing(np.abs(want['out']).astype(out.dtype)).astype(np.float64)
    e_out = (np.abs(out.astype(np.float64) - want['out']) - ulp).max() / bound
    e_q = np.abs(q - want['q']).max() / tol
    e_max = abs(max_reduction - want['max_reduction']) / tol
    assert e_out <= 1.0, (tag, 'out', e_out)
    assert e_q <= 1.0, (tag, 'q', e_q)
    assert e_max <= 1.0, (tag, 'max_reduction', max_reduction, want['max_reduction'])
    assert n_over == want['n_over'], (tag, 'n_over', n_over, want['n_over'])
    return max(e_out, 0.0), e_q, e_max


LENGTHS = ['1', '2', 'K-1', 'K', 'K+1', '2K+3', '64K+5', '256K+K+1']


@pytest.mark.parametrize('length', LENGTHS)
@pytest.mark.parametrize('name', PARAMS)
def test_parity_with_the_definition(env, name, length):
    ops, K, tile, longest, _ = env
    n = {'K-1': K - 1, 'K': K, 'K+1': K + 1, '2K+3': 2 * K + 3, '64K+5': 64 * K + 5, '256K+K+1': 257 * K + 1}.get(length) \
        or int(length)
    p = params(name, longest)
    args = curve_args(ops, p)
    worst = [0.0, 0.0, 0.0]
    reduced = 0.0
    for kind in ('bursts', 'am noise', 'zero'):
        for ch in (1, 2):
            for dtype in (np.float32, np.float64):
                if kind == 'bursts':
                    x = ref.bursts_on_a_bed(n, ch, seed=n + ch, boundaries=boundaries(K, tile))
                elif kind == 'am noise':
                    x = ref.am_noise(n, ch, seed=n + ch)
                    x[:, 0] = np.roll(x[:, 0], n // 2)             # the loud half of the envelope into a short row too
                else:
                    x = np.zeros((n, ch))
                x = x.astype(dtype)
                pre = None if dtype == np.float32 else 1.25
                want = ref.compress(x, *args, pre_gain=pre)
                reduced = max(reduced, want['max_reduction'])
                for out_dtype in (torch.float32, torch.float64):
                    out, q, mr, no = run(ops, x[None], args, planar=ch == 2 and dtype == np.float32, out_dtype=out_dtype,
                                         pre_gain=None if pre is None else [pre])
                    figures = check((out[0], q[0], mr[0], int(no[0])), want, p, (kind, ch, dtype.__name__, out_dtype))
                    worst = [max(a, b) for a, b in zip(worst, figures)]
                if kind == 'zero':
                    assert not out.any() and not q.any() and mr[0] == 0.0 and no[0] == 0
    print('%s, n %d: |dout| %.3g, |dq| %.3g, |dmax_reduction| %.3g of their bounds; up to %.2f dB of reduction'
          % (name, n, worst[0], worst[1], worst[2], reduced))
    assert reduced > 0.0                                # (a 10 ms attack reaches 0.007 dB in one sample)


@pytest.mark.parametrize('kind', ['bursts', 'am noise'])
def test_long_row_crosses_the_tile_scan(env, kind):
    """n = 2^20 + 7: more tiles than one pass of the tile scan takes, so the carried state is used; N = 3 with a pre_gain."""
    ops, K, tile, longest, _ = env
    n = 2 ** 20 + 7
    assert n > 256 * tile
    p = params('hard knee' if kind == 'bursts' else 'defaults', longest)
    args = curve_args(ops, p)
    if kind == 'bursts':
        x = ref.bursts_on_a_bed(n, 2, seed=4, boundaries=boundaries(K, tile)).astype(np.float32)
    else:
        x = ref.am_noise(n, 2, seed=4).astype(np.float32)
    sets = np.stack([x * 0.9, x * 0.5, x * 0.01])
    pre = [1.0, 2.0, 1.5]                               # (set 1 is x again: both factors are exact)
    out, q, mr, no = run(ops, sets, args, planar=True, pre_gain=pre)
    want = ref.compress(sets[1], *args, pre_gain=pre[1])
    figures = check((out[1], q[1], mr[1], int(no[1])), want, p, kind)
    print('%s, n %d: |dout| %.3g, |dq| %.3g, |dmax_reduction| %.3g of their bounds; %.2f dB of reduction, %d samples over'
          % (kind, n, figures[0], figures[1], figures[2], want['max_reduction'], want['n_over']))
    assert want['max_reduction'] > 0.5 and want['q'][256 * tile] > 0.0
    assert no[2] == 0 and mr[2] == 0.0 and not q[2].any()               # the third set stays under the knee


# ----------------------------------------------------------------------------- bitwise properties
def mixed_input(n, ch, K, tile, seed, dtype=np.float32):
    return (ref.am_noise(n, ch, seed=seed) + ref.bursts_on_a_bed(n, ch, seed=seed + 1, boundaries=boundaries(K, tile))).astype(dtype)


def test_a_row_set_does_not_depend_on_its_batch(env):
    ops, K, tile, longest, _ = env
    n = 2 * tile + K + 3
    args = curve_args(ops, params('defaults', longest))
    sets = np.stack([mixed_input(n, 2, K, tile, seed=s) * (1.0 + 0.4 * s) for s in range(3)])
    pre = [1.0, 0.7, 1.3]
    alone = [run(ops, sets[s:s + 1], args, pre_gain=pre[s:s + 1]) for s in range(3)]
    out, q, mr, no = run(ops, sets, args, pre_gain=pre)
    differ = sum(int((out[s] != alone[s][0][0]).sum()) + int((q[s] != alone[s][1][0]).sum()) for s in range(3))
    print('batch of three: %d values differ from three calls of one (bound 0); max reductions %s, over %s'
          % (differ, mr.tolist(), no.tolist()))
    for s in range(3):
        assert np.array_equal(out[s], alone[s][0][0]) and np.array_equal(q[s], alone[s][1][0])
        assert mr[s] == alone[s][2][0] and no[s] == alone[s][3][0]
    assert len(set(mr.tolist())) == 3 and no.min() > 0


def test_causality(env):
    ops, K, tile, longest, _ = env
    n = 2 * tile + K + 3
    args = curve_args(ops, params('defaults', longest))
    a = mixed_input(n, 2, K, tile, seed=11)[None]
    for m in (0, K - 1, K, 64 * K - 1, tile - 1, tile, tile + 5, n - 2):
        b = a.copy()
        b[0, m + 1:] = mixed_input(n, 2, K, tile, seed=12)[m + 1:] * 3.0
        ra, rb = run(ops, a, args), run(ops, b, args)
        differ = int((ra[0][0, :m + 1] != rb[0][0, :m + 1]).sum()) + int((ra[1][0, :m + 1] != rb[1][0, :m + 1]).sum())
        print('inputs equal up to sample %d: %d values of out and q up to it differ (bound 0); %d behind it'
              % (m, differ, int((ra[1][0, m + 1:] != rb[1][0, m + 1:]).sum())))
        assert differ == 0 and (m > n - 100 or not np.array_equal(ra[1][0, m + 1:], rb[1][0, m + 1:]))


def test_pass_through_until_the_first_sample_over_the_knee(env):
    ops, K, tile, longest, _ = env
    n = 2 * tile + K + 3
    p = params('defaults', longest)
    first = tile + 3 * K + 5                            # the first sample over the knee: behind a tile seam, inside a chunk
    x = (0.004 * np.random.default_rng(2).standard_normal((1, n, 2))).astype(np.float32)
    x[0, first:, :] += mixed_input(n, 2, K, tile, seed=3)[first:]
    x[0, first, 0] = 0.6
    for makeup_db, pre, out_dtype, np_dtype in ((0.0, None, torch.float64, np.float64), (0.0, None, torch.float32, np.float32),
                                                (4.0, [1.7], torch.float64, np.float64), (4.0, [1.7], torch.float32, np.float32)):
        args = curve_args(ops, dict(p, makeup_db=makeup_db))
        out, q, mr, no = run(ops, x, args, out_dtype=out_dtype, pre_gain=pre)
        xs = x[0, :first].astype(np.float64) * (1.0 if pre is None else pre[0])
        want = (xs * args[6]).astype(np_dtype)
        print('make-up %g dB, pre_gain %s, %s out: %d samples before %d differ from xs * M (bound 0), q there all zero: %s; q[%d] = %.3g'
              % (makeup_db, pre, np_dtype.__name__, int((out[0, :first] != want).sum()), first, not q[0, :first].any(), first,
                 q[0, first]))
        assert np.array_equal(out[0, :first], want) and not q[0, :first].any() and q[0, first] > 0.0 and mr[0] > 0.0
        if makeup_db == 0.0 and np_dtype == np.float64:
            assert np.array_equal(out[0, :first], x[0, :first].astype(np.float64))        # the float64 image of the input


def test_channel_swap_and_storage(env):
    ops, K, tile, longest, _ = env
    n = tile + K + 3
    args = curve_args(ops, params('infinite ratio', longest))
    for dtype in (np.float32, np.float64):
        x = mixed_input(n, 2, K, tile, seed=21, dtype=dtype)[None]
        a = run(ops, x, args)
        b = run(ops, np.ascontiguousarray(x[:, :, ::-1]), args)
        c = run(ops, x, args, planar=True)
        print('%s: channels swapped: %d out values differ from the swapped outputs, %d q values differ; planar view: %d / %d (bounds 0)'
              % (dtype.__name__, int((b[0][:, :, ::-1] != a[0]).sum()), int((b[1] != a[1]).sum()), int((c[0] != a[0]).sum()),
                 int((c[1] != a[1]).sum())))
        assert np.array_equal(b[0][:, :, ::-1], a[0]) and np.array_equal(b[1], a[1]) and b[2] == a[2] and b[3] == a[3]
        assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1]) and c[2] == a[2] and c[3] == a[3]
        assert a[2][0] > 0.5 and not np.array_equal(a[0][0, :, 0], a[0][0, :, 1])


def test_graph_capture(env):
    ops, K, tile, longest, lib = env
    n = 2 * tile + 3
    args = curve_args(ops, params('defaults', longest))
    contents = [torch.from_numpy(mixed_input(n, 2, K, tile, seed=s)[None] * (1.0 + s)).cuda() for s in (1, 2)]
    eager = []
    for c in contents:
        q = torch.empty((1, n), dtype=torch.float64, device='cuda')
        eager.append(ops.compressor_apply(c, *args, reduction_out=q) + (q,))
    x = torch.empty_like(contents[0])
    gain = torch.ones(1, dtype=torch.float64, device='cuda')
    ws = torch.empty(lib.dam_compressor_workspace_bytes(1, n) // 8, dtype=torch.float64, device='cuda')
    out = torch.empty((1, 2, n), dtype=torch.float64, device='cuda')
    q = torch.empty((1, n), dtype=torch.float64, device='cuda')
    mr, no = torch.empty(1, dtype=torch.float64, device='cuda'), torch.empty(1, dtype=torch.int64, device='cuda')

    def body():
        ops.compressor_apply(x, *args, pre_gain=gain, out=out, reduction_out=q, max_reduction_out=mr, n_over_out=no, workspace=ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for c, (want_out, want_mr, want_no, want_q) in zip(contents, eager):
        x.copy_(c)
        for replay in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            print('replay %d: %d samples differ from the eager call (bound 0), n_over %d / %d'
                  % (replay, int((out != want_out).sum()), int(no[0]), int(want_no[0])))
            assert torch.equal(out, want_out) and torch.equal(q, want_q) and torch.equal(mr, want_mr) and torch.equal(no, want_no)
    assert int(eager[0][2][0]) > 0 and not torch.equal(eager[0][0], eager[1][0])


def test_argument_errors(env):
    ops, K, tile, longest, lib = env
    n = 64
    x = torch.zeros((2, n), dtype=torch.float32, device='cuda')
    out = torch.full((2, n), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.zeros(lib.dam_compressor_workspace_bytes(1, n) // 8, dtype=torch.float64, device='cuda')
    mr, no = torch.zeros(1, dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')
    T, R, W, ks, aa, ar, M = curve_args(ops, params('defaults', longest))

    def call(x_ptr=x.data_ptr(), out_ptr=out.data_ptr(), ws_ptr=ws.data_ptr(), T=T, R=R, W=W, ks=ks, aa=aa, ar=ar, M=M, sets=1,
             samples=n, channels=2):
        return lib.dam_compressor_apply(x_ptr, 0, sets, samples, channels, 2 * n, 1, n, None, T, R, W, ks, aa, ar, M, out_ptr, 1,
                                        None, mr.data_ptr(), no.data_ptr(), ws_ptr, None)

    too_long = float(np.exp(-1.0 / (2.0 * longest)))
    bad = {'knee_start of another threshold': dict(T=T + 1e-6), 'knee_start 0': dict(ks=0.0), 'knee_start NaN': dict(ks=float('nan')),
           'R < 1': dict(R=0.5), 'R NaN': dict(R=float('nan')), 'W < 0': dict(W=-1.0, ks=10.0 ** ((T + 0.5) / 20.0)),
           'attack alpha 0': dict(aa=0.0), 'attack alpha 1': dict(aa=1.0), 'release alpha > 1': dict(ar=1.5),
           'release alpha < 0': dict(ar=-0.5), 'alpha NaN': dict(aa=float('nan')), 'attack above the cap': dict(aa=too_long),
           'release above the cap': dict(ar=too_long), 'make-up 0': dict(M=0.0), 'no sample': dict(samples=0),
           'no row set': dict(sets=0), 'no channel': dict(channels=0), 'NULL x': dict(x_ptr=None), 'NULL out': dict(out_ptr=None),
           'NULL workspace': dict(ws_ptr=None)}
    for name, kw in bad.items():
        got = call(**kw)
        print('%s -> %d (want %d)' % (name, got, BAD_ARG))
        assert got == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                     # nothing was launched
    assert call() == 0 and call(R=float('inf')) == 0 and call(aa=float(np.exp(-1.0 / longest)), ar=float(np.exp(-1.0))) == 0
    torch.cuda.synchronize()
    assert not out.any()
    assert lib.dam_compressor_workspace_bytes(0, n) == 0 and lib.dam_compressor_workspace_bytes(1, 0) == 0
    xd = torch.zeros((1, n, 2), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError):
        ops.compressor_apply(xd, T, 0.5, W, ks, aa, ar)
    with pytest.raises(ValueError):
        ops.compressor_apply(xd, T + 1.0, R, W, ks, aa, ar)
    with pytest.raises(ValueError):
        ops.compressor_constants(T, -1.0, 10.0, 100.0, SR)


def test_compress_wrappers(env):
    from deep_audio_mixer_amd import loudness
    ops, K, tile, longest, _ = env
    n = tile + 5
    x = mixed_input(n, 2, K, tile, seed=31)
    want = ref.compress(x, *curve_args(ops, dict(DEFAULTS, makeup_db=2.0)))
    out, info = loudness.compress(x, SR, makeup_db=2.0)
    tol = ref.tol_q(441.0, 4410.0, want['c'].max())
    print('compress(): max reduction %.6f dB (reference %.6f), over share %.4f, |dq| %.3g of its bound'
          % (info['max_reduction_db'], want['max_reduction'], info['over_share'], np.abs(info['reduction_db'] - want['q']).max() / tol))
    assert out.shape == x.shape and out.dtype == x.dtype and info['over_share'] == want['n_over'] / n
    assert abs(info['max_reduction_db'] - want['max_reduction']) <= tol and np.abs(info['reduction_db'] - want['q']).max() <= tol
    assert np.abs(out - want['out']).max() <= np.abs(want['out']).max() * 2.0 ** -23
    mono, _ = loudness.compress(x[:, 0].astype(np.float64), SR)
    assert mono.shape == (n,) and mono.dtype == np.float64
    dev, mr, no = loudness.compress_device(torch.from_numpy(x[None]).cuda(), SR, makeup_db=2.0)
    assert dev.dtype == torch.float64 and tuple(dev.shape) == (1, 2, n) and int(no[0]) == want['n_over']
