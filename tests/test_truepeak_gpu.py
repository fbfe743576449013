"""GPU: the batched true-peak meter (dam_true_peak_batch) and the gain clamp (dam_peak_limit_gains) against the numpy
definition (tests/_truepeak_ref.py) evaluated with the taps the library exports.

Tolerance: |got - want| <= 1e-13 * max|x * gain| of the row.  Each interpolated value is 12 products with sum|h_p| < 2.2
(tests/test_truepeak_ref_cpu.py prints 1.86), so either side is within about 12 * 1.1e-16 * 2.2 ~ 3e-15 of the exact
value times max|x|; the ~30x margin covers the kernel's FMA contraction and its summation order against numpy's.  The
sample peak is exact, and where the sample peak is the maximum the true peak is exact too.
Largest observed errors: NOT YET RECORDED -- no GPU could be obtained while this file was written, so these tests have not
run on an MI355X.  What exists is a host rehearsal: the kernel source compiled for the CPU (threads in place of lanes,
under the address and undefined-behaviour sanitizers) agreed with the definition to 2.2e-16 of max|x * gain| on the shapes
and gain counts below.  Every test prints its largest observed error before asserting."""
import ctypes

import numpy as np
import pytest
import torch

import _truepeak_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-13


@pytest.fixture(scope='module')
def env(dam_lib):
    from deep_audio_mixer_amd import loudness, ops
    h = (ctypes.c_double * 49)()
    assert dam_lib.dam_true_peak_taps_host(h) == 0
    taps = np.array(list(h))
    taps.setflags(write=False)
    T, max_blocks = ops.true_peak_geometry()
    return loudness, ops, taps, int(T), int(max_blocks)


def device_view(x, planar):
    """x numpy [N, n, ch] -> CUDA tensor of that shape, stored interleaved or as a transposed view of planar [N, ch, n]."""
    if planar:
        t = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().transpose(1, 2)
        assert tuple(t.shape) == x.shape and (x.shape[2] == 1 or x.shape[1] == 1 or not t.is_contiguous())
        return t
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def measure(ops, x, planar=False, gains=None):
    xd = device_view(x, planar)
    sp = torch.empty((x.shape[0], x.shape[2]), dtype=torch.float64, device='cuda')
    gd = None if gains is None else torch.from_numpy(np.asarray(gains, dtype=np.float64)).cuda()
    tp = ops.true_peak_batch(xd, gains=gd, sample_peak_out=sp)
    assert tp.is_cuda and tp.dtype == torch.float64 and tuple(tp.shape) == (x.shape[0], x.shape[2])
    return sp.cpu().numpy(), tp.cpu().numpy()


def compare(x, sp, tp, taps, gains=None):
    """Asserts both outputs of every row against the definition; returns the largest error as a fraction of max|x * gain|."""
    worst = 0.0
    for t in range(x.shape[0]):
        scaled = ref.apply_gains(x[t], gains[t]) if gains is not None else x[t].astype(np.float64)
        want_sp, want_tp = ref.sample_peak(scaled), ref.true_peak(scaled, taps)
        assert np.array_equal(sp[t], want_sp), (t, sp[t], want_sp)
        assert (tp[t] >= sp[t]).all()
        for c in range(x.shape[2]):
            scale = want_sp[c]
            if scale == 0.0:
                assert tp[t, c] == 0.0
                continue
            worst = max(worst, abs(tp[t, c] - want_tp[c]) / scale)
            if want_tp[c] == want_sp[c]:
                assert tp[t, c] == want_tp[c]
    return worst


def burst(length=16):
    """fs/4 at 45 degrees: every sample at 0.707 of the waveform's peak -- the extreme inter-sample peak; centred on index
    length // 2."""
    return np.sin(2 * np.pi * np.arange(-(length // 2), length - length // 2) / 4.0 + np.pi / 4)


def place(x, centre, amp=0.7):
    """Adds the burst so that its middle sits on sample `centre` of the 1-D array x (clipped at the array's ends)."""
    b = amp * burst()
    lo = centre - len(b) // 2
    a, z = max(lo, 0), min(lo + len(b), len(x))
    x[a:z] += b[a - lo: z - lo]


LAYOUTS = [(1, np.float32, False), (2, np.float64, True), (5, np.float32, True), (2, np.float32, False), (5, np.float64, False)]


@pytest.mark.parametrize('which', ['1', '5', '6', '7', '12', '13', 'T-1', 'T', 'T+1', '2T+3'])
def test_shapes_and_layouts(env, which):
    _, ops, taps, T, _ = env
    n = {'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+3': 2 * T + 3}.get(which) or int(which)
    worst = 0.0
    for ch, dtype, planar in LAYOUTS:
        rng = np.random.default_rng(n * 31 + ch)
        x = (0.3 * rng.standard_normal((2, n, ch))).astype(dtype)
        sp, tp = measure(ops, x, planar)
        worst = max(worst, compare(x, sp, tp, taps))
    print('n = %d: max err %.3g of max|x| (bound %g)' % (n, worst, TOL))
    assert worst <= TOL


def test_grid_stride_wrap(env):
    """One row longer than one pass of the capped grid: n = T * max_blocks + 7 (16.8 MB of float32 for T = 2048 and 2048
    workgroups -- the size itself is used, no reduced block share), the extreme burst across the grid-stride boundary."""
    _, ops, taps, T, max_blocks = env
    n = T * max_blocks + 7
    assert n * 4 < 100e6
    x = (1e-3 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    place(x, T * max_blocks)
    x = x.reshape(1, n, 1)
    sp, tp = measure(ops, x)
    assert tp[0, 0] > 1.3 * sp[0, 0]                                   # the peak that matters lies between the samples
    worst = compare(x, sp, tp, taps)
    print('grid wrap, n = %d: sample peak %.6f, true peak %.6f, err %.3g of max|x| (bound %g)' % (n, sp[0, 0], tp[0, 0], worst, TOL))
    assert worst <= TOL


def test_peak_placement_and_silence(env):
    loudness, ops, taps, T, _ = env
    n = 2 * T + 3
    rng = np.random.default_rng(2)
    centres = (0, n - 1, T, T - 5, T + 6)                              # row ends, the tile boundary, either end of its halo
    x = (1e-3 * rng.standard_normal((len(centres) + 1, n, 1)))
    for t, c in enumerate(centres):
        place(x[t, :, 0], c)
    x[-1] = 0.0
    for dtype in (np.float32, np.float64):
        xs = x.astype(dtype)
        sp, tp = measure(ops, xs, planar=True)
        worst = compare(xs, sp, tp, taps)
        print('%s: true / sample peak per placement %s, err %.3g of max|x| (bound %g)'
              % (np.dtype(dtype).name, np.round(tp[:-1, 0] / sp[:-1, 0], 4).tolist(), worst, TOL))
        assert worst <= TOL
        assert (tp[:-1, 0] > 1.3 * sp[:-1, 0]).all()                   # the inter-sample peak is found wherever the burst sits
        assert sp[-1, 0] == 0.0 and tp[-1, 0] == 0.0
    db = loudness.true_peak(np.zeros((100, 2), dtype=np.float32))
    assert db.shape == (2,) and (db == -np.inf).all()
    tone = np.sin(2 * np.pi * np.arange(4000) / 4 + np.pi / 4)
    assert abs(loudness.true_peak(tone)[0] - ref.to_db(ref.true_peak(tone, taps))[0]) < 1e-9


@pytest.mark.parametrize('n_gains', [1, 3, 7])
def test_gains_at_load(env, n_gains):
    """n = 13: segments of 4 and 1 samples; n = 6 T + 5: a segment longer than a tile image for 1 and 3 gains (one crossing
    per image at most), shorter for 7 (the index is divided out per element)."""
    _, ops, taps, T, _ = env
    worst = 0.0
    for n in (13, 6 * T + 5):
        assert n_gains == 1 or n % n_gains
        for ch, dtype, planar in LAYOUTS[:3]:
            rng = np.random.default_rng(n + n_gains)
            x = (0.3 * rng.standard_normal((3, n, ch))).astype(dtype)
            gains = rng.uniform(0.2, 3.0, (3, n_gains))
            sp, tp = measure(ops, x, planar, gains)
            worst = max(worst, compare(x, sp, tp, taps, gains))
    print('%d gains: max err %.3g of max|x * gain| (bound %g)' % (n_gains, worst, TOL))
    assert worst <= TOL


def test_batch_invariance_is_bitwise(env):
    _, ops, _, T, _ = env
    n = 2 * T + 3
    x = torch.from_numpy((0.3 * np.random.default_rng(3).standard_normal((5, n, 2))).astype(np.float32)).cuda()
    sp = torch.empty((5, 2), dtype=torch.float64, device='cuda')
    tp = ops.true_peak_batch(x, sample_peak_out=sp)
    for t in range(5):
        sp1 = torch.empty((1, 2), dtype=torch.float64, device='cuda')
        tp1 = ops.true_peak_batch(x[t:t + 1], sample_peak_out=sp1)
        assert torch.equal(tp1[0], tp[t]) and torch.equal(sp1[0], sp[t])
    perm = [3, 0, 4, 1, 2]
    sp2 = torch.empty((5, 2), dtype=torch.float64, device='cuda')
    tp2 = ops.true_peak_batch(x[perm].contiguous(), sample_peak_out=sp2)
    assert torch.equal(tp2, tp[perm]) and torch.equal(sp2, sp[perm])


def test_peak_limit_gains_is_bitwise(env):
    loudness, ops, _, _, _ = env
    rng = np.random.default_rng(4)
    gains = rng.uniform(0.1, 20.0, 300)
    peaks = rng.uniform(0.01, 2.0, (300, 5))
    peaks[7] = 0.0                                                      # a silent row: the gain stays
    gains[11], peaks[11] = 1e-3, 0.5                                    # already under the ceiling
    for ceiling_db, ppg in ((-1.0, 5), (-6.0, 1), (0.0, 2)):
        p = peaks[:, :ppg].copy()
        want = ref.limit_gains(gains, p, 10.0 ** (ceiling_db / 20.0))
        got = ops.peak_limit_gains(torch.from_numpy(gains.copy()).cuda(), torch.from_numpy(p).cuda(), ceiling_db).cpu().numpy()
        print('ceiling %g dBTP, %d peaks per gain: %d of 300 gains clamped, max |diff| %.3g (bitwise expected)'
              % (ceiling_db, ppg, int((want < gains).sum()), np.abs(got - want).max()))
        assert np.array_equal(got, want)
        assert got[7] == gains[7] and got[11] == gains[11] and (want < gains).any() and (want == gains).any()
    g = torch.tensor([4.0], dtype=torch.float64, device='cuda')
    assert loudness.limit_gains_device(g, torch.tensor([[0.5, 2.0]], dtype=torch.float64, device='cuda'), 0.0) is g
    assert g.item() == 0.5


def test_capture_and_replay(env):
    """Meter + clamp inside torch.cuda.graph on static buffers: capturing proves nothing synchronises or allocates outside
    the pool; a replay on new contents equals the eager call on those contents, bitwise."""
    _, ops, _, T, _ = env
    n = 2 * T + 3
    rng = np.random.default_rng(5)
    contents = [torch.from_numpy((a * rng.standard_normal((2, n, 2))).astype(np.float32)).cuda() for a in (0.3, 0.9, 0.05)]
    buf = contents[0].clone()
    gains = torch.from_numpy(rng.uniform(0.3, 1.7, (2, 3))).cuda()
    tp = torch.empty((2, 2), dtype=torch.float64, device='cuda')
    sp = torch.empty((2, 2), dtype=torch.float64, device='cuda')
    free = torch.full((2,), 1.5, dtype=torch.float64, device='cuda')
    lim = torch.empty(2, dtype=torch.float64, device='cuda')

    def body():
        ops.true_peak_batch(buf, gains=gains, out=tp, sample_peak_out=sp)
        lim.copy_(free)
        ops.peak_limit_gains(lim, tp, -1.0)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    seen = []
    for c in contents[1:]:
        buf.copy_(c)
        graph.replay()
        torch.cuda.synchronize()
        e_sp = torch.empty_like(sp)
        e_tp = ops.true_peak_batch(c, gains=gains.clone(), sample_peak_out=e_sp)
        e_lim = ops.peak_limit_gains(free.clone(), e_tp, -1.0)
        assert torch.equal(tp, e_tp) and torch.equal(sp, e_sp) and torch.equal(lim, e_lim)
        seen.append(lim.clone())
    assert (seen[0] < 1.5).all() and (seen[1] == 1.5).all()             # one content is clamped, the other is not


def test_argument_checks(env, dam_lib):
    loudness, ops, _, _, _ = env
    x = torch.zeros((1, 64, 2), dtype=torch.float32, device='cuda')
    out = torch.zeros(4, dtype=torch.float64, device='cuda')
    ws = torch.zeros(64, dtype=torch.float64, device='cuda')
    g = torch.ones(4, dtype=torch.float64, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_tracks=1, n=64, ch=2, gains=None, n_gains=0, true_peak=p(out), x_ptr=p(x), workspace=p(ws)):
        return dam_lib.dam_true_peak_batch(x_ptr, 0, n_tracks, n, ch, 128, 2, 1, gains, n_gains, None, true_peak, workspace, None)

    BAD_ARG = -1
    assert call() == 0
    assert call(ch=0) == BAD_ARG
    assert call(n_tracks=65536, ch=1) == BAD_ARG
    assert call(gains=p(g), n_gains=0) == BAD_ARG and call(gains=p(g), n_gains=-3) == BAD_ARG
    assert call(gains=p(g), n_gains=65) == BAD_ARG                      # more gains than samples, as the meter refuses
    assert call(true_peak=None) == BAD_ARG
    assert call(x_ptr=None) == BAD_ARG and call(workspace=None) == BAD_ARG and call(n=0) == BAD_ARG and call(n_tracks=0) == BAD_ARG
    assert dam_lib.dam_true_peak_workspace_bytes(0, 64, 2) == 0
    assert dam_lib.dam_peak_limit_gains(None, p(out), 1, 1, 1.0, None) == BAD_ARG
    assert dam_lib.dam_peak_limit_gains(p(g), p(out), 0, 1, 1.0, None) == BAD_ARG
    assert dam_lib.dam_peak_limit_gains(p(g), p(out), 1, 1, 0.0, None) == BAD_ARG
    torch.cuda.synchronize()
    # the Python surface refuses what the meter refuses
    with pytest.raises(RuntimeError, match='GPU only'):
        loudness.true_peak_batch(torch.zeros((1, 64, 2)))
    with pytest.raises(ValueError):
        loudness.true_peak_batch(torch.zeros((64, 2), device='cuda'))
    with pytest.raises(ValueError):
        loudness.true_peak_batch(torch.zeros((1, 64, 2), dtype=torch.int16, device='cuda'))
    with pytest.raises(ValueError):
        ops.true_peak_batch(x, gains=torch.ones((1, 65), dtype=torch.float64, device='cuda'))


def test_normalize_peak(env):
    loudness, _, taps, _, _ = env
    n = np.arange(4000)
    x = np.stack([0.5 * np.sin(2 * np.pi * n / 4 + np.pi / 4), 0.2 * np.sin(2 * np.pi * 0.01 * n)], axis=1)
    plain = loudness.normalize_peak(x, -1.0)                            # pyloudnorm normalize.peak, on the sample peak
    assert np.array_equal(plain, np.power(10.0, -1.0 / 20.0) / np.max(np.abs(x)) * x)
    true = loudness.normalize_peak(x, -1.0, true_peak=True)
    got = ref.to_db(ref.true_peak(true, taps).max())
    print('normalize_peak(true_peak=True): %.12f dBTP (target -1, bound 1e-9 dB); the sample-peak form leaves %.4f dBTP'
          % (got, ref.to_db(ref.true_peak(plain, taps).max())))
    assert abs(got + 1.0) < 1e-9
    assert ref.to_db(ref.true_peak(plain, taps).max()) > 1.0            # what the sample peak overlooks: +2 dBTP
