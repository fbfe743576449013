"""GPU: ModelTrainer.fit under a process group of two ranks (data parallel) and the replica digest kernel.

Two ranks share the box's one GPU over gloo (as tests/test_host_gpu.py's two-rank step does): at most three processes have
the GPU open.  Every spawned run has a join timeout, so a hang fails the test instead of blocking the suite."""
import gc
import io
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch

from _inputs import model_input

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT_S = 420
WORLD = 2
N_TRAIN, N_VAL, BATCH = 26, 6, 2          # 13 train items per rank: 6 full batches + a ragged one; 3 val items: 2 batches


@pytest.fixture(scope='module')
def dam(dam_lib):
    import deep_audio_mixer_amd as pkg
    return pkg


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawn(fn, *args, backend='gloo'):
    """Runs fn(rank, WORLD, port, backend, *args) on WORLD fresh processes; fails (and kills them) after JOIN_TIMEOUT_S."""
    import torch.multiprocessing as mp
    gc.collect()
    ctx = mp.start_processes(fn, args=(WORLD, _free_port(), backend) + args, nprocs=WORLD, join=False, start_method='spawn')
    deadline = time.time() + JOIN_TIMEOUT_S
    while not ctx.join(timeout=max(1.0, deadline - time.time())):
        if time.time() >= deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail('the ranks did not finish within %d s (a hang)' % JOIN_TIMEOUT_S)


def _init_rank(rank, world, port, backend):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank if backend == 'nccl' else 0),
                      MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import deep_audio_mixer_amd  # noqa: F401
    from deep_audio_mixer_amd import distributed as ddist
    dev = rank if backend == 'nccl' else 0
    torch.cuda.set_device(dev)
    ddist.init_process_group(backend)
    return torch.device('cuda', dev)


def _feature_loaders(rank, world, dev, n_train=N_TRAIN, n_val=N_VAL):
    """Rank-strided (x, gt) batches of one global feature set (every rank draws the same items, then takes its shard)."""
    from deep_audio_mixer_amd import distributed as ddist
    x, gt = (torch.from_numpy(a).to(dev) for a in model_input(n_train + n_val, 2, 1025, 17, seed=7))

    def batches(lo, n):
        idx = [lo + i for i in ddist.shard_indices(n, rank, world)]
        return [(x[idx[j:j + BATCH]], gt[idx[j:j + BATCH]]) for j in range(0, len(idx), BATCH)]
    return batches(0, n_train), batches(n_train, n_val)


def _model(seed, dev):
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.manual_seed(seed)
    return ResNet18(n_stems=2, input_shape=(1025, 17)).to(dev).train()


def _flat_params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()


def _run_fit(trainer, train, val, epochs=2):
    """fit() with this process's stdout captured; -> (train losses, val losses, stdout text)."""
    out, real = io.StringIO(), sys.stdout
    sys.stdout = out
    try:
        tl, vl = trainer.fit(train, val, 0, epochs)
    finally:
        sys.stdout = real
    return tl, vl, out.getvalue()


def _fit_worker(rank, world, port, backend, out_dir, mode):
    from deep_audio_mixer_amd.model_trainer import ModelTrainer
    dev = _init_rank(rank, world, port, backend)
    os.chdir(os.path.join(out_dir, 'r%d' % rank))
    model = _model(100 + rank, dev)                       # different replicas: fit() starts from rank 0's
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    if mode == 'sgd':
        opt = torch.optim.SGD(model.parameters(), lr=1e-7, momentum=0.9)
    else:
        opt = torch.optim.Adam(model.parameters(), weight_decay=1e-5)
    # 'eager': graph=False keeps a torch.optim.Adam as it is; 'sgd': the captured step is wanted but cannot be taken (warning)
    trainer = ModelTrainer(model, torch.nn.MSELoss(), opt, dev, model_name='dp', graph=(mode != 'eager'))
    train, val = _feature_loaders(rank, world, dev)
    per_batch = []
    real = trainer._train_batch
    trainer._train_batch = lambda b, real=real, acc=per_batch: acc.append(real(b).item()) or torch.tensor(acc[-1])
    tl, vl, text = _run_fit(trainer, train, val)
    del trainer._train_batch
    torch.cuda.synchronize()
    torch.save({'init': init, 'per_batch': per_batch, 'params': _flat_params(model), 'train': tl, 'val': vl, 'stdout': text,
                'weights': sorted(os.listdir('weights')), 'steps': (trainer.graph_steps, trainer.eager_steps),
                'adopted': trainer._adopted_from is opt,
                'world_size': getattr(trainer.optimizer, 'world_size', None)},
               os.path.join(out_dir, 'd%d.pt' % rank))
    trainer.close()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _two_rank_fit(tmp_path, mode, backend='gloo'):
    for r in range(WORLD):
        os.makedirs(tmp_path / ('r%d' % r) / 'weights')
    _spawn(_fit_worker, str(tmp_path), mode, backend=backend)
    return [torch.load(tmp_path / ('d%d.pt' % r)) for r in range(WORLD)]


def _check_rank0_only_output(res):
    r0, r1 = res
    assert r1['stdout'] == '' and r1['weights'] == []
    assert 'Epoch 0/1' in r0['stdout'] and 'Epoch 1 val loss' in r0['stdout']
    assert r0['weights'] == sorted('mixmodel_dp_1s_%04d_%.4f.pt' % (e, r0['train'][e]) for e in range(2))
    for e in range(2):
        assert 'Epoch %d train loss: %.4f' % (e, r0['train'][e]) in r0['stdout']


def _reference_run(init, dev):
    """One process, rank 0's initial replica: every step runs both ranks' micro-batches through forward_mse / backward
    (gradients written into the bound flat bucket, as the trainer's steps do), sums the two gradients and takes the
    Adam(world_size=2) update (1/2 folded into the launch).  The steps the trainer replays from its captured staged step
    take backward in the same two stages here (engine.TrainStep._stage1 / _stage2: autograd cut at the bucket boundary,
    the weight-gradient reductions flushed per stage), the others in one piece -- the same launches, so the same bits.
    -> (flat parameters, train means, val means, per-batch losses of each rank)."""
    from deep_audio_mixer_amd import distributed, ops
    from deep_audio_mixer_amd.model_trainer import ModelTrainer
    from deep_audio_mixer_amd.optim import Adam
    model = _model(0, dev)
    model.load_state_dict(init)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-5, world_size=WORLD)
    opt.set_bucket_boundaries([model.ddp_late_parameters()[0]])
    opt.bind_grad_slots()
    shards = [_feature_loaders(r, WORLD, dev) for r in range(WORLD)]
    train_means, val_means, per_batch = [], [], [[] for _ in range(WORLD)]
    for epoch in range(2):
        totals = [0.0] * WORLD
        for j in range(len(shards[0][0])):
            total = None
            full = shards[0][0][j][0].shape[0] == BATCH
            replayed = full and (epoch > 0 or j >= ModelTrainer.EAGER_BATCHES)
            for r in range(WORLD):
                opt.zero_grad()
                if replayed:
                    tap = []
                    loss = model.forward_mse(*shards[r][0][j], tap=tap)[0]
                    grads, dmid = distributed.backward_late(loss, opt.bucket_params(1), tap[0])
                    ops.wgrad_flush(dev)
                    opt.gather_grads(1, grads=grads)
                    distributed.backward_early(tap[0], dmid, opt.bucket_params(0))
                    ops.wgrad_flush(dev)
                    opt.gather_grads(0)
                else:
                    loss = model.forward_mse(*shards[r][0][j])[0]
                    loss.backward()
                    opt.gather_grads()
                per_batch[r].append(loss.item())
                totals[r] += per_batch[r][-1]
                g = opt.flat_grad.clone()
                total = g if total is None else total + g
            opt.flat_grad.copy_(total)
            opt.sync_hyper()
            opt.launch_update()
        train_means.append(sum(totals) / (WORLD * len(shards[0][0])))
        vt = [0.0] * WORLD
        with torch.no_grad():
            for r in range(WORLD):
                for b in shards[r][1]:
                    vt[r] += model.forward_mse(*b)[0].item()
        val_means.append(sum(vt) / (WORLD * len(shards[0][1])))
    ops.wgrad_flush(dev)
    return _flat_params(model), train_means, val_means, per_batch


def test_two_rank_fit_equals_averaged_micro_batches(dam, tmp_path):
    """training.ipynb cells 11-13 on two ranks: replicas from DIFFERENT seeds, a plain torch.optim.Adam (adopted with
    world_size=2), 6 full batches per epoch (eager, then captured and replayed) and a ragged last one (eager).  Both replicas
    end bit-identical, report the same global losses, only rank 0 prints and saves -- and the parameters are those of one
    process that averages the two micro-batches' gradients at every step."""
    res = _two_rank_fit(tmp_path, 'adopt')
    r0, r1 = res
    assert r0['adopted'] and r0['world_size'] == WORLD
    assert r0['steps'] == r1['steps'] == (10, 4)            # epoch 0: 2 eager + capture + 3 replays + ragged; epoch 1: 6 + 1
    assert not torch.equal(_flat_params_of_state(r0['init']), _flat_params_of_state(r1['init']))
    assert torch.equal(r0['params'], r1['params'])
    assert r0['train'] == r1['train'] and r0['val'] == r1['val']
    _check_rank0_only_output(res)
    want, want_train, want_val, want_batches = _reference_run(r0['init'], torch.device('cuda'))
    assert not torch.equal(want, _flat_params_of_state(r0['init']))
    diff = (r0['params'] - want).abs().max().item()
    rel = [[abs(a - b) / abs(b) for a, b in zip(r['per_batch'], w)] for r, w in zip(res, want_batches)]
    assert torch.equal(r0['params'], want), 'two-rank fit differs from the averaged single-process run by %g; per-batch ' \
        'loss rel. diffs rank 0 %s rank 1 %s' % (diff, ['%.1e' % v for v in rel[0]], ['%.1e' % v for v in rel[1]])
    np.testing.assert_allclose(r0['train'], want_train, rtol=1e-12)
    np.testing.assert_allclose(r0['val'], want_val, rtol=1e-12)


def _flat_params_of_state(state):
    model = _model(0, torch.device('cuda'))
    model.load_state_dict(state)
    return _flat_params(model)


@pytest.mark.parametrize('mode', ['eager', 'sgd'])
def test_two_rank_eager_configurations_average_gradients(dam, tmp_path, mode):
    """graph=False (a plain torch.optim.Adam, stepped by torch) and torch.optim.SGD: .grad is averaged over the ranks
    (distributed.GradBucket) before optimizer.step(), so replicas from different seeds end bit-identical."""
    r0, r1 = _two_rank_fit(tmp_path, mode)
    assert not r0['adopted'] and r0['steps'] == (0, 14)
    assert torch.equal(r0['params'], r1['params'])
    assert not torch.equal(r0['params'], _flat_params_of_state(r0['init']))
    assert r0['train'] == r1['train'] and r0['val'] == r1['val']
    assert all(np.isfinite(r0['train']))
    _check_rank0_only_output((r0, r1))


def _write_wav_song(root, name, n, sr, rng):
    import wave
    song = root / name / (name + '_STEMS_JOINED')
    song.mkdir(parents=True)
    for fn in ('%s_STEM_BASS.wav', '%s_STEM_DRUMS.wav', '%s_STEM_VOCALS.wav', '%s_STEM_OTHER.wav', '../%s_MIX.wav'):
        x = (rng.uniform(-0.5, 0.5, (n, 2)) * 32767).astype('<i2')
        with wave.open(str(song / (fn % name)), 'wb') as w:
            w.setnchannels(2), w.setsampwidth(2), w.setframerate(sr)
            w.writeframes(x.tobytes())


SR = 16384


def _pcm_worker(rank, world, port, backend, out_dir):
    from torch.utils.data import DataLoader
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    from deep_audio_mixer_amd.distributed import DistributedChunkSampler
    from deep_audio_mixer_amd.model_trainer import ModelTrainer
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    import multiprocessing
    # a rank started by torch.distributed.run forks its loader workers (the platform default); this one was spawned
    multiprocessing.set_start_method('fork', force=True)
    dev = _init_rank(rank, world, port, backend)
    os.chdir(os.path.join(out_dir, 'r%d' % rank))
    kw = dict(chunk_length=1, sr=SR, seed=321, normalize=False, compute_features=True, augment_data=False)
    d_train = MultitrackAudioDataset(os.path.join(out_dir, 'songs'), songlist=['A', 'B'], **kw)
    d_val = MultitrackAudioDataset(os.path.join(out_dir, 'songs'), songlist=['B'], **kw)
    train = DataLoader(d_train, BATCH, num_workers=2, pin_memory=True, sampler=DistributedChunkSampler(len(d_train)))
    val = DataLoader(d_val, BATCH, num_workers=2, pin_memory=True, sampler=DistributedChunkSampler(len(d_val)))
    torch.manual_seed(50 + rank)
    model = ResNet18(n_stems=4, input_shape=(1025, 17)).to(dev).train()
    trainer = ModelTrainer(model, torch.nn.MSELoss(), torch.optim.Adam(model.parameters(), weight_decay=1e-5), dev,
                           model_name='dp')
    gc.collect()            # no reference cycles for the forked loader workers to collect (tests/test_host_gpu.py)
    tl, vl, text = _run_fit(trainer, train, val)
    torch.cuda.synchronize()
    torch.save({'params': _flat_params(model), 'train': tl, 'val': vl, 'stdout': text, 'weights': sorted(os.listdir('weights')),
                'steps': (trainer.graph_steps, trainer.eager_steps), 'pcm': not trainer._step.from_features,
                'n_train': len(d_train)}, os.path.join(out_dir, 'd%d.pt' % rank))
    trainer.close()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_fit_over_pcm_loader_with_workers(dam, tmp_path):
    """training.ipynb cell 6 with a DistributedChunkSampler: DataLoader(dataset, batch_size, num_workers=2, pin_memory=True,
    sampler=...) yields HostPcmBatch items that feed the PCM-bound captured step on every rank.  Replicas end bit-identical."""
    rng = np.random.default_rng(8)
    _write_wav_song(tmp_path / 'songs', 'A', SR * 10 + 100, SR, rng)       # 10 + 9 = 19 chunks: 9 per rank, 4 full batches
    _write_wav_song(tmp_path / 'songs', 'B', SR * 9 + 5, SR, rng)          # + a ragged one
    for r in range(WORLD):
        os.makedirs(tmp_path / ('r%d' % r) / 'weights')
    _spawn(_pcm_worker, str(tmp_path))
    r0, r1 = [torch.load(tmp_path / ('d%d.pt' % r)) for r in range(WORLD)]
    assert r0['n_train'] == 19 and r0['pcm'] and r0['steps'][0] > 0 and r0['steps'] == r1['steps']
    assert torch.equal(r0['params'], r1['params'])
    assert r0['train'] == r1['train'] and r0['val'] == r1['val'] and all(np.isfinite(r0['train']))
    _check_rank0_only_output((r0, r1))


def _refusal_worker(rank, world, port, backend, out_dir):
    from deep_audio_mixer_amd.model_trainer import ModelTrainer
    from deep_audio_mixer_amd.optim import Adam
    dev = _init_rank(rank, world, port, backend)
    os.chdir(os.path.join(out_dir, 'r%d' % rank))
    model = _model(100 + rank, dev)
    train, val = _feature_loaders(rank, world, dev)
    seen = {}
    trainer = ModelTrainer(model, torch.nn.MSELoss(), torch.optim.Adam(model.parameters(), weight_decay=1e-5), dev)
    for name, tr, va in (('train_len', train[:3 + rank], val), ('val_len', train[:3], val[:1 + rank]),
                         ('no_len', (b for b in train[:3]), val)):
        try:
            _run_fit(trainer, tr, va, epochs=1)
            seen[name] = None
        except ValueError as e:
            seen[name] = str(e)
    trainer.close()
    model2 = _model(0, dev)
    try:
        ModelTrainer(model2, torch.nn.MSELoss(), Adam(model2.parameters(), weight_decay=1e-5), dev)
        seen['world_size'] = None
    except ValueError as e:
        seen['world_size'] = str(e)
    torch.save(seen, os.path.join(out_dir, 'd%d.pt' % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_refusals_do_not_hang(dam, tmp_path):
    """Loaders of unequal length (train or validation) and a loader without __len__ make BOTH ranks raise ValueError before a
    batch is run -- and both processes exit; optim.Adam(world_size=1) under a group of two is refused."""
    for r in range(WORLD):
        os.makedirs(tmp_path / ('r%d' % r) / 'weights')
    _spawn(_refusal_worker, str(tmp_path))
    r0, r1 = [torch.load(tmp_path / ('d%d.pt' % r)) for r in range(WORLD)]
    for seen in (r0, r1):
        assert seen['train_len'] and 'between 3 and 4' in seen['train_len'] and 'train_loader' in seen['train_len']
        assert seen['val_len'] and 'between 1 and 2' in seen['val_len'] and 'val_loader' in seen['val_len']
        assert seen['no_len'] and '__len__' in seen['no_len']
        assert seen['world_size'] and 'world_size=1' in seen['world_size'] and '2 ranks' in seen['world_size']


def _perturb_worker(rank, world, port, backend, out_dir):
    from deep_audio_mixer_amd import ops
    from deep_audio_mixer_amd.model_trainer import ModelTrainer
    from deep_audio_mixer_amd.optim import Adam
    dev = _init_rank(rank, world, port, backend)
    os.chdir(os.path.join(out_dir, 'r%d' % rank))
    model = _model(100 + rank, dev)
    opt = Adam(model.parameters(), weight_decay=1e-5, world_size=world)
    trainer = ModelTrainer(model, torch.nn.MSELoss(), opt, dev, model_name='dp')
    train, val = _feature_loaders(rank, world, dev, n_train=12)
    if rank == 1:           # a replica that drifts after epoch 0's checks: epoch 1's check must catch it
        real = trainer._validate_epoch

        def drift(loader, real=real):
            out = real(loader)
            with torch.no_grad():
                opt._flat[12345] += 1e-3
            ops.params_changed()
            return out
        trainer._validate_epoch = drift
    err = None
    try:
        _run_fit(trainer, train, val)
    except RuntimeError as e:
        err = str(e)
    torch.save({'err': err, 'weights': sorted(os.listdir('weights'))}, os.path.join(out_dir, 'd%d.pt' % rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_replica_check_raises_on_a_perturbed_replica(dam, tmp_path):
    """A replica that no longer matches the others after a training epoch: every rank raises RuntimeError naming the epoch,
    and rank 0 has not saved that epoch's checkpoint."""
    for r in range(WORLD):
        os.makedirs(tmp_path / ('r%d' % r) / 'weights')
    _spawn(_perturb_worker, str(tmp_path))
    r0, r1 = [torch.load(tmp_path / ('d%d.pt' % r)) for r in range(WORLD)]
    for res in (r0, r1):
        assert res['err'] is not None and 'epoch 1' in res['err'] and 'different parameters' in res['err']
    assert len(r0['weights']) == 1 and r0['weights'][0].startswith('mixmodel_dp_1s_0000_') and r1['weights'] == []


def test_two_rank_fit_rccl(dam, tmp_path):
    """The first test on RCCL, one rank per GPU -- runs on a box that shows two GPUs (counted from sysfs,
    bench.visible_gpu_count(): this process opens no second GPU runtime for it)."""
    import bench
    n = bench.visible_gpu_count() or 0
    if n < 2:
        pytest.skip('RCCL needs one GPU per rank: %d visible here' % n)
    r0, r1 = _two_rank_fit(tmp_path, 'adopt', backend='nccl')
    assert r0['adopted'] and r0['steps'] == (10, 4)
    assert torch.equal(r0['params'], r1['params'])
    assert r0['train'] == r1['train'] and r0['val'] == r1['val']
    _check_rank0_only_output((r0, r1))


# ---- the digest kernel (include/dam_hip.h: dam_digest64_u32)
_GOLDEN, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_MASK = (1 << 64) - 1


def _np_digest(bits, base=0):
    """NumPy restatement: sum mod 2^64 of splitmix64-finalised (bits[i] + (base + i) * golden)."""
    u = np.uint64
    z = bits.astype(np.uint32).astype(u) + (np.arange(bits.size, dtype=u) + u(base)) * u(_GOLDEN)
    z ^= z >> u(30)
    z *= u(_M1)
    z ^= z >> u(27)
    z *= u(_M2)
    z ^= z >> u(31)
    return int(z.sum(dtype=u))


def _gpu_digest(t, **kw):
    from deep_audio_mixer_amd import ops
    return int(ops.digest64(t, **kw).item()) & _MASK


_SPECIAL = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7FDA4D17, 0x7F800001, 0x7F800000, 0xFF800000,
                     0x00000001, 0x807FFFFF, 0x3F800000], dtype=np.uint32)     # +-0, NaN payloads, +-inf, denormals, 1.0


def _bits(n, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b[rng.integers(0, n, min(n, 3 * _SPECIAL.size))] = np.resize(_SPECIAL, min(n, 3 * _SPECIAL.size))
    return b


@pytest.mark.parametrize('n', [1, 3, 63, 64, 65, 1000, 4097, (1 << 20) + 7])
def test_digest_matches_numpy(dam, n):
    b = _bits(n, n)
    t = torch.from_numpy(b.view(np.int32)).cuda()
    want = _np_digest(b)
    assert _gpu_digest(t) == want
    assert _gpu_digest(t.view(torch.float32)) == want
    assert _gpu_digest(t, index_base=5) == _np_digest(b, 5)


def test_digest_is_independent_of_launch_splits(dam):
    n = 3 * 65536 + 11
    b = _bits(n, 1)
    t = torch.from_numpy(b.view(np.int32)).cuda()
    want = _gpu_digest(t)
    assert want == _np_digest(b)
    for blocks in (1, 2, 7, 300, 100000):
        assert _gpu_digest(t, max_blocks=blocks) == want
    from deep_audio_mixer_amd import ops
    for cuts in ([0, 1, n], [0, 63, 64, 5000, n], [0, n // 2, n]):
        out = torch.full((1,), 123, dtype=torch.int64, device='cuda')
        for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
            ops.digest64(t[lo:hi], out=out, index_base=lo, accumulate=k > 0, max_blocks=3 + k)
        assert int(out.item()) & _MASK == want
    empty = torch.empty(0, dtype=torch.float32, device='cuda')
    assert _gpu_digest(empty) == 0


def test_digest_changes_with_every_single_bit(dam):
    n = 40
    b = _bits(n, 2)
    base = _np_digest(b)
    t = torch.from_numpy(b.view(np.int32)).cuda()
    assert _gpu_digest(t) == base
    seen = set()
    for i in range(n):
        for k in range(32):
            f = b.copy()
            f[i] ^= np.uint32(1 << k)
            t.copy_(torch.from_numpy(f.view(np.int32)))
            d = _gpu_digest(t)
            assert d != base and d == _np_digest(f), (i, k)
            seen.add(d)
    assert len(seen) == 32 * n
    z = torch.tensor([0.0, -0.0], device='cuda')
    assert _gpu_digest(z[:1]) != _gpu_digest(z[1:])
    nans = torch.tensor([0x7FC00000, 0x7FC00001], dtype=torch.int32, device='cuda')
    assert _gpu_digest(nans[:1]) != _gpu_digest(nans[1:])
