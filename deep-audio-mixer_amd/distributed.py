"""Data-parallel training over the GPUs of one node: one process per GPU, torch.distributed (backend "nccl" =
RCCL over xGMI on ROCm; "gloo" on CPU for tests).

The reference is single-device; the semantics defined here are: clips (chunks) are sharded
rank-strided over the replicas, BatchNorm statistics stay local to a replica, gradients are summed over ranks
in ONE flat bucket (12.6 MB for ResNet18: a single all-reduce, sized for xGMI's per-link bandwidth rather than
many small ones; engine.TrainStep's staged step cuts it in two) and divided by the world size, rank 0 logs and writes
checkpoints.  An N-GPU step therefore equals a reference step over N micro-batches with averaged gradients.
model_trainer.ModelTrainer.fit implements these semantics for every optimizer and criterion ("N GPUs").
"""
import os

import torch
import torch.distributed as dist
from torch.utils.data import Sampler


def init_process_group(backend=None, device=None):
    """Reads RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* from the environment (torch.distributed.run sets them)."""
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    local = int(os.environ.get('LOCAL_RANK', 0))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if backend is None:
            backend = 'nccl' if torch.cuda.is_available() else 'gloo'
        if backend == 'nccl':
            torch.cuda.set_device(local)
            dist.init_process_group(backend, device_id=device or torch.device('cuda', local))
        else:
            dist.init_process_group(backend)
    return rank, world, local


def shard_indices(n_items, rank, world, drop_last=True):
    """Rank-strided partition of the global chunk index space (i = rank mod world); with drop_last every rank
    gets the same number of items so that collectives line up."""
    n = (n_items // world) * world if drop_last else n_items
    return list(range(rank, n, world))


class DistributedChunkSampler(Sampler):
    """Sequential rank-strided sampler (the reference loaders use shuffle=False, training.ipynb cell 6)."""

    def __init__(self, dataset_len, rank=None, world=None):
        self.rank = dist.get_rank() if rank is None else rank
        self.world = dist.get_world_size() if world is None else world
        self.indices = shard_indices(dataset_len, self.rank, self.world)

    def __iter__(self):
        return iter(self.indices)

    def __len__(self):
        return len(self.indices)


def world_size(group=None):
    """Size of the process group; 1 when torch.distributed is not initialised."""
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _wire(t, group=None):
    """Where a small host-side collective travels: RCCL takes device tensors only, gloo carries CPU tensors itself."""
    return t.cuda() if dist.get_backend(group) == 'nccl' else t


def all_reduce_max_min(values, group=None):
    """Maximum and minimum over ranks of a list of int64 values, in ONE collective (MAX of [v, ~v]: ~ reverses the order of
    int64 without overflow).  Returns (max list, min list), identical on every rank."""
    n = len(values)
    t = torch.tensor(list(values) + [~int(v) for v in values], dtype=torch.int64)
    w = _wire(t, group)
    dist.all_reduce(w, op=dist.ReduceOp.MAX, group=group)
    t = w.cpu().tolist()
    return t[:n], [~v for v in t[n:]]


def check_equal_lengths(loader, what, group=None):
    """Every rank must run the same number of batches, or a rank would wait forever in the next collective.  One small
    collective compares len(loader) over ranks; on a mismatch, or a loader without __len__ on any rank, EVERY rank raises
    ValueError (before its first batch).  Returns the length."""
    try:
        n = len(loader)
    except TypeError:
        n = -1
    (hi,), (lo,) = all_reduce_max_min([n], group)
    if lo < 0:
        raise ValueError('%s: a loader without __len__ on at least one of %d ranks -- data-parallel training needs loaders of '
                         'a known, equal length (DataLoader(..., sampler=DistributedChunkSampler(len(dataset))))'
                         % (what, world_size(group)))
    if hi != lo:
        raise ValueError('%s: the ranks have between %d and %d batches -- data-parallel training needs loaders of equal length '
                         '(DistributedChunkSampler drops the last len(dataset) %% world items for that)' % (what, lo, hi))
    return n


def all_gather_floats(values, group=None):
    """[rank][i] table of every rank's float64 values (one collective); identical on every rank, so a sum taken over it in
    rank order is bit-identical everywhere."""
    t = _wire(torch.tensor([float(v) for v in values], dtype=torch.float64), group)
    parts = [torch.empty_like(t) for _ in range(world_size(group))]
    dist.all_gather(parts, t, group=group)
    return [p.cpu().tolist() for p in parts]


def broadcast_tensors(tensors, src=0, group=None):
    """Rank `src`'s values of the given tensors everywhere, one broadcast per dtype (the tensors are packed into one flat
    buffer, staged through host memory for gloo)."""
    if world_size(group) == 1:
        return
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault(t.dtype, []).append(t)
    for ts in by_dtype.values():
        flat = torch.cat([t.detach().reshape(-1) for t in ts])
        wire = flat if dist.get_backend(group) == 'nccl' else flat.cpu()
        dist.broadcast(wire, src, group=group)
        off = 0
        for t in ts:
            k = t.numel()
            t.data.copy_(wire[off:off + k].view(t.shape))
            off += k


def broadcast_module(module, src=0, group=None):
    """Identical replicas: rank `src`'s parameters and buffers everywhere."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    for t in list(module.parameters()) + list(module.buffers()):
        dist.broadcast(t.data, src, group=group)


def backward_late(loss, late_params, boundary):
    """Stage 1 of the cut backward pass: gradients of `loss` w.r.t. the parameters BEHIND the bucket boundary (the deep
    end of the trunk + heads) and w.r.t. the boundary activation; nothing in front of the boundary is touched.
    Returns (list of parameter gradients, d loss / d boundary)."""
    grads = torch.autograd.grad(loss, list(late_params) + [boundary], allow_unused=True)
    return list(grads[:-1]), grads[-1]          # (None for parameters whose gradient went straight into a bound slot)


def backward_early(boundary, d_boundary, early_params):
    """Stage 2: continues backward from the boundary activation into the layers in front of it; accumulates into the
    .grad of `early_params` (meant to run while the late bucket is on the wire)."""
    torch.autograd.backward([boundary], [d_boundary], inputs=list(early_params))


class GradBucket:
    """One flat gradient bucket for an arbitrary list of parameters (works on CPU/gloo and GPU/RCCL), for use with
    any torch optimizer:   loss.backward(); bucket.all_reduce_mean(); optimizer.step().
    (deep_audio_mixer_amd.optim.Adam carries its own flat bucket and folds the 1/world into its kernel.)"""

    def __init__(self, params, group=None):
        self.params = [p for p in params if p.requires_grad]
        if any(hasattr(p, '_dam_grad') for p in self.params):
            raise RuntimeError('these parameters have gradient slots bound (optim.Adam.bind_grad_slots / engine.TrainStep): '
                               'their .grad stays None, a GradBucket over them would all-reduce zeros -- unbind first '
                               '(TrainStep.close()) or use optim.Adam\'s own buckets')
        self.group = group
        n = sum(p.numel() for p in self.params)
        p0 = self.params[0]
        self.flat = torch.zeros(n, dtype=p0.dtype, device=p0.device)

    def _views(self):
        off = 0
        for p in self.params:
            k = p.numel()
            yield p, self.flat[off:off + k].view(p.shape)
            off += k

    def fill(self, grads=None):
        """p.grad (or the given gradients, parameter order) -> the flat bucket."""
        for i, (p, v) in enumerate(self._views()):
            g = p.grad if grads is None else grads[i]
            if g is None:
                v.zero_()
            else:
                v.copy_(g)

    def start_all_reduce(self):
        """Asynchronous SUM over the group; returns the work handle (None on a single rank)."""
        if dist.is_initialized() and dist.get_world_size(self.group) > 1:
            if self.flat.is_cuda and dist.get_backend(self.group) == 'gloo':
                # gloo stages a CUDA tensor on its own and stalls for seconds while the producing stream is busy
                # (optim._HostStagedAllReduce); once that stream is idle the exchange takes milliseconds
                torch.cuda.current_stream(self.flat.device).synchronize()
            return dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        return None

    def finish(self, work=None):
        """Waits for start_all_reduce, divides by the world size and writes the mean back into the .grad fields."""
        if work is not None:
            work.wait()
        world = dist.get_world_size(self.group) if dist.is_initialized() else 1
        if world > 1:
            self.flat.div_(world)
        for p, v in self._views():
            if p.grad is None:
                p.grad = v.clone()
            else:
                p.grad.copy_(v)
        return self.flat

    def all_reduce_mean(self):
        self.fill()
        return self.finish(self.start_all_reduce())


def all_gather_gains(local_gains, group=None):
    """Inference over a sharded chunk axis: gathers [n_local, S] gain blocks of equal size from every rank and
    interleaves them back into chunk order (rank-strided sharding)."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return local_gains
    world = dist.get_world_size(group)
    parts = [torch.empty_like(local_gains) for _ in range(world)]
    dist.all_gather(parts, local_gains.contiguous(), group=group)
    return torch.stack(parts, 1).reshape(-1, local_gains.shape[-1])
