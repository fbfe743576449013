"""Whole-model gradient comparison against the float64 oracle under a caller-chosen loss (tests/test_heads_gpu.py,
tests/test_eval_backward_gpu.py): the best-over-seeds rule of test_models_gpu.test_gradients_tight_when_no_relu_flips."""
import numpy as np
import torch

from _inputs import model_input
from oracle import dropout_ref, models_ref

GAIN_RTOL = 1e-4


def no_dropout(m):
    for mod in m.modules():
        if hasattr(mod, 'dropout_p'):
            mod.dropout_p = -1          # oracle blocks
        elif getattr(mod, 'dropout', None) is not None and not isinstance(mod, torch.nn.Dropout):
            mod.dropout = None          # product blocks
    return m


def ref_named_grads(model):
    """Gradients of the product model keyed by the REFERENCE parameter names."""
    out = {}
    for n, p in model.named_parameters():
        if not n.startswith('_heads.'):
            out[n] = p.grad
    h = model._heads
    for i in range(h.n_stems):
        out['conv_head%d.weight' % (i + 1)] = h.conv_w.grad[i]
        out['conv_head%d.bias' % (i + 1)] = h.conv_b.grad[i:i + 1]
        out['fc_head%d.weight' % (i + 1)] = h.fc_w.grad[i]
        out['fc_head%d.bias' % (i + 1)] = h.fc_b.grad[i:i + 1]
    return out


def host_dropout_masks(ref, batch, hw, seed, offset):
    """The five keep masks (bool NCHW tensors) a scalar model's training-mode forward draws on the device when its dropout
    counter stands at `offset` and torch's seed is `seed` (oracle/dropout_ref.py), and the counter after that forward."""
    shapes = models_ref.scalar_block_shapes(batch, hw[0], hw[1], ref.first_dilation)
    ps = [getattr(ref, 'conv_b%d' % i).dropout_p for i in range(1, 6)]
    masks, end = dropout_ref.block_keep_masks(seed, offset, shapes, ps)
    return [torch.from_numpy(m) for m in masks], end


def best_over_seeds(ctor, ref_ctor, shape, loss_dev, loss_ref, eval_mode=False, seeds=(31, 32, 33, 34), dropout=False):
    """loss_dev(model, x, gt) / loss_ref(ref, x, gt) -> (scalar loss to backward, gains [B, S]) on the product model (cuda
    float32) and on the oracle (float32 and float64 CPU copies).  eval_mode: the product model first runs three training-mode
    forwards so that its running statistics are real, then all three models take them and switch to eval().

    For every parameter tensor the BEST agreement with float64 over the seeds must reach float32 level (3x the CPU float32
    oracle's own best distance, floor 2e-5 of the tensor norm): one ReLU decision flipped by rounding moves the gradients
    upstream of it by ~1e-3 in any float32 run, a wrong kernel is off in every run.  Returns {tensor: best error}.

    dropout (scalar models, training mode): dropout stays ON in all three models.  The device draws its masks from
    (torch.initial_seed(), its call counter); before every device forward the counter is read and both oracles are handed
    the host restatement of those masks (offsets: counter + running sum of the five block outputs' element counts).  The
    counter must have advanced by exactly that sum after the step.  Everything else, every bound included, is unchanged."""
    from deep_audio_mixer_amd import ops
    torch.set_num_threads(16)
    s, hw = shape[1], shape[2:]
    strip = (lambda m: m) if dropout else no_dropout
    assert not (dropout and eval_mode)
    ref32 = strip(models_ref.closed_form_fill(ref_ctor(n_stems=s, input_shape=hw))).train()
    ref64 = strip(models_ref.closed_form_fill(ref_ctor(n_stems=s, input_shape=hw))).double().train()
    model = strip(ctor(n_stems=s, input_shape=hw))
    if dropout:
        assert [getattr(model, 'conv_b%d' % i).dropout.p for i in range(1, 6)] == [0.2, 0.2, 0.2, 0.2, 0.3]
    model.load_state_dict(ref32.state_dict())
    model = model.cuda().train()
    if eval_mode:
        with torch.no_grad():
            for seed in (41, 42, 43):
                model(torch.from_numpy(model_input(*shape, seed=seed)[0]).cuda())
        for m in (model, ref32, ref64):
            m.eval()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    if eval_mode:
        rv = [v for k, v in state.items() if k.endswith('running_var')]
        assert rv and all(float((v - 1).abs().max()) > 1e-3 for v in rv), 'running statistics did not move'
    names = [n for n, _ in ref64.named_parameters()]
    best_hip, best_cpu = {n: np.inf for n in names}, {n: np.inf for n in names}
    for seed in seeds:
        x, gt = model_input(*shape, seed=seed)
        for m in (ref32, ref64, model):
            m.load_state_dict(state)
            m.zero_grad()
        if dropout:
            c0 = ops.dropout_counter(torch.device('cuda', torch.cuda.current_device()))
            masks, c_end = host_dropout_masks(ref64, shape[0], hw, torch.initial_seed(), c0)
            models_ref.set_keep_masks(ref32, masks), models_ref.set_keep_masks(ref64, masks)
        for ref, dt in ((ref32, torch.float32), (ref64, torch.float64)):
            loss_r, gains_r = loss_ref(ref, torch.from_numpy(x).to(dt), torch.from_numpy(gt).to(dt))
            loss_r.backward()
            if dt == torch.float64:
                gains64, loss64 = gains_r.detach(), float(loss_r.detach())
        loss, gains = loss_dev(model, torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda())
        loss.backward()
        if dropout:
            c1 = ops.dropout_counter(torch.device('cuda', torch.cuda.current_device()))
            assert c1 - c0 == c_end - c0 == sum(m.numel() for m in masks), (seed, c0, c1, c_end)
        e_g = float((gains.detach().double().cpu() - gains64).abs().max() / gains64.abs().max())
        assert e_g <= GAIN_RTOL, ('gains', seed, e_g)
        assert abs(float(loss) - loss64) <= 2e-4 * abs(loss64), ('loss', seed, float(loss), loss64)
        grads = ref_named_grads(model)
        p32 = dict(ref32.named_parameters())
        gmax = max(p.grad.norm().item() for p in ref64.parameters())
        for n, p in ref64.named_parameters():
            truth = p.grad.flatten()
            scale = truth.norm().item() + 1e-5 * gmax
            e_hip = (grads[n].detach().double().cpu().flatten() - truth).norm().item() / scale
            e_cpu = (p32[n].grad.double().flatten() - truth).norm().item() / scale
            assert e_hip <= 1e-1, (n, seed, e_hip)
            best_hip[n], best_cpu[n] = min(best_hip[n], e_hip), min(best_cpu[n], e_cpu)
    rows = sorted(((best_hip[n] / max(best_cpu[n], 2e-5 / 3), n, best_hip[n], best_cpu[n]) for n in names), reverse=True)
    print('worst (ratio, tensor, best hip err, best cpu-f32 err): %s'
          % [(round(r, 2), n, '%.1e' % a, '%.1e' % b) for r, n, a, b in rows[:4]])
    bad = [(n, a, b) for r, n, a, b in rows if a > max(3 * b, 2e-5)]
    assert not bad, bad[:5]
    return best_hip
