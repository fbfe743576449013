"""Whole-model gradient comparison against the float64 oracle under a caller-chosen loss (tests/test_heads_gpu.py,
tests/test_eval_backward_gpu.py): the best-over-seeds rule of test_models_gpu.test_gradients_tight_when_no_relu_flips."""
import numpy as np
import torch

from _inputs import model_input
from oracle import models_ref

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


def best_over_seeds(ctor, ref_ctor, shape, loss_dev, loss_ref, eval_mode=False, seeds=(31, 32, 33, 34)):
    """loss_dev(model, x, gt) / loss_ref(ref, x, gt) -> (scalar loss to backward, gains [B, S]) on the product model (cuda
    float32) and on the oracle (float32 and float64 CPU copies).  eval_mode: the product model first runs three training-mode
    forwards so that its running statistics are real, then all three models take them and switch to eval().

    For every parameter tensor the BEST agreement with float64 over the seeds must reach float32 level (3x the CPU float32
    oracle's own best distance, floor 2e-5 of the tensor norm): one ReLU decision flipped by rounding moves the gradients
    upstream of it by ~1e-3 in any float32 run, a wrong kernel is off in every run.  Returns {tensor: best error}."""
    torch.set_num_threads(16)
    s, hw = shape[1], shape[2:]
    ref32 = no_dropout(models_ref.closed_form_fill(ref_ctor(n_stems=s, input_shape=hw))).train()
    ref64 = no_dropout(models_ref.closed_form_fill(ref_ctor(n_stems=s, input_shape=hw))).double().train()
    model = no_dropout(ctor(n_stems=s, input_shape=hw))
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
        for ref, dt in ((ref32, torch.float32), (ref64, torch.float64)):
            loss_r, gains_r = loss_ref(ref, torch.from_numpy(x).to(dt), torch.from_numpy(gt).to(dt))
            loss_r.backward()
            if dt == torch.float64:
                gains64, loss64 = gains_r.detach(), float(loss_r.detach())
        loss, gains = loss_dev(model, torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda())
        loss.backward()
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
