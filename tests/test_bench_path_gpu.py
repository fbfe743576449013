"""GPU: the EXACT objects bench.py times for BASELINE config C3 -- `bench.build_model(C3)` (ResNet18, 8 stems, 1025 x 130),
`Adam(weight_decay=1e-5)`, `TrainStep(batch=8, use_graph=True)` over `bench.synth_clips` -- replayed for three
steps from the initial replica, every step compared with the CPU oracle on the same clips:
`oracle.features_ref.clip_features` (numpy STFT) -> `models_ref.RefResNet18` in float64 -> loss, backward; Adam by
torch.optim.Adam's update rule in float64 (model_trainer.py:25-44 + training.ipynb cell 11 of the reference).

Every step is checked FROM THE STATE THE DEVICE RUN HAD BEFORE IT (parameters, BatchNorm buffers, Adam moments are handed to
the oracle step by step).  A free-running comparison is meaningless after the first update: lr 1e-3 sign-like Adam steps on
a fresh network are chaotic at the 1e-2 level -- measured on the oracle itself, float32 against float64 from identical
weights and clips: loss 3e-7 / 2.7e-3 / 2.7e-2 apart at steps 1 / 2 / 3, gains 4e-6 / 1.8e-2 / 6e-2 (tools/ note in DESIGN.md
section 2).  Step by step, everything is deterministic and tight: forward at north_star's 1e-4, the optimizer at float32
rounding; gradients at the whole-model tolerance (ReLU decision flips, see tests/test_blocks_gpu.py for the tight check).

C1 and C2 (the scalar models) are pinned twice: with dropout stripped, and AS BUILT -- bench.build_model returns them in
train() mode with dropout on, and that is what bench.py times.  The device's dropout mask is a pure function of
(torch.initial_seed(), the device-side call counter, element index); oracle/dropout_ref.py restates it on the host, so in
the `_with_dropout` tests the oracle applies the SAME masks, at the offset the counter had before each replay, and every
threshold is the dropout-off one.  They also assert that a replay advances the counter exactly as an eager step does, that
block 1's output is exactly zero wherever the host mask drops, and that the three replays' block-1 masks differ."""
import numpy as np
import pytest
import torch

from _inputs import feature_error
from oracle import dropout_ref, features_ref, models_ref

pytestmark = pytest.mark.gpu


def _ref_state(model):
    """Reference-keyed float64 CPU copy of the product model's state."""
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in model.state_dict().items()}


def _ref_named_flat(model, flat, opt):
    """Slices of one of the optimizer's flat buffers keyed by the REFERENCE parameter names (heads are stored stacked)."""
    out = {}
    for (n, p), lo, hi in zip(model.named_parameters(), opt._offsets[:-1], opt._offsets[1:]):
        out[n] = flat[lo:hi].view(p.shape)
    h = model._heads
    for key, ref in (('_heads.conv_w', 'conv_head%d.weight'), ('_heads.conv_b', 'conv_head%d.bias'),
                     ('_heads.fc_w', 'fc_head%d.weight'), ('_heads.fc_b', 'fc_head%d.bias')):
        t = out.pop(key)
        for i in range(h.n_stems):
            out[ref % (i + 1)] = t[i]
    return out


def _no_dropout(m):
    """The dropout-off form of the comparison (the `_with_dropout` tests run the models as built, the oracle applying the
    host restatement of the device's masks)."""
    for mod in m.modules():
        if hasattr(mod, 'dropout_p'):
            mod.dropout_p = -1          # oracle blocks
        elif getattr(mod, 'dropout', None) is not None and not isinstance(mod, torch.nn.Dropout):
            mod.dropout = None          # product blocks
    return m


def _captured_step_matches_oracle(cfg_name, ref_ctor, feature_pairs, bn_keys, expect_descent=False, dropout=False):
    import bench
    from deep_audio_mixer_amd.engine import TrainStep
    from deep_audio_mixer_amd.optim import Adam
    cfg = bench.CONFIGS[cfg_name]
    S, Bsz, hop = cfg['n_stems'], cfg['batch'], cfg['hop']
    n = cfg['sr'] * cfg['seconds']
    device = torch.device('cuda', 0)
    strip = (lambda m: m) if dropout else _no_dropout
    model = strip(bench.build_model(cfg, device))
    assert model.training
    b1_out = {}
    if dropout:
        from deep_audio_mixer_amd import ops
        assert [getattr(model, 'conv_b%d' % i).dropout.p for i in range(1, 6)] == [0.2, 0.2, 0.2, 0.2, 0.3]
        # block 1's output of the captured forward stays referenced, so the graph's pool does not hand its memory to a later
        # allocation and it can be read after every replay (no launch is added to the step)
        model.conv_b1.register_forward_hook(lambda mod, inp, out: b1_out.__setitem__('out', out.detach()))
    state0 = _ref_state(model)
    lr, wd, b1, b2, eps = 1e-3, 1e-5, 0.9, 0.999, 1e-8
    opt = Adam(model.parameters(), weight_decay=wd)
    n_steps = 3
    clips = bench.synth_clips(n_steps * Bsz, S, n, device, 1234)
    step = TrainStep(model, opt, S, n, bench.CHANNELS, Bsz, bench.N_FFT, hop, use_graph=True)
    step.load_clips(clips[:Bsz])
    F_, T_ = bench.N_FFT // 2 + 1, 1 + n // hop
    if dropout:
        shapes = models_ref.scalar_block_shapes(Bsz, F_, T_, ref_ctor.first_dilation)
        per_step = sum(int(np.prod(sh)) for sh in shapes)
        c_before = ops.dropout_counter(device)
    step.capture(warmup=2)
    assert step._graphs is not None and len(step._graphs) == 1            # one hipGraph holds the whole step
    if dropout:
        # two eager warm-up steps drew per_step counters each; capturing draws nothing
        assert ops.dropout_counter(device) == c_before + 2 * per_step
        assert tuple(b1_out['out'].shape) == shapes[0]
        drop_seed = torch.initial_seed()            # (bench.build_model seeds torch; the captured launches carry this seed)
        ps = [b[2] for b in models_ref.SCALAR_BLOCKS]
        b1_masks = []
    # rewind to the initial replica (capture's eager warm-up steps moved parameters, moments and running statistics)
    model.load_state_dict({k: v.to(device) for k, v in state0.items()})
    opt._exp_avg.zero_(), opt._exp_avg_sq.zero_(), opt._step.zero_()

    torch.set_num_threads(16)
    ref = strip(ref_ctor(n_stems=S, input_shape=(F_, T_))).double().train()
    ref32 = strip(ref_ctor(n_stems=S, input_shape=(F_, T_))).train()
    host = clips.cpu().numpy()
    rel = lambda a, b: float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
    losses = []
    for k in range(n_steps):
        before = _ref_state(model)
        p0, m0, v0 = opt._flat.double().cpu(), opt._exp_avg.double().cpu(), opt._exp_avg_sq.double().cpu()
        step.bind_clips(clips[k * Bsz:(k + 1) * Bsz])
        if dropout:
            c0 = ops.dropout_counter(device)
            assert torch.initial_seed() == drop_seed
        loss = step().item()
        torch.cuda.synchronize()
        if dropout:
            # the replay advanced the device counter exactly as an eager step does, and drew the masks of ITS offset
            assert ops.dropout_counter(device) == c0 + per_step, (k, c0, ops.dropout_counter(device), per_step)
            masks, _ = dropout_ref.block_keep_masks(drop_seed, c0, shapes, ps)
            masks = [torch.from_numpy(m) for m in masks]
            models_ref.set_keep_masks(ref, masks), models_ref.set_keep_masks(ref32, masks)
            out1 = b1_out['out'].permute(0, 3, 1, 2).cpu()
            assert bool((out1[~masks[0]] == 0).all()), 'replay %d: block 1 kept an element the host mask drops' % k
            b1_masks.append((out1 != 0, masks[0]))
        gains = torch.cat(step.gains, 1).cpu().numpy().astype(np.float64)
        masked = step.masked[:, ::41, ::7].cpu().numpy().astype(np.float64)
        g_dev = opt._grad.double().cpu()
        after = _ref_state(model)
        assert int(opt._step.item()) == k + 1
        # ---- oracle from the same state: numpy front-end on the same PCM, float64 model
        ref.load_state_dict(before)
        items = [features_ref.clip_features(host[k * Bsz + b], bench.N_FFT, hop, np.float32) for b in range(Bsz)]
        x = torch.from_numpy(np.stack([i[0] for i in items])).double()
        gt = torch.from_numpy(np.stack([i[1] for i in items])).double()
        with torch.no_grad():
            masked_r, gains_r = ref(x)
            loss_r = torch.nn.functional.mse_loss(masked_r, gt)
        rs = {k_: v.clone() for k_, v in ref.state_dict().items()}      # running statistics after the numpy-feature forward
        e_loss = abs(loss - loss_r.item()) / loss_r.item()
        e_gain = rel(gains, torch.cat(gains_r, 1).detach().numpy())
        e_mask = rel(masked, masked_r.detach()[:, ::41, ::7].numpy())
        # north_star: gains within 1e-4 relative of the reference CPU path; loss 2e-4 (as the golden model tests)
        assert e_loss <= 2e-4 and e_gain <= 1e-4 and e_mask <= 1e-4, (k, e_loss, e_gain, e_mask)
        # The front-end itself against the numpy oracle, in the measure the feature tests use (linear magnitude relative to the
        # frame peak; dB only away from spectral nulls, where rounding is amplified without bound)
        x_dev = step.x.cpu().numpy()
        for b_, s_ in feature_pairs:
            rel_lin, db = feature_error(x_dev[b_, s_], items[b_][0][s_])
            assert rel_lin <= 2e-6 and db <= 2e-3, (k, b_, s_, rel_lin, db)
        # Gradients of the whole model: the oracle is fed the DEVICE's features here.  Five of the 8.5 M bins of a batch sit in
        # spectral nulls and differ by up to 0.1 dB between any two float32 STFTs; loss and gains do not care (checked above
        # from the numpy features) but an ill-conditioned gradient can: in the state after the first update the reference's own
        # conv_head1 gradient moves by 11 % (its bias gradient by a factor 2.3) when those five bins change
        # (tools/head_grad_debug.py) -- with the same features the device agrees to 7e-6 on every head tensor.  In the trunk
        # every float32 ReLU decision flip moves the tensors upstream of it by 2-5e-3, in ANY float32 implementation, so the
        # yardstick is the CPU oracle in float32 from the same state and features: a tensor passes at 3 x that oracle's own
        # distance to float64 (floor 2e-2).  The tight, deterministic gradient checks are per block
        # (tests/test_blocks_gpu.py: 2e-5 on every gradient of every block at these shapes)
        xd, gtd = step.x.cpu(), step.gt.cpu()
        ref.load_state_dict(before)
        ref.zero_grad()
        masked_d, _ = ref(xd.double())
        torch.nn.functional.mse_loss(masked_d, gtd.double()).backward()
        ref32.load_state_dict({k_: (v.float() if v.is_floating_point() else v) for k_, v in before.items()})
        ref32.zero_grad()
        masked32, _ = ref32(xd)
        torch.nn.functional.mse_loss(masked32, gtd).backward()
        g32 = {n_: p_.grad.double() for n_, p_ in ref32.named_parameters()}
        named = _ref_named_flat(model, g_dev, opt)
        gmax = max(p.grad.norm().item() for p in ref.parameters())
        errs = []
        for name, p in ref.named_parameters():
            if name.endswith('.conv.bias'):
                # a convolution bias in front of a training-mode BatchNorm has an exactly-zero true gradient (the mean is
                # subtracted again): every implementation returns rounding noise, compared with the model's gradient scale
                assert named[name].norm().item() <= 1e-4 * gmax, (k, name, named[name].norm().item(), gmax)
                continue
            scale = p.grad.norm().item() + 1e-5 * gmax
            e = (named[name].reshape(p.grad.shape) - p.grad).norm().item() / scale
            e32 = (g32[name] - p.grad).norm().item() / scale
            errs.append((e / max(3 * e32, 2e-2), name, e, e32))
        errs.sort(reverse=True)
        worst = max(e_[2] for e_ in errs)
        assert errs[0][0] <= 1.0, (k, [(n_, 'hip %.2e' % a, 'cpu-f32 %.2e' % b) for _, n_, a, b in errs[:6]])
        # Adam(+L2) of the captured step == torch.optim.Adam's rule applied to the step's OWN gradient, in float64
        t = k + 1
        g = g_dev + wd * p0
        m1, v1 = b1 * m0 + (1 - b1) * g, b2 * v0 + (1 - b2) * g * g
        want = p0 - (lr / (1 - b1 ** t)) * m1 / (v1.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        e_adam = (opt._flat.double().cpu() - want).abs().max().item()
        assert e_adam <= 3e-7, (k, e_adam)
        assert (opt._exp_avg.double().cpu() - m1).abs().max().item() <= 1e-6 * m1.abs().max().item()
        assert (opt._exp_avg_sq.double().cpu() - v1).abs().max().item() <= 1e-6 * v1.abs().max().item()
        # BatchNorm running statistics: the oracle's forward updated its buffers from the same starting values
        for key in bn_keys:
            np.testing.assert_allclose(after[key].numpy(), rs[key].numpy(), rtol=2e-5, atol=1e-6, err_msg='%d %s' % (k, key))
        nbt = bn_keys[0].rsplit('.', 1)[0] + '.num_batches_tracked'
        assert int(after[nbt]) == int(before[nbt]) + 1
        print('step %d: loss %.6f (oracle %.6f, rel %.1e) gains %.1e masked %.1e | worst grad tensor %.1e | adam max err %.1e'
              % (k, loss, loss_r.item(), e_loss, e_gain, e_mask, worst, e_adam))
        losses.append(loss)
    if dropout:
        for i in range(3):
            for j in range(3):
                if i != j:
                    # replay i's block-1 mask is not replay j's: device against device, host against host, device against host
                    assert not torch.equal(b1_masks[i][0], b1_masks[j][0]) and not torch.equal(b1_masks[i][1], b1_masks[j][1])
                    assert bool(b1_masks[i][0][~b1_masks[j][1]].any()), (i, j)
    if expect_descent:
        assert losses[-1] < losses[0]                                    # and it trains


def test_c3_captured_step_matches_oracle(dam_lib):
    """BASELINE config C3: model_resnet, 8 stems, 3 s @ 44.1 kHz, batch 8 -- the driver's bench line."""
    _captured_step_matches_oracle('C3', models_ref.RefResNet18, ((0, 0), (3, 5), (7, 7)),
                                  ('bn1.running_mean', 'bn1.running_var', 'layer1.1.bn2.running_var', 'layer3.0.bn2.running_mean',
                                   'layer3.0.shortcut.1.running_var', 'layer6.1.bn2.running_var'), expect_descent=True)


def test_c2_captured_step_matches_oracle(dam_lib):
    """BASELINE config C2: model_scalar_2s (models/model_scalar_2s.py:64-132: dilated strided stem, valid 5 / 5 / 7 / 9
    convolutions with bias, BatchNorm eps 1e-3 momentum 0.9), 4 stems, 3 s @ 44.1 kHz, batch 4 -- `bench.py --config C2`'s
    objects, captured, three steps against the float64 oracle from the device's state."""
    _captured_step_matches_oracle('C2', models_ref.RefMixingModelScalar2s, ((0, 0), (2, 1), (3, 3)),
                                  ('conv_b1.batch_norm.running_mean', 'conv_b1.batch_norm.running_var',
                                   'conv_b3.batch_norm.running_var', 'conv_b5.batch_norm.running_mean'))


def test_c1_captured_step_matches_oracle(dam_lib):
    """BASELINE config C1: model_scalar_1s (models/model_scalar_1s.py:207-275), 2 stems, 1 s @ 16 kHz, hop 256, batch 8."""
    _captured_step_matches_oracle('C1', models_ref.RefMixingModelScalar1s, ((0, 0), (5, 1), (7, 0)),
                                  ('conv_b1.batch_norm.running_mean', 'conv_b2.batch_norm.running_var',
                                   'conv_b5.batch_norm.running_var'))


def test_c2_captured_step_matches_oracle_with_dropout(dam_lib):
    """C2 exactly as bench.py times it: `bench.build_model(C2)` untouched (train mode, dropout 0.2 x 4 / 0.3 ON), captured,
    three replays from the device's state; the float64 oracle applies the host restatement of the device's masks at the
    offset the counter had before each replay.  Thresholds of the dropout-off test."""
    _captured_step_matches_oracle('C2', models_ref.RefMixingModelScalar2s, ((0, 0), (2, 1), (3, 3)),
                                  ('conv_b1.batch_norm.running_mean', 'conv_b1.batch_norm.running_var',
                                   'conv_b3.batch_norm.running_var', 'conv_b5.batch_norm.running_mean'), dropout=True)


def test_c1_captured_step_matches_oracle_with_dropout(dam_lib):
    """C1 exactly as bench.py times it (model_scalar_1s, 2 stems, 1 s @ 16 kHz, hop 256, batch 8, dropout ON)."""
    _captured_step_matches_oracle('C1', models_ref.RefMixingModelScalar1s, ((0, 0), (5, 1), (7, 0)),
                                  ('conv_b1.batch_norm.running_mean', 'conv_b2.batch_norm.running_var',
                                   'conv_b5.batch_norm.running_var'), dropout=True)


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(dam_lib, tmp_path):
    """`python bench.py --steps K --warmup W --dump-outputs DIR` as a fresh process: one JSON line with the headline only (the
    regions and probes of --full are not run) and the last timed step's outputs -- loss, masked mix, gains, parameters,
    BatchNorm running statistics -- as float32 .npy files under DIR."""
    import json
    import os
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out_dir = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '3', '--warmup', '1',
                        '--dump-outputs', str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['metric'] == 'stem-spectrogram-frames/sec (train)' and line['unit'] == 'stem-spectrogram-frames/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32' and line['steps'] == 3 and line['warmup'] == 1
    assert line['ms_per_step'] > 0 and line['value'] > 0
    assert not {'repeat', 'roofline', 'cpu_baseline', 'pcie_inclusive', 'per_rank', 'overlap_ab'} & set(line)
    cfg = bench.CONFIGS['C3']
    B, S, t = cfg['batch'], cfg['n_stems'], 1 + cfg['sr'] * cfg['seconds'] // cfg['hop']
    got = {f[:-4]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert set(got) == {'loss', 'masked', 'gains', 'params', 'buffers'}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got['masked'].shape == (B, bench.N_FFT // 2 + 1, t) and got['gains'].shape == (B, S)
    assert got['loss'].shape == (1,) and got['loss'][0] == np.float32(line['config']['final_loss'])
    with torch.random.fork_rng(devices=[]):          # (build_model seeds torch's generator)
        model = bench.build_model(cfg, torch.device('cpu'))
    assert got['params'].size == sum(p.numel() for p in model.parameters())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT_BYTES
