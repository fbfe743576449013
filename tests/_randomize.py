"""Random, non-trivial parameters and running statistics for block-level tests (shared by test_eval_backward_gpu.py and
test_conv_epilogue_gpu.py)."""
import torch


def _running_stats(C, gen):
    """Non-trivial running statistics: mean in [-2, 2], var in [0.1, 10]."""
    return 4 * torch.rand(C, generator=gen) - 2, 10 ** (2 * torch.rand(C, generator=gen) - 1)


def _randomize(module, gen):
    """Parameters as tests/test_blocks_gpu.py, plus running statistics: mean in [-0.5, 0.5] (the blocks' inputs are of order 1)
    and var in [0.1, 10]."""
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                rm, rv = _running_stats(m.num_features, gen)
                m.running_mean.copy_(0.25 * rm), m.running_var.copy_(rv)
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (2.0 / (m.weight[0].numel())) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
    return module
