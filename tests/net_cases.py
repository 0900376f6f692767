"""Nets that look trained, for the tests of the PV-net kernels: a freshly initialised Net has BatchNorm running mean 0, variance 1,
gamma 1 and beta 0, so every per-channel (scale, shift) a kernel applies is (1, 0) and a wrong channel index, a shift on the wrong
side of the residual add or a sign slip under LeakyReLU is the identity.  drifted_net gives every channel its own statistics."""
import copy

import numpy as np
import torch

from alphazero_openspiel_amd import fusednet
from alphazero_openspiel_amd.network import Net, ResidualBlock


def drifted_net(shape, A, n_blocks, n_filters, seed, w_scale=1.0):
    """Net(shape, A) in eval mode with seeded BatchNorm statistics - running mean in +-0.3, running variance in [0.25, 1.75], gamma of
    magnitude [0.5, 1.5] and negative with probability 0.25, beta in +-0.3 - and every conv weight multiplied by w_scale."""
    torch.manual_seed(seed)
    net = Net(shape, A, n_blocks=n_blocks, n_filters=n_filters)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.6 * torch.rand(n, generator=g) - 0.3)
                m.running_var.copy_(0.25 + 1.5 * torch.rand(n, generator=g))
                sign = torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0)
                m.weight.copy_(sign * (0.5 + torch.rand(n, generator=g)))
                m.bias.copy_(0.6 * torch.rand(n, generator=g) - 0.3)
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.mul_(w_scale)
    return net.eval()


def boards(shape, n, seed):
    """n random boards [n, shape[0] + 1, H, W]: random 0/1 observation planes and an alternating current-player plane."""
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(n, shape[0] + 1, shape[1], shape[2], generator=g) > 0.6).float()
    obs[:, shape[0]] = (torch.arange(n) % 2).float()[:, None, None]
    return obs


def tower_fp64(net, obs):
    """The tower output (the residual stream that fc1 reads) of net for obs in float64: [B][H*W][F]."""
    return fusednet.fold_forward(fusednet.fold_net(net), np.asarray(obs, dtype=np.float64))[2]


def max_activation_fp64(net, obs):
    """The largest magnitude any layer of net puts out for obs, in float64."""
    n64 = copy.deepcopy(net).double()
    top = [float(obs.abs().max())]
    hooks = [m.register_forward_hook(lambda _m, _i, out: top.append(float(out.abs().max())))
             for m in n64.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.BatchNorm2d, torch.nn.Linear, ResidualBlock))]
    with torch.no_grad():
        n64(obs.double())
    for h in hooks:
        h.remove()
    return max(top)
