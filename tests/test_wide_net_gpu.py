"""The wide PV-net path (az_net_create_wide: one az_conv_wide_kernel launch per conv) on the GPU: fp32-grade and fp16
accuracy against fp64, batch invariance, nets the tuned kernels refuse (more than 56 filters, a conv weight >= 32), and
self-play with a 64-filter net."""
import copy

import numpy as np
import pytest
import torch

from alphazero_openspiel_amd import fusednet
from alphazero_openspiel_amd.network import Net

pytestmark = pytest.mark.gpu

C4 = [3, 6, 7]


def _net(shape, A, nb, F, seed):
    torch.manual_seed(seed)
    net = Net(shape, A, n_blocks=nb, n_filters=F)
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():  # drifted eval-mode statistics: the fold is exercised
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(0.2 * torch.rand(n, generator=g) - 0.1)
            m.running_var.copy_(0.5 + torch.rand(n, generator=g))
            m.weight.data.copy_(0.75 + 0.5 * torch.rand(n, generator=g))
            m.bias.data.copy_(0.2 * torch.rand(n, generator=g) - 0.1)
    return net.eval()


def _boards(shape, n, seed):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(n, shape[0] + 1, shape[1], shape[2], generator=g) > 0.6).float()
    obs[:, shape[0]] = (torch.arange(n) % 2).float()[:, None, None]  # the current-player plane
    return obs


def _refs(net, obs):
    """(fp64 priors, fp64 values, torch fp32's max error against them), all run on the GPU."""
    with torch.no_grad():
        n64 = copy.deepcopy(net).double().cuda()
        p64, v64 = n64(obs.double().cuda())
        p32, v32 = copy.deepcopy(net).cuda()(obs.cuda())
    e32 = max((p32.double() - p64).abs().max().item(), (v32.double() - v64).abs().max().item())
    return p64, v64[:, 0], e32


def _err(fn, obs, p64, v64):
    pf, vf = fn.forward(obs.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(pf).all() and torch.isfinite(vf).all()
    assert (pf.double().sum(1) - 1).abs().max().item() < 1e-5
    return max((pf.double() - p64).abs().max().item(), (vf.double() - v64).abs().max().item())


@pytest.mark.parametrize("shape,A,nb,F,ns", [
    (C4, 7, 5, 64, (37,)),
    (C4, 7, 10, 128, (1, 37, 700, 4096)),
    ([3, 6, 6], 432, 3, 96, (40,)),
    ([3, 8, 8], 768, 2, 128, (37,)),
    (C4, 7, 2, 256, (100,)),
    ([3, 5, 4], 240, 2, 72, (33,)),
])
def test_wide_f32x_is_fp32_grade(shape, A, nb, F, ns):
    net = _net(shape, A, nb, F, seed=F + nb)
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=max(ns), precision="f32x")
    assert fn.wide and "az_conv_wide_kernel<X3> x%d" % (2 * nb) in fn.kernel_label()
    obs_all = _boards(shape, max(ns), seed=F)
    for n in ns:
        obs = obs_all[:n].contiguous()
        p64, v64, e32 = _refs(net, obs)
        ex = _err(fn, obs, p64, v64)
        print("wide f32x %s %dx%d n=%d: max err vs fp64 %.3g (torch fp32: %.3g)" % (shape, nb, F, n, ex, e32))
        assert ex <= max(4.0 * e32, 2e-6), (n, ex, e32)
        if n <= 40:  # the tower output against the fold's float64 forward
            _, _, tower = fusednet.fold_forward(fn.folded, obs.numpy().astype(np.float64))
            got = fn.read_tower(n)
            assert got.shape == (n, shape[1] * shape[2], fusednet.wide_fpad(F)) and not got[:, :, F:].any()
            assert np.abs(got[:, :, :F] - tower).max() / (np.abs(tower).max() + 1e-6) < 2e-5
    fn.close()


@pytest.mark.parametrize("shape,A,nb,F", [(C4, 7, 5, 64), ([3, 6, 6], 432, 3, 96)])
def test_wide_f16_error_is_bounded_by_torch_fp16(shape, A, nb, F):
    net = _net(shape, A, nb, F, seed=7)
    obs = _boards(shape, 256, seed=3)
    p64, v64, _ = _refs(net, obs)
    with torch.no_grad():
        p16, v16 = copy.deepcopy(net).half().cuda()(obs.half().cuda())
    e16 = max((p16.double() - p64).abs().max().item(), (v16.double()[:, 0] - v64).abs().max().item())
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=256, precision="f16")
    assert "az_conv_wide_kernel<F16>" in fn.kernel_label()
    ex = _err(fn, obs, p64, v64)
    print("wide f16 %dx%d: max err vs fp64 %.3g (torch fp16: %.3g)" % (nb, F, ex, e16))
    assert ex <= 2.0 * e16, (ex, e16)
    fn.close()


@pytest.mark.parametrize("precision", ["f32x", "f16"])
def test_wide_outputs_do_not_depend_on_the_batch_size(precision):
    net = _net(C4, 7, 3, 128, seed=11)
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=4096, precision=precision)
    obs = _boards(C4, 4096, seed=5).cuda()
    ref_p, ref_v = [t.clone() for t in fn.forward(obs)]
    torch.cuda.synchronize()
    ref_t = fn.read_tower(4096)
    for n in (1500, 513, 512, 64, 5, 1):
        p, v = fn.forward(obs[:n].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(p, ref_p[:n]) and torch.equal(v, ref_v[:n]), n
        assert (fn.read_tower(n) == ref_t[:n]).all(), n
    fn.close()


def test_a_large_conv_weight_takes_the_wide_path():
    torch.manual_seed(1)
    base = Net(C4, 7, n_blocks=5, n_filters=50).eval()
    normal = fusednet.FusedNet(base, "cuda:0", max_boards=4096, precision="f32x")
    assert not normal.wide
    labels = {n: normal.kernel_label(n) for n in (4096, 1500, 1024, 300)}
    assert labels[4096].startswith("az_tower_x3d_kernel") and labels[1500].startswith("az_tower_x3d_kernel")
    assert labels[1024].startswith("az_tower_x3b_kernel") and labels[300].startswith("az_tower_x3c_kernel")
    normal.close()
    net = copy.deepcopy(base)
    with torch.no_grad():
        net.resblock2.conv1.weight[3, 7, 1, 1] = 100.0  # the narrow path keeps weights x 2048 in fp16: refused there
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=512, precision="f32x")
    assert fn.wide and "az_conv_wide_kernel<X3>" in fn.kernel_label()
    obs = _boards(C4, 512, seed=9)
    p64, v64, e32 = _refs(net, obs)
    ex = _err(fn, obs, p64, v64)
    print("wide f32x, |w| = 100: max err vs fp64 %.3g (torch fp32: %.3g)" % (ex, e32))
    assert ex <= max(4.0 * e32, 2e-6), (ex, e32)
    fn.close()


def test_self_play_with_a_64_filter_net():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    torch.manual_seed(2)
    net = Net(C4, 7, n_filters=64).eval()
    runs = []
    for slots in (256, 64):
        gen = ExampleGenerator(net, "connect_four", torch.device("cuda:0"), n_playouts=50, seed=99, n_slots=slots)
        runs.append(gen.generate_examples(256))
    games = runs[0]
    assert len(games) == 256
    for g in games:
        for _, _, pi, z in g:
            assert abs(sum(pi) - 1.0) < 1e-6 and z in (-1, 0, 1)
    assert len(runs[1]) == len(games)
    for g0, g1 in zip(games, runs[1]):
        assert len(g0) == len(g1)
        for e0, e1 in zip(g0, g1):
            assert e0[0] == e1[0] and np.array_equal(e0[1], e1[1]) and e0[2] == e1[2] and e0[3] == e1[3]
