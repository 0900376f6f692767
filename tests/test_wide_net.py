"""The wide PV-net path (az_net_create_wide, csrc/az_net_wide.hip) on a CPU-only box: the BatchNorm fold its descriptor carries,
the descriptor's C layout, and the argument checks that run before any HIP call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from alphazero_openspiel_amd import _lib, fusednet
from alphazero_openspiel_amd.network import Net


def _drifted(net, seed):
    """Non-trivial eval-mode BatchNorm statistics, so the fold has something to fold."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            n = m.num_features
            m.running_mean.copy_(torch.rand(n, generator=g) - 0.5)
            m.running_var.copy_(0.3 + torch.rand(n, generator=g))
            m.weight.data.copy_(0.5 + torch.rand(n, generator=g))
            m.bias.data.copy_(0.4 * torch.rand(n, generator=g) - 0.2)
    return net.eval()


@pytest.mark.parametrize("shape,A,n_blocks,F", [
    ([3, 6, 7], 7, 2, 64), ([3, 6, 6], 432, 2, 96), ([3, 5, 4], 240, 2, 128),
    # the shapes of test_wide_net_edges_gpu: 3 and 1 input planes, fewer filters than input planes (arrays strided by C = 4), one
    # filter, a 5x5 board with 65 filters, 63 cells with 255 filters and a single block
    ([2, 6, 7], 7, 2, 70), ([0, 5, 4], 20, 2, 96), ([3, 6, 7], 7, 2, 3), ([3, 6, 7], 7, 2, 1), ([3, 5, 5], 300, 2, 65),
    ([3, 7, 9], 63, 1, 255),
])
def test_fold_forward_matches_torch_fp64(shape, A, n_blocks, F):
    torch.manual_seed(F)
    net = _drifted(Net(shape, A, n_blocks=n_blocks, n_filters=F), F)
    obs = np.random.RandomState(F).randint(0, 2, size=(5, shape[0] + 1, shape[1], shape[2])).astype(np.float64)
    f = fusednet.fold_net(net)
    C = max(F, shape[0] + 1)  # the conv arrays' input-channel stride
    assert f["conv_w"].shape == (2 * n_blocks, F, C, 3, 3) and f["skip_w"].shape == (F, shape[0] + 1)
    assert f["bn1_scale"].shape == (n_blocks, C) and not f["conv_w"][1:, :, F:].any()
    p, v, tower = fusednet.fold_forward(f, obs)
    ref = net.double()
    with torch.no_grad():
        tp, tv = ref(torch.from_numpy(obs))
        x = torch.from_numpy(obs)
        for blk in ref.blocks():
            x = blk(x)
    np.testing.assert_allclose(p, tp.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(v, tv.numpy()[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(tower, x.reshape(5, F, -1).permute(0, 2, 1).numpy(), rtol=0, atol=1e-9)


def test_fold_keeps_a_narrow_net_identity_skip():
    net = _drifted(Net([3, 6, 7], 7, n_blocks=1, n_filters=4), 1)  # in_planes == n_filters: identity skip, no conv3
    f = fusednet.fold_net(net)
    assert np.array_equal(f["skip_w"], np.eye(4))
    obs = np.random.RandomState(0).rand(3, 4, 6, 7)
    with torch.no_grad():
        tp, tv = net.double()(torch.from_numpy(obs))
    p, v, _ = fusednet.fold_forward(f, obs)
    np.testing.assert_allclose(p, tp.numpy(), atol=1e-12)


@pytest.mark.parametrize("wide", [True, False, 1])
def test_the_wide_keyword_leaves_the_device_check_first(wide):
    """FusedNet's tests-only wide= changes nothing before the routing: on a CPU device the error is the one it always was."""
    net = Net([3, 6, 7], 7, n_blocks=1, n_filters=8).eval()
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        fusednet.FusedNet(net, "cpu", wide=wide)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        fusednet.FusedNet(net, "cpu")


def test_wide_desc_ctypes_layout_matches_c(tmp_path):
    src = tmp_path / "wsz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "az_net.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(az_net_wide_desc), offsetof(az_net_wide_desc, conv_w), '
                   'offsetof(az_net_wide_desc, skip_w), offsetof(az_net_wide_desc, fc_b), (size_t)AZ_NET_WIDE_MAX_FILTERS);return 0;}\n')
    exe = tmp_path / "wsz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    D = _lib.AzNetWideDesc
    assert got == [ctypes.sizeof(D), D.conv_w.offset, D.skip_w.offset, D.fc_b.offset, _lib.NET_WIDE_MAX_FILTERS]


def _desc(F=64, **over):
    net = Net([3, 6, 7], 7, n_blocks=1, n_filters=F).eval()
    d, keep = fusednet.wide_desc(fusednet.fold_net(net), 0, _lib.NET_PREC["f32x"])
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


@pytest.mark.parametrize("change,msg", [
    ({"struct_size": 8}, b"struct_size"),
    ({"n_filters": 257}, b"n_filters"),
    ({"n_filters": 0}, b"n_filters"),
    ({"rows": 9, "cols": 8}, b"rows*cols"),
    ({"in_planes": 5}, b"in_planes"),
    ({"precision": 7}, b"precision"),
])
def test_create_wide_rejects_bad_descriptions_without_a_gpu_call(change, msg):
    lib = _lib.load()
    d, keep = _desc(**change)
    h = ctypes.c_void_p()
    assert lib.az_net_create_wide(ctypes.byref(d), ctypes.byref(h)) == -1
    assert msg in lib.az_net_last_error(None) and not h.value
    assert lib.az_net_create_wide(None, ctypes.byref(h)) == -1


@pytest.mark.parametrize("field", ["conv_w", "conv_b", "bn1_scale", "bn1_shift", "skip_w", "fc_w", "fc_b"])
def test_create_wide_rejects_null_buffers(field):
    lib = _lib.load()
    d, keep = _desc()
    setattr(d, field, ctypes.POINTER(ctypes.c_float)())
    h = ctypes.c_void_p()
    assert lib.az_net_create_wide(ctypes.byref(d), ctypes.byref(h)) == -1 and not h.value


def test_create_wide_rejects_a_non_finite_weight():
    lib = _lib.load()
    d, keep = _desc()
    keep[0][0] = np.inf
    h = ctypes.c_void_p()
    assert lib.az_net_create_wide(ctypes.byref(d), ctypes.byref(h)) == -1
    assert b"finite" in lib.az_net_last_error(None)
