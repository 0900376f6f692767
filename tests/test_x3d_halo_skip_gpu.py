"""az_tower_x3d_kernel leaves out the k-steps in which a column tile wholly on board row 0 (row H - 1) multiplies nothing but the
zero halo row above (below) it (csrc/az_tower_x3d.h: X3DS::tile_on; the tiles come from csrc/az_x3d_layout.h).  That removes MFMAs
which add exact zeros, so a board's priors and value must stay the BITS the kernels without the skip give it.

f32x, a connect_four 2-block x 50-filter net with per-channel BatchNorm statistics (net_cases.drifted_net, as
tests/test_trained_stats_net_gpu.py builds its nets).  1025 and 1032 boards are above the threshold of the packed-tile kernel
(8 boards per workgroup; at 1025 the last workgroup holds one board).  The boards mix empty ones, boards with full columns (rows 0
and 5 occupied, what the pure tiles hold), and random ones.  Every board is compared bit for bit with the same boards in batches of
24 (az_tower_x3c_kernel) and 600 (az_tower_x3b_kernel), and priors and value against a float64 torch forward within the bound
tests/test_fused_net.py sets for f32x: max(4 x torch-fp32's own error, 2e-6).

(6x6 and 8x8: their kernel variants are unchanged - only the order of their columns moved, which the existing tests of those
boards cover.)"""
import copy
import functools

import numpy as np
import pytest
import torch

from net_cases import boards, drifted_net
from alphazero_openspiel_amd import fusednet

pytestmark = pytest.mark.gpu

SHAPE, A, N_MAX = [3, 6, 7], 7, 1032
X3D, X3B, X3C = "az_tower_x3d_kernel + az_head_kernel<X3>", "az_tower_x3b_kernel + az_head_kernel<X3>", "az_tower_x3c_kernel"


def _mixed_boards(n):
    """Thirds, interleaved so that every workgroup holds all kinds: empty boards (only the 'empty' plane set), boards whose
    columns are either full or empty (at least one full: rows 0 and 5 occupied, pieces alternating), random 0/1 planes."""
    H, W = SHAPE[1:]
    obs = boards(SHAPE, n, seed=11)
    g = torch.Generator().manual_seed(12)
    for i in range(n):
        if i % 3 == 0:
            obs[i, :3] = 0
            obs[i, 2] = 1
        elif i % 3 == 1:
            full = torch.rand(W, generator=g) > 0.5
            full[int(torch.randint(W, (1,), generator=g))] = True
            who = ((torch.arange(H)[:, None] + torch.arange(W)[None, :] + i) % 2).float()
            obs[i, 0] = who * full[None, :].float()
            obs[i, 1] = (1 - who) * full[None, :].float()
            obs[i, 2] = (~full)[None, :].float().expand(H, W)
    return obs


@functools.lru_cache(maxsize=1)
def _case():
    """The net, the boards, the float64 reference and the bits of the kernels without the skip - computed once."""
    net = drifted_net(SHAPE, A, 2, 50, 31)
    obs = _mixed_boards(N_MAX)
    with torch.no_grad():
        p64, v64 = copy.deepcopy(net).double()(obs.double())
        p32, v32 = net(obs)
    p64, v64 = p64.numpy(), v64.numpy()[:, 0]
    e32 = float(max(np.abs(p32.numpy() - p64).max(), np.abs(v32.numpy()[:, 0] - v64).max()))
    fn = fusednet.FusedNet(net, "cuda:0", max_boards=N_MAX, precision="f32x")
    try:
        assert fn.kernel_label(24).startswith(X3C + " ") and fn.kernel_label(600) == X3B
        assert fn.kernel_label(1025) == X3D and fn.kernel_label(1032) == X3D
        got = {}
        for batch in (24, 600, 1025, 1032):
            ps, vs = [], []
            n_all = N_MAX if batch < 1025 else batch
            for i in range(0, n_all, batch):
                p, v = fn.forward(obs[i:i + batch].contiguous().cuda())
                torch.cuda.synchronize()
                ps.append(p.cpu().numpy().copy())
                vs.append(v.cpu().numpy().copy())
            got[batch] = (np.concatenate(ps), np.concatenate(vs))
    finally:
        fn.close()
    for a in (p64, v64) + sum(got.values(), ()):
        a.setflags(write=False)
    return p64, v64, e32, got


def test_the_boards_occupy_the_edge_rows():
    obs = _mixed_boards(64)
    assert not obs[0, :2].any() and obs[0, 2].all()
    occupied = obs[1::3, 0] + obs[1::3, 1]
    assert (occupied[:, 0].sum(1) >= 1).all() and (occupied[:, 0] == occupied[:, 5]).all()


@pytest.mark.parametrize("n", [1025, 1032])
@pytest.mark.parametrize("batch", [24, 600])
def test_bits_equal_the_kernels_without_the_skip(n, batch):
    _, _, _, got = _case()
    p, v = got[n]
    pr, vr = got[batch]
    assert p.shape == (n, A) and v.shape[0] == n
    assert (p.view(np.uint32) == pr[:n].view(np.uint32)).all()
    assert (v.view(np.uint32) == vr[:n].view(np.uint32)).all()


@pytest.mark.parametrize("n", [1025, 1032])
def test_error_against_float64(n):
    p64, v64, e32, got = _case()
    p, v = (a.astype(np.float64) for a in got[n])
    v = v.reshape(n, -1)[:, 0]
    assert np.isfinite(p).all() and np.isfinite(v).all()
    ex = max(np.abs(p - p64[:n]).max(), np.abs(v - v64[:n]).max())
    print("x3d with halo skip, n=%d: max err vs fp64 %.3g (torch fp32: %.3g)" % (n, ex, e32))
    assert ex <= max(4.0 * e32, 2e-6), (ex, e32)
