"""The hand-off of the trunk from az_tower_x3d_kernel to the head: the last conv's epilogue writes the workgroup's rows of the tower
output into LDS as they lie in memory, and the eight waves copy them out in whole lines, leaving out the boards past the batch.

A wrong image address, copy-out address or board mask shows as a moved or missing value of the tower output, so every case compares
BITS: with az_tower_x3b_kernel and az_tower_x3c_kernel (the same arithmetic, az_tower_x3b_parts.h, other stores) where a shape has
them, and between batch compositions on 8x8 boards, which always run az_tower_x3d_kernel.  Every case pins its kernels by their
label (as tests/test_trained_stats_net_gpu.py does).  The label is an assertion, not a switch: connect_four and 6x6 boards take
az_tower_x3d_kernel only above 128 workgroups (1024 boards), so their batch sizes are 1024 + (nb, nb + 1, 2 nb - 1, 3 nb) for the
nb = 8 boards of a workgroup - every workgroup full, a last workgroup with one live board, one with one dead board, three more full
ones; 8x8 boards (nb = 4) run nb, nb + 1, 2 nb - 1 and 3 nb themselves.

az_head_kernel<X3> is unchanged by the hand-off; tests/test_head_kernels_gpu.py compares it with float64 at 1, 15, 16, 17 and 33
boards (c4_a16) and is not repeated here."""
import copy
import functools

import numpy as np
import pytest
import torch

from net_cases import boards, drifted_net, head_fp32, head_fp64, head_weights, tower_fp64
from test_trained_stats_net_gpu import TOWER_TOL
from alphazero_openspiel_amd import fusednet

pytestmark = pytest.mark.gpu

HEAD_SMALL = " + az_head_kernel<X3>"
HEAD_GEMM = " + az_head_gemm_kernel<X3> + az_head_softmax_kernel<X3>"
X3C_FUSED = "az_tower_x3c_kernel (fc1 + softmax + tanh in the same launch)"

# key -> (state shape, actions, seed, boards per x3d workgroup, first batch size that runs x3d minus nb, head of the label)
NETS = {
    "c4": ([3, 6, 7], 7, 61, 8, 1024, HEAD_SMALL),      # variant 2: 8 boards in 21 tiles, 64-channel rows (one line per position)
    "bt6": ([3, 6, 6], 432, 62, 8, 1024, HEAD_GEMM),    # variant 0: 8 boards in 18 tiles, 52-channel rows
    "bt8": ([3, 8, 8], 768, 63, 4, 0, HEAD_GEMM),       # variant 1: 4 boards in 16 tiles, 52-channel rows
}
X3D = "az_tower_x3d_kernel"


def _sizes(key):
    nb, base = NETS[key][3], NETS[key][4]
    return [base + nb, base + nb + 1, base + 2 * nb - 1, base + 3 * nb]


@functools.lru_cache(maxsize=None)
def _net(key):
    shape, A, seed = NETS[key][:3]
    return drifted_net(shape, A, 2, 50, seed)   # two blocks of 50 filters, per-channel BatchNorm statistics, trained-like weights


@functools.lru_cache(maxsize=None)
def _obs(key, seed=9):
    return boards(NETS[key][0], max(_sizes(key)), seed=seed)


def _open(key, max_boards, net=None):
    fn = fusednet.FusedNet(_net(key) if net is None else net, "cuda:0", max_boards=max_boards, precision="f32x")
    assert not fn.wide
    return fn


def _run(fn, ob):
    """One forward: (priors, values, tower output) as numpy arrays, the device's own bits."""
    p, v = fn.forward(ob.contiguous().cuda())
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy(), fn.read_tower(ob.shape[0])


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _cat(parts):
    return [np.concatenate([p[i] for p in parts]) for i in range(3)]


@pytest.mark.parametrize("key", ["c4", "bt6"])
def test_same_bits_as_the_other_towers(key):
    """Priors, values and tower output of az_tower_x3d_kernel == those of az_tower_x3b_kernel (the first 1024 boards in one batch)
    and of az_tower_x3c_kernel (the boards behind them, and a batch of 512 that ends with the ragged workgroup's boards)."""
    head = NETS[key][5]
    ns = _sizes(key)
    ob = _obs(key)
    fn = _open(key, max(ns))
    try:
        assert fn.kernel_label(1024) == "az_tower_x3b_kernel" + head
        assert fn.kernel_label(512) == (X3C_FUSED if head == HEAD_SMALL else "az_tower_x3c_kernel" + head)
        want = _cat([_run(fn, ob[:1024]), _run(fn, ob[1024:])])
        for n in ns:
            assert fn.kernel_label(n) == X3D + head, (n, fn.kernel_label(n))
            got = _run(fn, ob[:n])
            assert _same(got, [a[:n] for a in want]), n
            assert _same(_run(fn, ob[n - 512:n]), [a[n - 512:n] for a in want]), n   # x3c on the boards of the last workgroups
    finally:
        fn.close()


def test_same_bits_in_every_workgroup_slot_8x8():
    """8x8 boards have no other tuned tower: a board's bits at nb, nb + 1, 2 nb - 1 and 3 nb boards are those of the batch
    reversed (another workgroup, another slot) and of the board alone, and the tower output meets the float64 bar of
    test_trained_stats_net_gpu.py."""
    key = "bt8"
    ns = _sizes(key)
    ob = _obs(key)
    fn = _open(key, max(ns))
    try:
        want = _run(fn, ob)
        ref = tower_fp64(_net(key), ob.numpy())
        et = np.abs(want[2][:, :, :50] - ref).max() / np.abs(ref).max()
        print("bt8 %d boards: tower rel err %.3g" % (len(ob), et))
        assert et < TOWER_TOL["f32x"], et
        assert not want[2][:, :, 50:].any()
        for n in ns + [1]:
            assert fn.kernel_label(n) == X3D + NETS[key][5]
            assert _same(_run(fn, ob[:n]), [a[:n] for a in want]), n
            assert _same(_run(fn, torch.flip(ob[:n], [0])), [a[:n][::-1] for a in want]), n
    finally:
        fn.close()


@pytest.mark.parametrize("key", ["c4", "bt6", "bt8"])
def test_a_board_keeps_its_bits(key):
    """nb + 1 boards after 3 nb OTHER boards on the same handle give the bits of a fresh handle; the rows of the tower output past
    the small batch keep the bits the large batch left (the copy-out does not write them) and are finite - the K-tail halves the
    head reads from board b + 1 at the 52-channel stride."""
    ns = _sizes(key)
    n_small, n_big = ns[1], ns[3]
    big, other = _obs(key), _obs(key, seed=10)[:n_small]
    assert not torch.equal(other, big[:n_small])
    fn = _open(key, n_big)
    try:
        assert fn.kernel_label(n_small).startswith(X3D + " ") and fn.kernel_label(n_big).startswith(X3D + " ")
        left = _run(fn, big)[2]
        got = _run(fn, other)
        after = fn.read_tower(n_big)
        assert np.array_equal(after[n_small:].view(np.uint32), left[n_small:].view(np.uint32)), "rows past the batch were written"
        assert np.isfinite(after).all()
        fresh = _open(key, n_small)
        try:
            assert _same(got, _run(fresh, other)), "a smaller batch after a larger one"
        finally:
            fresh.close()
    finally:
        fn.close()


def test_channels_48_and_49_reach_the_head():
    """A connect_four net whose fc1 sees only channels 48 and 49 (the compact plane inside the tower; no output-channel tile of
    their own): those channels of the tower output meet the float64 bar of test_trained_stats_net_gpu.py, and priors and values
    meet the head's bar of test_head_kernels_gpu.py - max(4 x numpy float32's error, 2e-6) against float64 on the device's own
    operands.  The two channels must matter: some prior lies 0.05 or more from the policy of the bias alone."""
    key = "c4"
    A, n = NETS[key][1], _sizes(key)[1]
    net = copy.deepcopy(_net(key))
    with torch.no_grad():
        w = net.fc1.weight.data.view(A + 1, net.n_filts, net.height * net.width)
        keep = w[:, 48:50].clone() * 8.0
        w.zero_()
        w[:, 48:50] = keep
    ob = _obs(key)[:n]
    fn = _open(key, n, net=net)
    try:
        assert fn.kernel_label(n) == X3D + HEAD_SMALL
        pf, vf, x = _run(fn, ob)
    finally:
        fn.close()
    ref = tower_fp64(net, ob.numpy())
    et = np.abs(x[:, :, 48:50] - ref[:, :, 48:50]).max() / np.abs(ref).max()
    wt, bias = head_weights(net, "tuned"), net.fc1.bias.detach().numpy()
    assert not wt[:, :, :48].any() and wt[:, :, 48:50].any()
    p64, v64, _ = head_fp64(x, wt, bias, A)
    p32, v32 = head_fp32(x, wt, bias, A)
    yard = max(np.abs(p32 - p64).max(), np.abs(v32 - v64).max())
    err = max(np.abs(pf - p64).max(), np.abs(vf - v64).max())
    spread = float(np.abs(p64 - head_fp64(np.zeros_like(x), wt, bias, A)[0]).max())   # against the policy of the bias alone
    print("channels 48, 49 only: tower rel err %.3g, head err %.3g, numpy fp32 err %.3g, largest move of a prior away from the bias's %.3g" % (et, err, yard, spread))
    assert et < TOWER_TOL["f32x"], et
    assert spread > 0.05, spread
    assert err <= max(4.0 * yard, 2e-6), (err, yard)
