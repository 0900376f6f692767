"""The head kernels - fc1 + softmax + tanh as az_head_kernel, az_head_gemm_kernel + az_head_softmax_kernel and x3_fused_head inside
az_tower_x3c_kernel - against float64 on nets whose fc1 looks trained (net_cases.trained_head: a peaked softmax next to a flat one,
a saturated value, biases of order 1, weights with subnormal fp16 halves), at the action counts, batch sizes and k-step counts where
their control flow changes (head_cases.NETS).

The head is tested ALONE: the reference of a forward is computed on the CPU in float64 from the operands the device multiplies -
the device's own tower output of that forward (FusedNet.read_tower: hi + lo / 2048) and the fc weights as the path rounds them
(net_cases.head_weights) - so no tower error enters.  The yardstick is the same head on the same operands in numpy float32; the bar
is max(4 x the yardstick's error against float64, 2e-6) over the boards of the case.  Every case pins its kernels by their label.

Measured on an MI355X (device error / bar of the worst batch size per case): see DESIGN_HISTORY.md, "Head kernels: float64 tests"."""
import copy
import functools

import numpy as np
import pytest
import torch

import head_cases as hc
from net_cases import head_fp32, head_fp64, head_weights, tower_fp64
from alphazero_openspiel_amd import fusednet

pytestmark = pytest.mark.gpu

WIDE_TOWER = {"f32x": "az_wide_input_kernel + az_conv_wide_kernel<X3> x4", "f16": "az_wide_input_kernel + az_conv_wide_kernel<F16> x4"}


def _label(key, precision, n):
    """The kernels a forward of n boards of the case must launch."""
    shape, A, F, wide = hc.NETS[key][:4]
    n_ot = (A + 1 + 15) // 16
    head = (hc.HEAD_SMALL if n_ot <= 8 else hc.HEAD_GEMM)[precision]
    if wide or F > 56:
        return WIDE_TOWER[precision] + head
    board = (shape[1], shape[2])
    if board == (8, 8):
        return ("az_tower_x3d_kernel" if precision == "f32x" else "az_tower_kernel") + head
    # row-pair boards (6x7, 6x6, 5x5): a board per workgroup (or two) up to 512 boards, a board per wave, packed column tiles
    if n <= 512:
        if precision == "f16":
            return "az_tower_f16c_kernel" + head
        return hc.X3C_FUSED if n_ot == 1 else "az_tower_x3c_kernel" + head
    assert board in ((6, 7), (6, 6)), board
    if precision == "f16":
        return "az_tower_kernel" + head
    return ("az_tower_x3b_kernel" if n <= 1024 else "az_tower_x3d_kernel") + head


@functools.lru_cache(maxsize=None)
def _weights(key, precision):
    w = head_weights(hc.net(key), hc.mode(key, precision))
    w.setflags(write=False)
    return w


def _open(key, precision, max_boards, net=None):
    wide = hc.NETS[key][3]
    fn = fusednet.FusedNet(hc.net(key) if net is None else net, "cuda:0", max_boards=max_boards, precision=precision, wide=wide)
    assert fn.wide == bool(wide or hc.NETS[key][2] > 56)
    return fn


def _run(fn, ob):
    """One forward: (priors, values, tower) as numpy arrays, the device's own bits."""
    p, v = fn.forward(ob.contiguous().cuda())
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy(), fn.read_tower(ob.shape[0])


def _head_errors(key, precision, out):
    """Device (priors, values, tower) of a forward of the case's reference net -> (device error, yardstick error, float64 priors
    and values): both errors against the float64 head on the device's own operands, the largest over boards, priors and value."""
    pf, vf, x = out
    A, net = hc.NETS[key][1], hc.net(key)
    w, bias = _weights(key, precision), net.fc1.bias.detach().numpy()
    p64, v64, _ = head_fp64(x, w, bias, A)
    p32, v32 = head_fp32(x, w, bias, A, fast_exp=precision == "f16")
    yard = max(np.abs(p32 - p64).max(), np.abs(v32 - v64).max())
    err = max(np.abs(pf - p64).max(), np.abs(vf - v64).max())
    return float(err), float(yard), p64, v64


def _bar(yard):
    return max(4.0 * yard, 2e-6)


MAIN = [(k, "f32x") for k in hc.NETS] + [(k, "f16") for k in hc.NETS if hc.NETS[k][6]]


@pytest.mark.parametrize("key,precision", MAIN, ids=["%s-%s" % c for c in MAIN])
def test_head_matches_fp64_on_its_own_operands(key, precision):
    """Priors and values of every batch size of the case against the float64 head on the device's own tower output and rounded
    weights: at most max(4 x numpy-float32's error on the same operands, 2e-6).  At n <= 64 also: the end-to-end bar of the tower
    tests (f32x: 4 x torch-fp32's own error against the float64 Net, at least 2e-6), priors that sum to 1 within 1e-5, everything
    finite, and a prior whose float64 value is below 1e-30 comes out >= 0 and < 1e-20."""
    ns = hc.NETS[key][5]
    fn = _open(key, precision, max(ns))
    misses = []
    try:
        for n in ns:
            assert fn.kernel_label(n) == _label(key, precision, n), (n, fn.kernel_label(n))
            out = _run(fn, hc.obs(key)[:n])
            err, yard, p64, v64 = _head_errors(key, precision, out)
            print("head %s %s n=%d: device err %.3g, numpy fp32 err %.3g, bar %.3g (ratio %.2f)" % (key, precision, n, err, yard, _bar(yard), err / _bar(yard)))
            assert err <= _bar(yard), (n, err, yard)
            if n > hc.N_E2E:
                continue
            pf, vf = out[0].astype(np.float64), out[1].astype(np.float64)
            assert np.isfinite(pf).all() and np.isfinite(vf).all() and np.isfinite(out[2]).all()
            assert np.abs(pf.sum(1) - 1).max() < 1e-5
            gone = p64 < 1e-30
            assert (pf[gone] >= 0).all() and (pf[gone] < 1e-20).all()
            if precision == "f32x":
                n64, w64, e32, t64, t32 = hc.e2e_reference(key)
                ee, e32n = max(np.abs(pf - n64[:n]).max(), np.abs(vf - w64[:n]).max()), float(e32[:n].max())
                td = np.abs(out[2][:, :, :t64.shape[2]] - t64[:n]).reshape(n, -1)
                print("head %s %s n=%d: end to end err %.3g vs the float64 Net (torch fp32: %.3g); tower abs err max %.3g rms %.3g (torch fp32: %.3g, %.3g)"
                      % (key, precision, n, ee, e32n, td.max(), np.sqrt((td ** 2).mean()), t32[:n].max(), np.sqrt((t32[:n] ** 2).mean())))
                if ee > max(4.0 * e32n, 2e-6):
                    misses.append((n, ee, e32n))
        assert not misses, "end to end (n, device error, torch-fp32 error): %s" % misses
    finally:
        fn.close()


# ---- negative controls: the device runs a net that differs from the reference's net --------------------------------------------
CONTROL_CASES = [("c4_a16", 17), ("c4_a128", 33), ("wc4_a16", 17), ("w7x9_a256", 33)]  # small head / GEMM head, tuned / wide path


def _fc(net):
    """fc1's weight as a view [A + 1][F][H*W] and its bias."""
    return net.fc1.weight.data.view(-1, net.n_filts, net.height * net.width), net.fc1.bias.data


def _swap_bias(net, x64, A):
    """the biases of the value output and of the policy output whose bias is farthest from it"""
    w, b = _fc(net)
    o = int((b[:A] - b[A]).abs().argmax())
    b[A], b[o] = float(b[o]), float(b[A])


def _swap_rows_at_one_k(net, x64, A):
    """the value row and the row of scale 32, at the (channel, position) where that moves the logits most"""
    w, b = _fc(net)
    r = A // 3
    gain = (w[r] - w[A]).abs().double().numpy().T * np.abs(x64).mean(0)  # [pos][c]
    pos, c = np.unravel_index(int(gain.argmax()), gain.shape)
    w[A, c, pos], w[r, c, pos] = float(w[r, c, pos]), float(w[A, c, pos])


def _swap_channels_48_49(net, x64, A):
    """channels 48 and 49 of every row at the position where that moves the logits most"""
    w, b = _fc(net)
    gain = ((w[:, 48] - w[:, 49]).abs().double().numpy().max(0)) * np.abs(x64[:, :, 48] - x64[:, :, 49]).mean(0)  # [pos]
    pos = int(gain.argmax())
    a48 = w[:, 48, pos].clone()
    w[:, 48, pos] = w[:, 49, pos]
    w[:, 49, pos] = a48


def _end_of_k(net, x64, A):
    """the value row's weight at the last cell's last channel - the end of K - moved by 0.5"""
    w, b = _fc(net)
    w[A, net.n_filts - 1, -1] += 0.5


CONTROLS = [(k, n, f) for k, n in CONTROL_CASES for f in (_swap_bias, _swap_rows_at_one_k, _swap_channels_48_49)] + [("c4_a128", 33, _end_of_k)]


@pytest.mark.parametrize("key,n,alter", CONTROLS, ids=["%s-%s" % (c[0], c[2].__name__.strip("_")) for c in CONTROLS])
def test_a_wrong_head_is_seen(key, n, alter):
    """The negative controls of the test above: the device runs the case's net with one small change to fc1 and is compared with the
    reference of the unchanged net - it misses the case's bar by at least 100 x."""
    A = hc.NETS[key][1]
    ob = hc.obs(key)[:n]
    net = copy.deepcopy(hc.net(key))
    before = [t.clone() for t in _fc(net)]
    with torch.no_grad():
        alter(net, tower_fp64(net, ob.numpy()), A)
    changed = sum(int((a != b).sum()) for a, b in zip(before, _fc(net)))
    assert 1 <= changed <= 2 * (A + 1), changed
    fn = _open(key, "f32x", n, net=net)
    try:
        assert fn.kernel_label(n) == _label(key, "f32x", n)
        err, yard, _, _ = _head_errors(key, "f32x", _run(fn, ob))
        print("control %s %s: device err %.3g, bar %.3g, ratio %.3g" % (key, alter.__doc__, err, _bar(yard), err / _bar(yard)))
        assert err >= 100.0 * _bar(yard), (err, yard)
    finally:
        fn.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """Equal bits of (priors, values) - and of the tower output, which the head's bits presuppose."""
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("key,precision", MAIN, ids=["%s-%s" % c for c in MAIN])
def test_a_board_keeps_its_bits(key, precision):
    """A board's priors and value are the same bits at every batch size of its case (whichever head and tower kernel that takes),
    with the batch reversed, and on a handle that has just run its largest batch of OTHER boards: with the 52-channel stride the last
    fc1 k-step of board b reads the first halves of row b + 1 of the tower output (times zero weights) - on a fresh handle zeros,
    here what the larger forward left there."""
    ns = hc.NETS[key][5]
    n_max = max(ns)
    ob = hc.obs(key)[:n_max]
    fn = _open(key, precision, n_max)
    try:
        ref = _run(fn, ob)
        for n in ns:
            assert _same(_run(fn, ob[:n]), [a[:n] for a in ref]), n
        assert _same(_run(fn, torch.flip(ob, [0])), [a[::-1] for a in ref]), "reversed order"
        n_small = sorted(ns)[len(ns) // 2]
        other = torch.flip(ob, [0])[:n_small]
        assert not torch.equal(other, ob[:n_small])
        _run(fn, ob)
        got = _run(fn, other)
        fresh = _open(key, precision, n_small)
        try:
            assert _same(got, _run(fresh, other)), "a smaller batch after a larger one"
        finally:
            fresh.close()
    finally:
        fn.close()


@pytest.mark.parametrize("key", ["c4_a7", "c4_a15"])
def test_fused_head_and_head_kernel_give_the_same_bits(key):
    """512 boards run x3_fused_head inside az_tower_x3c_kernel, 513 az_head_kernel<X3> behind az_tower_x3b_kernel: the same bits."""
    ob = hc.boards(hc.NETS[key][0], 513, seed=5)
    fn = _open(key, "f32x", 513)
    try:
        assert fn.kernel_label(512) == hc.X3C_FUSED and fn.kernel_label(513) == "az_tower_x3b_kernel" + hc.HEAD_SMALL["f32x"]
        ref = _run(fn, ob)
        assert _same(_run(fn, ob[:512]), [a[:512] for a in ref])
    finally:
        fn.close()
