"""The wide PV-net path (az_net_create_wide, csrc/az_net_wide.hip) at the edges of what it promises, on the GPU: filter counts that are
no multiple of 32, 16 or 8 (the zero padding to fpad = ceil32(F), the partly filled 16-channel tile, waves that only stage, a second
blockIdx.y), boards whose last column tile is ragged (5x5: 175 columns), 3-wide boards, HW = 63, 1 and 3 input planes, nets narrower
than their input (FusedNet(wide=True)), and BatchNorm statistics that differ by channel (net_cases.drifted_net).

The weight packing of this path happens inside az_net_create_wide and has no CPU emulation, so everything here is differential:
the device against the float64 forward of the same net, computed once per case on the CPU.  Every case pins the kernels it runs by
their label, and the bits a board gets must not depend on where in a workgroup, or in which workgroup, it sits."""
import copy
import functools

import numpy as np
import pytest
import torch

from net_cases import boards, drifted_net, max_activation_fp64, tower_fp64
from alphazero_openspiel_amd import fusednet

pytestmark = pytest.mark.gpu

TOWER_TOL = 2e-5  # f32x: max |got - ref| / max |ref| of the tower output (the bar of test_trained_stats_net_gpu, test_wide_net_gpu)
FP16_MAX = 65504.0

# id -> (state shape [C, H, W], actions, blocks, filters, w_scale, FusedNet's wide=); in_planes = C + 1, the net's seed is F
CASES = {
    "c4_57": ([3, 6, 7], 7, 2, 57, 1.0, None),         # fpad 64, one m-tile per wave, tile 3 partly filled (channel 56 alone in its octet)
    "bt5x5_65": ([3, 5, 5], 300, 2, 65, 1.0, None),    # fpad 96, two m-tiles per wave, wave 3 only stages; 175 columns; gemm head
    "bt6x5_100": ([3, 6, 5], 30, 2, 100, 1.0, None),   # fpad 128; 150 columns
    "bt8_129": ([3, 8, 8], 768, 2, 129, 1.0, None),    # fpad 160, two blockIdx.y; 2 boards per workgroup; 49 output tiles
    "b7x9_255": ([3, 7, 9], 63, 1, 255, 1.0, None),    # HW 63; fpad 256; a single block (conv 1 is WIDE_MODE_LAST)
    "b8x3_160": ([3, 8, 3], 72, 3, 160, 1.0, None),    # 3-wide board: every row is an edge for the dx = +-1 taps; F = fpad
    "b4x3_33_w3": ([3, 4, 3], 12, 2, 33, 3.0, True),   # 14 boards per workgroup; fpad 64 almost empty (33 filters: a tuned tower takes it)
    "c4_256_w3": ([3, 6, 7], 7, 2, 256, 3.0, None),    # tower maxima above 20
    "p3_70": ([2, 6, 7], 7, 2, 70, 1.0, None),         # in_planes 3
    "p1_96": ([0, 5, 4], 20, 2, 96, 1.0, None),        # in_planes 1
    "c4_4": ([3, 6, 7], 7, 2, 4, 1.0, True),           # identity skip (in_planes == n_filters)
    "c4_3": ([3, 6, 7], 7, 2, 3, 1.0, True),           # F < in_planes: conv arrays strided by C = 4
    "c4_1": ([3, 6, 7], 7, 2, 1, 1.0, True),
    "c4_50": ([3, 6, 7], 7, 2, 50, 1.0, True),         # a net the tuned towers take: test_wide_and_tuned_paths_agree
}


def _nbw(key):
    """Boards that share a workgroup of az_conv_wide_kernel (WIDE_NT = 11 column tiles of 16)."""
    shape = CASES[key][0]
    return 176 // (shape[1] * shape[2])


def _ns(key):
    nbw = _nbw(key)
    return sorted({n for n in (1, nbw - 1, nbw, nbw + 1, 2 * nbw + 1) if n >= 1})


@functools.lru_cache(maxsize=None)
def _net(key):
    shape, A, nb, F, w_scale, _ = CASES[key]
    return drifted_net(shape, A, nb, F, seed=F, w_scale=w_scale)


class _Ref:
    """float64 references of a net for a fixed batch of boards, computed once on the CPU; a case of n boards reads the first n."""

    def __init__(self, net, obs):
        self.obs = obs
        self.top = max_activation_fp64(net, obs)
        self.tower = tower_fp64(net, obs.numpy())
        with torch.no_grad():
            p64, v64 = copy.deepcopy(net).double()(obs.double())
            p32, v32 = net(obs)
        self.p64, self.v64 = p64.numpy(), v64.numpy()[:, 0]
        self.err32 = np.maximum(np.abs(p32.numpy() - self.p64).max(1), np.abs(v32.numpy()[:, 0] - self.v64))  # per board
        for a in (self.tower, self.p64, self.v64, self.err32):
            a.setflags(write=False)

    def e32(self, n):
        """torch float32's largest error against float64 over the first n boards (priors and value)."""
        return float(self.err32[:n].max())


@functools.lru_cache(maxsize=None)
def _ref(key):
    return _Ref(_net(key), boards(CASES[key][0], 2 * _nbw(key) + 1, seed=CASES[key][3]))


@functools.lru_cache(maxsize=None)
def _ref16(key):
    """(priors, value, tower [B][HW][F]) of torch's fp16 forward of the net on the device, as float64, for the boards of _ref."""
    net, ref = _net(key), _ref(key)
    with torch.no_grad():
        n16 = copy.deepcopy(net).half().cuda()
        x = ref.obs.half().cuda()
        p16, v16 = n16(x)
        for blk in n16.blocks():
            x = blk(x)
    B, F = x.shape[0], x.shape[1]
    return (p16.double().cpu().numpy(), v16.double().cpu().numpy()[:, 0],
            x.double().cpu().numpy().reshape(B, F, -1).transpose(0, 2, 1))


def _open(key, max_boards, precision="f32x", net=None):
    """The case's FusedNet; asserts that it runs the wide kernels, one conv launch per conv."""
    nb, wide = CASES[key][2], CASES[key][5]
    fn = fusednet.FusedNet(_net(key) if net is None else net, "cuda:0", max_boards=max_boards, precision=precision, wide=wide)
    want = "az_wide_input_kernel + az_conv_wide_kernel<%s> x%d" % ("X3" if precision == "f32x" else "F16", 2 * nb)
    assert fn.wide and fn.kernel_label().startswith(want), fn.kernel_label()
    return fn


def _run(fn, obs):
    """One forward: (priors, value, tower) as numpy arrays, the device's own bits."""
    p, v = fn.forward(obs.contiguous().cuda())
    torch.cuda.synchronize()
    return p.cpu().numpy(), v.cpu().numpy(), fn.read_tower(obs.shape[0])


def _errors(fn, ref, n, F, what):
    """One forward of the first n boards of ref: what holds at every precision (finite outputs, priors that sum to 1, the tower's
    shape and zero padding), then (tower rel err, prior err, value err) against float64 and the device's outputs."""
    HW = ref.tower.shape[1]
    pf, vf, got = _run(fn, ref.obs[:n])
    assert np.isfinite(pf).all() and np.isfinite(vf).all() and np.isfinite(got).all()
    assert np.abs(pf.astype(np.float64).sum(1) - 1).max() < 1e-5
    assert got.shape == (n, HW, fusednet.wide_fpad(F))
    assert not got[:, :, F:].any(), "channels past the net's filters must read as zero"
    tower = ref.tower[:n]
    et = np.abs(got[:, :, :F] - tower).max() / np.abs(tower).max()
    ep, ev = np.abs(pf - ref.p64[:n]).max(), np.abs(vf - ref.v64[:n]).max()
    print("%s n=%d: tower rel err %.3g (max |tower| %.3g), prior err %.3g, value err %.3g vs fp64 (torch fp32: %.3g)"
          % (what, n, et, np.abs(tower).max(), ep, ev, ref.e32(n)))
    return (et, ep, ev), (pf, vf, got)


def _check_f32x(fn, ref, n, F, what):
    """The f32x bars: tower 2e-5 of its maximum; priors and value 4 x torch-fp32's own error against float64 (at least 2e-6)."""
    (et, ep, ev), out = _errors(fn, ref, n, F, what)
    e32 = ref.e32(n)
    assert et < TOWER_TOL, (n, et)
    assert max(ep, ev) <= max(4.0 * e32, 2e-6), (n, ep, ev, e32)
    return (et, ep, ev), out


PRECISION_CASES = [(k, "f32x") for k in CASES] + [("c4_57", "f16"), ("bt5x5_65", "f16")]


@pytest.mark.parametrize("key,precision", PRECISION_CASES, ids=["%s-%s" % c for c in PRECISION_CASES])
def test_tower_and_outputs_match_fp64(key, precision):
    """Tower output (element-wise), priors and value against float64 at 1, nbw - 1, nbw, nbw + 1 and 2 nbw + 1 boards (nbw boards
    share a workgroup).  f32x: the bars of _check_f32x.  f16: at most 2 x the error of torch's fp16 forward of the same net, for
    priors and value (the rule of test_wide_net_gpu) and in the same form for the tower."""
    F = CASES[key][3]
    ref = _ref(key)
    assert ref.top < FP16_MAX  # precondition: no activation leaves fp16's range
    fn = _open(key, 2 * _nbw(key) + 1, precision)
    try:
        for n in _ns(key):
            what = "wide %s %s" % (key, precision)
            if precision == "f32x":
                _check_f32x(fn, ref, n, F, what)
                continue
            (et, ep, ev), _ = _errors(fn, ref, n, F, what)
            p16, v16, t16 = _ref16(key)
            e16 = max(np.abs(p16[:n] - ref.p64[:n]).max(), np.abs(v16[:n] - ref.v64[:n]).max())
            et16 = np.abs(t16[:n] - ref.tower[:n]).max() / np.abs(ref.tower[:n]).max()
            print("%s n=%d: torch fp16 tower rel err %.3g, prior/value err %.3g" % (what, n, et16, e16))
            assert max(ep, ev) <= 2.0 * e16, (n, ep, ev, e16)
            assert et <= 2.0 * et16, (n, et, et16)
    finally:
        fn.close()


def test_swapped_shifts_in_the_ragged_tile_are_seen():
    """The negative control of the test above: c4_57 with block 2's bn1 swapped between channels 55 and 56 - 56 is the net's last
    channel, the only real one among the last eight of the partly filled 16-channel tile 3 - misses the f32x tower bar by more than
    100 x."""
    key = "c4_57"
    ref = _ref(key)
    net = copy.deepcopy(_net(key))
    bn = net.resblock2.bn1
    with torch.no_grad():
        for t in (bn.bias, bn.running_mean, bn.running_var, bn.weight):
            a, b = float(t[55]), float(t[56])
            t[55], t[56] = b, a
    shift = fusednet.fold_net(_net(key))["bn1_shift"][1]
    assert abs(shift[55] - shift[56]) > 0.05
    swapped = fusednet.fold_net(net)["bn1_shift"][1]
    assert swapped[55] == shift[56] and swapped[56] == shift[55]
    n = 2 * _nbw(key) + 1
    fn = _open(key, n, net=net)
    try:
        _, _, got = _run(fn, ref.obs[:n])
        et = np.abs(got[:, :, :57] - ref.tower[:n]).max() / np.abs(ref.tower[:n]).max()
        print("swapped bn1 of channels 55, 56: tower rel err %.3g" % et)
        assert et > 100 * TOWER_TOL, et
    finally:
        fn.close()


def _same(a, b):
    """Equal bits of (priors, value, tower)."""
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


BITS_CASES = [("c4_57", "f32x"), ("bt5x5_65", "f32x"), ("bt8_129", "f32x"), ("b8x3_160", "f32x"), ("c4_57", "f16")]


@pytest.mark.parametrize("key,precision", BITS_CASES, ids=["%s-%s" % c for c in BITS_CASES])
def test_a_board_keeps_its_bits_wherever_it_sits(key, precision):
    """Priors, value and tower output of a board are the same bits in every prefix of the batch, with the batch reversed (every
    board in another column tile and another workgroup), and on a handle that has just run a larger batch of other boards (no
    operand row of an earlier forward is read)."""
    shape, nbw = CASES[key][0], _nbw(key)
    n_ref = 3 * nbw + 2
    obs = boards(shape, n_ref, seed=5)
    fn = _open(key, n_ref, precision)
    try:
        ref = _run(fn, obs)
        for n in _ns(key):
            assert _same(_run(fn, obs[:n]), [a[:n] for a in ref]), n
        assert _same(_run(fn, torch.flip(obs, [0])), [a[::-1] for a in ref]), "reversed order"
        assert _same(_run(fn, obs), ref)
        other = boards(shape, nbw + 1, seed=6)
        assert not torch.equal(other, obs[:nbw + 1])
        got = _run(fn, other)
        fresh = _open(key, nbw + 1, precision)
        try:
            assert _same(got, _run(fresh, other)), "a smaller batch after a larger one"
        finally:
            fresh.close()
    finally:
        fn.close()


def test_wide_and_tuned_paths_agree():
    """c4_50 on the wide path (wide=True) and on the tuned one: both meet the f32x bars at 40 boards, and they differ from each other
    by no more than the sum of their measured errors against float64."""
    key, n = "c4_50", 40
    shape, F = CASES[key][0], CASES[key][3]
    net = _net(key)
    ref = _Ref(net, boards(shape, n, seed=F))
    assert ref.top < FP16_MAX
    wide = _open(key, n)
    tuned = fusednet.FusedNet(net, "cuda:0", max_boards=n, precision="f32x")
    try:
        assert not tuned.wide and tuned.kernel_label(n).startswith("az_tower_x3c_kernel"), tuned.kernel_label(n)
        ew, (pw, vw, tw) = _check_f32x(wide, ref, n, F, "c4_50 wide")
        et, (pt, vt, tt) = _check_f32x(tuned, ref, n, F, "c4_50 tuned")
        top = np.abs(ref.tower).max()
        dt, dp, dv = np.abs(tw - tt).max() / top, np.abs(pw - pt).max(), np.abs(vw - vt).max()
        print("c4_50 wide vs tuned: tower rel diff %.3g, prior diff %.3g, value diff %.3g" % (dt, dp, dv))
        assert dt <= ew[0] + et[0] and dp <= ew[1] + et[1] and dv <= ew[2] + et[2]
    finally:
        wide.close()
        tuned.close()


def _rescaled(net, seed):
    """net with every conv1 output channel c of every block scaled by s_c = 2^k_c (bn2's gamma and beta x s_c) and conv2's input
    channel c divided by it: LeakyReLU is positively homogeneous, so the function is the same."""
    out = copy.deepcopy(net)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for blk in out.blocks():
            k = torch.randint(-4, 7, (blk.out_channels,), generator=g)
            s = torch.pow(2.0, k.float())
            blk.bn2.weight.mul_(s)
            blk.bn2.bias.mul_(s)
            blk.conv2.weight.div_(s[None, :, None, None])
    return out


@pytest.mark.parametrize("key", ["c4_57", "bt5x5_65"])
def test_per_channel_power_of_two_rescaling_is_exact_in_effect(key):
    """A second net that computes the same function with the folded conv-1 rows spread over 2^8 and more in magnitude: the
    per-channel power-of-two weight scale (and its inverse in the epilogue) then differs by channel, and the f32x bars against the
    float64 reference still hold."""
    F, nb = CASES[key][3], CASES[key][2]
    net, ref = _net(key), _ref(key)
    net2 = _rescaled(net, seed=F + 1)
    f1, f2 = fusednet.fold_net(net), fusednet.fold_net(net2)
    obs64 = ref.obs.numpy().astype(np.float64)
    for a, b in zip(fusednet.fold_forward(f1, obs64), fusednet.fold_forward(f2, obs64)):
        assert np.abs(a - b).max() <= 1e-12
    for b in range(nb):
        rows = np.abs(f2["conv_w"][2 * b]).reshape(F, -1).max(1)
        assert rows.min() > 0 and rows.max() / rows.min() >= 2.0 ** 8, (b, rows.max() / rows.min())
    assert max(ref.top, max_activation_fp64(net2, ref.obs)) < FP16_MAX
    n_max = 2 * _nbw(key) + 1
    fn = _open(key, n_max, net=net2)
    try:
        for n in (1, n_max):
            _check_f32x(fn, ref, n, F, "wide %s rescaled f32x" % key)
    finally:
        fn.close()
