"""DeviceReplay.sample(mirror=, out=) and GraphedNetStep(mirror=) (alphazero_openspiel_amd/replay.py) on the device: the
facade against the C entries called directly, and the graphed training step sampling straight into its input tensors."""
import os

import numpy as np
import pytest
import torch

import mirror_cases as MC
from conftest import GOLDEN
from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.network import load_npz_checkpoint

pytestmark = pytest.mark.gpu
BATCH = 64


@pytest.fixture(scope="module", params=["connect_four", "breakthrough(rows=6,columns=5)"])
def stores(request):
    """(game, n_unique, two fresh stores with the same content and the same call counter)"""
    a, n = MC.make_store(request.param)
    b, _ = MC.make_store(request.param)
    yield games.load_game(request.param), n, a, b
    a.close()
    b.close()


def test_sample_fills_and_returns_the_tensors_given_as_out(stores):
    game, n, a, b = stores
    idx = np.random.RandomState(0).randint(n, size=BATCH)
    out = MC.outputs(a, BATCH)
    got = a.sample(BATCH, indices=idx, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert bool(MC.rows_equal(out, a.sample(BATCH, indices=idx)).all())
    flips = np.arange(BATCH) % 3 == 0
    got = a.sample(BATCH, indices=idx, mirror=flips, out=list(out))  # any sequence of the three
    assert all(g is o for g, o in zip(got, out))
    assert (MC.recover_flips(game, a.sample(BATCH, indices=idx), out) == flips).all()


def test_sample_refuses_an_out_that_does_not_fit(stores):
    game, n, a, b = stores
    x, pi, z = MC.outputs(a, BATCH)
    wrong = [(x[:-1], pi, z), (x, pi[:, :-1], z), (x, pi, z.unsqueeze(1)),            # shape
             (x.double(), pi, z), (x, pi.half(), z), (x, pi, z.long()),               # dtype
             (x.transpose(2, 3).contiguous().transpose(2, 3), pi, z),                 # contiguity
             (x.cpu(), pi, z), (x, pi), (x, pi, None)]                                  # device, not three tensors
    assert wrong[6][0].shape == x.shape and not wrong[6][0].is_contiguous()
    for out in wrong:
        with pytest.raises(ValueError):
            a.sample(BATCH, out=out)
    with pytest.raises(ValueError):
        a.sample(BATCH, mirror=np.zeros(BATCH - 1, bool))
    with pytest.raises(ValueError):
        a.sample(BATCH, mirror=np.zeros(BATCH, np.float32))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (x, pi, z))  # a refused call writes nothing


def test_mirror_modes_agree_with_the_c_entries(stores):
    game, n, _, _ = stores
    a, b = MC.make_store(game.name)[0], MC.make_store(game.name)[0]  # a: the facade, b: the C entry, call for call from 0
    idx = np.random.RandomState(1).randint(n, size=BATCH)
    idx_dev = torch.as_tensor(idx).cuda()
    for mirror in (None, False):
        assert bool(MC.rows_equal(a.sample(BATCH, seed=3, mirror=mirror), MC.call_plain(b, BATCH, seed=3)).all())
        assert bool(MC.rows_equal(a.sample(BATCH, indices=idx, mirror=mirror), MC.call_plain(b, BATCH, idx_dev)).all())
    drawn = a.sample(BATCH, seed=3, mirror=True)
    assert bool(MC.rows_equal(drawn, MC.call_sym(b, BATCH, seed=3)).all())
    assert bool(MC.rows_equal(a.sample(BATCH, indices=idx, seed=4, mirror=True), MC.call_sym(b, BATCH, idx_dev, seed=4)).all())
    flips = np.random.RandomState(2).randint(0, 2, BATCH).astype(bool)
    want = MC.call_sym(b, BATCH, idx_dev, torch.as_tensor(flips.astype(np.uint8)).cuda())
    for i, given in enumerate((flips, flips.astype(np.uint8), torch.as_tensor(flips), torch.as_tensor(flips.astype(np.uint8)).cuda(),
                               flips.tolist())):
        assert bool(MC.rows_equal(a.sample(BATCH, indices=idx, mirror=given), want).all())
        if i:
            MC.call_sym(b, BATCH, idx_dev)  # (keeps the two call counters level)
    # the counters are level: the next device draw is the same on both
    assert bool(MC.rows_equal(a.sample(BATCH, seed=9, mirror=True), MC.call_sym(b, BATCH, seed=9)).all())
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the training step
STEPS, TRAIN_BATCH = 3, 32


def _net():
    return load_npz_checkpoint(os.path.join(GOLDEN, "checkpoint_connect_four.npz"), [3, 6, 7], 7).cuda().train()


def _bits(sd):
    return {k: v.detach().clone() for k, v in sd.items()}


@pytest.fixture(scope="module")
def runs():
    """Three steps of the 5-block connect_four net on batches of 32 drawn on the device with seeds 0, 1, 2, each run on a fresh
    store (call counter 0): graphed without and with the mirror, and the un-graphed net_step fed by store.sample.

    All of them run under torch's deterministic switches.  Without them the library's convolution weight-gradient kernels do not
    repeat their own bits: measured on an MI355X, two un-graphed runs differ from each other in 59 of the 74 state_dict entries
    (the first step's gradients of 11 conv weights already differ), two graphed runs likewise, so no run is bit-equal to any
    other, whatever this project does.  With the switches on, graphed, graphed again and un-graphed give the same bits.
    The un-graphed run uses the optimiser of the class, Adam with capturable (device-side) state, so that both runs are the
    same kernels; make_optimizer's Adam counts its steps on the host and rounds its step size differently."""
    from alphazero_openspiel_amd import replay
    assert len(_net().blocks()) == 5
    was = (torch.backends.cudnn.deterministic, torch.are_deterministic_algorithms_enabled(),
           torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.deterministic = True
    torch.use_deterministic_algorithms(True, warn_only=True)
    out = {}
    try:
        for tag, mirror in (("graphed", False), ("graphed_mirror", True)):
            store, _ = MC.make_store("connect_four")
            net = _net()
            step = replay.GraphedNetStep(net, TRAIN_BATCH, store, mirror=mirror)
            x_ptr = step.x.data_ptr()
            losses = []
            for seed in range(STEPS):
                lp, lv = step(seed=seed)
                losses.append((lp.clone(), lv.clone()))
            torch.cuda.synchronize()
            assert step.x.data_ptr() == x_ptr
            out[tag] = (losses, _bits(net.state_dict()), (step.x.clone(), step.pi.clone(), step.z.clone()))
            store.close()
        store, _ = MC.make_store("connect_four")
        net = _net()
        opt = torch.optim.Adam(net.parameters(), lr=0.001, weight_decay=0.0001, capturable=True)
        losses = []
        for seed in range(STEPS):
            x, pi, z = store.sample(TRAIN_BATCH, seed=seed)
            lp, lv = replay.net_step(net, opt, x, pi, z)
            losses.append((lp.detach().clone(), lv.detach().clone()))
        torch.cuda.synchronize()
        out["eager"] = (losses, _bits(net.state_dict()), (x, pi, z))
        store.close()
    finally:
        torch.backends.cudnn.deterministic = was[0]
        torch.use_deterministic_algorithms(was[1], warn_only=was[2])
    return out


def test_graphed_step_without_mirror_equals_the_ungraphed_step_bit_for_bit(runs):
    g, e = runs["graphed"], runs["eager"]
    for step, (lg, le) in enumerate(zip(g[0], e[0])):
        print("step %d: loss_p %.9g / %.9g  loss_v %.9g / %.9g" % (step, float(lg[0]), float(le[0]), float(lg[1]), float(le[1])))
    print("state_dict entries that differ:", [k for k in g[1] if not torch.equal(g[1][k], e[1][k])])
    assert bool(MC.rows_equal(g[2], e[2]).all())  # the last batch went into the graph's inputs whole
    for step in range(STEPS):
        assert torch.equal(MC.bits(g[0][step][0]), MC.bits(e[0][step][0])), step
        assert torch.equal(MC.bits(g[0][step][1]), MC.bits(e[0][step][1])), step
    assert list(g[1]) == list(e[1])
    for k in g[1]:
        assert torch.equal(g[1][k], e[1][k]), k


def test_graphed_step_with_mirror_trains_on_other_batches(runs):
    g, m = runs["graphed"], runs["graphed_mirror"]
    for lp, lv in m[0]:
        assert bool(torch.isfinite(lp)) and bool(torch.isfinite(lv))
    assert all(bool(torch.isfinite(v).all()) for v in m[1].values() if v.dtype.is_floating_point)
    game = games.load_game("connect_four")
    flips = MC.recover_flips(game, g[2], m[2])  # the same examples, some of them mirrored
    assert 0 < flips.sum() < TRAIN_BATCH
    assert any(not torch.equal(g[1][k], m[1][k]) for k in g[1] if k.endswith("conv1.weight"))
    assert not torch.equal(g[0][-1][0], m[0][-1][0])
