"""The reference's Trainer consuming engine output unchanged (BASELINE.json north_star: "the (state, pi, z)
training-example format [is] preserved so train.py's Trainer consumes the output unchanged").

The engine only runs on a GPU and the reference is not part of this repository, so the two meet through DATA fixtures:
tests/golden/engine_export_connect_four.npz, written on an MI355X by tools/make_engine_export_fixture.py - the packed
records of two engine-produced generations plus what the DEVICE replay store made of them (its remove_duplicates result,
one gathered training batch, the losses of one update on it) - and tests/golden/trainer_on_engine_export.npz, written by
oracle/gen_golden.py running the reference's own buffer handling (train.py:226-236), `Trainer.remove_duplicates`
(train.py:156-201) and `Trainer.net_step` (train.py:95-130) on those same records.

Here the records are turned into the reference's list format by `examples_from_export` and pushed through the Python
restatement of the Trainer (oracle/pyreplay.py, pinned to the reference by tests/golden/replay.json) and the facade's
`net_step` with the re-packed shipped checkpoint, and compared with both fixtures: pi / z of the de-duplicated list bit for
bit (float64), the sampled batch bit for bit (float32), the losses to 2e-6.
"""
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle import pyreplay

FIXTURE = os.path.join(GOLDEN, "engine_export_connect_four.npz")
TRAINER = os.path.join(GOLDEN, "trainer_on_engine_export.npz")


def _generations():
    from alphazero_openspiel_amd import distributed as azdist, games
    from alphazero_openspiel_amd.engine import examples_from_export
    fx = np.load(FIXTURE)
    game = games.load_game("connect_four")
    gens = [examples_from_export(game, azdist.unpack_export(fx["gen%d_payload" % g])) for g in range(2)]
    return fx, game, gens


def test_engine_records_have_the_format_the_trainer_requires():
    fx, game, gens = _generations()
    assert [len(g) for g in gens] == [24, 16]
    for games_ in gens:
        for plies in games_:
            s = game.new_initial_state()
            for i, rec in enumerate(plies):
                assert type(rec) is list and len(rec) == 4                      # mutable list of 4 (train.py:177-198)
                assert rec[0] == s.information_state()                          # hashable key, equal for equal histories
                assert isinstance(rec[1], np.ndarray) and rec[1].shape == (4, 6, 7) and rec[1].dtype == np.float64
                assert type(rec[2]) is list and len(rec[2]) == 7 and all(type(v) is float for v in rec[2])
                assert bool(rec[2]) and type(rec[3]) is float                   # truthiness is tested (train.py:117,179)
                if i + 1 < len(plies):
                    s.apply_action(int(plies[i + 1][0].split(", ")[-1]))


def test_reference_remove_duplicates_on_engine_output_equals_the_device_store():
    from alphazero_openspiel_amd import replay
    from alphazero_openspiel_amd.network import load_npz_checkpoint
    ref = np.load(TRAINER)                           # what the reference's Trainer made of these records
    fx, game, gens = _generations()
    buffer = []
    for g, games_ in enumerate(gens):
        for examples in games_:                      # Trainer.generate_examples (train.py:226-227)
            buffer.append(examples)
        n_games_buffer = int(fx["gen%d_capacity" % g])
        while len(buffer) > n_games_buffer:          # train.py:233-236
            del buffer[0]
        flattened = [sample for game_ in buffer for sample in game_]
        out = pyreplay.remove_duplicates(flattened)  # train.py:156-201, including its write-back into `buffer`
        assert len(out) == int(fx["gen%d_n_unique" % g]) == len(ref["gen%d_unique_z" % g])
        for want in (fx, ref):
            assert [it[2] for it in out] == want["gen%d_unique_pi" % g].tolist()
            assert [it[3] for it in out] == want["gen%d_unique_z" % g].tolist()
            # first-occurrence order: the device store reports the flat-buffer index of every unique record
            assert [id(it) for it in out] == [id(flattened[i]) for i in want["gen%d_unique_index" % g]]
    # ---- net_step on the de-duplicated list: the same draw, the same batch, the same losses ----
    net = load_npz_checkpoint(os.path.join(GOLDEN, "checkpoint_connect_four.npz"), [3, 6, 7], 7)
    net.train()
    torch.set_num_threads(1)
    np.random.seed(5)
    ids = np.random.randint(len(out), size=16)
    x = np.array([out[i][1] for i in ids], dtype=np.float32)
    pi = np.array([out[i][2] for i in ids]).astype(np.float32)
    z = np.array([out[i][3] for i in ids]).astype(np.float32)
    for want in (fx, ref):
        assert ids.tolist() == want["batch_ids"].tolist()
        assert (x == want["batch_x"]).all() and (pi == want["batch_pi"]).all() and (z == want["batch_z"]).all()
    loss_p, loss_v = replay.net_step(net, replay.make_optimizer(net), torch.from_numpy(x), torch.from_numpy(pi), torch.from_numpy(z))
    loss_p, loss_v = float(loss_p.detach()), float(loss_v.detach())
    for want in (fx, ref):
        assert abs(loss_p - float(want["loss_p"])) < 2e-6 and abs(loss_v - float(want["loss_v"])) < 2e-6
        assert np.abs(net.fc1.bias.detach().numpy() - want["fc1_bias_after"]).max() < 2e-6
