"""ExampleGenerator(continuous=True): the reference's per-generation call on ONE engine in stream mode that lives across the
calls.  With an unchanged net the calls return, concatenated, the closed generation of the generator's first seed; a replaced
net is taken over at the next call; several ranks each take their share from a stream of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from alphazero_openspiel_amd import games
from conftest import ROOT
from net_cases import drifted_net

pytestmark = pytest.mark.gpu

S, G, SEED = 16, 64, 909


def _assert_same_examples(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert len(a) == len(b)
        for ra, rb in zip(a, b):
            assert ra[0] == rb[0] and (ra[1] == rb[1]).all() and ra[2] == rb[2] and ra[3] == rb[3]


def _assert_legal(game_name, examples):
    """Every game's keys spell one legal line of play from the initial position, boards match, pi lives on the legal actions."""
    from alphazero_openspiel_amd.network import state_to_board
    game = games.load_game(game_name)
    shape = game.information_state_normalized_vector_shape()
    for plies in examples:
        s = game.new_initial_state()
        assert 7 <= len(plies) <= 42
        for i, (key, board, pi, z) in enumerate(plies):
            assert key == s.information_state() and (board == state_to_board(s, shape)).all()
            legal = s.legal_actions()
            assert abs(sum(pi) - 1) < 1e-12 and all(p == 0 for a, p in enumerate(pi) if a not in legal)
            assert z in (-1.0, 0.0, 1.0)
            if i + 1 < len(plies):
                nxt = plies[i + 1][0]
                a = int(nxt.split(", ")[-1])
                assert a in legal
                s.apply_action(a)
                assert nxt == s.information_state()


def test_calls_with_an_unchanged_net_are_one_closed_generation_in_pieces():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    from alphazero_openspiel_amd.fusednet import FusedNet
    net = drifted_net([3, 6, 7], 7, 1, 50, seed=41)
    gen = ExampleGenerator(net, "connect_four", torch.device("cuda:0"), continuous=True, n_slots=G, seed=SEED, n_playouts=S)
    try:
        got, owners = [], []
        for _ in range(3):
            got.extend(gen.generate_examples(48))
            owners.append((gen._stream, gen._stream_engine, gen._stream_evaluator))
            assert gen.last_progress["error_flags"] == 0
        assert all(o[0] is owners[0][0] and o[1] is owners[0][1] and o[2] is owners[0][2] for o in owners)
        assert owners[0][1].sizes.max_games == 48 + 2 * G
        with pytest.raises(ValueError, match="capacity"):
            gen.generate_examples(48 + 2 * G + 1)
    finally:
        gen.close()
    assert gen._stream is None
    eng = E.SelfPlayEngine("connect_four", G, n_playouts=S, max_games=144, device=0, seed=SEED)  # the generator's first seed
    fn = FusedNet(net, "cuda:0", max_boards=G, precision="f32x")
    try:
        assert E.run_selfplay(eng, fn, 144, use_graph=True)["games_done"] == 144
        want = E.examples_from_export(eng.game, eng.export())
    finally:
        E.close_all(eng, fn)
    _assert_same_examples(got, want)


def test_a_replaced_net_is_taken_over_at_the_next_call():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    gen = ExampleGenerator(drifted_net([3, 6, 7], 7, 1, 50, seed=41), "connect_four", torch.device("cuda:0"), continuous=True,
                           n_slots=G, seed=SEED, n_playouts=S)
    try:
        first = gen.generate_examples(48)
        engine, evaluator = gen._stream_engine, gen._stream_evaluator
        gen.net = drifted_net([3, 6, 7], 7, 1, 50, seed=42)
        second = gen.generate_examples(48)
        assert gen._stream_engine is engine and gen._stream_evaluator is not evaluator
        assert gen.last_progress["error_flags"] == 0 and gen.last_progress["games_done"] >= 96
        third = gen.generate_examples(48)   # unchanged again: the evaluator stays
        assert gen.last_progress["error_flags"] == 0
    finally:
        gen.close()
    for out in (first, second, third):
        assert len(out) == 48
        _assert_legal("connect_four", out)


def test_combinations_continuous_does_not_cover_are_refused():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    net = drifted_net([3, 6, 7], 7, 1, 50, seed=41)
    dev = torch.device("cuda:0")
    for kw in ({"n_pools": 2, "pool_devices": ["cuda:0", "cuda:0"]}, {"overlap": 2}, {"eval_backend": "torch"}):
        with pytest.raises(ValueError, match="continuous=True"):
            ExampleGenerator(net, "connect_four", dev, continuous=True, n_slots=G, **kw)


_WORKER = r"""
import hashlib, json, os, sys
import torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
from alphazero_openspiel_amd import engine as E
from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
from alphazero_openspiel_amd.fusednet import FusedNet
from alphazero_openspiel_amd.network import load_npz_checkpoint
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
net = load_npz_checkpoint(os.path.join(%(root)r, "tests", "golden", "checkpoint_connect_four.npz"), [3, 6, 7], 7)
gen = ExampleGenerator(net, "connect_four", torch.device("cuda:0"), continuous=True, n_playouts=12, n_slots=8, seed=77)
calls = [gen.generate_examples(64) for _ in range(2)]      # 32 per rank and call, each rank from its own stream
engine = gen._stream_engine
flags = gen.last_progress["error_flags"]
gen.close()
# this rank's stream order against its own one-shot generation (the generator's seed for rank r)
eng = E.SelfPlayEngine("connect_four", 8, n_playouts=12, max_games=64, device=0, seed=77 + 7919 * r)
fn = FusedNet(gen.net, "cuda:0", max_boards=8, precision="f32x")
assert E.run_selfplay(eng, fn, 64, use_graph=True)["games_done"] == 64
want = E.examples_from_export(eng.game, eng.export())
E.close_all(eng, fn)
def same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(p[0] == q[0] and (p[1] == q[1]).all() and p[2] == q[2] and p[3] == q[3]
                                                             for p, q in zip(x, y)) for x, y in zip(a, b))
ok = [same(calls[c][r * 32:(r + 1) * 32], want[c * 32:(c + 1) * 32]) for c in range(2)]
digest = [hashlib.sha256(json.dumps([[(rec[0], rec[2], rec[3]) for rec in g] for g in games]).encode()).hexdigest() for games in calls]
json.dump({"n": [len(c) for c in calls], "digest": digest, "own_half_ok": ok, "flags": flags,
           "halves_differ": [rec[0] for g in calls[0][:32] for rec in g] != [rec[0] for g in calls[0][32:] for rec in g]},
          open(os.path.join(os.environ["AZ_TEST_OUT"], "rank%%d.json" %% r), "w"))
dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_each_take_their_share_from_their_own_stream(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                   PYTHONDONTWRITEBYTECODE="1", AZ_TEST_OUT=str(tmp_path))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:   # each process under a time limit of its own
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]
    a = json.load(open(tmp_path / "rank0.json"))
    b = json.load(open(tmp_path / "rank1.json"))
    assert a["n"] == b["n"] == [64, 64]
    assert a["digest"] == b["digest"] and a["digest"][0] != a["digest"][1]   # the same gathered list on every rank, new games per call
    assert a["own_half_ok"] == b["own_half_ok"] == [True, True]              # ids 0..31, then 32..63, of the rank's own stream
    assert a["flags"] == b["flags"] == 0 and a["halves_differ"] and b["halves_differ"]
