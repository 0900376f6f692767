"""Playout cap randomisation, the parts that need no GPU: the ABI surface, the pure-Python restatement of the engine's draw in
tests/philox_cases.py (the schedule's model for tests/test_playout_cap_gpu.py), examples_from_export(keep=) and the
ExampleGenerator refusals.

The draw (include/az_engine.h, az_engine_set_playout_cap): u = the first philox_u01 of the Philox4x32-10 stream
(seed, game id, ply, purpose 3, index 0); the move is a full search iff u < p_full."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import replay_cases as RC
from alphazero_openspiel_amd import _lib, games
from alphazero_openspiel_amd.engine import examples_from_export
from philox_cases import M32, cap_uniform, philox4x32_10, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the schedule's model
def test_philox_model_reproduces_the_published_vectors():
    # Random123's known-answer vectors for philox4x32-10
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_schedule_is_a_function_of_seed_game_and_ply():
    u = [cap_uniform(777, i, t) for i in range(12) for t in range(42)]
    assert all(0.0 <= x < 1.0 for x in u) and len(set(u)) == len(u)
    assert 0.35 < np.mean(u) < 0.65                                      # 504 uniforms: the mean is within 0.15 of 1/2
    assert cap_uniform(777, 3, 5) != cap_uniform(778, 3, 5) != cap_uniform(777 + (1 << 32), 3, 5)   # both halves of the seed key it
    assert cap_uniform(777, 3, 5) not in (cap_uniform(777, 3, 5, purpose=1), cap_uniform(777, 3, 5, purpose=0))
    s = schedule(777, 4, 42, 0.5)
    assert s.dtype == np.uint8 and s.shape == (4, 42) and 0 < s.sum() < s.size
    assert schedule(777, 4, 42, 1.0).all() and not schedule(777, 4, 42, 0.0).any()


# ------------------------------------------------------------------------------------------------ ABI surface
def test_abi_surface():
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    vp = C.c_void_p
    assert protos["az_engine_set_playout_cap"] == (C.c_int, [vp, C.c_int32, C.c_double])
    assert protos["az_engine_full_moves_device"] == (C.c_int, [vp, vp, C.c_int64, vp])
    assert protos["az_replay_append_device_kept"] == (C.c_int, [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp])
    eng_h = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    rep_h = open(os.path.join(ROOT, "include", "az_replay.h")).read()
    assert re.search(r"int az_engine_set_playout_cap\(az_engine \*e, int32_t n_fast, double p_full\);", eng_h)
    assert re.search(r"int az_engine_full_moves_device\(az_engine \*e, uint8_t \*full_out_dev, int64_t n_games, void \*stream\);", eng_h)
    assert re.search(r"int az_replay_append_device_kept\(az_replay \*r, const void \*dev_buf, int64_t n_games, int32_t start_ply,\s*"
                     r"const int32_t \*start_ply_dev,\s*const uint64_t \*keys_dev, const uint8_t \*keep_dev, void \*stream\);", rep_h)
    lib = _lib.load()                                                     # (raises if the library lacks a declared symbol)
    for name in ("az_engine_set_playout_cap", "az_engine_full_moves_device", "az_replay_append_device_kept"):
        assert getattr(lib, name).argtypes == protos[name][1]
    # az_config keeps its layout (include/az_engine.h): 14 int32, 2 int64, 4 doubles, the seed, 4 int32, a double, 4 int32
    assert C.sizeof(_lib.AzConfig) == 152 and _lib.AzConfig.seed.offset == 104 and _lib.AzConfig.spare_pools.offset == 148


# ------------------------------------------------------------------------------------------------ examples_from_export(keep=)
@pytest.mark.parametrize("start_history", [[], [3], [3, 2, 4]])
def test_examples_from_export_drops_fast_plies(start_history):
    game = games.load_game("connect_four")
    ex = RC.fake_export(game, n_games=5, seed=4, start_history=start_history)
    p0, mp = len(start_history), game.max_game_length()
    keep = schedule(99, 5, mp, 0.5)
    keep[2] = 0                                                           # a game with no kept ply
    keep[3] = 1                                                           # ... and one that keeps every ply
    keep[:, :p0] = 1                                                      # (bytes outside the games' plies do not matter here)
    full = examples_from_export(game, ex, start_history)
    got = examples_from_export(game, ex, start_history, keep=keep)
    assert len(got) == 5 and got[2] == [] and len(got[3]) == len(full[3])
    for g in range(5):
        n = int(ex["game_len"][g])
        want = [full[g][i] for i in range(n) if keep[g, p0 + i]]
        assert len(got[g]) == len(want)
        kept_plies = [p0 + i for i in range(n) if keep[g, p0 + i]]
        for rec, ref, t in zip(got[g], want, kept_plies):
            assert rec[0] == ref[0] and (rec[1] == ref[1]).all() and rec[2] == ref[2] and rec[3] == ref[3]
            # the key is the full history up to the ply, fast moves included; z has the sign of the absolute ply
            hist = list(start_history) + [int(a) for a in ex["move"][g, p0:t]]
            assert rec[0] == ", ".join(map(str, hist))
            assert rec[3] == float(ex["game_ret0"][g]) * (-1.0 if t & 1 else 1.0)
    if len(start_history) == 0:
        assert any(0 < len(a) < len(b) for a, b in zip(got, full))       # the mask did drop some plies
    ones = examples_from_export(game, ex, start_history, keep=np.ones((5, mp), np.uint8))    # an all-ones mask drops nothing
    assert [[(r[0], r[2], r[3]) for r in g] for g in ones] == [[(r[0], r[2], r[3]) for r in g] for g in full]


# ------------------------------------------------------------------------------------------------ facade refusals
def test_example_generator_refuses_what_the_mask_cannot_follow(monkeypatch):
    from alphazero_openspiel_amd import distributed as azdist
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    net = torch.nn.Identity()
    kw = dict(n_playouts=24, playout_cap=(6, 0.5))
    g = ExampleGenerator(net, "connect_four", "cuda:0", **kw)             # (no device is touched before a generation is asked for)
    assert g.playout_cap == (6, 0.5)
    for bad, pattern in ((dict(continuous=True), "continuous"), (dict(n_pools=2), "n_pools"),
                         (dict(pool_devices=["cuda:0"]), "pool_devices"), (dict(overlap=2), "overlap > 1")):
        with pytest.raises(ValueError, match="playout_cap is not supported with " + pattern):
            ExampleGenerator(net, "connect_four", "cuda:0", **kw, **bad)
    for cap in ((0, 0.5), (25, 0.5), (6, 1.5), (6, -0.1), 6, (6,), ("a", 0.5)):
        with pytest.raises(ValueError, match="playout_cap"):
            ExampleGenerator(net, "connect_four", "cuda:0", n_playouts=24, playout_cap=cap)
    monkeypatch.setattr(azdist, "world_size", lambda: 2)                 # a rank of a world of two
    with pytest.raises(ValueError, match="playout_cap is not supported with torch.distributed with world size 2"):
        ExampleGenerator(net, "connect_four", "cuda:0", **kw)
    for call in (lambda: g.generate_examples(8), lambda: g.generate_into(None, 8)):
        with pytest.raises(ValueError, match="playout_cap is not supported with torch.distributed with world size 2"):
            call()
