"""MCTS-Solver without a GPU: the Python model of tests/solver_cases.py against the C oracle (solver off) and against a brute-force
negamax (every status it assigns), the effects the rules must show on the inputs of tests/test_solver_gpu.py, the ABI surface and
the facade's refusals."""
import ctypes as C
import os
import re

import pytest
import torch

import forced_playouts_cases as FC
import solver_cases as SC
from alphazero_openspiel_amd import _lib
from oracle import binding as orc
from oracle import fakepolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("idx", [i for i, c in enumerate(SC.CASES) if c["start"] is None])
def test_model_without_the_solver_is_play_game_self(idx):
    """(The C oracle plays from the initial position: the cases with a start prefix are pinned by the engine with the solver
    cleared, tests/test_solver_gpu.py.)"""
    case = SC.CASES[idx]
    A = FC.geometry(case["game"])[0]
    etas, us = FC.draws(case["seed"], case["game"], case["n_games"])
    for i, got in enumerate(SC.model_games(idx, solver=False)):
        want = orc.play_game_self(lambda b: fakepolicy.fake_eval(b, A, case["salt"]), case["game"], etas=etas[i], us=us[i],
                                  n_playouts=SC.S, **case["kw"])
        assert got["actions"] == want["actions"] and got["ret0"] == want["ret0"], (idx, i)
        assert got["counters"] == want["counters"], (idx, i)
        assert not any(got["solver_effects"].values())
        for j, ply in enumerate(got["plies"]):
            assert ply["raw"] == ply["recorded"] == want["root_cN"][j] and ply["status"] == SC.UNKNOWN, (idx, i, j)
            assert ply["pi"] == want["examples"][j][2] and ply["value"] == want["examples"][j][3], (idx, i, j)


@pytest.mark.parametrize("idx", [i for i, c in enumerate(SC.CASES) if c["game"] != SC.B66])
def test_every_status_is_the_negamax_value(idx):
    """Soundness: breakthrough 5x4 games, and connect_four positions started within 10 plies of a full board (and whole games)."""
    seen = []

    def audit(state, status, mover):
        assert status in (SC.WIN, SC.DRAW, SC.LOSS)
        assert SC.check_status(state, status, mover), (idx, status, mover, state.board().tolist())
        seen.append(status)

    games = SC.model_games(idx, solver=True, audit=audit)
    assert len(seen) > 0
    assert games == SC.model_games(idx, solver=True)                     # (the audit changes nothing)


def test_the_rules_bite_on_the_inputs_of_the_gpu_test():
    total = dict.fromkeys(SC.EFFECTS, 0)
    moves_differ = 0
    for idx, case in enumerate(SC.CASES):
        on, off = SC.model_games(idx, True), SC.model_games(idx, False)
        for a, b in zip(on, off):
            for k in SC.EFFECTS:
                total[k] += a["solver_effects"][k]
            moves_differ += a["actions"] != b["actions"]
            assert a["counters"]["sims"] == sum(p["ran"] for p in a["plies"]) <= SC.S * len(a["plies"])
            for ply in a["plies"]:
                assert sum(ply["recorded"]) > 0                          # every proven node has N >= 1
                assert ply["ran"] == SC.S or ply["status"] != SC.UNKNOWN  # only a proven root ends a search early
                if ply["status"] == SC.UNKNOWN:
                    assert ply["recorded"] == ply["raw"]
    # a proof propagated two or more levels, a LOSS child skipped, a playout stopped at a proven non-terminal node, searches ended
    # early at a won and at a lost root, a DRAW root, a kept root proven when armed, counts zeroed, a game that plays differently
    assert all(total[k] > 0 for k in SC.EFFECTS), total
    assert moves_differ > 0
    assert 42 - len(SC.case_start(SC.CASES[4])) <= 4 and 42 - len(SC.case_start(SC.CASES[0])) <= 10
    draw = [a["solver_effects"]["draw_root"] for a in SC.model_games(4, True)]
    assert sum(draw) > 0                                                 # the DRAW root: connect_four, at most 4 empty cells


def test_negamax_on_known_positions():
    s = orc.State(SC.C4)
    for a in (0, 1, 0, 1, 0, 1):                                         # three in column 0, player 0 to move: mate in one
        s.apply_action(a)
    assert SC.solved_value(s) == 1.0
    s.apply_action(6)                                                    # player 1 has three in column 1 as well
    assert SC.solved_value(s) == 1.0
    s = orc.State(SC.C4)
    assert SC.negamax(s, 3) is None                                      # nothing is decided three plies from an empty board


def test_abi_surface():
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    assert protos["az_engine_set_solver"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert protos["az_engine_read_proofs"] == (C.c_int64, [C.c_void_p, C.c_int32, C.POINTER(C.c_int8), C.c_int64])
    assert protos["az_engine_proofs_device_bytes"] == (C.c_int64, [C.c_void_p])
    assert protos["az_engine_export_proofs_device"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    header = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"int az_engine_set_solver\(az_engine \*e, int32_t on\);", header)
    assert re.search(r"int64_t az_engine_read_proofs\(az_engine \*e, int32_t slot, int8_t \*out, int64_t n\);", header)
    assert re.search(r"int az_engine_export_proofs_device\(az_engine \*e, void \*dev_buf, int64_t bytes, void \*stream\);", header)
    for name, value in (("UNKNOWN", 0), ("WIN", 1), ("DRAW", 2), ("LOSS", 3)):
        assert re.search(r"#define AZ_PROOF_%s %d\b" % (name, value), header) and getattr(_lib, "PROOF_" + name) == value
    # az_engine_read_tree keeps its signature
    assert re.search(r"int64_t az_engine_read_tree\(az_engine \*e, int32_t slot, int64_t max_nodes, int32_t \*parent, int32_t \*action,",
                     header)
    lib = _lib.load()                                                    # (raises if the library lacks a declared symbol)
    assert lib.az_engine_set_solver.argtypes == protos["az_engine_set_solver"][1]
    assert C.sizeof(_lib.AzConfig) == 152 and _lib.AzConfig.seed.offset == 104 and _lib.AzConfig.spare_pools.offset == 148
    assert (SC.UNKNOWN, SC.WIN, SC.DRAW, SC.LOSS) == (_lib.PROOF_UNKNOWN, _lib.PROOF_WIN, _lib.PROOF_DRAW, _lib.PROOF_LOSS)


def test_example_generator_takes_and_refuses_the_setting():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    net = torch.nn.Identity()
    kw = dict(n_playouts=24)                                             # (no device is touched before a generation is asked for)
    assert ExampleGenerator(net, "connect_four", "cuda:0", solver=True, **kw).solver is True
    assert ExampleGenerator(net, "connect_four", "cuda:0", **kw).solver is False
    for ok in (dict(continuous=True), dict(n_pools=2), dict(playout_cap=(6, 0.5)), dict(eval_mirror=0.5)):
        assert ExampleGenerator(net, "connect_four", "cuda:0", solver=True, **kw, **ok).solver is True
    with pytest.raises(ValueError, match="solver.*is_test=True"):
        ExampleGenerator(net, "connect_four", "cuda:0", solver=True, is_test=True, **kw)
    with pytest.raises(ValueError, match="solver.*use_puct=False"):
        ExampleGenerator(net, "connect_four", "cuda:0", solver=True, use_puct=False, **kw)
    with pytest.raises(ValueError, match="solver.*forced_playouts"):
        ExampleGenerator(net, "connect_four", "cuda:0", solver=True, forced_playouts=2.0, **kw)
