"""Host side of the batched position analysis (no GPU): the packed root-export layout against a hand-built byte string, and
the argument checks analyze_positions makes before it touches the device."""
import struct

import numpy as np
import pytest

from alphazero_openspiel_amd import analysis, engine, games
from analysis_positions import random_positions


def _pad16(b):
    return b + b"\0" * (-len(b) % 16)


def test_roots_export_layout_against_hand_built_bytes():
    """include/az_engine.h, az_engine_export_roots_device: G = 3 slots, mc = 2 children, every array 16-byte aligned."""
    G, mc = 3, 2
    raw = b"".join(_pad16(part) for part in (
        struct.pack("<4i", 2, G, mc, 0),                              # header: finished, G, mc, error flags
        struct.pack("<3i", 0, 1, -1),                                 # game_id
        struct.pack("<3i", 5, 4, 0),                                  # phase
        struct.pack("<3i", 7, 0, 0),                                  # ply
        struct.pack("<3i", 32, 9, 0),                                 # sims_done
        struct.pack("<3i", 2, 1, 0),                                  # n_children
        struct.pack("<3I", 32, 9, 0),                                 # root_n
        struct.pack("<3d", -0.25, 0.5, 0.0),                          # root_q
        struct.pack("<6i", 1, 4, 3, -1, -1, -1),                      # child_action
        struct.pack("<6I", 20, 11, 8, 0, 0, 0),                       # child_n
        struct.pack("<6d", 0.125, -0.5, 0.75, 0.0, 0.0, 0.0),         # child_q
        struct.pack("<6d", 0.6, 0.4, 1.0, 0.0, 0.0, 0.0),             # child_p
    ))
    layout, total = engine.roots_export_layout(G, mc)
    assert total == len(raw) == 16 * 7 + 32 + 32 + 32 + 48 + 48
    assert [(name, off) for name, _, _, off in layout] == [
        ("header", 0), ("game_id", 16), ("phase", 32), ("ply", 48), ("sims_done", 64), ("n_children", 80), ("root_n", 96),
        ("root_q", 112), ("child_action", 144), ("child_n", 176), ("child_q", 208), ("child_p", 256)]
    r = engine.unpack_roots_export(np.frombuffer(raw, dtype=np.uint8), G, mc)
    assert r["n_finished"] == 2 and r["error_flags"] == 0
    assert r["game_id"].tolist() == [0, 1, -1] and r["phase"].tolist() == [5, 4, 0] and r["ply"].tolist() == [7, 0, 0]
    assert r["sims_done"].tolist() == [32, 9, 0] and r["n_children"].tolist() == [2, 1, 0]
    assert r["root_n"].tolist() == [32, 9, 0] and r["root_n"].dtype == np.int64
    assert r["root_q"].tolist() == [-0.25, 0.5, 0.0]
    assert r["child_action"].tolist() == [[1, 4], [3, -1], [-1, -1]]
    assert r["child_n"].tolist() == [[20, 11], [8, 0], [0, 0]] and r["child_n"].dtype == np.int64
    assert r["child_q"].tolist() == [[0.125, -0.5], [0.75, 0.0], [0.0, 0.0]]
    assert r["child_p"].tolist() == [[0.6, 0.4], [1.0, 0.0], [0.0, 0.0]]
    d = analysis.dense_roots(r, 2, 7)
    assert d["visits"].tolist() == [[0, 20, 0, 0, 11, 0, 0], [0, 0, 0, 8, 0, 0, 0]]
    assert d["q"][0].tolist() == [0, 0.125, 0, 0, -0.5, 0, 0] and d["priors"][1].tolist() == [0, 0, 0, 1.0, 0, 0, 0]
    assert d["best_action"].tolist() == [1, 3] and d["root_n"].tolist() == [32, 9]
    with pytest.raises(ValueError):
        engine.unpack_roots_export(np.frombuffer(raw[:-1], dtype=np.uint8), G, mc)
    with pytest.raises(ValueError):
        engine.unpack_roots_export(np.frombuffer(raw, dtype=np.uint8), G, mc + 1)


def test_best_action_is_the_first_maximum():
    roots = {"child_action": np.array([[0, 2, 5], [1, 3, -1]], dtype=np.int32), "child_n": np.array([[4, 9, 9], [0, 0, 0]]),
             "child_q": np.zeros((2, 3)), "child_p": np.full((2, 3), 0.25), "root_q": np.zeros(2), "root_n": np.array([23, 0]),
             "phase": np.array([5, 1])}
    d = analysis.dense_roots(roots, 2, 6)
    assert d["best_action"].tolist() == [2, 1]  # ties: the lower action; no visits yet: the first child


def test_pack_histories():
    actions, lengths, stride = engine.pack_histories([[3, 3, 4], [], [6]])
    assert stride == 3 and lengths.tolist() == [3, 0, 1] and actions.dtype == np.int32 and lengths.dtype == np.int32
    assert actions.tolist() == [[3, 3, 4], [0, 0, 0], [6, 0, 0]]
    actions, lengths, stride = engine.pack_histories([[]])
    assert stride == 1 and actions.shape == (1, 1)


def test_argument_checks_come_before_any_device_call():
    """None of these reaches the engine (they pass on a machine without a GPU)."""
    with pytest.raises(ValueError, match="at least one position"):
        analysis.analyze_positions(None, "connect_four", [])
    bt = games.load_game("breakthrough(rows=6,columns=6)").new_initial_state()
    with pytest.raises(ValueError, match="position 1 is a state of breakthrough"):
        analysis.analyze_positions(None, "connect_four", [[3], bt])
    over = games.state_from_history(games.load_game("connect_four"), [0, 1, 0, 1, 0, 1, 0])
    assert over.is_terminal()
    with pytest.raises(ValueError, match="position 0 is terminal"):
        analysis.analyze_positions(None, "connect_four", [over])
    with pytest.raises(ValueError, match="n_slots"):
        analysis.analyze_positions(None, "connect_four", [[3]], n_slots=-2)


@pytest.mark.parametrize("game", ["connect_four", "breakthrough(rows=6,columns=6)"])
def test_states_and_action_lists_give_the_same_prefixes(game):
    hist = random_positions(game, 20, 21, 0, 20)
    g = games.load_game(game)
    states = [games.state_from_history(g, h) for h in hist]
    assert analysis.position_prefixes(game, states) == hist
    assert analysis.position_prefixes(g, hist) == hist
    mixed = [s if i % 2 else h for i, (s, h) in enumerate(zip(states, hist))]
    assert analysis.position_prefixes(game, mixed) == hist
    assert all(isinstance(a, int) for h in analysis.position_prefixes(game, [np.array(h, dtype=np.int64) for h in hist]) for a in h)


def test_public_entry_points():
    import alphazero_openspiel_amd as pkg
    assert pkg.analyze_positions is analysis.analyze_positions and pkg.Analyzer is analysis.Analyzer
