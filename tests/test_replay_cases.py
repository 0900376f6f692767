"""CPU checks of the replay-store test helpers (tests/replay_cases.py) and of the host reference on the edges they write:
the GPU tests trust both."""
import numpy as np
import pytest

import replay_cases as RC
from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.alphazerobot import remove_illegal_actions
from alphazero_openspiel_amd.engine import pis_from_visits, unpack_device_export

BOARDS = ["connect_four", "breakthrough(rows=5,columns=4)", "breakthrough(rows=6,columns=6)", "breakthrough(rows=8,columns=8)"]


@pytest.mark.parametrize("name", BOARDS)
def test_one_move_prefixes_end_in_a_position_with_one_legal_move(name):
    game = games.load_game(name)
    assert game.name == name
    s = games.state_from_history(game, RC.ONE_MOVE_PREFIX[name])   # (apply_action refuses an illegal action)
    assert not s.is_terminal() and len(s.legal_actions()) == 1


@pytest.mark.parametrize("name", BOARDS)
def test_host_reference_on_the_visit_count_edges(name):
    """Before the reference is trusted with them: on plies with unvisited children, one child, and counts up to 2^31 whose
    total exceeds 2^32, pis_from_visits must be float(v) / sum(v) with Python ints (mcts.py:161-162) followed by
    remove_illegal_actions (alphazerobot.py:7-18)."""
    game = games.load_game(name)
    A = game.num_distinct_actions()
    ex = RC.fake_export(game, n_games=4, seed=11, openings=[RC.ONE_MOVE_PREFIX[name], []], visits="edges")
    seen = {"one": 0, "zero": 0, "wide": 0}
    for g in range(4):
        n = int(ex["game_len"][g])
        bulk = pis_from_visits(ex["child_action"][g, :n], ex["child_visits"][g, :n], ex["n_children"][g, :n], A)
        for i in range(n):
            nc = int(ex["n_children"][g, i])
            acts = [int(a) for a in ex["child_action"][g, i, :nc]]
            vis = [int(v) for v in ex["child_visits"][g, i, :nc]]
            assert sum(vis) > 0
            seen["one"] += nc == 1
            seen["zero"] += 0 in vis
            seen["wide"] += sum(vis) > 2 ** 32
            dense = [0] * A
            for a, v in zip(acts, vis):
                dense[a] = v
            total = sum(dense)                                  # a Python int: no wrap, no rounding
            want = remove_illegal_actions(np.array([float(v) / total for v in dense]), acts)
            assert bulk[i].tolist() == want.tolist(), (g, i)
    assert all(seen.values()), seen


def test_start_history_moves_the_records_and_keeps_the_absolute_sign():
    game = games.load_game("connect_four")
    for hist in ([3], [3, 3, 2, 4]):
        p0 = len(hist)
        ex = RC.fake_export(game, n_games=5, seed=2, start_history=hist, openings=RC.random_openings(game, 3, 2, 1, hist))
        assert ex["start_ply"] == p0
        for g in range(5):
            n = int(ex["game_len"][g])
            s = games.state_from_history(game, hist)
            assert not ex["n_children"][g, :p0].any() and not ex["n_children"][g, p0 + n:].any()
            for i in range(p0, p0 + n):
                assert ex["states"][g, i].tolist() == s.bb
                s.apply_action(int(ex["move"][g, i]))
            assert s.is_terminal() and s.returns()[0] == ex["game_ret0"][g]
            # the value target of a ply is the return of the player to move there
            assert ex["value"][g, p0:p0 + n].tolist() == [s.returns()[i & 1] for i in range(p0, p0 + n)]
        keys = [r[0] for g in RC.reference_games(game, ex, hist) for r in g]
        assert keys[0] == ", ".join(str(a) for a in hist)


def test_pack_device_export_is_the_inverse_of_unpack():
    game = games.load_game("breakthrough(rows=5,columns=4)")
    ex = RC.fake_export(game, n_games=3, seed=5, visits="edges")
    back = unpack_device_export(RC.pack_device_export(ex), 3, game.max_game_length(), game.max_children())
    for k in ("game_len", "game_ret0", "states", "move", "n_children", "child_action", "child_visits", "value"):
        assert back[k].dtype == ex[k].dtype and (back[k] == ex[k]).all(), k


def test_fifo_model_applies_both_limits_in_the_stores_order():
    m = RC.FifoModel(max_games=4, max_examples=10)
    gen = lambda *lens: [[[str(k)] for k in range(n)] for n in lens]
    assert m.append(gen(3, 3))[1:] == (2, 6, 0)
    assert m.append(gen(0, 2))[1:] == (3, 8, 0)                   # an empty game is not a game
    assert m.append(gen(4))[1:] == (3, 9, 1) and m.ring_evictions == 1   # 8 + 4 > 10: the oldest game leaves first
    m.set_capacity(2)
    assert m.n_games == 3                                          # the trim happens at the append
    assert m.append(gen(1))[1:] == (2, 5, 3) and m.cap_evictions == 2
    with pytest.raises(ValueError):
        m.append(gen(6, 5))
    assert (m.n_games, m.n_examples, m.games_dropped) == (2, 5, 3)  # a refused generation changes nothing
    assert m.append(gen(5, 5))[1:] == (2, 10, 5)                  # room is made for exactly max_examples
