"""Host side of the arena match (az_engine_set_arena_search, az_engine_set_arena_openings, arena.play_match): the model of
tests/arena_match_cases.py against the C oracle, the cases of tests/test_arena_match_gpu.py doing what they are for, the opening
generator and the match statistics.  No GPU."""
import math

import numpy as np
import pytest

import arena_match_cases as AM
from alphazero_openspiel_amd import arena, games
from oracle import binding as orc
from oracle import fakepolicy


# ------------------------------------------------------------------------------------------------ the model is the oracle's game
@pytest.mark.parametrize("game_name,opponent,S,sims", [
    ("connect_four", "uct", 24, 40), ("connect_four", "random", 16, 0), ("breakthrough(rows=6,columns=6)", "uct", 12, 20)])
def test_model_arena_games_equal_the_oracle(game_name, opponent, S, sims):
    """Every setting off, an empty opening, the parameters of tests/test_arena_gpu.py: move for move orc.play_arena_game."""
    A, salt, seed = orc.State(game_name).num_actions, 6, 2024
    for gid in range(12):
        want = orc.play_arena_game(lambda b: fakepolicy.fake_eval(b, A, salt), game_name, gid, agent="zero", opponent=opponent,
                                   opponent_sims=sims, n_playouts=S, seed=seed)
        got = AM.play_arena_game(game_name, gid, salt, seed, opponent=opponent, opponent_sims=sims, n_playouts=S)
        assert got["actions"] == want["actions"] and got["ret0"] == want["ret0"], gid


@pytest.mark.parametrize("game_name,opponent,S,sims,npa", [
    ("connect_four", "random", 20, 0, 1000), ("connect_four", "uct", 16, 30, 3), ("breakthrough(rows=6,columns=6)", "random", 10, 0, 1000)])
def test_model_probabilistic_agent_equals_the_oracle(game_name, opponent, S, sims, npa):
    A, salt, seed = orc.State(game_name).num_actions, 6, 77
    for gid in range(12):
        want = orc.play_arena_game(lambda b: fakepolicy.fake_eval(b, A, salt), game_name, gid, agent="zero", opponent=opponent,
                                   opponent_sims=sims, n_playouts=S, seed=seed, use_probabilistic_actions=True,
                                   num_probabilistic_actions=npa)
        got = AM.play_arena_game(game_name, gid, salt, seed, opponent=opponent, opponent_sims=sims, n_playouts=S,
                                 use_probabilistic_actions=True, num_probabilistic_actions=npa)
        assert got["actions"] == want["actions"] and got["ret0"] == want["ret0"], gid


@pytest.mark.parametrize("game_name,S1,S2", [("connect_four", 24, 12), ("breakthrough(rows=6,columns=6)", 10, 16)])
def test_model_duel_games_equal_the_oracle(game_name, S1, S2):
    A = orc.State(game_name).num_actions
    for gid in range(10):
        want = orc.play_duel_game(lambda b: fakepolicy.fake_eval(b, A, 3), lambda b: fakepolicy.fake_eval(b, A, 8), game_name, gid,
                                  n_playouts1=S1, n_playouts2=S2, c_puct1=2.5, c_puct2=1.5)
        got = AM.play_duel_game(game_name, gid, dict(salt=3, seed=1, n_playouts=S1, c_puct=2.5),
                                dict(salt=8, seed=2, n_playouts=S2, c_puct=1.5))
        assert got["actions"] == want["actions"] and got["ret0"] == want["ret0"], gid


# ------------------------------------------------------------------------------------------------ the cases do what they are for
def test_openings_of_the_cases_cover_both_first_phases_for_both_sides():
    for key, c in AM.ARENA.items():
        ops = AM.arena_openings(key)
        assert [len(o) for o in ops] == c["lengths"] and len(ops) == AM.ARENA_GAMES > AM.ARENA_SLOTS
        first = {(i & 1, (len(o) & 1) == (i & 1)) for i, o in enumerate(ops)}    # (agent's side, does the agent move first?)
        assert first == {(0, True), (0, False), (1, True), (1, False)}, key
        assert any(len(o) >= 2 for o in ops) and any(len(o) == 0 for o in ops)   # update_root before the first search, and not
        late = [i for i in range(AM.ARENA_SLOTS, AM.ARENA_GAMES)]                # games a slot takes mid-run: both first phases
        assert {(len(ops[i]) & 1) == (i & 1) for i in late} == {True, False}, key
    for key in AM.DUEL:
        ops = AM.duel_openings(key)
        assert all(ops[2 * k] == ops[2 * k + 1] for k in range(len(ops) // 2)) and len(ops) == 10
        assert {len(o) & 1 for o in ops} == {0, 1}


def test_solver_case_moves_at_proven_roots_of_every_kind():
    ws = AM.solver_models()
    steps = [s for w in ws for s in w["agent"].steps]
    won = [s for s in steps if s["status"] == AM.LOSS]
    drawn = [s for s in steps if s["status"] == AM.DRAW]
    lost = [s for s in steps if s["status"] == AM.WIN]
    assert won and drawn and lost
    assert any(s["kept_status"] != AM.UNKNOWN and s["ran"] == 0 for s in steps)   # a kept subtree already proven: no playout runs
    assert any(s["counts"] != s["raw"] for s in won)                            # rule 6 changes the counts the move is drawn from
    for s in won:                                                               # a won root plays a proven win ...
        i = s["actions"].index(s["move"])
        assert s["child_status"][i] == AM.WIN
        best = max(n for n, st in zip(s["raw"], s["child_status"]) if st == AM.WIN)
        assert s["raw"][i] == best and all(not (st == AM.WIN and n == best) for n, st in zip(s["raw"][:i], s["child_status"][:i]))
    for s in drawn:                                                             # ... a drawn root never a proven loss
        assert s["child_status"][s["actions"].index(s["move"])] != AM.LOSS
    for s in lost:                                                              # ... a lost root plays as before
        assert s["counts"] == s["raw"] and s["move"] == s["actions"][s["raw"].index(max(s["raw"]))]
    for w in ws:                                                                # a won root is followed by the win
        for s in w["agent"].steps:
            if s["status"] == AM.LOSS:
                side = 1.0 if AM.agent_side(w["agent"].gid) == 0 else -1.0
                assert w["ret0"] == side


def test_fpu_and_mirror_cases_change_games():
    plain = AM.arena_models("c4_uct", None)
    fpu = AM.arena_models("c4_uct", "fpu")
    assert any(a["actions"] != b["actions"] for a, b in zip(plain, fpu))
    assert sum(w["agent"].fpu_differs for w in fpu) > 0
    for key in ("c4_uct", "bt6_uct"):
        mir = AM.arena_models(key, "mirror")
        there, back = sum(w["agent"].mirrored[1] for w in mir), sum(w["agent"].mirrored[0] for w in mir)
        assert there > 0 and back > 0, key
        assert all(w["agent"].mirrored[0] > 0 and w["agent"].mirrored[1] > 0 for w in mir), key
    table = AM.action_mirror_table(games.load_game(AM.B66))
    assert table != list(range(len(table)))                                     # breakthrough: the action map is not the identity
    assert any(a["actions"] != b["actions"] for a, b in zip(AM.arena_models("bt6_uct", None), AM.arena_models("bt6_uct", "mirror")))


def test_duel_case_carries_its_settings():
    ws = AM.duel_models("c4")
    assert sum(w["a"].fpu_differs for w in ws) > 0 and sum(w["b"].mirrored[1] for w in ws) > 0
    assert all(w["a"].mirrored[1] == 0 for w in ws) and all(w["b"].fpu_differs == 0 for w in ws)
    assert any(s["status"] != AM.UNKNOWN for w in ws for s in w["a"].steps)      # A's solver proves roots
    assert all(s["status"] == AM.UNKNOWN for w in ws for s in w["b"].steps)      # B's never does


# ------------------------------------------------------------------------------------------------ random_openings
@pytest.mark.parametrize("game_name,n,plies", [("connect_four", 64, 4), ("breakthrough(rows=6,columns=6)", 40, 3), ("connect_four", 7, 1),
                                               ("connect_four", 1, 0)])
def test_random_openings_are_distinct_legal_and_deterministic(game_name, n, plies):
    ops = arena.random_openings(game_name, n, plies, seed=5)
    assert len(ops) == n and len({tuple(o) for o in ops}) == n and all(len(o) == plies for o in ops)
    game = games.load_game(game_name)
    for o in ops:
        s = game.new_initial_state()
        for a in o:
            assert a in s.legal_actions()
            s.apply_action(a)
        assert not s.is_terminal()
    assert arena.random_openings(game_name, n, plies, seed=5) == ops
    if plies >= 3:
        assert arena.random_openings(game_name, n, plies, seed=6) != ops


def test_random_openings_says_when_the_game_has_too_few():
    with pytest.raises(ValueError, match="distinct"):
        arena.random_openings("connect_four", 8, 1, seed=0)                     # connect_four has 7 first moves
    with pytest.raises(ValueError, match="distinct"):
        arena.random_openings("connect_four", 2, 0, seed=0)                     # ... and one empty opening


# ------------------------------------------------------------------------------------------------ the statistics of a match
def test_match_stats_on_hand_written_results():
    # game 2k: A is player 0, game 2k + 1: A is player 1; ret0 = returns()[0]
    st = arena.match_stats([1, -1, 1, -1])                                      # A wins all four
    assert (st["wins"], st["draws"], st["losses"]) == (4, 0, 0) and st["pair_scores"].tolist() == [1.0, 1.0]
    assert st["score"] == 1.0 and st["stderr"] == 0.0 and st["elo"] == math.inf and st["elo_lo"] == math.inf and st["elo_hi"] == math.inf
    st = arena.match_stats([-1, 1])                                             # A loses both, one pair
    assert (st["wins"], st["draws"], st["losses"]) == (0, 0, 2) and st["score"] == -1.0 and st["stderr"] == 0.0
    assert st["elo"] == -math.inf
    st = arena.match_stats([1, 1, -1, -1, 0, 0])                                # each pair: one game seen from both sides
    assert st["pair_scores"].tolist() == [0.0, 0.0, 0.0] and st["pair_scores"].dtype == np.float64
    assert (st["wins"], st["draws"], st["losses"]) == (2, 2, 2)
    assert st["score"] == 0.0 and st["stderr"] == 0.0 and st["elo"] == 0.0 and st["elo_lo"] == 0.0 and st["elo_hi"] == 0.0
    st = arena.match_stats([1, -1, 1, 1, 0, 0, -1, 0])                          # pair scores 1, 0, 0, -1/2
    assert st["pair_scores"].tolist() == [1.0, 0.0, 0.0, -0.5]
    assert (st["wins"], st["draws"], st["losses"]) == (3, 3, 2) and st["wins"] + st["draws"] + st["losses"] == 8
    assert st["score"] == 0.125
    sd = math.sqrt(sum((x - 0.125) ** 2 for x in (1.0, 0.0, 0.0, -0.5)) / 3)
    assert st["stderr"] == pytest.approx(sd / 2.0, rel=1e-15)
    p = (0.125 + 1.0) / 2.0
    assert st["elo"] == pytest.approx(-400.0 * math.log10(1.0 / p - 1.0), rel=1e-15)
    half = 1.96 * st["stderr"] / 2.0
    assert st["elo_lo"] == pytest.approx(-400.0 * math.log10(1.0 / (p - half) - 1.0), rel=1e-12)
    assert st["elo_hi"] == pytest.approx(-400.0 * math.log10(1.0 / (p + half) - 1.0), rel=1e-12)
    assert st["elo_lo"] < st["elo"] < st["elo_hi"]
    flipped = arena.match_stats([1, -1, 1, 1, 0, 0, -1, 0], flip=True)          # the same match seen from B
    assert flipped["score"] == -0.125 and flipped["wins"] == 2 and flipped["losses"] == 3 and flipped["elo"] == pytest.approx(-st["elo"])
    st = arena.match_stats([1, -1, 1, -1, 1, -1, 1, 1])                         # an interval that reaches past p = 1
    assert st["elo_hi"] == math.inf and math.isfinite(st["elo"]) and math.isfinite(st["elo_lo"])
    for bad in ([], [1.0], [1, -1, 0]):
        with pytest.raises(ValueError):
            arena.match_stats(bad)


def test_elo_of():
    assert arena.elo_of(0.5) == 0.0 and arena.elo_of(0.0) == -math.inf and arena.elo_of(1.0) == math.inf
    assert arena.elo_of(-0.1) == -math.inf and arena.elo_of(1.1) == math.inf
    assert arena.elo_of(10.0 / 11.0) == pytest.approx(400.0) and arena.elo_of(0.25) == pytest.approx(-arena.elo_of(0.75))


def test_play_match_checks_its_arguments_before_it_builds_anything():
    with pytest.raises(ValueError, match="pairs"):
        arena.play_match(None, None, "connect_four", 0, device="cuda:0")
    with pytest.raises(ValueError, match="openings"):
        arena.play_match(None, None, "connect_four", 2, openings=[[3]], device="cuda:0")


def test_abi_surface():
    import ctypes
    import os
    import re
    from alphazero_openspiel_amd import _lib
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"int az_engine_set_arena_search\(az_engine \*e, const az_arena_search \*s\);", header)
    assert re.search(r"int az_engine_set_arena_openings\(az_engine \*e, const int32_t \*actions, const int32_t \*lengths, int64_t stride, "
                     r"int64_t n_games\);", header)
    assert ctypes.sizeof(_lib.AzArenaSearch) == 40 and _lib.AzArenaSearch.p_mirror.offset == 32
    assert _lib.AzArenaSearch.fpu_reduction.offset == 8 and _lib.AzArenaSearch.solver.offset == 24
    names = {n for n, _, _ in _lib.PROTOTYPES}
    assert {"az_engine_set_arena_search", "az_engine_set_arena_openings"} <= names
