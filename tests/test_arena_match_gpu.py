"""Arena matches between search settings on the device: az_engine_set_arena_search (first-play urgency, the MCTS-Solver and the
evaluation mirror on an arena agent) and az_engine_set_arena_openings (a start position per evaluation game) against the plain-Python
model of tests/arena_match_cases.py, which tests/test_arena_match_host.py pins to the C oracle.  Same evaluator on both sides (the
deterministic fake policy through HostPolicyEvaluator) and the same Philox keys: every game is the model's, move for move."""
import functools
import math

import numpy as np
import pytest
import torch

import arena_match_cases as AM
from net_cases import drifted_net
from oracle import fakepolicy

pytestmark = pytest.mark.gpu

C4, B66 = AM.C4, AM.B66
AZ_E_INVALID, AZ_E_STATE = -1, -3
PH_MOVE = 2


def _fake(eng, salt):
    from alphazero_openspiel_amd import engine as E
    A = eng.A
    return E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, A, salt))


def _played(ex, gid):
    """The moves game `gid` PLAYED: records are indexed by absolute ply, game_len counts from the game's own start."""
    p0 = int(np.asarray(ex["start_ply"]).reshape(-1)[gid]) if np.ndim(ex["start_ply"]) else int(ex["start_ply"])
    return ex["move"][gid, p0:p0 + int(ex["game_len"][gid])].tolist()


def _live(ex):
    """[n_games, max_plies] bool: the plies that were played (absolute ply, from the game's own start)."""
    p0 = np.asarray(ex["start_ply"]).reshape(-1, 1)
    ply = np.arange(ex["move"].shape[1])[None, :]
    return (ply >= p0) & (ply < p0 + ex["game_len"].astype(np.int64)[:, None])


def _same_export(a, b):
    """Byte-equal records: lengths and results, every per-ply array on the plies that were played, the child arrays on the
    children a ply has (the rows and columns beyond them are never written)."""
    if not ((a["game_len"] == b["game_len"]).all() and (a["game_ret0"].view(np.uint32) == b["game_ret0"].view(np.uint32)).all()):
        return False
    live = _live(a)
    kids = live[:, :, None] & (np.arange(a["child_visits"].shape[2])[None, None, :] < a["n_children"][:, :, None])
    return all((a[k][live] == b[k][live]).all() for k in ("states", "move", "n_children")) and \
        (a["value"][live].view(np.uint64) == b["value"][live].view(np.uint64)).all() and \
        all((a[k][kids] == b[k][kids]).all() for k in ("child_action", "child_visits"))


# ------------------------------------------------------------------------------------------------ model parity, arena
@pytest.mark.parametrize("setting", ["fpu", "solver", "mirror", "all"])
@pytest.mark.parametrize("key", ["c4_uct", "c4_random", "bt6_uct"])
def test_arena_games_with_settings_and_openings_equal_the_model(key, setting):
    """5 slots, 12 games: slots refill from the opening table mid-run; openings of length 0-5 (0-3 on breakthrough), so the first
    phase is the agent's in some games and the opponent's in others, on both sides."""
    from alphazero_openspiel_amd import arena
    c = AM.ARENA[key]
    ops = AM.arena_openings(key)
    eng = arena.arena_engine(c["game"], AM.ARENA_SLOTS, AM.ARENA_GAMES, "zero", c["opponent"], opponent_sims=c["sims"], device=0,
                             seed=AM.ARENA_SEED, n_playouts=c["S"], openings=ops, **AM.SETTINGS[setting])
    assert eng.arena_search is not None and eng.game_starts.tolist() == c["lengths"]
    try:
        ret0, prog, ex = arena.run_arena(eng, _fake(eng, AM.ARENA_SALT), AM.ARENA_GAMES, use_graph=False, check_every=4)
    finally:
        eng.close()
    assert prog["games_done"] == AM.ARENA_GAMES and prog["error_flags"] == 0
    assert np.asarray(ex["start_ply"]).tolist() == c["lengths"]
    want = AM.arena_models(key, setting)
    for gid, w in enumerate(want):
        assert _played(ex, gid) == w["actions"], (key, setting, gid)
        assert float(ret0[gid]) == w["ret0"] and int(ex["game_len"][gid]) == w["game_len"], (key, setting, gid)


# ------------------------------------------------------------------------------------------------ the solver at an arena root
def test_solver_agent_proofs_and_moves_at_proven_roots_equal_the_model():
    """connect_four from late positions (12-14 empty cells), one game per slot, eager ticks: whenever a slot stands at a proven
    root with its move pending, read_proofs(slot) is the model's tree, status for status, and the move it then plays is the
    model's (the games are compared move for move at the end)."""
    from alphazero_openspiel_amd import arena
    c = AM.SOLVER_CASE
    ops = AM.solver_openings()
    n = len(ops)
    want = AM.solver_models()
    steps = [{s["ply"]: s for s in w["agent"].steps} for w in want]
    eng = arena.arena_engine(c["game"], n, n, "zero", c["opponent"], opponent_sims=c["sims"], device=0, seed=c["seed"],
                             n_playouts=c["S"], openings=ops, solver=True)
    checked = {AM.WIN: 0, AM.DRAW: 0, AM.LOSS: 0}
    try:
        ev = _fake(eng, c["salt"])
        eng.reset(n)
        obs, pri, val = eng.alloc_io()
        roots_buf = eng.alloc_roots()
        for tick in range(20000):
            eng.advance(pri, val, obs)
            eng.opponent_moves()
            ev(obs, pri, val)
            roots = eng.read_roots(roots_buf)
            proofs = eng.export_proofs_device().cpu().numpy()
            for g in range(n):
                if roots["phase"][g] == PH_MOVE and proofs[g, 0] != AM.UNKNOWN:
                    s = steps[int(roots["game_id"][g])][int(roots["ply"][g])]
                    assert int(proofs[g, 0]) == s["status"]
                    assert proofs[g, 1:1 + len(s["child_status"])].tolist() == s["child_status"]
                    assert eng.read_proofs(g).tolist() == s["statuses"], (g, s["ply"])
                    assert roots["child_n"][g, :len(s["raw"])].tolist() == s["raw"]     # the tree keeps the raw counts
                    checked[s["status"]] += 1
            if eng.games_done() >= n:
                break
        prog = eng.progress()
        ex = eng.export()
    finally:
        eng.close()
    assert prog["games_done"] == n and prog["error_flags"] == 0
    assert checked[AM.WIN] > 0 and checked[AM.DRAW] > 0 and checked[AM.LOSS] > 0        # lost, drawn and won roots were met
    assert sum(checked.values()) == sum(1 for w in want for s in w["agent"].steps if s["status"] != AM.UNKNOWN)
    for gid, w in enumerate(want):
        assert _played(ex, gid) == w["actions"], gid
        assert float(ex["game_ret0"][gid]) == w["ret0"]
        for s in w["agent"].steps:                                                       # no policy target is pruned: raw counts
            nc = len(s["raw"])
            assert int(ex["n_children"][gid, s["ply"]]) == nc
            assert ex["child_visits"][gid, s["ply"], :nc].tolist() == s["counts"]         # ... adjusted by rule 6 where it acts


# ------------------------------------------------------------------------------------------------ model parity, duel
def _duel_engines(key, settings=True, openings=True, **extra):
    from alphazero_openspiel_amd import engine as E
    c = AM.DUEL[key]
    ops = AM.duel_openings(key)
    n = len(ops)
    kw = dict(max_games=n, device=0, use_dirichlet=False, arena_agent="zero", opponent="external", n_playouts=c["S"], **extra)
    ea = E.SelfPlayEngine(c["game"], n, c_puct=AM.DUEL_A["c_puct"], seed=1, arena_flip=False, **kw)
    eb = E.SelfPlayEngine(c["game"], n, c_puct=AM.DUEL_B["c_puct"], seed=2, arena_flip=True, **kw)
    if settings:
        ea.set_arena_search(fpu=AM.DUEL_A["fpu"], solver=True)
        eb.set_arena_search(eval_mirror=AM.DUEL_B["eval_mirror"])
    if openings:
        ea.set_arena_openings(ops)
        eb.set_arena_openings(ops)
    return ea, eb, n


@pytest.mark.parametrize("key", ["c4", "bt6"])
def test_duel_between_two_settings_from_paired_openings_equals_the_model(key):
    """A: fpu=(0.3, 0.1) and the solver; B: eval_mirror=0.5 on its own seed; games 2k and 2k + 1 share an opening."""
    from alphazero_openspiel_amd import arena
    ea, eb, n = _duel_engines(key)
    try:
        ret0, prog, ex = arena.run_duel(ea, eb, _fake(ea, AM.DUEL_A["salt"]), _fake(eb, AM.DUEL_B["salt"]), n, seed=AM.DUEL_SEED,
                                        use_graph=False, check_every=4)
        ex_b = eb.export()
    finally:
        ea.close()
        eb.close()
    assert prog["error_flags"] == 0
    for gid, w in enumerate(AM.duel_models(key)):
        assert _played(ex, gid) == w["actions"], (key, gid)
        assert float(ret0[gid]) == w["ret0"] and int(ex["game_len"][gid]) == w["game_len"]
        assert _played(ex_b, gid) == w["actions"], (key, gid)                             # both engines export the same games
    assert (ex["game_len"] == ex_b["game_len"]).all() and (ex["game_ret0"] == ex_b["game_ret0"]).all()
    live = _live(ex)
    assert (ex["states"][live] == ex_b["states"][live]).all() and (ex["move"][live] == ex_b["move"][live]).all()


# ------------------------------------------------------------------------------------------------ nothing set changes nothing
def test_cleared_settings_and_empty_openings_change_no_byte():
    from alphazero_openspiel_amd import arena
    n_games, salt = 12, 6
    exports = []
    for touched in (False, True):
        eng = arena.arena_engine(C4, 5, n_games, "zero", "uct", opponent_sims=40, device=0, seed=2024, n_playouts=24)
        if touched:
            eng.set_arena_search(fpu=AM.FPU, solver=True, eval_mirror=0.5)
            eng.set_arena_search()
            assert eng.arena_search is None
            eng.set_arena_openings([[] for _ in range(n_games)])
        ret0, prog, ex = arena.run_arena(eng, _fake(eng, salt), n_games, use_graph=False, check_every=4)
        eng.close()
        assert prog["games_done"] == n_games and prog["error_flags"] == 0
        exports.append(ex)
    assert _same_export(*exports)
    assert np.asarray(exports[1]["start_ply"]).tolist() == [0] * n_games and exports[0]["start_ply"] == 0
    duels = []
    for touched in (False, True):
        ea, eb, n = _duel_engines("c4", settings=False, openings=False)
        if touched:
            for e in (ea, eb):
                e.set_arena_search(fpu=AM.FPU, solver=True, eval_mirror=0.5)
                e.set_arena_search(fpu=None, solver=False, eval_mirror=0.0)
                e.set_arena_openings([[] for _ in range(n)])
        ret0, prog, ex = arena.run_duel(ea, eb, _fake(ea, 3), _fake(eb, 8), n, seed=AM.DUEL_SEED, use_graph=False, check_every=4)
        ex_b = eb.export()
        ea.close()
        eb.close()
        assert prog["error_flags"] == 0
        duels.append((ex, ex_b))
    assert _same_export(duels[0][0], duels[1][0]) and _same_export(duels[0][1], duels[1][1])


# ------------------------------------------------------------------------------------------------ graph equals eager
@functools.lru_cache(maxsize=None)
def _net(name):
    from alphazero_openspiel_amd import games
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def test_match_with_a_captured_graph_plays_the_eager_games():
    from test_arena_gpu import _graph_and_eager_runs
    from alphazero_openspiel_amd import arena, engine as E, fusednet
    n_pairs = 8
    n_games = 2 * n_pairs
    ops = [o for o in arena.random_openings(C4, n_pairs, 3, seed=9) for _ in (0, 1)]

    def play(use_graph, check_every):
        kw = dict(max_games=n_games, device=0, use_dirichlet=False, arena_agent="zero", opponent="external", chain_window_us=-1,
                  n_playouts=16)
        ea = E.SelfPlayEngine(C4, n_games, seed=1, arena_flip=False, **kw)
        eb = E.SelfPlayEngine(C4, n_games, seed=2, arena_flip=True, **kw)
        ea.set_arena_search(fpu=AM.FPU, solver=True, eval_mirror=0.5)
        eb.set_arena_search(solver=True)
        evs = [fusednet.FusedNet(_net(C4), "cuda:0", max_boards=n_games, precision="f32x") for _ in (0, 1)]
        try:
            for e in (ea, eb):
                e.set_arena_openings(ops)
            return arena.run_duel(ea, eb, evs[0], evs[1], n_games, seed=5, use_graph=use_graph, check_every=check_every)
        finally:
            for x in (ea, eb, evs[0], evs[1]):
                x.close()

    _graph_and_eager_runs(play, 8)


# ------------------------------------------------------------------------------------------------ play_match on a real net
def test_play_match_of_a_setting_against_itself_scores_every_pair_zero():
    """The same network and the same settings on both sides, no mirror, greedy agents without root noise: the two games of a pair
    are ONE game seen from both sides, so every pair score is exactly 0."""
    from alphazero_openspiel_amd import arena
    n_pairs = 16
    ops = arena.random_openings(C4, n_pairs, 2, seed=3)
    settings = dict(n_playouts=32, fpu=(0.3, 0.0), solver=True)
    out = arena.play_match(_net(C4), None, C4, n_pairs, settings_a=settings, settings_b=dict(settings), openings=ops, device="cuda:0",
                           seed=11)
    assert out["pair_scores"].dtype == np.float64 and out["pair_scores"].shape == (n_pairs,)
    assert out["pair_scores"].tolist() == [0.0] * n_pairs
    assert out["score"] == 0.0 and out["stderr"] == 0.0 and out["elo"] == 0.0 and out["elo_lo"] == 0.0 and out["elo_hi"] == 0.0
    assert out["wins"] == out["losses"] and out["wins"] + out["draws"] + out["losses"] == 2 * n_pairs
    assert out["progress"]["error_flags"] == 0 and out["progress"]["games_done"] == 2 * n_pairs


def test_play_match_with_a_setting_on_one_side_is_well_formed():
    from alphazero_openspiel_amd import arena
    n_pairs = 16
    ops = arena.random_openings(C4, n_pairs, 2, seed=3)
    out = arena.play_match(_net(C4), None, C4, n_pairs, settings_a=dict(n_playouts=32, fpu=(0.3, 0.0)), settings_b=dict(n_playouts=32),
                           openings=ops, device="cuda:0", seed=11)
    assert out["wins"] + out["draws"] + out["losses"] == 32
    assert set(out) == {"wins", "draws", "losses", "pair_scores", "score", "stderr", "elo", "elo_lo", "elo_hi", "progress"}
    ps = out["pair_scores"]
    assert ps.shape == (n_pairs,) and set(np.unique(ps * 2.0)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert out["score"] == float(ps.mean()) and out["stderr"] == pytest.approx(float(ps.std(ddof=1)) / 4.0)
    assert out["wins"] - out["losses"] == int(round(float(ps.sum()) * 2.0))
    assert out["elo_lo"] <= out["elo"] <= out["elo_hi"] and not math.isnan(out["elo"])
    assert out["progress"]["error_flags"] == 0


# ------------------------------------------------------------------------------------------------ guards
def _arena(agent="zero", opponent="random", **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", 1 if agent == "net" else 8)
    if agent == "net":
        kw.setdefault("keep_search_tree", False)
    return E.SelfPlayEngine(C4, 4, max_games=8, device=0, use_dirichlet=False, arena_agent=agent, opponent=opponent, **kw)


def test_new_entries_refuse_what_they_are_not_for_and_name_the_reason():
    from alphazero_openspiel_amd import engine as E
    cases = (("a self-play engine", E.SelfPlayEngine(C4, 4, n_playouts=8, device=0), True),
             ("a manual_moves engine", E.SelfPlayEngine(C4, 4, n_playouts=8, device=0, manual_moves=True), True),
             ("AZ_ARENA_NET", _arena("net"), False), ("AZ_SELECT_UCT", _arena(use_puct=False), False))
    for what, eng, openings_too in cases:
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_arena_search is for AZ_ARENA_ZERO.*%s" % (AZ_E_INVALID, what)):
            eng.set_arena_search(solver=True)
        assert eng.arena_search is None
        if openings_too:
            with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_arena_openings is for arena engines.*%s" % (AZ_E_INVALID, what)):
                eng.set_arena_openings([[3], [2]])
            assert eng.game_starts is None
        else:                                                # openings are for both agent kinds and both select rules
            eng.set_arena_openings([[3], [2]])
            assert eng.game_starts.tolist() == [1, 1]
        eng.close()


def test_arena_search_checks_its_values_and_its_struct_size():
    import ctypes as C
    from alphazero_openspiel_amd import _lib, engine as E
    eng = _arena(opponent="external")                        # every opponent kind is allowed
    eng.set_arena_search(fpu=(0.3, 0.1), solver=True, eval_mirror=0.25)
    held = dict(eng.arena_search)
    assert held == dict(fpu=(0.3, 0.1), solver=True, eval_mirror=0.25)

    def call(**fields):
        rec = _lib.AzArenaSearch()
        rec.struct_size = C.sizeof(_lib.AzArenaSearch)
        for k, v in fields.items():
            setattr(rec, k, v)
        rc = eng.lib.az_engine_set_arena_search(eng._h, C.byref(rec))
        return rc, eng.lib.az_last_error(eng._h).decode()

    for bad in (dict(fpu_on=1, fpu_reduction=-0.1), dict(fpu_on=1, fpu_reduction=0.3, fpu_reduction_root=float("nan")),
                dict(fpu_on=1, fpu_reduction=float("inf")), dict(fpu_on=1, fpu_reduction=0.3, fpu_reduction_root=-1.0)):
        rc, err = call(**bad)
        assert rc == AZ_E_INVALID and "fpu_reduction and fpu_reduction_root must be finite and >= 0" in err, bad
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        rc, err = call(p_mirror=bad)
        assert rc == AZ_E_INVALID and "p_mirror must be finite and in [0, 1]" in err, bad
    rc, err = call(struct_size=C.sizeof(_lib.AzArenaSearch) - 8, solver=1)
    assert rc == AZ_E_INVALID and "struct_size" in err
    assert call(fpu_on=0, fpu_reduction=-5.0, reserved=77, solver=1)[0] == 0      # checks apply to a setting that is on; reserved is not looked at
    with pytest.raises(ValueError):
        eng.set_arena_search(fpu=(-1.0, 0.0))                 # the facade's own check of fpu=
    assert eng.arena_search == held
    # playout cap and forced playouts stay refused on arena engines, and so do the old setters - with the texts they had
    for name, args, text in (("set_playout_cap", (4, 0.5), "an arena engine"), ("set_forced_playouts", (2.0,), "an arena engine"),
                             ("set_fpu", (0.3,), "az_engine_set_fpu is for PUCT self-play and manual_moves engines: refused for an arena engine"),
                             ("set_solver", (True,), "az_engine_set_solver is for PUCT self-play and manual_moves engines: refused for an arena engine"),
                             ("set_eval_mirror", (0.5,), "az_engine_set_eval_mirror is for self-play and manual_moves engines: refused for an arena engine"),
                             ("set_game_starts", ([[3]],), "az_engine_set_game_starts is for plain self-play engines in a closed generation: refused for an arena engine")):
        with pytest.raises(E.EngineError) as info:
            getattr(eng, name)(*args)
        assert text in str(info.value), name
    assert eng.lib.az_engine_set_arena_search(eng._h, None) == 0                  # NULL clears
    eng.close()


def test_bad_openings_name_the_game_and_leave_the_earlier_table_in_force():
    from alphazero_openspiel_amd import arena, engine as E
    eng = arena.arena_engine(C4, 4, 8, "zero", "random", device=0, seed=3, n_playouts=8)
    good = [[3], [3, 3], [], [0, 1, 2], [6], [5, 5], [4], [2, 2, 2]]
    eng.set_arena_openings(good)
    with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_arena_openings: game 2: illegal prefix action" % AZ_E_INVALID):
        eng.set_arena_openings([[3], [2], [7]])
    with pytest.raises(E.EngineError, match=r"az_engine_set_arena_openings: game 1: illegal prefix action"):
        eng.set_arena_openings([[3], [0] * 7])                                    # a full column
    with pytest.raises(E.EngineError, match=r"az_engine_set_arena_openings: game 1: prefix ends the game"):
        eng.set_arena_openings([[3], [0, 1, 0, 1, 0, 1, 0]])
    assert eng.game_starts.tolist() == [len(h) for h in good]
    ply, keys = eng.game_starts_device(8)                                         # the read-back answers for arena engines
    assert ply.cpu().tolist() == [len(h) for h in good]
    ret0, prog, ex = arena.run_arena(eng, _fake(eng, 6), 8, use_graph=False, check_every=4)
    assert prog["games_done"] == 8 and prog["error_flags"] == 0
    for gid, h in enumerate(good):                                                # the earlier table is what the games start from
        s = E.Game(C4).new_initial_state()
        for a in h:
            s.apply_action(a)
        assert [int(x) for x in ex["states"][gid, len(h)]] == [int(b) for b in s.bb]
    short = [[3], [2]]
    eng.set_arena_openings(short)
    with pytest.raises(E.EngineError, match="n_games exceeds the games given"):
        eng.reset(3)                                                              # more games than the table holds
    eng.set_start_prefix([])                                                      # clears the table
    assert eng.game_starts is None
    eng.reset(8)
    eng.close()


def test_a_duel_whose_opening_tables_differ_is_refused():
    from alphazero_openspiel_amd import engine as E
    kw = dict(max_games=8, device=0, use_dirichlet=False, arena_agent="zero", opponent="external", n_playouts=8)
    ea = E.SelfPlayEngine(C4, 4, seed=1, arena_flip=False, **kw)
    eb = E.SelfPlayEngine(C4, 4, seed=2, arena_flip=True, **kw)
    ea.set_arena_openings([[3], [3], [2, 2], [2, 2]])
    eb.set_arena_openings([[3], [3], [2, 2], [2]])                                # game 3 starts at another ply
    ea.reset(4)
    eb.reset(4)
    with pytest.raises(E.EngineError, match=r"\(%d\).*openings differ: game 3" % AZ_E_STATE):
        ea.exchange_moves(eb)
    eb.set_arena_openings([[3], [3], [2, 2], [2, 2], [1]])                        # another length
    eb.reset(4)
    with pytest.raises(E.EngineError, match=r"\(%d\).*opening tables differ in length" % AZ_E_STATE):
        ea.exchange_moves(eb)
    eb.set_start_prefix([])                                                       # one side without a table
    eb.reset(4)
    with pytest.raises(E.EngineError, match=r"opening tables differ in length"):
        ea.exchange_moves(eb)
    eb.set_arena_openings([[3], [3], [2, 2], [2, 2]])
    eb.reset(4)
    ea.exchange_moves(eb)                                                         # equal tables pass
    torch.cuda.synchronize()
    ea.close()
    eb.close()
