"""Forced playouts and policy target pruning on the device (az_engine_set_forced_playouts and its Python facade).

References, all compared with == (there are no tolerances):
  * the rules: the Python model of tests/forced_playouts_cases.py (pinned to the C oracle at k = 0 and shown to bite on these very
    inputs by tests/test_forced_playouts_host.py) - same fake policy, same injected draws;
  * clearing, fast moves and the ways to tick: engines against engines;
  * the store: tests/replay_cases.FifoModel fed the exported (pruned) counts.
4 slots, at most 8 games, 24 playouts (fast 6)."""
import functools

import numpy as np
import pytest

import forced_playouts_cases as FC
import replay_cases as RC
from alphazero_openspiel_amd import games
from net_cases import drifted_net
from oracle import fakepolicy
from playout_cap_cases import check_store as _check, expect as _expect, same_game as _same_game
from philox_cases import schedule

pytestmark = pytest.mark.gpu

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
K, S, FAST, G, N = FC.K, FC.S, FC.S_FAST, 4, 8
SEED = 701
AZ_E_INVALID, AZ_E_STATE = -1, -3


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _engine(name, forced=None, cap=None, n_slots=G, max_games=N, **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", S)
    kw.setdefault("seed", SEED)
    eng = E.SelfPlayEngine(name, n_slots, max_games=max_games, device=0, **kw)
    if forced is not None:
        eng.set_forced_playouts(*forced)
    if cap is not None:
        eng.set_playout_cap(*cap)
    return eng


def _play(eng, ev, n=N, **kw):
    from alphazero_openspiel_amd import engine as E
    prog = E.run_selfplay(eng, ev, n, **kw)
    assert prog["games_done"] == n and prog["error_flags"] == 0
    return eng.export(), prog


def _same_games(got, want, what, n=None):
    n = len(want["game_len"]) if n is None else n
    assert got["game_len"][:n].tolist() == want["game_len"][:n].tolist(), what
    for j in range(n):
        _same_game(got, j, want, j, 0, "%s: game %d" % (what, j))


def _differ(a, b):
    n = min(int(a["game_len"][0]), int(b["game_len"][0]))
    return a["game_len"].tolist() != b["game_len"].tolist() or (a["child_visits"][0, :n] != b["child_visits"][0, :n]).any()


# ------------------------------------------------------------------------------------------------ 1. clearing
@pytest.mark.parametrize("name", [C4, B66])
def test_k_zero_and_a_cleared_setting_are_the_plain_engine(name):
    kw = dict(keep_search_tree=True, use_dirichlet=True)
    ev = _fused(name)
    plain = _engine(name, **kw)
    want, prog_plain = _play(plain, ev)
    plain.close()
    zero = _engine(name, forced=(0.0, 1), **kw)
    assert zero.forced_playouts is None
    got, prog = _play(zero, ev)
    zero.close()
    _same_games(got, want, "k = 0")
    assert prog["sims"] == prog_plain["sims"] and prog["evals"] == prog_plain["evals"]
    cleared = _engine(name, forced=(K, 1), **kw)
    forced, _ = _play(cleared, ev)                                       # a generation under the setting, then the same engine without
    assert _differ(forced, want)
    cleared.set_forced_playouts(0.0)
    got, prog = _play(cleared, ev)
    cleared.close()
    ev.close()
    _same_games(got, want, "set, then cleared")


# ------------------------------------------------------------------------------------------------ 2. the engine against the model
def _run_injected(case, forced, cap=None, small_pool=False):
    """The case's games on an engine with injected draws and the fake policy -> (reference-format games, export, progress)."""
    from alphazero_openspiel_amd import engine as E
    _, _, mc, _ = FC.geometry(case["game"])
    etas, us = FC.draws(case["seed"], case["game"], case["n_games"])
    kw = dict(case["kw"], **case["eng"])
    if small_pool:                                                       # three searches' worth of nodes: re-rooting has to compact
        kw["nodes_per_slot"] = 3 * (S + 1) * mc + 80
    eng = _engine(case["game"], forced=forced, cap=cap, n_slots=case["n_slots"], max_games=case["n_games"], rng="injected", **kw)
    try:
        eng.reset(case["n_games"])
        eng.set_injected_rng([[row[:mc] for row in e] for e in etas], us)
        A, salt = eng.A, case["salt"]
        ev = E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, A, salt))
        obs, pri, val = eng.alloc_io()
        for _ in range(200000):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
            if eng.progress()["games_done"] >= case["n_games"]:
                break
        else:
            pytest.fail("games did not finish")
        prog, ex = eng.progress(), eng.export()
        return E.examples_from_export(eng.game, ex), ex, prog
    finally:
        eng.close()


def _run_case(case, forced, cap=None):
    from alphazero_openspiel_amd import engine as E
    if case["small_pool"]:
        try:
            return _run_injected(case, forced, cap, small_pool=True)
        except E.EngineError as err:    # a kept subtree can outgrow any fixed pool: the engine says so and does not play on -
            assert "POOL_EXHAUSTED" in str(err)  # then the case is checked with the default pool (as the fuzz test does)
    return _run_injected(case, forced, cap)


def _assert_equals_model(got, want, prune, what):
    games_, ex, prog = got
    assert prog["error_flags"] == 0, what
    for i, w in enumerate(want):
        n = len(w["actions"])
        assert int(ex["game_len"][i]) == n and ex["move"][i, :n].tolist() == w["actions"], (what, i)
        assert float(ex["game_ret0"][i]) == w["ret0"], (what, i)
        for j, ply in enumerate(w["plies"]):
            nc = int(ex["n_children"][i, j])
            counts = ply["recorded"] if prune else ply["raw"]
            assert ex["child_action"][i, j, :nc].tolist() == ply["actions"], (what, i, j)
            assert ex["child_visits"][i, j, :nc].tolist() == counts, (what, i, j, ply["raw"], ply["recorded"])
            assert games_[i][j][2] == (ply["pi"] if prune else ply["pi_raw"]), (what, i, j)
            assert games_[i][j][3] == ply["value"], (what, i, j)
    for key, mkey in (("sims", "sims"), ("evals", "evals"), ("sum_depth", "sum_depth"), ("terminal_hits", "terminal_hits"),
                      ("sum_children", "sum_children")):
        assert prog[key] == sum(w["counters"][mkey] for w in want), (what, key)


@pytest.mark.parametrize("prune", [0, 1])
@pytest.mark.parametrize("idx", range(len(FC.CASES)))
def test_engine_equals_the_model(idx, prune):
    """Every move, recorded visit vector, pi, value target and counter.  prune = 0 records raw counts: selection on its own."""
    case = FC.CASES[idx]
    want = FC.model_games(idx, K)
    _assert_equals_model(_run_case(case, (K, prune)), want, prune, "case %d, prune %d" % (idx, prune))


# ------------------------------------------------------------------------------------------------ 3. with a playout cap
@pytest.mark.parametrize("name", [C4, B66])
def test_fast_moves_are_searched_and_recorded_as_without_forcing(name):
    kw = dict(keep_search_tree=True, use_dirichlet=True, cap=(FAST, 0.0))
    ev = _fused(name)
    plain = _engine(name, **kw)
    want, prog_plain = _play(plain, ev)
    plain.close()
    eng = _engine(name, forced=(K, 1), **kw)
    got, prog = _play(eng, ev)
    assert not eng.full_moves_device().any()
    eng.close()
    ev.close()
    _same_games(got, want, "all moves fast")
    assert prog["sims"] == prog_plain["sims"]


@pytest.mark.parametrize("idx", [0, 1])
def test_mixed_schedule_equals_the_model(idx):
    """Full plies are forced and pruned, fast plies are plain (kept tree: case 0, fresh trees: case 1)."""
    case = FC.CASES[idx]
    _, mp, _, _ = FC.geometry(case["game"])
    sched = schedule(SEED, case["n_games"], mp, 0.5)                     # the Python Philox model of the engine's draw
    per_game = [[(S if sched[i, t] else FAST, bool(sched[i, t])) for t in range(mp)] for i in range(case["n_games"])]
    want = FC.model_games(idx, K, schedules=per_game)
    kinds = {ply["full"] for w in want for ply in w["plies"]}
    assert kinds == {True, False}
    assert any(ply["recorded"] != ply["raw"] for w in want for ply in w["plies"])
    assert all(ply["recorded"] == ply["raw"] for w in want for ply in w["plies"] if not ply["full"])
    _assert_equals_model(_run_case(case, (K, 1), cap=(FAST, 0.5)), want, 1, "case %d under a cap" % idx)


# ------------------------------------------------------------------------------------------------ 4. scheduling invariance
def _play_with_tail(eng, ev, n=N):
    """Eager ticks; once every game is handed out and a slot has gone idle, dense request rows (compact_rows / advance_rows)."""
    eng.reset(n)
    obs, pri, val = eng.alloc_io()
    rows, compactions = None, 0
    for tick in range(200000):
        if rows is None:
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        else:
            eng.advance_rows(rows, pri, val, obs)
            ev(obs[:rows], pri[:rows], val[:rows])
        if tick % 8 == 7:
            p = eng.progress()
            if p["games_done"] >= n:
                break
            if p["games_started"] >= n and p["slots_idle"] > (0 if rows is None else eng.G - rows):
                rows = eng.compact_rows()
                compactions += 1
    assert compactions >= 1 and rows < eng.G
    return eng.export(), eng.progress()


def test_stream_graph_and_dense_rows_play_the_same_games():
    from alphazero_openspiel_amd import engine as E
    kw = dict(keep_search_tree=True, use_dirichlet=True)
    ev = _fused(C4)
    eng = _engine(C4, forced=(K, 1), **kw)
    want, prog = _play(eng, ev)
    eng.close()
    plain = _engine(C4, **kw)
    assert _differ(_play(plain, ev)[0], want)                            # (the setting does act on this seed)
    plain.close()
    eng = _engine(C4, forced=(K, 1), **kw)
    got, p = _play(eng, ev, use_graph=True, ticks_per_graph=16, check_every=32)
    eng.close()
    _same_games(got, want, "a 16-tick captured graph")
    assert p["sims"] == prog["sims"]
    eng = _engine(C4, forced=(K, 1), **kw)
    got, p = _play_with_tail(eng, ev)
    eng.close()
    _same_games(got, want, "dense rows in the tail")
    assert p["sims"] == prog["sims"]
    eng = _engine(C4, max_games=2 * N, **kw)
    stream = E.SelfPlayStream(eng, ev, seed=SEED, use_graph=False, forced_playouts=(K, True))
    try:
        assert eng.forced_playouts == (K, True)
        buf, first = stream.take(N, max_ticks=200000)
        assert first == 0
        got = E.unpack_device_export(buf.cpu().numpy(), N, eng.max_plies, eng.max_children)
    finally:
        stream.close()
        E.close_all(eng, ev)
    _same_games(got, want, "a stream")


# ------------------------------------------------------------------------------------------------ 5. the store
def test_store_takes_the_pruned_counts_through_both_append_paths():
    from alphazero_openspiel_amd import replay
    game = games.load_game(C4)
    ev = _fused(C4)
    eng = _engine(C4, forced=(K, 1), keep_search_tree=True)
    ex, _ = _play(eng, ev)
    stores = [replay.DeviceReplay(C4, device=0, max_games=40), replay.DeviceReplay(C4, device=0, max_games=40)]
    stores[0].append_engine(eng)
    stores[1].append_device(eng.export_device(), N)
    eng.close()
    plain = _engine(C4, keep_search_tree=True)
    assert _differ(_play(plain, ev)[0], ex)
    plain.close()
    ev.close()
    model = RC.FifoModel(40, 40 * game.max_game_length())
    model.append(RC.reference_games(game, ex))                           # pi from the exported counts, by the host reference
    e = _expect(model)
    for rep in stores:
        _check(rep, e)
        rep.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    for what, eng in (("arena", _engine(C4, arena_agent="zero", opponent="random")),
                      ("manual_moves", _engine(C4, manual_moves=True)),
                      ("AZ_SELECT_UCT", _engine(C4, use_puct=False))):
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_forced_playouts is for plain PUCT self-play.*%s" % (AZ_E_INVALID, what)):
            eng.set_forced_playouts(K)
        assert eng.forced_playouts is None
        eng.close()
    eng = _engine(C4)
    for k, prune in ((-0.5, 1), (float("nan"), 1), (float("inf"), 0), (K, 2), (K, -1)):
        with pytest.raises(E.EngineError, match=r"\(%d\).*k must be finite and >= 0.*prune 0 or 1" % AZ_E_INVALID):
            eng.set_forced_playouts(k, prune)
        assert eng.forced_playouts is None
    eng.reset(4)
    eng.set_forced_playouts(K, False)
    assert eng.forced_playouts == (K, False)
    obs, pri, val = eng.alloc_io()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):     # the caller starts a generation after the call
        eng.advance(pri, val, obs)
    eng.set_playout_cap(FAST, 0.5)                                       # composes with a cap, either order
    eng.set_forced_playouts(K)
    eng.reset(4)
    eng.advance(pri, val, obs)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. facade
def _flat(games_):
    return [(r[0], r[2], r[3]) for g in games_ for r in g]


def test_example_generator_passes_the_setting_to_its_engines():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    kw = dict(n_playouts=S, n_slots=G, seed=5, use_graph=False)
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", forced_playouts=K, **kw)
    out = gen.generate_examples(N)
    gen.close()
    eng = _engine(C4, forced=(K, True), seed=5)                          # the generator's first generation
    ev = _fused(C4)
    ex, _ = _play(eng, ev)
    eng.close()
    ev.close()
    assert _flat(out) == _flat(E.examples_from_export(eng.game, ex))
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", **kw)
    plain = gen.generate_examples(N)
    gen.close()
    assert [r[1] for r in _flat(out)] != [r[1] for r in _flat(plain)]    # the visit-derived pi differs on the same seed
    for more in (dict(n_pools=2), dict(pool_devices=["cuda:0", "cuda:0"]), dict(continuous=True)):
        gen = ExampleGenerator(_net(C4), C4, "cuda:0", forced_playouts=K, **kw, **more)
        got = gen.generate_examples(N)
        gen.close()
        assert len(got) == N and all(len(g) >= 7 for g in got)
        assert gen.last_progress["error_flags"] == 0
        if "pool_devices" not in more:                                   # one engine, the first generation's seed: the same games
            assert _flat(got) == _flat(out)
        else:                                                            # two engines of 4 games with seeds of their own
            assert _flat(got) != _flat(plain)
