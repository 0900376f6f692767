"""The MCTS-Solver kernels (az_advance_kernel<..., SOLVER = true> and move_step's rule 6) at the playout counts the project ships
- connect_four at 400, breakthrough 6x6 at 800 and 8x8 at 1600, on kept trees - and on select paths deeper than 64 and 128 plies,
against the Python model of tests/solver_cases.py, WHOLE TREE by whole tree.

tests/test_solver_gpu.py runs the same kernels at 24 playouts, where a search stays above depth 16 and a proof climbs two or three
levels; here a search skips thousands of lost children, stops playouts at proven non-terminal nodes, climbs 9 levels, walks a
proof across lane 63 / lane 0 of the path registers, ends early at proven roots, re-roots into trees with hundreds of proven
nodes and carries them through compact_jobs.  tests/test_solver_scale_host.py asserts on the CPU that the cases reach all that,
pins the model to the C oracle (solver off, whole trees) and to a brute-force negamax (solver on).

Bar: ==.  Integers as integers, Q and P as bit patterns; no tolerance anywhere.  All engines are fed by a HostPolicyEvaluator over
the memoised policies of product_scale_cases.py and deep_line_cases.py: no net is involved.  The model's runs are computed once
per case in fixtures (pytest counts them in a test's setup, not its call)."""
import numpy as np
import pytest
import torch

import forced_playouts_cases as FC
import product_scale_cases as PS
import solver_cases as SC

pytestmark = pytest.mark.gpu

PH_SEARCH_DONE = 5
SCHEDULES = {"default": dict(), "one_per_tick": dict(max_sims_per_tick=1, chain_window_us=-1),
             "three_per_tick": dict(max_sims_per_tick=3, chain_window_us=-1)}


def _E():
    from alphazero_openspiel_amd import engine
    return engine


@pytest.fixture
def scale_want(key):
    return SC.scale_model(key)


@pytest.fixture
def deep_want(key):
    return SC.deep_model(key)


@pytest.fixture
def games_want(key):
    return SC.game_models(key), SC.small_pool(key)


@pytest.fixture
def deep_game_want():
    return SC.deep_game_model()


def _assert_same_tree(eng, want, where):
    """read_tree and read_proofs of slot 0 against a dump of the model."""
    got, proofs = eng.read_tree(0), eng.read_proofs(0)
    assert len(got["N"]) == len(want["N"]) == len(proofs), where
    for f in ("parent", "action", "N"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (where, f)
    for f in ("Q", "P"):                                               # bit patterns: -0.0 and NaN cannot hide
        assert np.array_equal(got[f].view(np.int64), want[f].view(np.int64)), (where, f)
    assert proofs.dtype == want["status"].dtype and np.array_equal(proofs, want["status"]), (where, "status")
    return proofs


def _assert_root_proofs(eng, tree, proofs, where):
    """export_proofs_device == read_proofs at the root and its children (rows 1..nc of a breadth-first tree), 0 beyond."""
    dev = eng.export_proofs_device().cpu().numpy()
    assert dev.shape == (1, 1 + eng.max_children), where
    nc = int((tree["parent"] == 0).sum())
    assert dev[0, 0] == proofs[0] and dev[0, 1:1 + nc].tolist() == proofs[1:1 + nc].tolist() and not dev[0, 1 + nc:].any(), where


def _search(eng, ev, io, buf):
    """advance + evaluate until the root export's header says that the slot is done."""
    obs, pri, val = io
    for _ in range(4 * eng.cfg.n_playouts + 16):
        for _ in range(4):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        eng.export_roots_device(buf)
        if int(buf[:16].view(torch.int32)[0].item()) == eng.G:
            return
    pytest.fail("the search did not finish")


def _manual_engine(game, n_playouts, policy, start=(), **sched):
    E = _E()
    eng = E.SelfPlayEngine(game, 1, n_playouts=n_playouts, use_dirichlet=False, manual_moves=True, rng="injected", max_games=1,
                           **sched)
    eng.set_start_positions([list(start)])
    eng.set_solver(True)
    eng.reset(1)
    eng.set_injected_rng([[[0.0]] * eng.max_plies], [[0.0] * eng.max_plies], absolute_ply=True)
    return eng, E.HostPolicyEvaluator(eng, policy), eng.alloc_io(), eng.alloc_roots()


def _check_search(eng, buf, ply, where):
    roots = eng.read_roots(buf)
    assert roots["error_flags"] == 0 and (roots["phase"] == PH_SEARCH_DONE).all(), where
    proofs = _assert_same_tree(eng, ply["tree"], where)
    _assert_root_proofs(eng, ply["tree"], proofs, where)
    assert proofs[0] == ply["status"], where
    assert eng.read_slot(0)["sims_done"] == ply["ran"], where
    nc = len(ply["actions"])
    assert roots["child_action"][0, :nc].tolist() == ply["actions"] and roots["child_n"][0, :nc].tolist() == ply["raw"], where
    prog = eng.progress()
    assert prog["error_flags"] == 0, where
    for f in SC.COUNTERS:
        assert prog[f] == ply["counters"][f], (where, f)
    return prog


# ------------------------------------------------------------------------------------------------ a. whole trees of sequences
def _run_sequence(key, want, **sched):
    c = SC.SCALE_CASES[key]
    eng, ev, io, buf = _manual_engine(c["game"], c["n_playouts"], PS.policy(c["game"]), c["start"], **sched)
    try:
        sims = 0
        for k, ply in enumerate(want["plies"]):
            where = (key, "search", k)
            if k:
                eng.update_root([want["plies"][k - 1]["move"]], keep_subtree=True)
                proofs = _assert_same_tree(eng, ply["kept"], (key, "re-rooting", k))   # kept subtree and statuses, before the search
                _assert_root_proofs(eng, ply["kept"], proofs, (key, "re-rooting", k))
            _search(eng, ev, io, buf)
            prog = _check_search(eng, buf, ply, where)
            if k and ply["kept"]["status"][0] != SC.UNKNOWN:            # a kept proven root: armed, found proven, done
                assert ply["ran"] == 0 and eng.read_slot(0)["sims_done"] == 0 and prog["sims"] == sims, where
            assert prog["sims"] == sims + ply["ran"], where
            sims = prog["sims"]
    finally:
        eng.close()


@pytest.mark.parametrize("sched", ["default", "one_per_tick"])
@pytest.mark.parametrize("key", sorted(SC.SCALE_CASES))
def test_whole_trees_of_a_sequence(key, sched, scale_want):
    """Search, update_root(the model's move), search again, to the end of the game on one kept tree: after every search the whole
    tree, its statuses, sims_done and the counters are the model's; after every re-rooting the kept subtree and its statuses,
    before it is searched; a kept proven root ends its search with no playout.  With the default chain window and with one
    playout per tick and no window (in c4_late 300 of a search's 400 playouts end on a terminal or a proven node: the chained
    path with the cached root-child statuses reruns inside most ticks)."""
    _run_sequence(key, scale_want, **SCHEDULES[sched])


# ------------------------------------------------------------------------------------------------ b. whole self-play games
def _play_games(c, nodes_per_slot=0):
    from test_solver_gpu import _engine
    E = _E()
    _, _, mc, _ = FC.geometry(c["game"])
    etas, us = FC.draws(c["seed"], c["game"], c["n_games"])
    eng = _engine(c["game"], solver=True, n_slots=c["n_games"], max_games=c["n_games"], rng="injected", start=c["start"],
                  n_playouts=c["n_playouts"], keep_search_tree=True, backup=c["backup"], nodes_per_slot=nodes_per_slot)
    try:
        eng.reset(c["n_games"])
        left = eng.max_plies - len(c["start"])                           # plies a game can still take from the start position
        eng.set_injected_rng([[row[:mc] for row in e[:left]] for e in etas], [u[:left] for u in us])
        ev = E.HostPolicyEvaluator(eng, PS.policy(c["game"]))
        obs, pri, val = eng.alloc_io()
        for _ in range(200000):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
            if eng.games_done() >= c["n_games"]:
                break
        else:
            pytest.fail("games did not finish")
        return eng.export(), eng.progress()
    finally:
        eng.close()


@pytest.mark.parametrize("small_pool", [False, True])
@pytest.mark.parametrize("key", sorted(SC.GAME_CASES))
def test_whole_games(key, small_pool, games_want):
    """Self-play from late positions with root noise, kept trees and injected draws: every move, recorded visit vector, value
    target (soft-Z and off-policy), result and the five counters are the model's.  small_pool: the pool of
    solver_cases.small_pool() - the largest kept subtree plus one search plus slack, shown to fit on the CPU - so re-rootings hand
    trees with hundreds of proven nodes to compact_jobs, and the games stay the same."""
    from test_solver_gpu import _assert_equals_model
    want, (cap, expected) = games_want
    c = SC.GAME_CASES[key]
    ex, prog = _play_games(c, nodes_per_slot=cap if small_pool else 0)
    print(key, "pool", cap if small_pool else "default", "compactions", prog["compactions"], "expected", expected)
    if small_pool:
        assert prog["compactions"] >= 1
    _assert_equals_model((ex, prog), want, c["start"], "%s, small pool %s" % (key, small_pool))


# ------------------------------------------------------------------------------------------------ c. deep lines
@pytest.mark.parametrize("sched", ["default", "one_per_tick", "three_per_tick"])
@pytest.mark.parametrize("key", sorted(SC.DEEP_CASES))
def test_whole_tree_of_a_deep_line(key, sched, deep_want):
    """One search under the line policy: proofs at depths 63..92 (bt8x8), 129 with climbs across depth 128 (bt26x2_128) and
    145..152 with a 5-level climb (bt26x2).  The whole tree and its statuses are the model's, however many playouts a tick runs -
    with one per tick the path is spilled and reloaded between ticks while a proof is about to climb it."""
    c = SC.DEEP_CASES[key]
    eng, ev, io, buf = _manual_engine(c["game"], c["n_playouts"], SC.deep_policy(c), **SCHEDULES[sched])
    try:
        _search(eng, ev, io, buf)
        _check_search(eng, buf, deep_want["plies"][0], (key, sched))
    finally:
        eng.close()


def test_a_self_play_game_along_a_deep_line(deep_game_want):
    """bt8x8's line as a kept-tree self-play game with the solver on (soft-Z, no root noise, no sampled move): move for move and
    value for value the model's - a chain-shaped tree with up to 2600 proven nodes keeps its statuses through every re-rooting."""
    from test_solver_gpu import _assert_equals_model, _engine
    E = _E()
    c, want = SC.DEEP_GAME, deep_game_want
    eng = _engine(c["game"], solver=True, n_slots=1, max_games=1, rng="injected", n_playouts=c["n_playouts"], keep_search_tree=True,
                  backup="soft-Z", use_dirichlet=False, num_probabilistic_actions=0)
    try:
        eng.reset(1)
        eng.set_injected_rng(None, [[0.0] * eng.max_plies])
        ev = E.HostPolicyEvaluator(eng, SC.deep_policy(c))
        obs, pri, val = eng.alloc_io()
        for _ in range(200000):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
            if eng.games_done() >= 1:
                break
        else:
            pytest.fail("the game did not finish")
        _assert_equals_model((eng.export(), eng.progress()), [want], [], "deep game")
    finally:
        eng.close()
