"""MCTS-Solver on the device (az_engine_set_solver and its Python facade).

References, all compared with == (there are no tolerances):
  * the rules: the Python model of tests/solver_cases.py (pinned to the C oracle with the solver off, audited against a brute-force
    negamax and shown to bite on these very inputs by tests/test_solver_host.py) - same fake policy, same injected draws;
  * clearing and the ways to tick: engines against engines.
4 slots, at most 8 games, 24 playouts."""
import functools

import numpy as np
import pytest

import forced_playouts_cases as FC
import solver_cases as SC
from alphazero_openspiel_amd import games
from net_cases import drifted_net
from oracle import fakepolicy
from philox_cases import schedule
from playout_cap_cases import same_game as _same_game

pytestmark = pytest.mark.gpu

C4, B66 = SC.C4, SC.B66
S, G, N = SC.S, 4, 8
SEED = 811
AZ_E_INVALID, AZ_E_STATE = -1, -3
PH_SEARCH_DONE = 5


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _engine(name, solver=None, n_slots=G, max_games=N, start=None, cap=None, mirror=None, **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", S)
    kw.setdefault("seed", SEED)
    eng = E.SelfPlayEngine(name, n_slots, max_games=max_games, device=0, **kw)
    if start:
        eng.set_start_prefix(start)
    if solver is not None:
        eng.set_solver(solver)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if mirror is not None:
        eng.set_eval_mirror(mirror)
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
    return a["game_len"].tolist() != b["game_len"].tolist() or (a["child_visits"] != b["child_visits"]).any()


# ------------------------------------------------------------------------------------------------ 1. the engine against the model
def _run_injected(case, solver, small_pool=False, **settings):
    from alphazero_openspiel_amd import engine as E
    _, _, mc, _ = FC.geometry(case["game"])
    etas, us = FC.draws(case["seed"], case["game"], case["n_games"])
    kw = dict(case["kw"], **case["eng"])
    if small_pool:                                                       # three searches' worth of nodes: re-rooting has to compact
        kw["nodes_per_slot"] = 3 * (S + 1) * mc + 80
    eng = _engine(case["game"], solver=solver, n_slots=case["n_slots"], max_games=case["n_games"], rng="injected",
                  start=SC.case_start(case), **settings, **kw)
    try:
        eng.reset(case["n_games"])
        left = eng.max_plies - len(SC.case_start(case))                  # plies a game can still take from the start position
        eng.set_injected_rng([[row[:mc] for row in e[:left]] for e in etas], [u[:left] for u in us])
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
        return eng.export(), eng.progress()
    finally:
        eng.close()


def _run_case(case, solver, **settings):
    from alphazero_openspiel_amd import engine as E
    if case["small_pool"]:
        try:
            return _run_injected(case, solver, small_pool=True, **settings)
        except E.EngineError as err:    # a kept subtree can outgrow any fixed pool: the engine says so and does not play on -
            assert "POOL_EXHAUSTED" in str(err)  # then the case is checked with the default pool (as the fuzz test does)
    return _run_injected(case, solver, **settings)


def _assert_equals_model(got, want, start, what):
    ex, prog = got
    assert prog["error_flags"] == 0, what
    p0 = len(start)
    for i, w in enumerate(want):
        n = len(w["actions"])
        assert int(ex["game_len"][i]) == n and ex["move"][i, p0:p0 + n].tolist() == w["actions"], (what, i)
        assert float(ex["game_ret0"][i]) == w["ret0"], (what, i)
        for j, ply in enumerate(w["plies"]):
            nc = int(ex["n_children"][i, p0 + j])
            assert ex["child_action"][i, p0 + j, :nc].tolist() == ply["actions"], (what, i, j)
            assert ex["child_visits"][i, p0 + j, :nc].tolist() == ply["recorded"], (what, i, j, ply["raw"], ply["recorded"])
            assert float(ex["value"][i, p0 + j]) == ply["value"], (what, i, j, ply["status"])
    for key in SC.COUNTERS:
        assert prog[key] == sum(w["counters"][key] for w in want), (what, key)


@pytest.mark.parametrize("solver", [True, False])
@pytest.mark.parametrize("idx", range(len(SC.CASES)))
def test_engine_equals_the_model(idx, solver):
    """Every move, recorded visit vector, value target, result and counter; kept and fresh trees, refill, a three-searches pool
    (compaction), max_sims_per_tick 1 / 3 without a chain window, all four value targets.  solver=False: set, then cleared - the
    plain engine, which the model without the solver is."""
    case = SC.CASES[idx]
    want = SC.model_games(idx, solver=solver)
    _assert_equals_model(_run_case(case, solver), want, SC.case_start(case), "case %d, solver %s" % (idx, solver))


@pytest.mark.parametrize("idx", [0, 1, 4])
def test_with_a_playout_cap_and_eval_mirror_the_engine_equals_the_model(idx):
    """Solver + playout cap (6, 0.5) + eval mirror p = 0.5.  The model takes the schedule from the Python Philox model of the cap's
    draw (tests/philox_cases.py) and the orientation of every request from the coin model of tests/eval_mirror_cases.py;
    the coin's index is the count of playouts the search has run, from 0 in a fast search too, and a search that ends early at a
    proven root - a fast one included - ends on that count.  Kept trees (cases 0 and 4), fresh ones (case 1), both games."""
    import eval_mirror_cases as EM
    from mirror_cases import action_mirror_table
    case = SC.CASES[idx]
    n, p0 = case["n_games"], len(SC.case_start(case))
    _, mp, _, _ = FC.geometry(case["game"])
    sched = schedule(SEED, n, mp, 0.5)                                   # by game id and ABSOLUTE ply
    per_game = [[(S if sched[i, p0 + t] else SC.S_FAST, bool(sched[i, p0 + t])) for t in range(mp - p0)] for i in range(n)]
    table = action_mirror_table(games.load_game(case["game"]))
    mirrors = [((lambda ply, phase, sims, i=i: EM.coin(SEED, i, ply, phase, sims, 0.5)), table) for i in range(n)]
    want = SC.model_games(idx, solver=True, schedules=per_game, mirrors=mirrors)
    plies = [ply for w in want for ply in w["plies"]]
    assert {ply["full"] for ply in plies} == {True, False}
    assert any(not ply["full"] and ply["status"] != SC.UNKNOWN and ply["ran"] < SC.S_FAST for ply in plies)   # a fast search cut short
    assert any(ply["full"] and ply["status"] != SC.UNKNOWN and ply["ran"] < S for ply in plies)               # ... and a full one
    assert any(ply["raw"] != ply["recorded"] for ply in plies)
    assert min(sum(w["mirrored"][k] for w in want) for k in (0, 1)) >= 10                                      # both orientations
    unmirrored = SC.model_games(idx, solver=True, schedules=per_game)
    assert [w["actions"] for w in want] != [w["actions"] for w in unmirrored] or \
        [ply["raw"] for ply in plies] != [ply["raw"] for w in unmirrored for ply in w["plies"]]                # the coin matters here
    got = _run_case(case, True, cap=(SC.S_FAST, 0.5), mirror=0.5)
    _assert_equals_model(got, want, SC.case_start(case), "case %d: solver + cap + mirror" % idx)


# ------------------------------------------------------------------------------------------------ 2. clearing
@pytest.mark.parametrize("name", [C4, B66])
def test_never_set_and_a_cleared_setting_are_the_plain_engine(name):
    kw = dict(keep_search_tree=True, use_dirichlet=True)
    ev = _fused(name)
    plain = _engine(name, **kw)
    want, prog_plain = _play(plain, ev)
    assert not plain.read_proofs(0).any()                                # a plain engine never writes the status word
    plain.close()
    eng = _engine(name, solver=True, **kw)
    assert eng.solver is True
    solved, prog = _play(eng, ev)                                        # a generation under the setting, then the same engine without
    assert _differ(solved, want) and prog["sims"] < prog_plain["sims"]
    eng.set_solver(False)
    assert eng.solver is False
    got, prog = _play(eng, ev)
    eng.close()
    ev.close()
    _same_games(got, want, "set, then cleared")
    assert prog["sims"] == prog_plain["sims"] and prog["evals"] == prog_plain["evals"]


# ------------------------------------------------------------------------------------------------ 3. scheduling invariance
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
    eng = _engine(C4, solver=True, **kw)
    want, prog = _play(eng, ev)
    eng.close()
    eng = _engine(C4, solver=True, **kw)
    got, p = _play(eng, ev, use_graph=True, ticks_per_graph=16, check_every=32)
    eng.close()
    _same_games(got, want, "a 16-tick captured graph")
    assert p["sims"] == prog["sims"]
    eng = _engine(C4, solver=True, **kw)
    got, p = _play_with_tail(eng, ev)
    eng.close()
    _same_games(got, want, "dense rows in the tail")
    assert p["sims"] == prog["sims"]
    eng = _engine(C4, max_games=N // 2, **kw)                            # a ring of 4 rows: 8 games wrap it
    stream = E.SelfPlayStream(eng, ev, seed=SEED, use_graph=False, solver=True)
    try:
        assert eng.solver is True
        for first_want in (0, N // 2):
            buf, first = stream.take(N // 2, max_ticks=200000)
            assert first == first_want
            got = E.unpack_device_export(buf.cpu().numpy(), N // 2, eng.max_plies, eng.max_children)
            for j in range(N // 2):
                _same_game(got, j, want, first + j, 0, "a stream: game %d" % (first + j))
    finally:
        stream.close()
        E.close_all(eng, ev)


# ------------------------------------------------------------------------------------------------ 4. analysis: proofs read back
def _search_manual(eng, ev_fn, max_ticks=4 * S + 64):
    from alphazero_openspiel_amd import engine as E
    ev = E.HostPolicyEvaluator(eng, ev_fn)
    obs, pri, val = eng.alloc_io()
    for tick in range(max_ticks):
        if eng.read_slot(0)["phase"] == PH_SEARCH_DONE:
            return tick
        eng.advance(pri, val, obs)
        ev(obs, pri, val)
    pytest.fail("the search did not finish")


@pytest.mark.parametrize("idx", [0])
def test_read_proofs_equals_the_models_tree_and_a_proven_root_ends_the_search(idx):
    """A manual_moves engine on the start position of a late connect_four case (lost for the side to move): the whole tree's statuses against the model's,
    PH_SEARCH_DONE before n_playouts, export_proofs_device == read_proofs at the root, and a search armed again at the proven
    root returns at once."""
    from alphazero_openspiel_amd import _lib
    case = SC.CASES[idx]
    start, salt = SC.case_start(case), case["salt"]
    trees = []
    w = SC.play_game(case["game"], salt, None, [0.5] * 42, solver=True, n_playouts=4 * S, start=start, use_dirichlet=False,
                     keep_search_tree=True, backup="soft-Z", trees=trees)
    first = w["plies"][0]
    assert first["status"] != SC.UNKNOWN and first["ran"] < 4 * S       # the model proves this root before the playouts run out
    eng = _engine(case["game"], solver=True, n_slots=1, max_games=1, manual_moves=True, use_dirichlet=False, n_playouts=4 * S)
    try:
        eng.set_start_positions([start])
        eng.reset(1)
        A = eng.A
        fn = lambda b: fakepolicy.fake_eval(b, A, salt)
        _search_manual(eng, fn)
        slot = eng.read_slot(0)
        assert slot["phase"] == PH_SEARCH_DONE and slot["sims_done"] == first["ran"] < 4 * S
        # (the model's later searches grew nothing below the first root: every one of them ended at a proven root)
        statuses, counts = SC.tree_statuses(trees[0])
        tree, proofs = eng.read_tree(0), eng.read_proofs(0)
        assert tree["N"].tolist() == counts and proofs.tolist() == statuses
        root = eng.read_root(0)
        dev = eng.export_proofs_device().cpu().numpy()
        assert dev.shape == (1, 1 + eng.max_children)
        nc = len(root["actions"])
        kids = [i for i, p in enumerate(tree["parent"].tolist()) if p == 0]
        assert dev[0, 0] == proofs[0] == first["status"] and dev[0, 1:1 + nc].tolist() == proofs[kids].tolist()
        assert not dev[0, 1 + nc:].any()
        # what Analyzer.results() adds with solver=True: the values for the side to move, by action
        from alphazero_openspiel_amd import analysis
        dense = analysis.dense_proofs(dev, eng.read_roots(), 1, A)
        assert dense["solved"][0] == -SC.VALUE[first["status"]]
        want_children = {a: c.status for a, c in zip(trees[0].actions, trees[0].children)}
        for a in range(A):
            st = want_children.get(a, SC.UNKNOWN)
            assert dense["solved_children"][0, a] == (analysis.SOLVED_UNKNOWN if st == SC.UNKNOWN else SC.VALUE[st]), a
        progress = eng.progress()
        eng.update_root([_lib.ACTION_SEARCH_AGAIN])
        assert _search_manual(eng, fn) <= 2                              # armed, found proven, done
        assert eng.read_slot(0)["sims_done"] == 0 and eng.progress()["sims"] == progress["sims"]
    finally:
        eng.close()


MATE_IN_ONE = [3, 0, 3, 0, 3, 0]          # connect_four: three in column 3 for the side to move (and three in column 0 against it)
OPEN = [3]                               # nothing is proven here in 96 playouts


def _model_search(start, salt, n_playouts):
    """The model's first search from `start` without root noise -> (its ply record, the root Node)."""
    trees = []
    w = SC.play_game(C4, salt, None, [0.5] * 42, solver=True, n_playouts=n_playouts, start=start, use_dirichlet=False,
                     keep_search_tree=True, backup="soft-Z", trees=trees)
    return w["plies"][0], trees[0]


def test_analysis_reports_a_mate_in_one_a_lost_position_and_an_open_one():
    """analyze_positions(solver=True) -> Analyzer.results(): solved and solved_children of three positions searched side by side,
    against the model's statuses, the rules of the game and the brute-force negamax; every search of a proven root ends early."""
    import types
    from alphazero_openspiel_amd import analysis
    from alphazero_openspiel_amd import engine as E
    from oracle import binding as orc
    case = SC.CASES[0]
    lost, salt, A, n_playouts = SC.case_start(case), case["salt"], 7, 4 * S
    positions = [MATE_IN_ONE, lost, OPEN]
    model = [_model_search(h, salt, n_playouts) for h in positions]
    (mate, mate_root), (lose, _), (open_, _) = model
    # what the model says is what the game says: a won root with the winning move proven, a lost root, an open one
    assert mate["status"] == SC.LOSS and lose["status"] == SC.WIN and open_["status"] == SC.UNKNOWN
    assert mate_root.children[mate_root.actions.index(3)].status == SC.WIN
    for h, want in ((MATE_IN_ONE, 1.0), (lost, -1.0)):
        s = orc.State(C4)
        for a in h:
            s.apply_action(a)
        assert SC.solved_value(s) == want
    assert mate["ran"] < n_playouts and lose["ran"] < n_playouts and open_["ran"] == n_playouts
    ev = E.HostPolicyEvaluator(types.SimpleNamespace(A=A), lambda b: fakepolicy.fake_eval(b, A, salt))
    res = analysis.analyze_positions(ev, C4, positions, n_playouts=n_playouts, solver=True, seed=SEED)
    assert res["progress"]["error_flags"] == 0
    assert res["solved"].tolist() == [1, -1, None]
    assert res["solved_children"].dtype == np.int8 and res["solved_children"].shape == (3, A)
    for i, (ply, root) in enumerate(model):
        want = [analysis.SOLVED_UNKNOWN] * A
        for a, c in zip(root.actions, root.children):
            want[a] = analysis.SOLVED_UNKNOWN if c.status == SC.UNKNOWN else int(SC.VALUE[c.status])
        assert res["solved_children"][i].tolist() == want, i
        assert res["visits"][i, root.actions].tolist() == ply["raw"] and int(res["root_n"][i]) == root.N, i
    assert res["solved_children"][0, 3] == 1                             # the mate is there to be played
    assert (res["solved_children"][1, res["visits"][1] > 0] == -1).all() # every move of the lost position loses
    assert (res["solved_children"][2] == analysis.SOLVED_UNKNOWN).all()
    assert res["progress"]["sims"] == sum(ply["ran"] for ply, _ in model) < 3 * n_playouts
    plain = analysis.analyze_positions(ev, C4, positions, n_playouts=n_playouts, seed=SEED)
    assert "solved" not in plain and "solved_children" not in plain and plain["progress"]["sims"] == 3 * n_playouts


def test_analyzer_reports_the_mate_of_either_side_and_searching_on_returns_at_once():
    """Analyzer(solver=True).results() on a 2-slot engine: MATE_IN_ONE and the same position a move later, where the other side has
    a mate of its own; search_again at the proven roots runs no playout."""
    from alphazero_openspiel_amd import analysis
    from alphazero_openspiel_amd import engine as E
    salt, n_playouts = 11, 4 * S
    positions = [MATE_IN_ONE, MATE_IN_ONE + [6]]
    model = [_model_search(h, salt, n_playouts) for h in positions]
    assert [ply["status"] for ply, _ in model] == [SC.LOSS, SC.LOSS] and all(ply["ran"] < n_playouts for ply, _ in model)
    an = analysis.Analyzer(None, C4, 2, n_playouts=n_playouts, solver=True, seed=SEED)
    try:
        assert an.solver is True and an.engine.solver is True
        an.evaluator = E.HostPolicyEvaluator(an.engine, lambda b: fakepolicy.fake_eval(b, 7, salt))
        an.load(positions)
        an.search()
        res = an.results()
        assert res["phase"].tolist() == [PH_SEARCH_DONE] * 2
        assert res["solved"].tolist() == [1, 1] and res["solved_children"][0, 3] == 1 and res["solved_children"][1, 0] == 1
        assert res["root_n"].tolist() == [root.N for _, root in model] and int(res["root_n"].max()) < n_playouts
        for i, (ply, root) in enumerate(model):
            assert res["visits"][i, root.actions].tolist() == ply["raw"], i
        sims, ticks = an.engine.progress()["sims"], an.ticks
        assert sims == sum(ply["ran"] for ply, _ in model)
        an.search_again()
        an.search()
        again = an.results()
        assert again["solved"].tolist() == [1, 1] and an.engine.progress()["sims"] == sims
        assert an.ticks - ticks <= an.check_every
        assert again["visits"].tolist() == res["visits"].tolist()
    finally:
        an.close()


def test_reanalyser_takes_the_setting():
    """Reanalyser(solver=True): the searches of stored positions end at proven roots (fewer playouts than without the setting,
    on a store of whole random games: their last positions are mates in one), every refreshed pi is a distribution."""
    import replay_cases as RC
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd import replay as R
    game = games.load_game(C4)
    ex = RC.fake_export(game, n_games=4, seed=3)
    sims, targets = [], []
    for solver in (False, True):
        rep = R.DeviceReplay(C4, max_games=4, device=0)
        rep.append_export(ex)
        U = rep.dedupe()
        re = R.Reanalyser(rep, None, U, 4 * S, value_target="soft-Z", solver=solver)
        try:
            assert re.analyzer.solver is solver and re.analyzer.engine.solver is solver
            re.analyzer.evaluator = E.HostPolicyEvaluator(re.analyzer.engine, lambda b: fakepolicy.fake_eval(b, 7, 9))
            assert re.reanalyse() == U
            p = re.analyzer.engine.progress()
            assert p["error_flags"] == 0 and rep.stats()["fault_flags"] == 0
            sims.append(p["sims"])
            n = rep.stats()["n_examples"]
            targets.append(np.array([rep.read_example(i)[0] for i in range(n)]))
        finally:
            re.close()
            rep.close()
    assert sims[0] == U * 4 * S and sims[1] < sims[0]
    assert (np.abs(targets[1].sum(axis=1) - 1.0) <= 7 * 2.0 ** -52).all()   # 7 quotients n / total, each rounded once
    assert (targets[1] != targets[0]).any()


# ------------------------------------------------------------------------------------------------ 5. refusals and the facade
def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    for what, eng in (("arena", _engine(C4, arena_agent="zero", opponent="random")), ("AZ_SELECT_UCT", _engine(C4, use_puct=False))):
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_solver is for PUCT self-play and manual_moves.*%s" % (AZ_E_INVALID, what)):
            eng.set_solver(True)
        assert eng.solver is False
        eng.close()
    eng = _engine(C4)
    eng.set_forced_playouts(2.0)
    with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_solver.*forced" % AZ_E_INVALID):
        eng.set_solver(True)
    eng.set_forced_playouts(0.0)
    eng.set_solver(True)
    with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_forced_playouts.*az_engine_set_solver" % AZ_E_INVALID):
        eng.set_forced_playouts(2.0)
    obs, pri, val = eng.alloc_io()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):     # the caller starts a generation after the call
        eng.advance(pri, val, obs)
    eng.set_playout_cap(6, 0.5)                                          # composes with a cap and the mirror
    eng.set_eval_mirror(0.5)
    eng.reset(4)
    eng.advance(pri, val, obs)
    eng.close()
    man = _engine(C4, manual_moves=True)
    man.set_solver(True)                                                 # analysis and reanalyse engines take it
    man.close()


def _flat(games_):
    return [(r[0], r[2], r[3]) for g in games_ for r in g]


def test_example_generator_passes_the_setting_to_its_engines():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    kw = dict(n_playouts=S, n_slots=G, seed=5, use_graph=False)
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", solver=True, **kw)
    out = gen.generate_examples(N)
    gen.close()
    eng = _engine(C4, solver=True, seed=5)                               # the generator's first generation
    ev = _fused(C4)
    ex, _ = _play(eng, ev)
    eng.close()
    ev.close()
    assert _flat(out) == _flat(E.examples_from_export(eng.game, ex))
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", solver=True, continuous=True, **kw)
    got = gen.generate_examples(N)
    gen.close()
    assert gen.last_progress["error_flags"] == 0 and _flat(got) == _flat(out)
