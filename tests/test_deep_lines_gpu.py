"""The tick kernel on select paths deeper than 64 and 128 plies, against the C oracle (which tests/golden/mcts_trace_deep.json
pins to the reference at these depths).

az_advance_kernel keeps a playout's path in lanes and registers: depth d sits in lane d & 63 of register d >> 6 (one register
for connect_four, three for breakthrough).  Under oracle/fakepolicy.fake_eval no playout gets past depth 16, so nothing that
depends on d >= 64 - Path::set, backup_path's sign across a register boundary, the spill and reload of the path between
ticks, the 16-bit depth beside the leaf's action, chained playouts, greedy_line, the line export, the Cheney copy of a
chain-shaped tree - runs in any other bit-exact test.  The line policy of deep_line_cases.py takes every case's search down to
depth 42 / 67 / 100 / 148 (test_deep_lines_host.py asserts that on the CPU).

Bar: bit-exact, through the C ABI with injected random draws.  Integers and IEEE doubles are compared with ==."""
import numpy as np
import pytest
import torch

import deep_line_cases as DL
import lines_cases as LC
from conftest import load_golden
from oracle import binding as orc

pytestmark = pytest.mark.gpu

KEYS = sorted(DL.CASES)
BT8 = DL.CASES["bt8x8"]["game"]
COUNTERS = ("sims", "evals", "sum_depth", "terminal_hits", "sum_children")


def _E():
    from alphazero_openspiel_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ the one search of a case
_ORACLE = {}


def _oracle(key, use_puct):
    """(root statistics after the search, the five counters, the descent [(action, root statistics)]): computed once."""
    if (key, use_puct) not in _ORACLE:
        m, _, depths, _ = DL.oracle_search(key, use_puct)
        _ORACLE[key, use_puct] = (m.root_stats(), m.counters(), DL.oracle_descent(m), max(depths))
    return _ORACLE[key, use_puct]


def _run_search(E, eng, ev, io):
    obs, pri, val = io
    for _ in range(4 * eng.cfg.n_playouts + 8):
        eng.advance(pri, val, obs)
        ph = eng.read_slot(0)["phase"]
        if ph == 5:
            return
        if ph in (3, 4):
            ev(obs, pri, val)
    pytest.fail("search did not finish")


def _searched_engine(key, use_puct=True):
    E = _E()
    c = DL.CASES[key]
    eng = E.SelfPlayEngine(c["game"], 1, n_playouts=c["n_playouts"], use_dirichlet=c["eta"] is not None, manual_moves=True,
                           rng="injected", max_games=1, use_puct=use_puct)
    eng.reset(1)
    eng.set_injected_rng([[c["eta"] or [0.0]]], [[0.0]])
    ev, io = E.HostPolicyEvaluator(eng, DL.case_policy(key)), eng.alloc_io()
    _run_search(E, eng, ev, io)
    return eng, ev, io


# ------------------------------------------------------------------------------------------------ 1. every node of a deep line
@pytest.mark.parametrize("use_puct", [True, False])
@pytest.mark.parametrize("key", KEYS)
def test_every_node_of_a_deep_line(key, use_puct):
    """One search, then update_root(keep_subtree) down the most visited line: N, actions, child N / Q / P of every node on it
    equal the oracle's after the same update_root - a wrong sign or a lost visit 70 or 140 plies down never reaches the root
    of the search, but it is the root here.  (use_puct=False changes nothing in a tree that descends from a constructor
    root, mcts.py:122 - in the oracle and in the engine alike.)"""
    root, counters, descent, deepest = _oracle(key, use_puct)
    eng, _, _ = _searched_engine(key, use_puct)
    assert eng.read_root(0) == root
    prog = eng.progress()
    assert prog["error_flags"] == 0
    assert {k: prog[k] for k in COUNTERS} == counters
    golden = {c["key"]: c for c in load_golden("mcts_trace_deep.json")}.get(key)
    if golden:
        assert root == golden["trace"][str(DL.CASES[key]["n_playouts"])]
    steps = {d["depth"]: d for d in golden["descent"]} if golden else {}
    for depth, (a, want) in enumerate(descent, 1):
        assert DL.most_visited(eng.read_root(0)) == a, depth
        eng.update_root([a], keep_subtree=True)
        got = eng.read_root(0)
        assert got == want, "depth %d" % depth
        if depth in steps:
            assert a == steps[depth]["action"] and got == steps[depth]["root"], "depth %d" % depth
    assert not eng.read_root(0)["actions"] and eng.read_root(0)["N"] > 0   # the visited leaf the line ends in
    assert not golden or len(descent) == max(steps)
    print(key, "use_puct", use_puct, "deepest playout", deepest, "nodes compared", len(descent))
    eng.close()


def test_searching_again_below_a_deep_kept_tree():
    """26x2, three moves: search, move, search again on the kept subtree - from the second search on the first playout already
    runs 140 plies down the kept chain, and terminal hits chain inside one tick."""
    key = "bt26x2"
    c = DL.CASES[key]
    eng, ev, io = _searched_engine(key)
    m, s, _, _ = DL.oracle_search(key)
    orc.max_depth()
    for move in range(3):
        a = DL.most_visited(m.root_stats())
        m.update_root(a)
        s.apply_action(a)
        eng.update_root([a], keep_subtree=True)
        assert eng.read_root(0) == m.root_stats()
        for _ in range(c["n_playouts"]):
            m.playout(s)
        _run_search(_E(), eng, ev, io)
        assert eng.read_root(0) == m.root_stats(), move
        assert eng.read_root(0)["N"] > c["n_playouts"]                 # a kept root: its earlier visits stay
    assert orc.max_depth() >= 128
    prog = eng.progress()
    assert prog["error_flags"] == 0 and {k: prog[k] for k in COUNTERS} == m.counters()
    for depth, (a, want) in enumerate(DL.oracle_descent(m), 1):
        eng.update_root([a], keep_subtree=True)
        assert eng.read_root(0) == want, depth
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. line export
@pytest.mark.parametrize("key", ["bt26x2", "bt8x8"])
def test_line_export_of_a_deep_search(key):
    """az_engine_export_lines_device at the largest depth it accepts, and at 64 and 65: steps, full length and the A0GB value
    equal lines_cases.walk_tree on the tree read back."""
    E = _E()
    eng, _, _ = _searched_engine(key)
    tree = eng.read_tree(0)
    line, _, _ = LC.walk_tree(tree)
    assert len(line) >= 66                                             # (past lane 63 of the first path register)
    for D in (eng.max_plies, 64, 65):
        lines = E.read_lines(eng.export_lines_device(D))
        assert (lines["n_finished"], lines["max_depth"], lines["error_flags"]) == (1, D, 0)
        LC.assert_slot_equals_walk(lines, 0, tree, D)
    with pytest.raises(E.EngineError):
        eng.export_lines_device(eng.max_plies + 1)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. whole games on kept trees
def _draws(game, n_games, seed):
    gid, rows, cols = orc.parse_game(game)
    mp = orc.max_plies(gid, rows, cols)
    rng = np.random.RandomState(seed)
    etas = [[rng.dirichlet(0.3 * np.ones(3 * rows * cols)).tolist() for _ in range(mp)] for _ in range(n_games)]
    us = [rng.random_sample(mp).tolist() for _ in range(n_games)]
    mc = min(64, 6 * cols) if gid else 7
    return etas, us, [[row[:mc] for row in e] for e in etas]


def _assert_games(E, game, ex, prog, want):
    from alphazero_openspiel_amd import games as G
    games = E.examples_from_export(G.load_game(game) if isinstance(game, str) else game, ex)
    assert prog["error_flags"] == 0
    for i, w in enumerate(want):
        n = len(w["actions"])
        assert int(ex["game_len"][i]) == n, i
        assert ex["move"][i, :n].tolist() == w["actions"], i
        assert float(ex["game_ret0"][i]) == w["ret0"]
        for j in range(n):
            nc = int(ex["n_children"][i, j])
            assert ex["child_visits"][i, j, :nc].tolist() == w["root_cN"][j], (i, j)
            assert games[i][j][2] == w["examples"][j][2], (i, j)
            assert games[i][j][3] == w["examples"][j][3], (i, j)
            assert (games[i][j][1] == w["examples"][j][1]).all()
    for k in COUNTERS:
        assert prog[k] == sum(w["counters"][k] for w in want), k


@pytest.mark.parametrize("use_dirichlet", [False, True])
@pytest.mark.parametrize("backup", ["on-policy", "soft-Z", "A0C", "off-policy"])
@pytest.mark.parametrize("key", ["bt8x8", "c4"])
def test_whole_game_on_kept_trees(key, backup, use_dirichlet):
    """Self-play with keep_search_tree under the line policy: moves, root visit vectors, pi, value targets (off-policy is
    greedy_line on a line 40-67 plies long), the return and the five counters equal the oracle's."""
    from test_engine_parity import _run_games
    E = _E()
    c = DL.CASES[key]
    etas, us, eta_rows = _draws(c["game"], 1, 77)
    kw = dict(n_playouts=c["n_playouts"], keep_search_tree=True, backup=backup, use_dirichlet=use_dirichlet)
    orc.max_depth()
    want = orc.play_game_self(DL.case_policy(key), c["game"], etas=etas[0] if use_dirichlet else None, us=us[0], **kw)
    deepest = orc.max_depth()
    print(key, backup, use_dirichlet, "moves", len(want["actions"]), "deepest playout", deepest, want["counters"])
    assert deepest >= (64 if key == "bt8x8" else 41) and want["counters"]["terminal_hits"] > 0
    _, ex, prog = _run_games(E, c["game"], 1, 1, DL.case_policy(key), eta_rows if use_dirichlet else None, us, **kw)
    _assert_games(E, c["game"], ex, prog, [want])


# ------------------------------------------------------------------------------------------------ 4. compaction of a chain
def _kept_sizes(pol, game, S, etas, want):
    """The oracle's game again, search by search: (nodes created by each search, nodes alive after each update_root)."""
    L = orc.lib()
    base = L.orc_nodes_alive()
    m = orc.MCTS(pol, game, n_playouts=S, use_dirichlet=True)
    s = orc.State(game)
    created, kept = [], []
    for j, a in enumerate(want["actions"]):
        t0 = L.orc_nodes_total()
        m.search(s, etas[j])
        assert [n for n in m.root_stats()["cN"]] == want["root_cN"][j]
        created.append(L.orc_nodes_total() - t0)
        s.apply_action(a)
        m.update_root(a)
        kept.append(L.orc_nodes_alive() - base)
    return created, kept


def test_compaction_of_a_chain_shaped_tree():
    """A pool just large enough for the largest kept subtree plus one search: every re-rooting that cannot go on in place
    copies a tree that is one long chain (a Cheney step per node) - and the game stays the oracle's.  The pool is sized on the
    CPU from the oracle's own node counts, so POOL_EXHAUSTED cannot be the outcome."""
    from test_engine_parity import _run_games
    E = _E()
    key = "bt8x8"
    c, S = DL.CASES[key], DL.CASES[key]["n_playouts"]
    etas, us, eta_rows = _draws(c["game"], 1, 78)
    want = orc.play_game_self(DL.case_policy(key), c["game"], n_playouts=S, etas=etas[0], us=us[0])
    created, kept = _kept_sizes(DL.case_policy(key), c["game"], S, etas[0], want)
    need = (S + 1) * 48                                                # (n_playouts + 1) * max_children: a search's room
    cap = need + max(kept) + 64
    alloc, compactions = 1, 0
    for new, k in zip(created[:-1], kept[:-1]):                        # the engine's bookkeeping (reroot), on the CPU
        alloc += new
        if alloc + need > cap:
            alloc, compactions = k, compactions + 1
            assert alloc + need <= cap
    print("pool", cap, "largest kept subtree", max(kept), "compactions expected", compactions)
    assert compactions > 0 and max(kept) > 1000
    _, ex, prog = _run_games(E, c["game"], 1, 1, DL.case_policy(key), eta_rows, us, n_playouts=S, nodes_per_slot=cap)
    assert prog["compactions"] == compactions
    _assert_games(E, c["game"], ex, prog, [want])


# ------------------------------------------------------------------------------------------------ 3. neighbouring slots
N_MIXED, DEEP_GAMES = 5, (1, 3)
_MIXED = {}


def _mixed_policies():
    deep, flat = DL.case_policy("bt8x8"), DL.policy(BT8, DL.SHORT_SALT, 1.0, L=0)
    return [deep if g in DEEP_GAMES else flat for g in range(N_MIXED)]


def _mixed_oracle():
    if "want" not in _MIXED:
        etas, us, eta_rows = _draws(BT8, N_MIXED, 79)
        want, deepest = [], []
        for g, pol in enumerate(_mixed_policies()):
            orc.max_depth()
            want.append(orc.play_game_self(pol, BT8, n_playouts=DL.CASES["bt8x8"]["n_playouts"], etas=etas[g], us=us[g]))
            deepest.append(orc.max_depth())
        _MIXED["want"] = (want, deepest, eta_rows, us)
    return _MIXED["want"]


def _play_mixed(mode):
    """3 slots, 5 games of breakthrough 8x8; games 1 and 3 under the line policy, the others under the flat one: the evaluator
    looks up whose game a row's request belongs to.  mode: "plain", "rows" (the thinned-out tail on dense rows), or the
    max_sims_per_tick of a run without a chain window."""
    if mode in _MIXED:
        return _MIXED[mode]
    E = _E()
    _, _, eta_rows, us = _mixed_oracle()
    pols = _mixed_policies()
    kw = {} if mode in ("plain", "rows") else dict(max_sims_per_tick=int(mode), chain_window_us=-1)
    G = 3
    eng = E.SelfPlayEngine(BT8, G, rng="injected", max_games=N_MIXED, n_playouts=DL.CASES["bt8x8"]["n_playouts"], **kw)
    eng.reset(N_MIXED)
    eng.set_injected_rng(eta_rows, us)
    obs, pri, val = eng.alloc_io()
    rbuf = eng.alloc_roots()
    rows, slots, switched_at = None, list(range(G)), 0
    hp = np.empty((G, eng.A), dtype=np.float32)
    hv = np.empty((G,), dtype=np.float32)
    for _ in range(200000):
        if rows is None:
            eng.advance(pri, val, obs)
        else:
            eng.advance_rows(rows, pri, val, obs)
        r = eng.read_roots(rbuf)
        n = len(slots)
        boards = obs[:n].cpu().numpy().astype(np.float64)
        for i, g in enumerate(slots):
            if r["phase"][g] in (3, 4):                                # the slot waits for an evaluation: of ITS game's policy
                hp[i], hv[i] = pols[int(r["game_id"][g])](boards[i])
        pri[:n].copy_(torch.from_numpy(hp[:n]))
        val[:n].copy_(torch.from_numpy(hv[:n]))
        done = eng.games_done()
        if done >= N_MIXED:
            break
        if mode == "rows" and done >= 3 and done > switched_at:        # every game is handed out and a slot has gone idle
            switched_at = done
            slots = [g for g in range(G) if r["phase"][g] != 0]
            rows = eng.compact_rows()
            assert rows == len(slots) == N_MIXED - done
    else:
        pytest.fail("games did not finish")
    prog, ex = eng.progress(), eng.export()
    eng.close()
    assert mode != "rows" or switched_at >= 3
    _MIXED[mode] = (ex, prog)
    return ex, prog


@pytest.mark.parametrize("mode", ["plain", "rows", "1", "3"])
def test_deep_and_shallow_paths_in_neighbouring_slots(mode):
    """Deep and shallow select paths in one launch and in adjacent rows of the path buffer: every game equals the oracle's game
    of the same id, whichever slot or dense row played it and however many playouts a tick chains."""
    from test_tail_rows_gpu import _same
    want, deepest, _, _ = _mixed_oracle()
    print("deepest playout per game", deepest)
    assert all((d >= 64) == (g in DEEP_GAMES) for g, d in enumerate(deepest)) and max(deepest[g] for g in (0, 2, 4)) < 32
    ex, prog = _play_mixed(mode)
    _assert_games(_E(), BT8, ex, prog, want)
    _same(_play_mixed("plain")[0], ex)


# ------------------------------------------------------------------------------------------------ 6. the limit
def test_largest_accepted_and_smallest_refused_boards():
    """A select path holds 192 depths: 12x5 (max_plies 191) and 26x2 (189) are created; the smallest boards beyond - 27x2
    (197), 19x3 (199), 15x4 (201), which pass every other create-time rule - are refused with the path's message."""
    E = _E()
    for game, mp in (("breakthrough(rows=12,columns=5)", 191), ("breakthrough(rows=26,columns=2)", 189)):
        eng = E.SelfPlayEngine(game, 1, n_playouts=4)
        assert eng.max_plies == mp == orc.max_plies(*orc.parse_game(game))
        eng.close()
    for game, mp in (("breakthrough(rows=27,columns=2)", 197), ("breakthrough(rows=19,columns=3)", 199),
                     ("breakthrough(rows=15,columns=4)", 201)):
        assert orc.max_plies(*orc.parse_game(game)) == mp >= 193
        with pytest.raises(E.EngineError, match="a game may last %d plies, the select path holds 191" % mp):
            E.SelfPlayEngine(game, 1, n_playouts=4)
