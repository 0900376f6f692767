"""The tick kernel at the playout counts the project ships and times - connect_four at 400, breakthrough 6x6 at 800 and 8x8 at
1600, on kept trees - against the C oracle, WHOLE TREE by whole tree: after every search each slot's az_engine_read_tree equals
the oracle's dump_tree (node count, parent, action and N as integers, Q and P as bit patterns).

Every other bit-exact test of the search stays below 200 playouts, so trees that are wide AND large (pool indices past 2^16,
kept roots with N up to 4211, a Cheney copy of 68 000 nodes), searches in which most playouts end on a terminal node (the
chained-playout path reruns inside a tick) and select paths 14-19 plies deep through nodes with 7-40 siblings exist only here.
test_product_scale_host.py asserts on the CPU that the cases of product_scale_cases.py reach all that.

Bar: bit-exact, through the C ABI with injected random draws.

Which copy a compaction is: on a manual_moves engine (the sequences) update_root copies with compact_subtree, one wave's
Cheney copy; in self-play (the whole games) the copies are handed to compact_jobs, the workgroup copy.  A destination index
past 2^16 is met by compact_subtree only (test_compaction_past_65536_nodes); compact_jobs copies at most 3339 nodes here.

Measured on an MI355X (pytest --durations=0, call phase, seconds; a case's oracle run is computed once and counted in the
first test that needs it): compaction_past_65536_nodes 1.63, breakthrough_trees[bt6_800] 1.30, whole_games[False] 1.21,
whole_games[True] 1.05, breakthrough_trees[bt8_1600] 1.02, connect_four_trees[c4_400] 0.59, compaction_of_a_wide_tree 0.22,
chaining_is_scheduling_only 0.12, connect_four_trees[c4_400_uct] and [c4_400_noise] below 0.1; the file about 9 in all."""
import numpy as np
import pytest
import torch

import product_scale_cases as PS

pytestmark = pytest.mark.gpu


def _E():
    from alphazero_openspiel_amd import engine
    return engine


def _assert_same_tree(got, want, where):
    assert len(got["N"]) == len(want["N"]), where
    for f in ("parent", "action", "N"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (where, f)
    for f in ("Q", "P"):                                               # bit patterns: -0.0 and NaN cannot hide
        assert np.array_equal(got[f].view(np.int64), want[f].view(np.int64)), (where, f)


def _root_row(roots, g):
    n = int(roots["n_children"][g])
    return {"N": int(roots["root_n"][g]), "Q": float(roots["root_q"][g]), "actions": roots["child_action"][g, :n].tolist(),
            "cN": roots["child_n"][g, :n].tolist(), "cQ": roots["child_q"][g, :n].tolist(), "cP": roots["child_p"][g, :n].tolist()}


def _search_all(eng, ev, io, buf):
    """advance + evaluate until the root export's header says that every slot is done."""
    obs, pri, val = io
    for _ in range(4 * eng.cfg.n_playouts + 16):
        for _ in range(4):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        eng.export_roots_device(buf)
        if int(buf[:16].view(torch.int32)[0].item()) == eng.G:
            return
    pytest.fail("searches did not finish")


def _run_sequence(key, slots=None, **sched):
    """The case's positions (or those of `slots`) in one manual_moves engine, a slot per position, compared with the oracle
    after every search -> the slots' pool index after the last one."""
    E = _E()
    c = PS.SEQUENCES[key]
    slots = list(range(len(c["positions"]))) if slots is None else slots
    want = [PS.oracle_sequence(key)[p] for p in slots]
    hist = [c["positions"][p] for p in slots]
    n = len(slots)
    eng = E.SelfPlayEngine(c["game"], n, n_playouts=c["n_playouts"], use_dirichlet=c["eta"] is not None, manual_moves=True,
                           rng="injected", max_games=n, use_puct=c["use_puct"], **sched)
    eng.set_start_positions([h[:-1] for h in hist] if c["leaf_update"] else hist)
    eng.reset(n)
    eng.set_injected_rng([[[0.0]] * len(h) + [c["eta"] or [0.0]] for h in hist], [[0.0] * (len(h) + 1) for h in hist],
                         absolute_ply=True)
    if c["leaf_update"]:
        eng.update_root([h[-1] for h in hist], keep_subtree=True)
    ev, io, buf = E.HostPolicyEvaluator(eng, PS.policy(c["game"])), eng.alloc_io(), eng.alloc_roots()
    alloc, compactions = [1] * n, 0
    need, cap = (c["n_playouts"] + 1) * eng.max_children, eng.sizes.nodes_per_slot
    for k in range(max(len(rows) for rows in want)):
        live = [g for g in range(n) if k < len(want[g])]
        if k:
            eng.update_root([want[g][k - 1]["move"] if g in live else -1 for g in range(n)], keep_subtree=True)
            for g in live:                                             # the engine's bookkeeping (reroot), on the CPU
                kept = PS.kept_tree(want[g][k - 1])
                if alloc[g] + need > cap:
                    alloc[g], compactions = len(kept["N"]), compactions + 1
                where = (key, "position", slots[g], "re-rooting", k)
                assert eng.read_slot(g)["alloc"] == alloc[g], where
                _assert_same_tree(eng.read_tree(g), kept, where)      # the kept subtree, in place or copied, before it is searched
        _search_all(eng, ev, io, buf)
        roots = eng.read_roots(buf)
        assert roots["error_flags"] == 0 and (roots["phase"] == 5).all()
        for g in live:
            w = want[g][k]
            where = (key, "position", slots[g], "search", k)
            _assert_same_tree(eng.read_tree(g), w["tree"], where)
            assert _root_row(roots, g) == eng.read_root(g) == w["root"], where
            alloc[g] += w["created"]
            assert eng.read_slot(g)["alloc"] == alloc[g], where      # the pool index grows by the nodes the search created
        prog = eng.progress()
        assert prog["error_flags"] == 0
        for f in PS.COUNTERS:
            assert prog[f] == sum(rows[min(k, len(rows) - 1)]["counters"][f] for rows in want), (key, k, f)
    assert prog["compactions"] == compactions
    eng.close()
    return alloc, compactions


@pytest.mark.parametrize("key", ["c4_400", "c4_400_noise", "c4_400_uct"])
def test_connect_four_trees_at_400_playouts(key):
    """Initial, mid-game and late positions, three searches each on kept trees; one search under a given root noise; two
    under the UCT rule (log_table read at N up to 692)."""
    _run_sequence(key)


@pytest.mark.parametrize("key", ["bt6_800", "bt8_1600"])
def test_breakthrough_trees_past_65536_nodes(key):
    """6x6 at 800 and 8x8 at 1600 playouts: the child-block arithmetic c0 + lane on pool indices past 2^16, kept roots with
    N up to 2876, playouts down to depth 17."""
    alloc, compactions = _run_sequence(key)
    print(key, "pool index after the last search, per slot", alloc)
    assert alloc[0] > 65536 and compactions == 0


def test_compaction_of_a_wide_tree():
    """8x8 at 1600 in the pool of pool_plan(): one search plus the subtree kept after the first one.  The re-rooting copies
    29 746 nodes with compact_subtree, 20-40 to a block (the copies of the other files move a few thousand nodes 7 wide, or
    a chain); the copy is compared node by node, then searched.  The pool index still passes 2^16."""
    cap, copies = PS.pool_plan("bt8_1600")
    assert len(copies) == 1 and copies[0] > 20000
    alloc, compactions = _run_sequence("bt8_1600", nodes_per_slot=cap)
    print("pool", cap, "copied", copies, "pool index after the last search", alloc)
    assert compactions == 1 and alloc[0] > 65536


def test_compaction_past_65536_nodes():
    """8x8 at 1600 from a mid-game position, three searches in the pool of pool_plan(): the second re-rooting keeps 68 733
    nodes of 73 935 and has to copy them - compact_subtree with destination indices past 2^16.  The copy is compared node by
    node with the sub-BFS of the oracle's tree, and so is the tree after the third search, which runs on it."""
    cap, copies = PS.pool_plan("bt8_1600_mid")
    assert copies and max(copies) > 65536
    alloc, compactions = _run_sequence("bt8_1600_mid", nodes_per_slot=cap)
    print("pool", cap, "copied", copies, "pool index after the last search", alloc)
    assert compactions == len(copies)


def test_chaining_is_scheduling_only():
    """The late connect_four position (107, 300 and 370 of a search's 400 playouts end on a terminal node) with the default
    chain window - already compared in test_connect_four_trees_at_400_playouts - and with one playout per tick and no window:
    both trees are the oracle's."""
    late = [PS.LATE["c4_400"]]
    _run_sequence("c4_400", late)
    _run_sequence("c4_400", late, max_sims_per_tick=1, chain_window_us=-1)


# ------------------------------------------------------------------------------------------------ whole games
@pytest.mark.parametrize("small_pool", [False, True])
def test_whole_games_at_400_playouts(small_pool):
    """Two connect_four games on two slots, kept trees, injected etas and uniforms: moves, root visit vectors, pi, value
    targets, ret0 and the five counters equal orc.play_game_self's.  small_pool: a pool of the largest kept subtree plus one
    search plus slack, sized on the CPU from the oracle's node counts - re-rootings compact, and POOL_EXHAUSTED cannot be the
    outcome.  This is a self-play engine: its copies (up to 3339 nodes, 7 children wide) are handed to compact_jobs, the
    workgroup copy of the same launch, not to compact_subtree."""
    from test_deep_lines_gpu import _assert_games
    from test_engine_parity import _run_games
    key = "game_c4_400"
    c = PS.GAMES[key]
    want = PS.oracle_games(key)
    _, us, eta_rows = PS.draws(key)
    kw = dict(n_playouts=c["n_playouts"])
    if small_pool:
        kw["nodes_per_slot"], expected = PS.small_pool(key)
    _, ex, prog = _run_games(_E(), c["game"], c["n_games"], c["n_games"], PS.policy(c["game"]), eta_rows, us, **kw)
    print(key, kw, "compactions", prog["compactions"])
    if small_pool:
        assert prog["compactions"] >= 3
        assert prog["compactions"] == expected
    else:
        assert prog["compactions"] == 0
    _assert_games(_E(), c["game"], ex, prog, want)
