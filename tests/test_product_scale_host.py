"""What keeps test_product_scale_gpu.py from passing vacuously, asserted with the C oracle alone (no GPU): MCTS.dump_tree - the
expected result of every comparison there - agrees with the read-backs that are already pinned (root_stats, the counters,
update_root), and the cases of product_scale_cases.py reach what they are for: pool indices past 2^16, kept roots with
N >= 2500, searches full of terminal hits, playouts 14 and more plies deep in trees 7-40 children wide."""
import numpy as np
import pytest

import product_scale_cases as PS
from oracle import binding as orc

KEYS = sorted(PS.SEQUENCES)
TREE_FIELDS = ("parent", "action", "N", "Q", "P")


def _children_sum(tree):
    """(sum of the children's N, number of children) of every row."""
    tot, cnt = np.zeros(len(tree["N"]), dtype=np.int64), np.zeros(len(tree["N"]), dtype=np.int64)
    np.add.at(tot, tree["parent"][1:], tree["N"][1:])
    np.add.at(cnt, tree["parent"][1:], 1)
    return tot, cnt


def _same_tree(a, b):
    for f in TREE_FIELDS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("key", KEYS)
def test_dump_tree_agrees_with_the_pinned_read_backs(key):
    c = PS.SEQUENCES[key]
    for p, rows in enumerate(PS.oracle_sequence(key)):
        prev, prev_counters = None, dict.fromkeys(PS.COUNTERS, 0)
        for k, r in enumerate(rows):
            tree, root = r["tree"], r["root"]
            n = len(tree["N"])
            assert [tree[f].dtype for f in TREE_FIELDS] == [np.int32, np.int32, np.int64, np.float64, np.float64]
            assert all(len(tree[f]) == n for f in TREE_FIELDS)
            # breadth-first, children consecutive and in ascending-action order
            assert tree["parent"][0] == -1 and tree["action"][0] == -1
            assert (np.diff(tree["parent"][1:]) >= 0).all() and (tree["parent"][1:] < np.arange(1, n)).all()
            same_parent = np.diff(tree["parent"][1:]) == 0
            assert (np.diff(tree["action"][1:])[same_parent] > 0).all()
            # row 0 and the first level are root_stats()
            nc = len(root["actions"])
            assert (int(tree["N"][0]), float(tree["Q"][0])) == (root["N"], root["Q"])
            assert (tree["parent"][1:1 + nc] == 0).all() and int((tree["parent"] == 0).sum()) == nc
            assert tree["action"][1:1 + nc].tolist() == root["actions"]
            assert tree["N"][1:1 + nc].tolist() == root["cN"]
            assert tree["Q"][1:1 + nc].tolist() == root["cQ"] and tree["P"][1:1 + nc].tolist() == root["cP"]
            # visit conservation.  A node is expanded by its first visit, which stops there; every later visit goes on to
            # exactly one child: children's N sum to N - 1.  That holds for the root too - a constructor root, the fresh root
            # a leaf update_root makes and a re-rooted child are all expanded by a visit - EXCEPT a root that
            # expand_root_dirichlet expanded before its first visit: there every visit goes on to a child, the sum is N.
            tot, cnt = _children_sum(tree)
            expanded = cnt > 0
            want = tree["N"] - 1
            if c["eta"] is not None and k == 0:
                want[0] = tree["N"][0]
            assert (tot[expanded] == want[expanded]).all()
            assert (tree["N"][~expanded] >= 0).all() and (tree["N"][expanded] >= 1).all()
            # the counters: a playout of depth d visits d + 1 nodes
            visits = sum(r["counters"][f] - prev_counters[f] for f in ("sims", "sum_depth"))
            kept = 0 if prev is None else int(PS.sub_bfs(prev["tree"], 1 + prev["root"]["actions"].index(prev["move"]))["N"].sum())
            assert int(tree["N"].sum()) == kept + visits
            assert r["counters"]["sims"] == (k + 1) * c["n_playouts"]
            assert root["N"] == c["n_playouts"] + (0 if prev is None else prev["root"]["cN"][prev["root"]["actions"].index(prev["move"])])
            prev, prev_counters = r, r["counters"]
        print(key, "position", p, [(len(r["tree"]["N"]), r["root"]["N"], r["created"], r["deepest"], r["counters"]["terminal_hits"])
                                   for r in rows])


@pytest.mark.parametrize("game,hist,S", [(PS.C4, PS.SEQUENCES["c4_400"]["positions"][2], 400),
                                         (PS.BT6, PS.SEQUENCES["bt6_800"]["positions"][1], 800)])
def test_update_root_leaves_the_sub_bfs_of_the_child(game, hist, S):
    """After update_root(a) the dump equals the sub-BFS under child a of the dump before, array for array - also for an
    unvisited child and down to a leaf root."""
    m = orc.MCTS(PS.policy(game), game, n_playouts=S, use_dirichlet=False)
    s = orc.State(game)
    for a in hist:
        s.apply_action(a)
    m.search(s)
    before = m.dump_tree()
    assert len(before["N"]) > 2000
    root = m.root_stats()
    a = PS.most_visited(root)
    m.update_root(a)
    after = m.dump_tree()
    _same_tree(after, PS.sub_bfs(before, 1 + root["actions"].index(a)))
    assert after["N"][0] == max(root["cN"]) and after["action"][0] == -1 and after["parent"][0] == -1
    while len(after["N"]) > 1:                                          # down the LEAST visited line, to a leaf root
        root = m.root_stats()
        i = int(np.argmin(root["cN"]))
        m.update_root(root["actions"][i])
        before, after = after, m.dump_tree()
        _same_tree(after, PS.sub_bfs(before, 1 + i))
    assert orc.lib().orc_mcts_dump_tree(m._m, 0, None, None, None, None, None) == 1


def test_dump_tree_respects_max_nodes():
    m = orc.MCTS(PS.policy(PS.C4), PS.C4, n_playouts=50, use_dirichlet=False)
    m.search(orc.State(PS.C4))
    full = m.dump_tree()
    n, k = len(full["N"]), 20
    par, act = np.full(k + 1, 77, np.int32), np.full(k + 1, 77, np.int32)
    N, Q, P = np.full(k + 1, 77, np.int64), np.full(k + 1, 77.0), np.full(k + 1, 77.0)
    got = orc.lib().orc_mcts_dump_tree(m._m, k, orc._ip(par), orc._ip(act), orc._lp(N), orc._dp(Q), orc._dp(P))
    assert got == n > k
    for arr, f in ((par, "parent"), (act, "action"), (N, "N"), (Q, "Q"), (P, "P")):
        assert np.array_equal(arr[:k], full[f][:k]) and arr[k] == 77    # k rows and not one more
    assert m.root_stats()["N"] == 50 and m.counters()["sims"] == 50    # read-only


# ------------------------------------------------------------------------------------------------ what the cases are for
def test_no_sequence_ends_its_game_early():
    """update_root with a move that ends the game idles the slot: only the last search of a position may be followed by one."""
    for key in KEYS:
        for rows in PS.oracle_sequence(key):
            assert not any(r["ends"] for r in rows[:-1]), key


def test_a_kept_root_reaches_2500_visits():
    best = max(r["root"]["N"] for key in KEYS for rows in PS.oracle_sequence(key) for r in rows[1:])
    print("largest kept root N", best)
    assert best >= 2500


@pytest.mark.parametrize("key", ["bt6_800", "bt8_1600"])
def test_breakthrough_pools_pass_65536_nodes_and_depth_14(key):
    """The device pool index grows with created nodes (1 for the root, then every expansion's children), not with live ones."""
    seq = PS.oracle_sequence(key)
    allocs = [1 + sum(r["created"] for r in rows) for rows in seq]
    print(key, "pool index after the last search, per position", allocs, "deepest", [[r["deepest"] for r in rows] for rows in seq])
    assert allocs[0] > 65536
    assert max(r["deepest"] for rows in seq for r in rows) >= 14
    assert max(len(r["tree"]["N"]) for rows in seq for r in rows) > (65536 if key == "bt8_1600" else 40000)


def test_a_re_rooting_copies_more_than_65536_nodes():
    """In the pools of pool_plan(): bt8_1600's one re-rooting copies a wide subtree, and the second re-rooting of
    bt8_1600_mid copies one of more than 2^16 nodes - the destination index of the Cheney copy passes 2^16 - into a pool
    that has room for it and for the search that follows."""
    cap, copies = PS.pool_plan("bt8_1600")
    print("bt8_1600 pool", cap, "copies", copies)
    assert len(copies) == 1 and copies[0] > 20000
    cap, copies = PS.pool_plan("bt8_1600_mid")
    rows = PS.oracle_sequence("bt8_1600_mid")[0]
    kept = [len(PS.kept_tree(r)["N"]) for r in rows[:-1]]
    print("bt8_1600_mid pool", cap, "kept by the re-rootings", kept, "copies", copies, "trees", [len(r["tree"]["N"]) for r in rows])
    assert kept[1] > 65536 and copies == [kept[1]]
    assert kept[1] + (1600 + 1) * 48 <= cap and len(rows[2]["tree"]["N"]) > kept[1]


def test_late_searches_are_full_of_terminal_hits():
    c4 = PS.oracle_sequence("c4_400")[PS.LATE["c4_400"]]
    bt6 = PS.oracle_sequence("bt6_800")[PS.LATE["bt6_800"]]
    print("c4 late", [r["counters"]["terminal_hits"] for r in c4], "bt6 late", [r["counters"]["terminal_hits"] for r in bt6])
    assert 14 <= len(PS.SEQUENCES["c4_400"]["positions"][PS.LATE["c4_400"]]) <= 16
    assert c4[0]["counters"]["terminal_hits"] >= 30
    assert bt6[-1]["counters"]["terminal_hits"] >= 100


def test_uct_case_searches_under_the_uct_rule():
    """The leaf update_root hands the tree MCTS.use_puct = False (mcts.py:199-200): its searches differ from the PUCT ones of
    the same position (c4_400's mid-game slot), and the kept root passes N = 400, so log(N) is taken up to 800."""
    uct, puct = PS.oracle_sequence("c4_400_uct")[0], PS.oracle_sequence("c4_400")[1]
    assert PS.SEQUENCES["c4_400_uct"]["positions"][0] == PS.SEQUENCES["c4_400"]["positions"][1]
    assert uct[0]["root"]["cN"] != puct[0]["root"]["cN"]
    assert 400 < uct[1]["root"]["N"] <= 800
    noise = PS.oracle_sequence("c4_400_noise")[0]                      # same position again, with the given root noise
    assert PS.SEQUENCES["c4_400_noise"]["positions"][0] == PS.SEQUENCES["c4_400"]["positions"][1]
    assert noise[0]["root"]["cP"] != puct[0]["root"]["cP"] and noise[0]["root"]["cN"] != puct[0]["root"]["cN"]


def test_whole_games_are_long_and_the_small_pool_compacts():
    for key in PS.GAMES:
        want = PS.oracle_games(key)
        print(key, "plies", [len(w["actions"]) for w in want], [w["counters"] for w in want])
        assert all(len(w["actions"]) > 15 for w in want)
        cap, compactions = PS.small_pool(key)
        print(key, "small pool", cap, "compactions expected", compactions)
        assert compactions >= 3
