"""Shared by test_product_scale_host.py and test_product_scale_gpu.py: searches and games at the playout counts the project
ships and times - connect_four at 400, breakthrough 6x6 at 800 and 8x8 at 1600, on kept trees - under the hashed softmax of
oracle/fakepolicy.fake_eval, with the C oracle's whole tree (MCTS.dump_tree) as the expected result.

A sequence is: search, update_root(most visited child, keep_subtree=True), search again, ... from a given position; a position
is the action list that leads to it from the initial position.  The positions below are prefixes of oracle games played at 30
playouts under the same policy (temperature 1, fixed uniforms), picked on the CPU so that test_product_scale_host.py's
conditions hold: a later edit that moves one has to keep them.

Every evaluation goes through one memo per game, keyed by fakepolicy.board_key: the oracle's run and the engine's share their
evaluations, and a HostPolicyEvaluator (which asks for every row again each tick) costs a dictionary lookup per row."""
import numpy as np

from oracle import binding as orc
from oracle import fakepolicy

SALT = 5
C4, BT6, BT8 = "connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=8,columns=8)"

_C4_GAME = [0, 1, 3, 2, 6, 1, 2, 6, 3, 0, 2, 2, 0, 3, 1, 3, 0]                       # 17 plies
_BT6_GAME = [76, 344, 2, 308, 124, 270, 108, 354, 50, 330, 122, 370, 101, 404, 16, 322, 156, 263, 74, 235, 185, 426, 85, 382,
             265, 344, 325]                                                          # 27 plies
_BT8_GAME = [180, 666, 148, 754, 256, 608, 364, 514, 86, 426, 168, 558, 252, 668, 74, 714, 40, 634, 110, 764, 156, 622, 266, 550,
             134, 462, 62, 356, 182, 610, 14, 704, 336, 728, 160, 584, 230, 490, 244, 570, 470, 260, 328, 164]   # 44 plies

# key -> game, playouts per search, positions, searches per position, root noise vector (one search with use_dirichlet and the
# vector injected; None: no root noise), use_puct, leaf_update (the LAST action of the position is played with update_root on
# the untouched leaf root, which gives the tree MCTS.use_puct's rule, mcts.py:199-200).
#
# bt6_800's initial position runs SIX searches: a 6x6 search at 800 playouts creates at most 14 000 nodes, so the pool index
# of a slot passes 2^16 in the fifth one; the late position's game is over before that, it runs two.
SEQUENCES = {
    "c4_400": dict(game=C4, n_playouts=400, positions=[[], _C4_GAME[:8], _C4_GAME[:15]], searches=[3, 3, 3]),
    "c4_400_noise": dict(game=C4, n_playouts=400, positions=[_C4_GAME[:8]], searches=[1],
                         eta=[0.05, 0.4, 0.0, 0.3, 0.05, 0.15, 0.05]),
    "c4_400_uct": dict(game=C4, n_playouts=400, positions=[_C4_GAME[:8]], searches=[2], use_puct=False, leaf_update=True),
    "bt6_800": dict(game=BT6, n_playouts=800, positions=[[], _BT6_GAME[:23]], searches=[6, 2]),
    "bt8_1600": dict(game=BT8, n_playouts=1600, positions=[_BT8_GAME[:40]], searches=[2]),
    # a mid-game position whose most visited child gets almost every playout: the subtree kept by the SECOND re-rooting holds
    # more than 2^16 nodes.  Run in the pool of pool_plan(), that re-rooting is a Cheney copy whose destination passes 2^16.
    "bt8_1600_mid": dict(game=BT8, n_playouts=1600, positions=[_BT8_GAME[:24]], searches=[3]),
}
for _c in SEQUENCES.values():
    _c.setdefault("eta", None)
    _c.setdefault("use_puct", True)
    _c.setdefault("leaf_update", False)
LATE = {"c4_400": 2, "bt6_800": 1}   # the late position's slot

# Whole games, kept tree, root noise and move draws injected: key -> game, playouts, games = slots, seed of the draws.
GAMES = {"game_c4_400": dict(game=C4, n_playouts=400, n_games=2, seed=400)}

COUNTERS = ("sims", "evals", "terminal_hits", "sum_depth", "sum_children")

_MEMO = {}


def policy(game_name, salt=SALT):
    """board -> (priors float32[A], value float32): fake_eval, memoised by board key."""
    memo = _MEMO.setdefault((game_name, salt), {})
    g, r, c = orc.parse_game(game_name)
    A = orc.lib().orc_num_actions(g, r, c)

    def fn(board):
        key = fakepolicy.board_key(board)
        got = memo.get(key)
        if got is None:
            got = memo[key] = fakepolicy.fake_eval(board, A, salt)
        return got

    return fn


def most_visited(root):
    """The root child update_root descends to: the most visited one, the first maximum."""
    return root["actions"][int(np.argmax(root["cN"]))]


_SEQ = {}


def oracle_sequence(key):
    """The case with the C oracle, computed once -> per position, per search: dict(tree = dump_tree(), root = root_stats(),
    counters = the MCTS object's counters so far, created = nodes the search created, deepest = its deepest playout, move =
    the most visited child, ends = whether that move ends the game)."""
    if key in _SEQ:
        return _SEQ[key]
    c, L = SEQUENCES[key], orc.lib()
    out = []
    for hist, n_search in zip(c["positions"], c["searches"]):
        m = orc.MCTS(policy(c["game"]), c["game"], n_playouts=c["n_playouts"], use_dirichlet=c["eta"] is not None,
                     use_puct=c["use_puct"])
        s = orc.State(c["game"])
        for a in hist:
            s.apply_action(a)
        if c["leaf_update"]:
            m.update_root(hist[-1])
        rows = []
        for k in range(n_search):
            if k:
                m.update_root(rows[-1]["move"])
            t0 = L.orc_nodes_total()
            orc.max_depth()
            m.search(s, c["eta"])
            root = m.root_stats()
            rows.append(dict(tree=m.dump_tree(), root=root, counters=m.counters(), created=L.orc_nodes_total() - t0,
                             deepest=orc.max_depth(), move=most_visited(root)))
            s.apply_action(rows[-1]["move"])
            rows[-1]["ends"] = s.is_terminal()
        out.append(rows)
    _SEQ[key] = out
    return out


def sub_bfs(tree, row):
    """The subtree under `row` of a breadth-first dump, as a dump of its own (what update_root to that node leaves)."""
    par = tree["parent"]
    first = np.full(len(par), -1, dtype=np.int64)      # first child row of every row: children are consecutive
    count = np.zeros(len(par), dtype=np.int64)
    for i in range(len(par) - 1, 0, -1):
        first[par[i]] = i
        count[par[i]] += 1
    order, parent = [row], [-1]
    for i, r in enumerate(order):                      # (the list grows while it is walked)
        for ch in range(first[r], first[r] + count[r]):
            order.append(ch)
            parent.append(i)
    order = np.asarray(order, dtype=np.int64)
    action = tree["action"][order].copy()
    action[0] = -1
    return {"parent": np.asarray(parent, dtype=np.int32), "action": action, "N": tree["N"][order], "Q": tree["Q"][order],
            "P": tree["P"][order]}


def max_children(game_name):
    gid, _, cols = orc.parse_game(game_name)
    return min(64, 6 * cols) if gid else 7


def kept_tree(row):
    """The dump of the subtree that update_root(row's move) keeps, computed once per row."""
    if "kept" not in row:
        row["kept"] = sub_bfs(row["tree"], 1 + row["root"]["actions"].index(row["move"]))
    return row["kept"]


def pool_plan(key):
    """A pool that makes a sequence's re-rootings compact -> (nodes_per_slot, nodes copied by each compacting re-rooting, in
    order): one search's room plus the largest subtree a re-rooting of the case keeps plus slack, and the engine's bookkeeping
    (reroot) replayed on the CPU - a re-rooting copies the kept subtree into a spare pool when the slot's pool has no room
    for another search.  On a manual_moves engine that copy is compact_subtree, a wave's Cheney copy."""
    c = SEQUENCES[key]
    need = (c["n_playouts"] + 1) * max_children(c["game"])
    seq = oracle_sequence(key)
    kept = [[len(kept_tree(r)["N"]) for r in rows[:-1]] for rows in seq]
    cap = need + max(max(ks) for ks in kept if ks) + 64
    copies = []
    for rows, ks in zip(seq, kept):
        alloc = 1
        for r, k in zip(rows[:-1], ks):
            alloc += r["created"]
            if alloc + need > cap:
                alloc = k
                copies.append(k)
    return cap, copies


# ------------------------------------------------------------------------------------------------ whole games
def draws(key):
    """-> (etas per game per ply, uniforms per game per ply, the etas cut to the engine's row length)."""
    c = GAMES[key]
    gid, rows, cols = orc.parse_game(c["game"])
    mp = orc.max_plies(gid, rows, cols)
    rng = np.random.RandomState(c["seed"])
    etas = [[rng.dirichlet(0.3 * np.ones(3 * rows * cols)).tolist() for _ in range(mp)] for _ in range(c["n_games"])]
    us = [rng.random_sample(mp).tolist() for _ in range(c["n_games"])]
    mc = min(64, 6 * cols) if gid else 7
    return etas, us, [[row[:mc] for row in e] for e in etas]


_GAMES = {}


def oracle_games(key):
    """orc.play_game_self of every game of the case, computed once."""
    if key not in _GAMES:
        c = GAMES[key]
        etas, us, _ = draws(key)
        _GAMES[key] = [orc.play_game_self(policy(c["game"]), c["game"], n_playouts=c["n_playouts"], etas=etas[g], us=us[g])
                       for g in range(c["n_games"])]
    return _GAMES[key]


def kept_sizes(key, g):
    """Game g again, search by search -> (nodes created by each search, nodes alive after each update_root)."""
    c, L = GAMES[key], orc.lib()
    etas, want = draws(key)[0][g], oracle_games(key)[g]
    base = L.orc_nodes_alive()
    m = orc.MCTS(policy(c["game"]), c["game"], n_playouts=c["n_playouts"], use_dirichlet=True)
    s = orc.State(c["game"])
    created, kept = [], []
    for j, a in enumerate(want["actions"]):
        t0 = L.orc_nodes_total()
        m.search(s, etas[j])
        assert m.root_stats()["cN"] == want["root_cN"][j]
        created.append(L.orc_nodes_total() - t0)
        s.apply_action(a)
        m.update_root(a)
        kept.append(L.orc_nodes_alive() - base)
    return created, kept


def small_pool(key):
    """-> (nodes_per_slot, compactions expected): the largest kept subtree of the case's games plus one search plus slack, and
    the engine's bookkeeping (reroot) replayed on the CPU - a re-rooting compacts when the pool has no room for another
    search, and the copy leaves the kept subtree alone in the new pool."""
    c = GAMES[key]
    sizes = [kept_sizes(key, g) for g in range(c["n_games"])]
    need = (c["n_playouts"] + 1) * 7                   # (n_playouts + 1) * max_children: a search's room (connect_four)
    cap = need + max(max(kept) for _, kept in sizes) + 64
    compactions = 0
    for created, kept in sizes:
        alloc = 1
        for new, k in zip(created[:-1], kept[:-1]):
            alloc += new
            if alloc + need > cap:
                alloc, compactions = k, compactions + 1
                assert alloc + need <= cap
    return cap, compactions
