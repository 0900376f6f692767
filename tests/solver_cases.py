"""The cases of tests/test_solver_host.py and tests/test_solver_gpu.py: self-play under the seven rules of az_engine_set_solver
(include/az_engine.h) as tests/search_model.py states them: proof status on the nodes, propagation after a terminal's backup, no
selection of a child proven lost, a playout that stops at a proven node, a search that ends at a proven root, the move and the
targets at a proven root, and a status that travels with a kept subtree.  With solver=False the model is play_game_self itself,
which tests/test_solver_host.py pins against the C oracle.  Also here: a brute-force negamax for small positions, the shared cases,
and (at the end) the cases of tests/test_solver_scale_host.py and tests/test_solver_scale_gpu.py: sequences and games at 400-1600
playouts and deep lines.  No test lives here."""
import functools

import numpy as np

import deep_line_cases as DL
import forced_playouts_cases as FC
import product_scale_cases as PS
import search_model as SM
from oracle import binding as orc
from search_model import COUNTERS, DRAW, LOSS, UNKNOWN, VALUE, WIN, event_stats, tree_statuses   # (the tests read them here)
from search_model import SOLVER_EFFECTS as EFFECTS

play_game = functools.partial(SM.play_game, solver=True)


# ------------------------------------------------------------------------------------------------ brute force
def negamax(state, depth):
    """The game-theoretic value of the non-terminal `state` for the player to move if `depth` plies of full-width search decide
    it, else None.  Exhaustive and memo-free: it shares nothing with the model's bookkeeping."""
    best, unknown = -2.0, False
    me = state.current_player()
    for a in state.legal_actions():
        s = state.clone()
        s.apply_action(a)
        if s.is_terminal():
            v = s.player_return(me)
        elif depth <= 1:
            v = None
        else:
            r = negamax(s, depth - 1)
            v = None if r is None else -r
        if v is None:
            unknown = True
        else:
            if v >= 1.0:
                return 1.0
            best = max(best, v)
    return None if unknown else best


def solved_value(state, max_depth=12):
    """Iterative deepening over negamax: the value for the player to move as soon as some depth decides it (None: none did)."""
    for d in range(1, max_depth + 1):
        v = negamax(state, d)
        if v is not None:
            return v
    return None


def check_status(state, status, mover, max_depth=12):
    """Is `status`, seen by `mover` (the player who moved into `state`), the negamax value of the position?  A terminal position
    is read off the game itself."""
    if state.is_terminal():
        return VALUE[status] == state.player_return(mover)
    assert state.current_player() == 1 - mover
    v = solved_value(state, max_depth)
    return v is not None and VALUE[status] == -v


# ------------------------------------------------------------------------------------------------ the shared cases
C4, B54, B66 = "connect_four", "breakthrough(rows=5,columns=4)", "breakthrough(rows=6,columns=6)"
S, S_FAST = 24, 6


def c4_late_prefix(seed, empties):
    """A connect_four move list that leaves `empties` empty cells and no winner: random legal moves, retried from a seeded
    generator until a game gets that far."""
    r = np.random.RandomState(9000 + seed)
    while True:
        s, hist = orc.State(C4), []
        while len(hist) < 42 - empties and not s.is_terminal():
            a = int(r.choice(s.legal_actions()))
            s.apply_action(a)
            hist.append(a)
        if len(hist) == 42 - empties and not s.is_terminal():
            return hist


# The configurations of the engine-against-model test (tests/test_solver_gpu.py); tests/test_solver_host.py shows on these very
# games that every rule bites.  24 playouts, at most 4 slots and 8 games.  Together: kept and fresh trees, fewer slots than games
# (refill), a pool of three searches (compaction), max_sims_per_tick 1 and 3 without a chain window, all four value targets,
# connect_four from late positions (draws and short forced lines) and both breakthrough boards.
CASES = [
    dict(seed=1, game=C4, n_games=6, n_slots=4, salt=11, small_pool=False, start=("late", 3, 10),
         kw=dict(keep_search_tree=True, backup="on-policy"), eng=dict(max_sims_per_tick=1, chain_window_us=-1)),
    dict(seed=2, game=B66, n_games=3, n_slots=2, salt=5, small_pool=False, start=None,
         kw=dict(keep_search_tree=False, backup="A0C", temperature=0.5), eng=dict(max_sims_per_tick=3, chain_window_us=-1)),
    dict(seed=3, game=C4, n_games=3, n_slots=3, salt=42, small_pool=True, start=None,
         kw=dict(keep_search_tree=True, backup="soft-Z", c_puct=1.0), eng=dict()),
    dict(seed=4, game=B54, n_games=5, n_slots=4, salt=77, small_pool=False, start=None,
         kw=dict(keep_search_tree=True, backup="off-policy", dirichlet_ratio=0.5, num_probabilistic_actions=7), eng=dict()),
    dict(seed=5, game=C4, n_games=4, n_slots=4, salt=3, small_pool=False, start=("late", 11, 4),
         kw=dict(keep_search_tree=True, backup="soft-Z"), eng=dict()),
]


def case_start(case):
    return [] if case["start"] is None else c4_late_prefix(case["start"][1], case["start"][2])


_MODEL = {}


def model_games(idx, solver=True, schedules=None, audit=None, trees=None, mirrors=None):
    """The model's games of CASES[idx]; computed once per (case, solver) and shared by the tests unless a schedule, an audit, a
    tree list or the games' mirror coins are given."""
    key = (idx, bool(solver))
    cached = schedules is None and audit is None and trees is None and mirrors is None
    if cached and key in _MODEL:
        return _MODEL[key]
    c = CASES[idx]
    etas, us = FC.draws(c["seed"], c["game"], c["n_games"])
    start = case_start(c)
    out = [play_game(c["game"], c["salt"], etas[i], us[i], solver=solver, n_playouts=S, start=start,
                     schedule=None if schedules is None else schedules[i], audit=audit,
                     trees=None if trees is None else trees[i], mirror=None if mirrors is None else mirrors[i], **c["kw"])
           for i in range(c["n_games"])]
    if cached:
        _MODEL[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the solver at product scale
# Shared by tests/test_solver_scale_host.py and tests/test_solver_scale_gpu.py.  A sequence is play_game on ONE kept tree without
# root noise and with num_probabilistic_actions=0 (the move is the first maximum of the recorded counts, no uniform is drawn): search,
# re-root to the move, search again, to the end of the game.  Policies are the memoised ones of product_scale_cases.py (hashed
# softmax) and deep_line_cases.py (the line policy), so the model, the C oracle and an engine's HostPolicyEvaluator share evaluations.
# The positions were picked on the CPU so that the conditions of tests/test_solver_scale_host.py hold: an edit that moves one has
# to keep them.
SCALE_CASES = {
    "c4_mid": dict(game=C4, n_playouts=400, start=PS._C4_GAME[:8]),
    "c4_late": dict(game=C4, n_playouts=400, start=PS._C4_GAME[:15]),
    "c4_5_16": dict(game=C4, n_playouts=400, start=c4_late_prefix(5, 16)),
    "c4_3_14": dict(game=C4, n_playouts=400, start=c4_late_prefix(3, 14)),
    "bt6_800": dict(game=PS.BT6, n_playouts=800, start=PS._BT6_GAME[:23]),
    # (the model's sequence from _BT8_GAME[:40] runs seven full searches; this is its position after four moves: four full searches,
    # one that ends after 716 playouts and three proven roots - the whole sequence took too long for one GPU test)
    "bt8_1600": dict(game=PS.BT8, n_playouts=1600, start=PS._BT8_GAME[:40] + [48, 598, 421, 260]),
}
LATE_C4 = ("c4_5_16", "c4_3_14")

# One search from the initial position under the line policy: key -> game, playouts, salt, value scale.  bt8x8: proofs at depths
# 63..92, the walk up the path crosses lane 63 of register 0 / lane 0 of register 1.  bt26x2_128: the first terminal lies at depth
# 129 (the salt search is in DESIGN_HISTORY.md), climbs of 3 and 5 levels from there cross register 2 / register 1.  bt26x2: a
# 5-level climb from depth 149, all inside register 2.
DEEP_CASES = {
    "bt8x8": dict(game="breakthrough(rows=8,columns=8)", n_playouts=290, salt=15, vs=0.01),
    "bt26x2_128": dict(game="breakthrough(rows=26,columns=2)", n_playouts=177, salt=90, vs=0.01),
    "bt26x2": dict(game="breakthrough(rows=26,columns=2)", n_playouts=340, salt=13, vs=0.01),
}
DEEP_GAME = dict(game="breakthrough(rows=8,columns=8)", n_playouts=90, salt=15, vs=0.01)   # the self-play game along bt8x8's line

# Whole self-play games with root noise and injected draws (FC.draws(seed, game, n_games)), kept trees, n_games = n_slots.
GAME_CASES = {
    "c4_5_16_soft_z": dict(game=C4, n_playouts=400, start=c4_late_prefix(5, 16), n_games=2, seed=21, backup="soft-Z"),
    "c4_3_14_off_policy": dict(game=C4, n_playouts=400, start=c4_late_prefix(3, 14), n_games=2, seed=22, backup="off-policy"),
    "bt6_soft_z": dict(game=PS.BT6, n_playouts=800, start=PS._BT6_GAME[:23], n_games=1, seed=23, backup="soft-Z"),
}

_SCALE = {}


def scale_model(key, solver=True, audit=None):
    """The model's sequence of SCALE_CASES[key] with tree dumps, computed once per (case, solver).  solver=False: as many searches
    as the solver's sequence has."""
    if audit is None and (key, solver) in _SCALE:
        return _SCALE[key, solver]
    c = SCALE_CASES[key]
    out = play_game(c["game"], PS.SALT, None, None, solver=solver, n_playouts=c["n_playouts"], use_dirichlet=False,
                    keep_search_tree=True, backup="soft-Z", num_probabilistic_actions=0, start=c["start"], policy=PS.policy(c["game"]),
                    dumps=audit is None, audit=audit, max_searches=None if solver else len(scale_model(key, True)["plies"]))
    if audit is None:
        _SCALE[key, solver] = out
    return out


def oracle_sequence(key, n_searches):
    """SCALE_CASES[key] with the C oracle as product_scale_cases.oracle_sequence runs a sequence: search, update_root(most visited
    child), search again -> per search dict(tree, root, counters, move)."""
    c = SCALE_CASES[key]
    m = orc.MCTS(PS.policy(c["game"]), c["game"], n_playouts=c["n_playouts"], use_dirichlet=False)
    s = orc.State(c["game"])
    for a in c["start"]:
        s.apply_action(a)
    rows = []
    while len(rows) < n_searches and not s.is_terminal():
        if rows:
            m.update_root(rows[-1]["move"])
        m.search(s)
        root = m.root_stats()
        rows.append(dict(tree=m.dump_tree(), root=root, counters=m.counters(), move=PS.most_visited(root)))
        s.apply_action(rows[-1]["move"])
    return rows


def deep_policy(c):
    return DL.policy(c["game"], c["salt"], c["vs"])


def deep_model(key, solver=True):
    """The model's one search of DEEP_CASES[key] from the initial position, with its tree dump, computed once."""
    if ("deep", key, solver) not in _SCALE:
        c = DEEP_CASES[key]
        _SCALE["deep", key, solver] = play_game(c["game"], c["salt"], None, None, solver=solver, n_playouts=c["n_playouts"],
                                                use_dirichlet=False, keep_search_tree=True, backup="soft-Z",
                                                num_probabilistic_actions=0, policy=deep_policy(c), dumps=True, max_searches=1)
    return _SCALE["deep", key, solver]


def oracle_deep(key):
    """DEEP_CASES[key] with the C oracle as deep_line_cases.oracle_search runs a case -> (dump_tree(), counters)."""
    c = DEEP_CASES[key]
    m = orc.MCTS(deep_policy(c), c["game"], n_playouts=c["n_playouts"], use_dirichlet=False)
    s = orc.State(c["game"])
    for _ in range(c["n_playouts"]):
        m.playout(s)
    return m.dump_tree(), m.counters()


def deep_game_model(solver=True):
    """The self-play game along bt8x8's line: kept tree, soft-Z, no root noise, num_probabilistic_actions=0; computed once."""
    if ("deep_game", solver) not in _SCALE:
        c = DEEP_GAME
        _SCALE["deep_game", solver] = play_game(c["game"], c["salt"], None, None, solver=solver, n_playouts=c["n_playouts"],
                                                use_dirichlet=False, keep_search_tree=True, backup="soft-Z",
                                                num_probabilistic_actions=0, policy=deep_policy(c))
    return _SCALE["deep_game", solver]


def game_models(key):
    """The model's games of GAME_CASES[key], computed once."""
    if ("game", key) not in _SCALE:
        c = GAME_CASES[key]
        etas, us = FC.draws(c["seed"], c["game"], c["n_games"])
        _SCALE["game", key] = [play_game(c["game"], PS.SALT, etas[i], us[i], solver=True, n_playouts=c["n_playouts"],
                                         keep_search_tree=True, backup=c["backup"], start=c["start"], policy=PS.policy(c["game"]))
                               for i in range(c["n_games"])]
    return _SCALE["game", key]


def small_pool(key):
    """A pool that makes the re-rootings of GAME_CASES[key] compact -> (nodes_per_slot, compactions expected): one search's room
    plus the largest subtree a re-rooting keeps plus slack, and the engine's bookkeeping (reroot) replayed on the model's tree
    sizes as product_scale_cases.small_pool replays it on the oracle's.  Asserts that the kept subtree plus a search's room fits
    at every re-rooting: POOL_EXHAUSTED cannot be the outcome."""
    c = GAME_CASES[key]
    games = game_models(key)
    need = (c["n_playouts"] + 1) * PS.max_children(c["game"])
    cap = need + max(p["kept_nodes"] for w in games for p in w["plies"]) + 64
    compactions = 0
    for w in games:
        alloc = 1
        for p, nxt in zip(w["plies"][:-1], w["plies"][1:]):
            alloc += p["nodes"] - p["kept_nodes"]
            assert alloc <= cap
            if alloc + need > cap:
                alloc, compactions = nxt["kept_nodes"], compactions + 1
            assert alloc + need <= cap
    return cap, compactions
