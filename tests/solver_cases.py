"""The model of tests/test_solver_host.py and tests/test_solver_gpu.py: play_game of tests/forced_playouts_cases.py (self-play,
game_utils.py:148-206, in plain Python with IEEE doubles and the original's association) restated with the seven rules of
az_engine_set_solver (include/az_engine.h): proof status on the nodes, propagation after a terminal's backup, no selection of a
child proven lost, a playout that stops at a proven node, a search that ends at a proven root, the move and the targets at a proven
root, and a status that travels with a kept subtree.  With solver=False it is play_game itself, which tests/test_solver_host.py
pins against the C oracle.  Also here: a brute-force negamax for small positions, the shared cases, and (at the end) the cases of
tests/test_solver_scale_host.py and tests/test_solver_scale_gpu.py: sequences and games at 400-1600 playouts and deep lines.  No
test lives here."""
import math

import numpy as np

import deep_line_cases as DL
import forced_playouts_cases as FC
import product_scale_cases as PS
from oracle import binding as orc
from oracle import fakepolicy

INF = float("inf")
UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3             # seen by the player who moved INTO the node, as its Q
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}
COUNTERS = FC.COUNTERS
PH_WAIT_ROOT, PH_WAIT_LEAF = 3, 4                 # the phases of a slot with a request outstanding (include/az_engine.h)
EFFECTS = ("levels2", "loss_skipped", "stopped_nonterminal", "early_won_root", "early_lost_root", "draw_root", "kept_proven_root",
           "counts_zeroed")


def status_of(x):
    return WIN if x > 0.0 else (LOSS if x < 0.0 else DRAW)


class Node(FC.Node):
    __slots__ = ("status",)

    def __init__(self, parent, prior, use_puct):
        FC.Node.__init__(self, parent, prior, use_puct)
        self.status = UNKNOWN

    def expand(self, priors, legal):                  # mcts.py:54-66; a re-expansion rewrites P alone (rule 7)
        for a in legal:
            if a in self.actions:
                self.children[self.actions.index(a)].P = priors[a]
            else:
                self.actions.append(a)
                self.children.append(Node(self, priors[a], self.use_puct))


def select(node, c_puct, solver):
    """The first maximal child (mcts.py:38-52); rule 3: a LOSS child counts as -infinity.  -> (index, index without the rule)."""
    best, bv, plain, pv = 0, None, 0, None
    for i, c in enumerate(node.children):
        v0 = c.value(c_puct)
        v = -INF if solver and c.status == LOSS else v0
        if bv is None or v > bv:
            best, bv = i, v
        if pv is None or v0 > pv:
            plain, pv = i, v0
    return best, plain


def propagate(node, path_states, audit):
    """Rule 2, from the node that has just become proven upward -> levels climbed.  path_states[d]: the state at depth d."""
    levels, d = 0, len(path_states) - 1
    while node.parent is not None:
        par = node.parent
        if node.status == WIN:
            new = LOSS
        elif any(c.status == UNKNOWN for c in par.children):
            break
        else:
            new = 4 - min(c.status for c in par.children)   # minus the best child value: the codes ascend from WIN to LOSS
        assert par.status == UNKNOWN                  # the descent never passes through a proven node
        par.status = new
        d -= 1
        if audit is not None:
            audit(path_states[d], new, 1 - path_states[d].current_player())
        levels += 1
        node = par
    return levels


def play_game(game, salt, etas, us, solver=True, schedule=None, n_playouts=100, c_puct=2.5, temperature=1.0, dirichlet_ratio=0.25,
              use_dirichlet=True, keep_search_tree=True, backup="on-policy", num_probabilistic_actions=1000, start=(), audit=None,
              trees=None, mirror=None, policy=None, max_searches=None, dumps=False):
    """One game of self-play from the position after `start`.  etas[i][j]: the Dirichlet draw of the j-th legal action at the i-th
    ply played, us[i]: the uniform behind that move.  schedule: per ply played (playouts, is_full) - a playout cap.
    audit(state, status, mover): called with a clone of the position of every node that takes a status, the status, and the player
    who moved into the node (whose view the status is).
    trees: a list that takes the root Node after every search.
    mirror: (coin, table) - az_engine_set_eval_mirror: coin(absolute ply of the root, phase of the waiting slot (3: the root request,
    4: a leaf), playouts of this search already run) says whether the request is evaluated left-right mirrored; the net then sees
    the board with its columns reversed and the search reads the prior of action a at table[a].  The value is left alone.
    policy: board -> (priors, value) in place of fakepolicy.fake_eval(board, A, salt).
    max_searches: stop after that many searches (the last move is still chosen and recorded, but not played; ret0 is None then).
    dumps: every ply also carries tree = tree_dump(root) after its search and kept = the dump of the subtree the re-rooting kept,
    before it is searched (None at the first ply and where the search starts on a fresh root).
    -> dict(plies=[dict(raw, recorded, actions, move, pi, value, ran, status, counters (so far), nodes (in the tree after the
    search), kept_nodes, kept_proven (nodes / proven nodes in the tree the search started on))], actions, ret0, counters, effects,
    mirrored, events=[(ply played, depth of the terminal node that became proven, levels its proof climbed)])."""
    state = orc.State(game)
    for a in start:
        state.apply_action(a)
    A = int(state.num_actions)
    cnt = dict.fromkeys(COUNTERS, 0)
    eff = dict.fromkeys(EFFECTS, 0)
    events = []
    net = policy if policy is not None else (lambda b: fakepolicy.fake_eval(b, A, salt))

    cur = {"ply": len(start), "ran": 0}                                # the search under way: its root's absolute ply, playouts run
    mirrored = [0, 0]                                                   # requests evaluated as they are / mirrored

    def evaluate(s, phase=PH_WAIT_LEAF):
        board = np.asarray(s.board())
        flip = mirror is not None and bool(mirror[0](cur["ply"], phase, cur["ran"] if phase == PH_WAIT_LEAF else 0))
        pri, val = net(board[..., ::-1] if flip else board)
        if flip:
            pri = pri[np.asarray(mirror[1])]
        mirrored[int(flip)] += 1
        cnt["evals"] += 1
        return [float(x) for x in pri], float(val)

    def playout(root, s):
        node, depth, mover = root, 0, s.current_player()
        states = [s.clone()] if audit is not None else [None]
        while node.children and not s.is_terminal() and not (solver and node is not root and node.status != UNKNOWN):
            mover = s.current_player()                                  # mcts.py:126-153
            cnt["sum_children"] += len(node.children)
            i, plain = select(node, c_puct, solver)
            if i != plain:
                eff["loss_skipped"] += 1
            s.apply_action(node.actions[i])
            node = node.children[i]
            depth += 1
            states.append(s.clone() if audit is not None else None)
        if s.is_terminal() or (solver and node is not root and node.status != UNKNOWN):
            if solver and node.status != UNKNOWN:                       # rule 4: the proven value, as a terminal's
                x = VALUE[node.status]
                if not s.is_terminal():
                    eff["stopped_nonterminal"] += 1
                node.update_recursive(x)
            else:
                x = -(-s.player_return(mover))                          # leaf_value = -player_return(mover); update(-leaf_value)
                node.update_recursive(x)
                if solver:                                              # rules 1 and 2
                    node.status = status_of(x)
                    if audit is not None:
                        audit(states[-1], node.status, mover)
                    levels = propagate(node, states, audit)
                    events.append((len(plies), depth, levels))
                    if levels >= 2:
                        eff["levels2"] += 1
            cnt["terminal_hits"] += 1
        else:
            priors, leaf_value = evaluate(s)
            node.expand(priors, s.legal_actions())
            node.update_recursive(-leaf_value)
        cnt["sims"] += 1
        cnt["sum_depth"] += depth

    root, plies, hist = Node(None, 0.0, True), [], []
    n_prob = int(num_probabilistic_actions) if int(num_probabilistic_actions) > 0 else 0
    while not state.is_terminal():
        ply = len(hist)
        playouts, full = schedule[ply] if schedule is not None else (n_playouts, True)
        if keep_search_tree:                                            # alphazerobot.py:44-58 (plain self-play: PUCT throughout)
            if hist:
                if not root.children:
                    root = Node(None, 0.0, True)
                else:
                    root = root.children[root.actions.index(hist[-1])]
                    root.parent = None
        else:
            root = Node(None, 0.0, True)
        legal = state.legal_actions()
        kept_nodes, kept_proven = tree_size(root)
        kept = tree_dump(root) if dumps and hist and keep_search_tree else None
        if solver and root.status != UNKNOWN:
            eff["kept_proven_root"] += 1
        cur["ply"], cur["ran"] = len(start) + ply, 0
        if use_dirichlet:                                               # mcts.py:182-190; made at a proven root as well (rule 5)
            priors, _ = evaluate(state, PH_WAIT_ROOT)
            priors = [(1.0 - dirichlet_ratio) * p for p in priors]
            for i, a in enumerate(legal):
                priors[a] = priors[a] + 0.25 * etas[ply][i]
            root.expand(priors, legal)
        ran = 0
        for _ in range(playouts):
            if solver and root.status != UNKNOWN:                       # rule 5
                break
            cur["ran"] = ran
            playout(root, state.clone())
            ran += 1
        raw = [c.N for c in root.children]
        counts = list(raw)
        if solver and root.status != UNKNOWN:                           # rule 6
            if ran < playouts:
                eff["early_won_root" if root.status == LOSS else ("early_lost_root" if root.status == WIN else "draw_root")] += 1
            if root.status == LOSS:                                     # won for the player to move
                counts = [n if c.status == WIN else 0 for n, c in zip(raw, root.children)]
            elif root.status == DRAW:
                counts = [0 if c.status == LOSS else n for n, c in zip(raw, root.children)]
            if counts != raw:
                eff["counts_zeroed"] += 1
        rec = dict(raw=raw, recorded=counts, actions=list(root.actions), ran=ran, status=root.status, full=bool(full),
                   counters=dict(cnt), nodes=tree_size(root)[0], kept_nodes=kept_nodes, kept_proven=kept_proven)
        if dumps:
            rec["tree"], rec["kept"] = tree_dump(root), kept
        if trees is not None:
            trees.append(root)

        tot = sum(counts)                                               # mcts.py:155-162 + alphazerobot.py:7-18
        nv = np.zeros(A, dtype=np.float64)
        for a, n in zip(root.actions, counts):
            nv[a] = float(n) / float(tot)
        nv = orc.remove_illegal_actions(nv, legal)
        e, tot = 1.0 / temperature, 0
        ap = [FC.np_pow(float(x), e) for x in nv]
        for x in ap:
            tot = tot + x
        ap = [x / tot for x in ap]
        if ply + len(start) < n_prob:                                   # np.random.choice with its one uniform
            acc, cdf = 0.0, []
            for x in ap:
                acc += x
                cdf.append(acc)
            cdf = [x / cdf[-1] for x in cdf]
            move = next((i for i, x in enumerate(cdf) if x > us[ply]), A - 1)
        else:
            move = max(range(A), key=lambda a: (ap[a], -a))             # np.argmax: the first maximum
        rec["pi"] = nv.tolist()
        if backup == "on-policy":
            rec["value"] = 0.0
        elif solver and root.status != UNKNOWN:                         # the proven value for the player to move
            rec["value"] = -VALUE[root.status]
        elif backup == "soft-Z":                                        # game_utils.py:172-194
            rec["value"] = -root.Q
        elif backup == "A0C":
            rec["value"] = max(c.Q if c.N > 0 else -99.0 for c in root.children)
        else:
            rec["value"] = FC.a0gb_value(root)
        rec["move"] = move
        plies.append(rec)
        if max_searches is not None and len(plies) >= max_searches:
            break
        state.apply_action(move)
        hist.append(move)
    ret0 = state.player_return(0) if state.is_terminal() else None
    if backup == "on-policy" and ret0 is not None:                                           # game_utils.py:200-204
        reward = ret0 if len(start) % 2 == 0 else -ret0                 # (seen by the player to move at the first recorded ply)
        for rec in plies:
            rec["value"] = reward
            reward *= -1
    return {"plies": plies, "actions": hist, "ret0": ret0, "counters": cnt, "effects": eff, "mirrored": mirrored, "events": events}


def tree_statuses(root, full=False):
    """The statuses of a tree in the breadth-first order of SelfPlayEngine.read_tree / read_proofs, with the visit counts.
    full: -> (statuses, counts, parent rows, actions, Q, P) - every column of az_engine_read_tree; the root's row has parent -1
    and action -1."""
    order, parent, action, i = [root], [-1], [-1], 0
    while i < len(order):
        n = order[i]
        order.extend(n.children)
        parent.extend([i] * len(n.children))
        action.extend(n.actions)
        i += 1
    if not full:
        return [n.status for n in order], [n.N for n in order]
    return [n.status for n in order], [n.N for n in order], parent, action, [n.Q for n in order], [n.P for n in order]


def tree_dump(root):
    """tree_statuses(full=True) as the arrays of SelfPlayEngine.read_tree (parent, action, N, Q, P) plus status as read_proofs'."""
    st, n, parent, action, q, p = tree_statuses(root, full=True)
    return {"parent": np.asarray(parent, dtype=np.int32), "action": np.asarray(action, dtype=np.int32),
            "N": np.asarray(n, dtype=np.int64), "Q": np.asarray(q, dtype=np.float64), "P": np.asarray(p, dtype=np.float64),
            "status": np.asarray(st, dtype=np.int8)}


def tree_size(root):
    """-> (nodes, proven nodes) of a tree."""
    stack, nodes, proven = [root], 0, 0
    while stack:
        n = stack.pop()
        nodes += 1
        proven += n.status != UNKNOWN
        stack.extend(n.children)
    return nodes, proven


def event_stats(events):
    """What the proof events of a game reach -> dict(events, max_levels, max_depth, cross64, cross128: events whose walk up the
    path goes from depth 64 (128) to depth 63 (127), i.e. depth - levels <= 63 (127) < depth)."""
    return dict(events=len(events), max_levels=max((lv for _, _, lv in events), default=0),
                max_depth=max((d for _, d, _ in events), default=0),
                cross64=sum(1 for _, d, lv in events if d - lv <= 63 < d),
                cross128=sum(1 for _, d, lv in events if d - lv <= 127 < d))


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
