"""The search model of the suite: MCTS (mcts.py), AlphaZeroBot.step (alphazerobot.py) and self-play (play_game_self,
game_utils.py:148-206) restated once in plain Python with the search settings of include/az_engine.h added as rules - forced
playouts and policy target pruning (az_engine_set_forced_playouts), the seven rules of the MCTS-Solver (az_engine_set_solver),
first-play urgency (az_engine_set_fpu), the evaluation mirror (az_engine_set_eval_mirror).  Python floats are IEEE doubles and
every expression keeps the association of the original, so a game of the model is compared with the engine's by `==`.  Game
dynamics, numpy's pairwise sum and the fake network come from oracle/; the random draws are injected.  With every setting off
play_game is play_game_self itself, which the host tests pin to the C oracle; with a setting on, tests/test_search_model_host.py
pins it to recorded results.  The case modules (forced_playouts_cases, solver_cases, fpu_cases, arena_match_cases) hold the
inputs; a new setting is one more rule here.  No test lives here."""
import collections
import math

import numpy as np

from oracle import binding as orc
from oracle import fakepolicy

INF = float("inf")
COUNTERS = ("sims", "evals", "terminal_hits", "sum_depth", "sum_children")
UNKNOWN, WIN, DRAW, LOSS = 0, 1, 2, 3             # proof status, seen by the player who moved INTO the node, as its Q
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}
PH_WAIT_ROOT, PH_WAIT_LEAF = 3, 4                 # the phases of a slot with a request outstanding (include/az_engine.h)
SOLVER_EFFECTS = ("levels2", "loss_skipped", "stopped_nonterminal", "early_won_root", "early_lost_root", "draw_root",
                  "kept_proven_root", "counts_zeroed")
# playouts whose selection at some depth differs from the one the rule without FPU makes on the same tree (forcing and the solver's
# -infinity applied to both): an unvisited child chosen where the plain rule chose a visited one, the reverse, and any difference
# at the root
FPU_EFFECTS = ("unvisited_preferred", "unvisited_deferred", "root_differs")


class Node:
    __slots__ = ("parent", "P", "Q", "N", "use_puct", "actions", "children", "status")

    def __init__(self, parent, prior, use_puct):
        self.parent, self.P, self.Q, self.N, self.use_puct, self.status = parent, prior, 0.0, 0, use_puct, UNKNOWN
        self.actions, self.children = [], []          # insertion order = ascending action

    def value(self, c_puct, fpu_q=None):              # mcts.py:68-80; fpu_q: q_eff(parent, f) while first-play urgency is in force
        if fpu_q is not None and self.N == 0:
            return fpu_q + c_puct * self.P * math.sqrt(self.parent.N) / (0 + 1)
        if self.use_puct:
            return self.Q + c_puct * self.P * math.sqrt(self.parent.N) / (self.N + 1)
        if self.N == 0:
            return INF
        return self.Q + c_puct * self.P * math.sqrt(math.log(self.parent.N) / self.N)

    def expand(self, priors, legal):                  # mcts.py:54-66; a re-expansion rewrites P alone (the solver's rule 7)
        for a in legal:
            if a in self.actions:
                self.children[self.actions.index(a)].P = priors[a]
            else:
                self.actions.append(a)
                self.children.append(Node(self, priors[a], self.use_puct))

    def update_recursive(self, value):                # mcts.py:82-89
        node = self
        while node is not None:
            node.Q = (node.N * node.Q + value) / (node.N + 1)
            node.N += 1
            node, value = node.parent, -value


def update_root(root, action, use_puct=True):         # mcts.py:192-203
    if not root.children:
        return Node(None, 0.0, use_puct)
    root = root.children[root.actions.index(action)]
    root.parent = None
    return root


# ------------------------------------------------------------------------------------------------ forced playouts and pruning
def forced(child, k):
    """The forcing rule: a visited root child with n * n < (k * P) * N, all in doubles, no sqrt."""
    n = child.N
    return n > 0 and float(n) * float(n) < (k * child.P) * float(child.parent.N)


def forced_budget(k, prior, root_n):
    """F: the largest integer f >= 0 with f * f <= (k * P) * N."""
    bound, f = (k * prior) * float(root_n), 0
    while float(f + 1) * float(f + 1) <= bound:
        f += 1
    return f


def prune(root, c_puct, k):
    """The pruning rule, straight from its statement -> (recorded counts m, budgets F, children where the PUCT bound stopped the
    pruning above lo, children cut to 0 by the single-playout rule)."""
    raw = [c.N for c in root.children]
    b = raw.index(max(raw))
    sq = math.sqrt(float(root.N))
    u = [(c_puct * c.P) * sq for c in root.children]
    v = root.children[b].Q + u[b] / float(raw[b] + 1)
    m, budgets, by_puct, singles = list(raw), [0] * len(raw), [], []
    for i, c in enumerate(root.children):
        if i == b or raw[i] == 0:
            continue
        budgets[i] = forced_budget(k, c.P, root.N)
        lo = max(raw[i] - budgets[i], 0)
        mi = raw[i]
        while mi > lo and c.Q + u[i] / float((mi - 1) + 1) < v:   # may the child be left with mi - 1 visits?
            mi -= 1
        if mi > lo:
            by_puct.append(i)
        if mi < raw[i] and mi == 1:
            mi = 0
            singles.append(i)
        m[i] = mi
    return m, budgets, by_puct, singles


# ------------------------------------------------------------------------------------------------ the solver
def status_of(x):
    return WIN if x > 0.0 else (LOSS if x < 0.0 else DRAW)


def propagate(node, path_states=None, audit=None):
    """Rule 2, from the node that has just become proven upward -> levels climbed.  path_states[d]: the state at depth d, for
    audit(state, status, mover) alone."""
    levels = 0
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
        levels += 1
        if audit is not None:
            s = path_states[len(path_states) - 1 - levels]
            audit(s, new, 1 - s.current_player())
        node = par
    return levels


def proven_counts(root, raw):
    """Rule 6: the counts behind the move and the policy target at a proven root - a won root keeps its winning children only, a
    drawn root drops the losing ones."""
    if root.status == LOSS:                           # won for the player to move
        return [n if c.status == WIN else 0 for n, c in zip(raw, root.children)]
    if root.status == DRAW:
        return [0 if c.status == LOSS else n for n, c in zip(raw, root.children)]
    return list(raw)


# ------------------------------------------------------------------------------------------------ first-play urgency
def butterfly(xs):
    """wave_sum_d of csrc/az_engine.hip on 64 values: for off = 32, 16, 8, 4, 2, 1 every position l takes x[l] + x[l ^ off]; the
    result is position 0.  Fewer than 64 values are padded with +0.0."""
    x = [float(v) for v in xs] + [0.0] * (64 - len(xs))
    assert len(x) == 64
    off = 32
    while off:
        x = [x[l] + x[l ^ off] for l in range(64)]
        off >>= 1
    return x[0]


def explored_mass(node):
    """m: the priors of the visited children, child i in position i, +0.0 for the unvisited ones."""
    return butterfly([c.P if c.N > 0 else 0.0 for c in node.children])


def q_eff(node, f):
    """What an unvisited child of `node` is worth: v - f * sqrt(m), v = -node.Q - two roundings."""
    v = -node.Q
    pen = f * math.sqrt(explored_mass(node))
    return v - pen


# ------------------------------------------------------------------------------------------------ the search
def select(node, c_puct, k=0.0, solver=False, f=None):
    """The first maximal child (mcts.py:38-52).  k > 0: a forced child counts as +infinity; solver: a LOSS child as -infinity
    (rule 3); f: the FPU reduction in force at this node, None = the reference's Q = 0."""
    fq = None if f is None else q_eff(node, f)
    best, bv = 0, None
    for i, c in enumerate(node.children):
        if solver and c.status == LOSS:
            v = -INF
        elif k > 0.0 and forced(c, k):
            v = INF
        else:
            v = c.value(c_puct, fq)
        if bv is None or v > bv:
            best, bv = i, v
    return best


# c_puct; k: the forcing constant at the root of THIS search (0 in a fast one); solver; fpu: (reduction, reduction_root) or None
Settings = collections.namedtuple("Settings", "c_puct k solver fpu")
# What a playout did beside the tree: the depth it reached; levels: its terminal became proven and the proof climbed that many
# levels (None: no proof); stopped: it ended at a proven node that is no terminal; loss_skipped: selections rule 3 changed;
# fpu_differs: per selection FPU changed (at the root?, chosen child unvisited?, the plain rule's child unvisited?);
# order_sensitive: selections under FPU at which the left-to-right sum of the visited children's priors is not the butterfly's
Trace = collections.namedtuple("Trace", "depth levels stopped loss_skipped fpu_differs order_sensitive")


def playout(root, s, st, evaluate, cnt, audit=None):
    """One playout from `root` on the state `s`, which it plays forward (mcts.py:126-153).  evaluate(state) -> (priors, value);
    cnt takes the engine's counters; audit: see play_game.  What a rule chose differently from the rule without it is worked out
    only for the settings that are on, and for rule 3 only where a LOSS child stands."""
    c_puct, k, solver, fpu = st
    node, depth, mover = root, 0, s.current_player()
    states = [s.clone()] if audit is not None else None
    loss_skipped, order_sensitive, fpu_differs = 0, 0, []
    while node.children and not s.is_terminal() and not (solver and node is not root and node.status != UNKNOWN):
        mover = s.current_player()
        cnt["sum_children"] += len(node.children)
        at_root = node is root
        kf = k if at_root else 0.0
        f = None if fpu is None else fpu[1 if at_root else 0]
        i = select(node, c_puct, kf, solver, f)
        if solver and any(c.status == LOSS for c in node.children):
            loss_skipped += i != select(node, c_puct, kf, False, f)
        if f is not None:
            ps = [c.P if c.N > 0 else 0.0 for c in node.children]
            order_sensitive += butterfly(ps) != sum(ps, 0.0)
            plain = select(node, c_puct, kf, solver, None)
            if i != plain:
                fpu_differs.append((at_root, node.children[i].N == 0, node.children[plain].N == 0))
        s.apply_action(node.actions[i])
        node = node.children[i]
        depth += 1
        if audit is not None:
            states.append(s.clone())
    levels, stopped = None, False
    if s.is_terminal() or (solver and node is not root and node.status != UNKNOWN):
        if solver and node.status != UNKNOWN:         # rule 4: the proven value, as a terminal's
            stopped = not s.is_terminal()
            node.update_recursive(VALUE[node.status])
        else:
            x = -(-s.player_return(mover))            # leaf_value = -player_return(mover); update(-leaf_value)
            node.update_recursive(x)
            if solver:                                # rules 1 and 2
                node.status = status_of(x)
                if audit is not None:
                    audit(states[-1], node.status, mover)
                levels = propagate(node, states, audit)
        cnt["terminal_hits"] += 1
    else:
        priors, leaf_value = evaluate(s)
        cnt["evals"] += 1
        node.expand(priors, s.legal_actions())
        node.update_recursive(-leaf_value)
    cnt["sims"] += 1
    cnt["sum_depth"] += depth
    return Trace(depth, levels, stopped, loss_skipped, fpu_differs, order_sensitive)


def fpu_effects_of(trace):
    """-> the FPU_EFFECTS a playout counts for."""
    seen = set()
    for at_root, got_unvisited, plain_unvisited in trace.fpu_differs:
        hits = (got_unvisited and not plain_unvisited, plain_unvisited and not got_unvisited, at_root)
        seen.update(key for key, hit in zip(FPU_EFFECTS, hits) if hit)
    return seen


def evaluate(net, s, flip=False, table=None):
    """The network on the position -> (priors as a list, value).  flip (az_engine_set_eval_mirror): the net sees the board with its
    columns reversed and the search reads the prior of action a at table[a]; the value is left alone."""
    board = np.asarray(s.board())
    pri, val = net(board[..., ::-1] if flip else board)
    if flip:
        pri = pri[np.asarray(table)]
    return [float(x) for x in pri], float(val)


# ------------------------------------------------------------------------------------------------ the move step
def np_pow(x, e):                                     # numpy's fast paths for ndarray ** python float
    if e == 1.0:
        return x
    if e == 2.0:
        return x * x
    if e == 0.5:
        return math.sqrt(x)
    if e == -1.0:
        return 1.0 / x
    return math.pow(x, e)


def visit_fractions(root, counts, legal, A):          # mcts.py:155-162 + alphazerobot.py:7-18
    tot = sum(counts)
    nv = np.zeros(A, dtype=np.float64)
    for a, n in zip(root.actions, counts):
        nv[a] = float(n) / float(tot)
    return orc.remove_illegal_actions(nv, legal)


def choose_move(root, counts, legal, A, temperature, u):
    """AlphaZeroBot's move from the children's counts: visit fractions, tempered, then np.random.choice with its one uniform u, or
    - u is None - np.argmax, the first maximum.  -> (move, the visit fractions as an array)."""
    nv = visit_fractions(root, counts, legal, A)
    e, tot = 1.0 / temperature, 0
    ap = [np_pow(float(x), e) for x in nv]
    for x in ap:
        tot = tot + x
    ap = [x / tot for x in ap]
    if u is None:
        return max(range(A), key=lambda a: (ap[a], -a)), nv
    acc, cdf = 0.0, []
    for x in ap:
        acc += x
        cdf.append(acc)
    cdf = [x / cdf[-1] for x in cdf]
    return next((i for i, x in enumerate(cdf) if x > u), A - 1), nv


def a0gb_value(root):                                 # game_utils.py:182-194
    node, value, mult = root, 0.0, 1.0
    while node.children:
        value = node.Q
        best, bv = 0, None
        for i, c in enumerate(node.children):
            v = float(c.N) + c.P if c.N > 0 else -99.0
            if bv is None or v > bv:
                best, bv = i, v
        node = node.children[best]
        mult *= -1.0
    if node.N > 0:
        value = node.Q
        mult *= -1.0
    return value * mult


def value_target(root, backup, solver):
    """The value a ply records (game_utils.py:172-194); on-policy: a placeholder until the game's result is known."""
    if backup == "on-policy":
        return 0.0
    if solver and root.status != UNKNOWN:             # the proven value for the player to move
        return -VALUE[root.status]
    if backup == "soft-Z":
        return -root.Q
    if backup == "A0C":
        return max(c.Q if c.N > 0 else -99.0 for c in root.children)
    return a0gb_value(root)


# ------------------------------------------------------------------------------------------------ self-play
def play_game(game, salt, etas, us, fpu=None, k=0.0, prune_targets=False, solver=False, schedule=None, n_playouts=100, c_puct=2.5,
              temperature=1.0, dirichlet_ratio=0.25, use_dirichlet=True, use_puct=True, keep_search_tree=True, backup="on-policy",
              num_probabilistic_actions=1000, start=(), mirror=None, policy=None, audit=None, trees=None, dumps=False,
              max_searches=None, again=0):
    """One game of self-play from the position after `start`.  etas[i][j]: the Dirichlet draw of the j-th legal action at the i-th
    ply played, us[i]: the uniform behind that move.
    fpu: (reduction, reduction_root) or None.  k, prune_targets: az_engine_set_forced_playouts (k > 0 and solver exclude each
    other, as the engine's setters do).  schedule: per ply played (playouts, is_full) - a playout cap; None = every search is a
    full one of n_playouts.  use_puct: of the root that replaces a kept root without children (mcts.py:192-203).
    mirror: (coin, table) - coin(absolute ply of the root, phase of the waiting slot (3: the root request, 4: a leaf), playouts of
    this search already run) says whether the request is evaluated left-right mirrored (see evaluate).
    policy: board -> (priors, value) in place of fakepolicy.fake_eval(board, A, salt).
    audit(state, status, mover): called with a clone of the position of every node that takes a status, the status, and the player
    who moved into the node (whose view the status is).
    trees: a list that takes the root Node after every search (the Node lives on: a later search of a kept tree changes it).
    dumps: every ply also carries tree = tree_dump(root) after its searches and kept = the dump of the subtree the re-rooting kept,
    before it is searched (None at the first ply and where the search starts on a fresh root).
    max_searches: stop after that many plies (the last move is still chosen and recorded, but not played; ret0 is None then).
    again: every search is followed by that many further searches of the same size on the same root and tree
    (AZ_ACTION_SEARCH_AGAIN) before the move is made.
    -> dict(plies=[dict(raw, recorded, actions, move, pi, pi_raw, value, ran, status, full, budgets, by_puct, singles, carried: a
    kept subtree's visits, playouts, counters (so far), nodes (in the tree after the search), kept_nodes, kept_proven (nodes /
    proven nodes in the tree the search started on))], actions, ret0, counters, solver_effects, fpu_effects, mirrored,
    events=[(ply played, depth of the terminal node that became proven, levels its proof climbed)], max_depth: the deepest node a
    playout reached, order_sensitive: see Trace).  The move and pi_raw come from the raw counts, or rule 6's at a proven root; pi
    from the recorded ones, which pruning may have cut further."""
    assert not (solver and k > 0.0)
    state = orc.State(game)
    for a in start:
        state.apply_action(a)
    A = int(state.num_actions)
    cnt = dict.fromkeys(COUNTERS, 0)
    seff, feff = dict.fromkeys(SOLVER_EFFECTS, 0), dict.fromkeys(FPU_EFFECTS, 0)
    events, mirrored, max_depth, order_sensitive = [], [0, 0], 0, 0         # mirrored: requests evaluated as they are / mirrored
    net = policy if policy is not None else (lambda b: fakepolicy.fake_eval(b, A, salt))
    cur = {"ply": len(start), "ran": 0}                                 # the search under way: its root's absolute ply, playouts run

    def request(s, phase=PH_WAIT_LEAF):
        flip = mirror is not None and bool(mirror[0](cur["ply"], phase, cur["ran"] if phase == PH_WAIT_LEAF else 0))
        mirrored[int(flip)] += 1
        return evaluate(net, s, flip, mirror[1] if flip else None)

    root, plies, hist = Node(None, 0.0, True), [], []
    n_prob = int(num_probabilistic_actions) if int(num_probabilistic_actions) > 0 else 0    # (oracle.binding: 0 = never sample)
    while not state.is_terminal():
        ply = len(hist)
        playouts, full = schedule[ply] if schedule is not None else (n_playouts, True)
        if not keep_search_tree:                                        # alphazerobot.py:44-58
            root = Node(None, 0.0, True)                                # a new MCTS (mcts.py:122)
        elif hist:
            root = update_root(root, hist[-1], use_puct)
        legal = state.legal_actions()
        kept_nodes, kept_proven = tree_size(root)
        kept = tree_dump(root) if dumps and hist and keep_search_tree else None
        if solver and root.status != UNKNOWN:
            seff["kept_proven_root"] += 1
        st = Settings(c_puct, k if full else 0.0, solver, fpu)
        carried = sum(c.N for c in root.children)
        for _ in range(1 + again):
            cur["ply"], cur["ran"] = len(start) + ply, 0
            if use_dirichlet:                                           # mcts.py:182-190; made at a proven root as well (rule 5)
                priors, _ = request(state, PH_WAIT_ROOT)
                cnt["evals"] += 1
                priors = [(1.0 - dirichlet_ratio) * p for p in priors]
                for i, a in enumerate(legal):
                    priors[a] = priors[a] + 0.25 * etas[ply][i]
                root.expand(priors, legal)
            ran = 0
            for _ in range(playouts):
                if solver and root.status != UNKNOWN:                   # rule 5
                    break
                cur["ran"] = ran
                t = playout(root, state.clone(), st, request, cnt, audit)
                ran += 1
                max_depth, order_sensitive = max(max_depth, t.depth), order_sensitive + t.order_sensitive
                seff["loss_skipped"] += t.loss_skipped
                seff["stopped_nonterminal"] += t.stopped
                if t.levels is not None:
                    events.append((len(plies), t.depth, t.levels))
                    seff["levels2"] += t.levels >= 2
                for key in fpu_effects_of(t):                           # (per playout, however many of its selections differed)
                    feff[key] += 1
            if trees is not None:
                trees.append(root)
        raw = [c.N for c in root.children]
        counts = proven_counts(root, raw) if solver else list(raw)
        if solver and root.status != UNKNOWN:
            if ran < playouts:
                seff["early_won_root" if root.status == LOSS else ("early_lost_root" if root.status == WIN else "draw_root")] += 1
            seff["counts_zeroed"] += counts != raw
        rec = dict(raw=raw, recorded=list(counts), actions=list(root.actions), ran=ran, status=root.status, full=bool(full),
                   budgets=[0] * len(raw), by_puct=[], singles=[], carried=carried, playouts=playouts, counters=dict(cnt),
                   nodes=tree_size(root)[0], kept_nodes=kept_nodes, kept_proven=kept_proven)
        if st.k > 0.0 and prune_targets:
            rec["recorded"], rec["budgets"], rec["by_puct"], rec["singles"] = prune(root, c_puct, st.k)
        if dumps:
            rec["tree"], rec["kept"] = tree_dump(root), kept
        rec["move"], nv = choose_move(root, counts, legal, A, temperature, us[ply] if ply + len(start) < n_prob else None)
        rec["pi_raw"] = nv.tolist()
        rec["pi"] = rec["pi_raw"] if rec["recorded"] == counts else visit_fractions(root, rec["recorded"], legal, A).tolist()
        rec["value"] = value_target(root, backup, solver)
        plies.append(rec)
        if max_searches is not None and len(plies) >= max_searches:
            break
        state.apply_action(rec["move"])
        hist.append(rec["move"])
    ret0 = state.player_return(0) if state.is_terminal() else None
    if backup == "on-policy" and ret0 is not None:                      # game_utils.py:200-204
        reward = ret0 if len(start) % 2 == 0 else -ret0                 # (seen by the player to move at the first recorded ply)
        for rec in plies:
            rec["value"] = reward
            reward *= -1
    return {"plies": plies, "actions": hist, "ret0": ret0, "counters": cnt, "solver_effects": seff, "fpu_effects": feff,
            "mirrored": mirrored, "events": events, "max_depth": max_depth, "order_sensitive": order_sensitive}


# ------------------------------------------------------------------------------------------------ reading a tree
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
