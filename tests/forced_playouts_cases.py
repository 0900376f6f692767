"""The model of tests/test_forced_playouts_host.py and tests/test_forced_playouts_gpu.py: self-play (play_game_self,
game_utils.py:148-206: AlphaZeroBot.step over MCTS.get_action_probabilities) restated in plain Python with the two rules of
az_engine_set_forced_playouts (include/az_engine.h) added - forced playouts at the root and policy target pruning.  Python floats
are IEEE doubles and every expression keeps the association of the original, so a game of the model can be compared with `==`.
Game dynamics, numpy's pairwise sum and the fake network come from oracle/ (State, remove_illegal_actions, np_sum, fake_eval);
the random draws are injected (etas, us) as in tests/test_fuzz_parity_gpu.py.  With k = 0 the model is play_game_self itself,
which tests/test_forced_playouts_host.py pins against the C oracle.  No test lives here."""
import math

import numpy as np

from oracle import binding as orc
from oracle import fakepolicy

INF = float("inf")
COUNTERS = ("sims", "evals", "terminal_hits", "sum_depth", "sum_children")


class Node:
    __slots__ = ("parent", "P", "Q", "N", "use_puct", "actions", "children")

    def __init__(self, parent, prior, use_puct):
        self.parent, self.P, self.Q, self.N, self.use_puct = parent, prior, 0.0, 0, use_puct
        self.actions, self.children = [], []          # insertion order = ascending action

    def value(self, c_puct):                          # mcts.py:68-80
        if self.use_puct:
            return self.Q + c_puct * self.P * math.sqrt(self.parent.N) / (self.N + 1)
        if self.N == 0:
            return INF
        return self.Q + c_puct * self.P * math.sqrt(math.log(self.parent.N) / self.N)

    def expand(self, priors, legal):                  # mcts.py:54-66
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


def forced(child, k):
    """The forcing rule: a visited root child with n * n < (k * P) * N, all in doubles, no sqrt."""
    n = child.N
    return n > 0 and float(n) * float(n) < (k * child.P) * float(child.parent.N)


def select(node, c_puct, k):
    """The first maximal child (mcts.py:38-52); k > 0: at the root of a full search a forced child counts as +infinity."""
    best, bv = 0, None
    for i, c in enumerate(node.children):
        v = INF if k > 0.0 and forced(c, k) else c.value(c_puct)
        if bv is None or v > bv:
            best, bv = i, v
    return best


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


def play_game(game, salt, etas, us, k=0.0, prune_targets=False, schedule=None, n_playouts=100, c_puct=2.5, temperature=1.0,
              dirichlet_ratio=0.25, use_dirichlet=True, use_puct=True, keep_search_tree=True, backup="on-policy",
              num_probabilistic_actions=1000):
    """One game of self-play.  etas[ply][i]: the Dirichlet draw of the i-th legal action, us[ply]: the uniform behind the move.
    k, prune_targets: az_engine_set_forced_playouts.  schedule: per ply (playouts, is_full) - a playout cap; None = every search
    is a full one of n_playouts.  -> dict(plies=[dict(raw, recorded, actions, move, pi, pi_raw, value, full, budgets, by_puct,
    singles, carried, playouts)], actions, ret0, counters); pi is formed from the recorded counts, pi_raw from the raw ones."""
    state = orc.State(game)
    A = int(state.num_actions)
    cnt = dict.fromkeys(COUNTERS, 0)

    def evaluate(s):
        pri, val = fakepolicy.fake_eval(s.board(), A, salt)
        cnt["evals"] += 1
        return [float(x) for x in pri], float(val)

    def playout(root, s, kf):
        node, depth, mover = root, 0, s.current_player()
        while node.children and not s.is_terminal():                    # mcts.py:126-153
            mover = s.current_player()
            cnt["sum_children"] += len(node.children)
            i = select(node, c_puct, kf if node is root else 0.0)
            s.apply_action(node.actions[i])
            node = node.children[i]
            depth += 1
        if not s.is_terminal():
            priors, leaf_value = evaluate(s)
            node.expand(priors, s.legal_actions())
        else:
            leaf_value = -s.player_return(mover)
            cnt["terminal_hits"] += 1
        node.update_recursive(-leaf_value)
        cnt["sims"] += 1
        cnt["sum_depth"] += depth

    root, plies, hist = Node(None, 0.0, True), [], []
    n_prob = int(num_probabilistic_actions) if int(num_probabilistic_actions) > 0 else 0    # (oracle.binding: 0 = never sample)
    while not state.is_terminal():
        ply = len(hist)
        playouts, full = schedule[ply] if schedule is not None else (n_playouts, True)
        if keep_search_tree:                                            # alphazerobot.py:44-58
            if hist:
                if not root.children:                                   # mcts.py:192-203
                    root = Node(None, 0.0, use_puct)
                else:
                    root = root.children[root.actions.index(hist[-1])]
                    root.parent = None
        else:
            root = Node(None, 0.0, True)                                # a new MCTS (mcts.py:122)
        legal = state.legal_actions()
        if use_dirichlet:                                               # mcts.py:182-190
            priors, _ = evaluate(state)
            priors = [(1.0 - dirichlet_ratio) * p for p in priors]
            for i, a in enumerate(legal):
                priors[a] = priors[a] + 0.25 * etas[ply][i]
            root.expand(priors, legal)
        kf = k if full else 0.0
        carried = sum(c.N for c in root.children)                       # a kept subtree's visits
        for _ in range(playouts):
            playout(root, state.clone(), kf)
        raw = [c.N for c in root.children]
        rec = dict(raw=raw, recorded=list(raw), actions=list(root.actions), full=bool(full), budgets=[0] * len(raw), by_puct=[],
                   singles=[], carried=carried, playouts=playouts)
        if kf > 0.0 and prune_targets:
            rec["recorded"], rec["budgets"], rec["by_puct"], rec["singles"] = prune(root, c_puct, kf)

        def visit_fractions(counts):                                    # mcts.py:155-162 + alphazerobot.py:7-18
            tot = sum(counts)
            nv = np.zeros(A, dtype=np.float64)
            for a, n in zip(root.actions, counts):
                nv[a] = float(n) / float(tot)
            return orc.remove_illegal_actions(nv, legal)

        nv = visit_fractions(raw)                                       # the move comes from the RAW counts
        e, tot = 1.0 / temperature, 0
        ap = [np_pow(float(x), e) for x in nv]
        for x in ap:
            tot = tot + x
        ap = [x / tot for x in ap]
        if ply < n_prob:                                                # np.random.choice with its one uniform
            acc, cdf = 0.0, []
            for x in ap:
                acc += x
                cdf.append(acc)
            cdf = [x / cdf[-1] for x in cdf]
            move = next((i for i, x in enumerate(cdf) if x > us[ply]), A - 1)
        else:
            move = max(range(A), key=lambda a: (ap[a], -a))             # np.argmax: the first maximum
        rec["pi"], rec["pi_raw"] = visit_fractions(rec["recorded"]).tolist(), nv.tolist()
        if backup == "soft-Z":                                          # game_utils.py:172-194
            rec["value"] = -root.Q
        elif backup == "A0C":
            rec["value"] = max(c.Q if c.N > 0 else -99.0 for c in root.children)
        elif backup == "off-policy":
            rec["value"] = a0gb_value(root)
        else:
            rec["value"] = 0.0
        rec["move"] = move
        plies.append(rec)
        state.apply_action(move)
        hist.append(move)
    ret0 = state.player_return(0)
    if backup == "on-policy":                                           # game_utils.py:200-204
        reward = ret0
        for rec in plies:
            rec["value"] = reward
            reward *= -1
    return {"plies": plies, "actions": hist, "ret0": ret0, "counters": cnt}


# ------------------------------------------------------------------------------------------------ the shared cases
# The configurations of the engine-against-model test (tests/test_forced_playouts_gpu.py), whose model games
# tests/test_forced_playouts_host.py checks for the effects the rules must show.  S = 24, k = 2, at most 4 slots and 8 games.
# Together: kept and fresh trees, fewer slots than games (refill), a pool of three searches (compaction), max_sims_per_tick 1 and
# 3 with chain_window_us = -1 (no time window: playouts chain on the register-cached root), all four value targets.
K, S, S_FAST = 2.0, 24, 6
CASES = [
    dict(seed=1, game="connect_four", n_games=6, n_slots=4, salt=11, small_pool=False,
         kw=dict(keep_search_tree=True, backup="on-policy"), eng=dict(max_sims_per_tick=1, chain_window_us=-1)),
    dict(seed=2, game="breakthrough(rows=6,columns=6)", n_games=3, n_slots=2, salt=5, small_pool=False,
         kw=dict(keep_search_tree=False, backup="A0C", temperature=0.5), eng=dict(max_sims_per_tick=3, chain_window_us=-1)),
    dict(seed=3, game="connect_four", n_games=3, n_slots=3, salt=42, small_pool=True,
         kw=dict(keep_search_tree=True, backup="soft-Z", c_puct=1.0), eng=dict()),
    dict(seed=4, game="breakthrough(rows=5,columns=4)", n_games=5, n_slots=4, salt=77, small_pool=False,
         kw=dict(keep_search_tree=True, backup="off-policy", dirichlet_ratio=0.5, num_probabilistic_actions=7), eng=dict()),
]


def geometry(game):
    """-> (A, max_plies, max_children, cells) of a game string."""
    gid, rows, cols = orc.parse_game(game)
    return (int(orc.lib().orc_num_actions(gid, rows, cols)), orc.max_plies(gid, rows, cols), min(64, 6 * cols) if gid else 7,
            rows * cols)


def draws(seed, game, n_games):
    """The injected draws of a case: per game, per ply a Dirichlet(0.3) vector over 3 * cells entries, and a uniform."""
    _, mp, _, cells = geometry(game)
    r = np.random.RandomState(7000 + seed)
    etas = [[r.dirichlet(0.3 * np.ones(3 * cells)).tolist() for _ in range(mp)] for _ in range(n_games)]
    us = [r.random_sample(mp).tolist() for _ in range(n_games)]
    return etas, us


_MODEL = {}


def model_games(idx, k, schedules=None):
    """The model's games of CASES[idx] under forcing constant k with pruning (raw counts and their pi are kept beside the recorded
    ones, so prune = 0 is read off the same games).  Computed once per (case, k) and shared by the tests; schedules: per game,
    a per-ply list of (playouts, is_full) - not cached."""
    key = (idx, float(k))
    if schedules is None and key in _MODEL:
        return _MODEL[key]
    c = CASES[idx]
    etas, us = draws(c["seed"], c["game"], c["n_games"])
    out = [play_game(c["game"], c["salt"], etas[i], us[i], k=k, prune_targets=True, n_playouts=S,
                     schedule=None if schedules is None else schedules[i], **c["kw"]) for i in range(c["n_games"])]
    if schedules is None:
        _MODEL[key] = out
    return out
