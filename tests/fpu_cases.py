"""The model of tests/test_fpu_host.py and tests/test_fpu_gpu.py: self-play as tests/forced_playouts_cases.py and
tests/solver_cases.py restate it (plain Python, IEEE doubles, the original's association) with the rule of az_engine_set_fpu
(include/az_engine.h) added: an unvisited child enters the PUCT comparison with Q_eff = -X.Q - f * sqrt(m), m the butterfly sum of
the visited children's priors.  play_game here carries BOTH older models' settings - forced playouts with pruning (k,
prune_targets) and the solver, a playout cap's schedule, the evaluation mirror, a start prefix - so the rule is checked composed
with each.  With fpu=None it is forced_playouts_cases.play_game (solver off) and solver_cases.play_game (k = 0), which
tests/test_fpu_host.py pins on the cases the older host tests pin to the C oracle.  Also here: the 64-slot butterfly, the effect
counters and the shared cases.  No test lives here."""
import math

import numpy as np

import forced_playouts_cases as FC
import solver_cases as SC
from oracle import binding as orc
from oracle import fakepolicy

INF = float("inf")
UNKNOWN, WIN, DRAW, LOSS = SC.UNKNOWN, SC.WIN, SC.DRAW, SC.LOSS
COUNTERS = FC.COUNTERS
PH_WAIT_ROOT, PH_WAIT_LEAF = SC.PH_WAIT_ROOT, SC.PH_WAIT_LEAF
# playouts whose selection at some depth differs from the one the rule without FPU makes on the same tree (forcing and the solver's
# -infinity applied to both): an unvisited child chosen where the plain rule chose a visited one, the reverse, and any difference
# at the root
EFFECTS = ("unvisited_preferred", "unvisited_deferred", "root_differs")
FPU = (0.3, 0.1)                                       # reduction != reduction_root: a mix-up of the two shows


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


class Node(SC.Node):
    __slots__ = ()

    def value(self, c_puct, fpu_q=None):                # mcts.py:68-80; fpu_q: q_eff(parent, f) while the setting is in force
        if fpu_q is not None and self.N == 0:
            return fpu_q + c_puct * self.P * math.sqrt(self.parent.N) / (0 + 1)
        return SC.Node.value(self, c_puct)

    def expand(self, priors, legal):                    # mcts.py:54-66; a re-expansion rewrites P alone
        for a in legal:
            if a in self.actions:
                self.children[self.actions.index(a)].P = priors[a]
            else:
                self.actions.append(a)
                self.children.append(Node(self, priors[a], self.use_puct))


def select(node, c_puct, k, solver, f):
    """The first maximal child (mcts.py:38-52).  k > 0: a forced child counts as +infinity; solver: a LOSS child as -infinity;
    f: the FPU reduction in force at this node, None = the reference's Q = 0.  -> (index, index with f = None)."""
    fq = None if f is None else q_eff(node, f)
    best, bv, plain, pv = 0, None, 0, None
    for i, c in enumerate(node.children):
        force = k > 0.0 and FC.forced(c, k)
        lost = solver and c.status == LOSS
        v = -INF if lost else (INF if force else c.value(c_puct, fq))
        v0 = -INF if lost else (INF if force else c.value(c_puct))
        if bv is None or v > bv:
            best, bv = i, v
        if pv is None or v0 > pv:
            plain, pv = i, v0
    return best, plain


def play_game(game, salt, etas, us, fpu=None, k=0.0, prune_targets=False, solver=False, schedule=None, n_playouts=100, c_puct=2.5,
              temperature=1.0, dirichlet_ratio=0.25, use_dirichlet=True, keep_search_tree=True, backup="on-policy",
              num_probabilistic_actions=1000, start=(), trees=None, mirror=None, max_searches=None, again=0):
    """One game of self-play from the position after `start`.  fpu: (reduction, reduction_root) or None.  k, prune_targets:
    forced_playouts_cases.play_game's; solver, schedule, start, trees, mirror, max_searches: solver_cases.play_game's (k > 0 and
    solver exclude each other, as the engine's setters do).  again: every search is followed by that many further searches of
    n_playouts on the same root and tree (AZ_ACTION_SEARCH_AGAIN) before the move is made; `trees` takes tree_dump(root) after each.
    -> dict(plies=[dict(raw, recorded, actions, move, pi, value, ran, status, full)], actions, ret0, counters, effects, mirrored,
    max_depth: the deepest node a playout reached, order_sensitive: the selections under the rule at which the left-to-right sum of
    the visited children's priors is another number than the butterfly's)."""
    assert not (solver and k > 0.0)
    state = orc.State(game)
    for a in start:
        state.apply_action(a)
    A = int(state.num_actions)
    cnt = dict.fromkeys(COUNTERS, 0)
    eff = dict.fromkeys(EFFECTS, 0)
    cur = {"ply": len(start), "ran": 0, "max_depth": 0, "order_sensitive": 0}
    mirrored = [0, 0]

    def evaluate(s, phase=PH_WAIT_LEAF):
        board = np.asarray(s.board())
        flip = mirror is not None and bool(mirror[0](cur["ply"], phase, cur["ran"] if phase == PH_WAIT_LEAF else 0))
        pri, val = fakepolicy.fake_eval(board[..., ::-1] if flip else board, A, salt)
        if flip:
            pri = pri[np.asarray(mirror[1])]
        mirrored[int(flip)] += 1
        cnt["evals"] += 1
        return [float(x) for x in pri], float(val)

    def playout(root, s, kf):
        node, depth, mover = root, 0, s.current_player()
        seen = set()
        while node.children and not s.is_terminal() and not (solver and node is not root and node.status != UNKNOWN):
            mover = s.current_player()                                  # mcts.py:126-153
            cnt["sum_children"] += len(node.children)
            f = None if fpu is None else (fpu[1] if node is root else fpu[0])
            i, plain = select(node, c_puct, kf if node is root else 0.0, solver, f)
            if f is not None:                                           # (bookkeeping) would summing in child order give another m?
                ps = [c.P if c.N > 0 else 0.0 for c in node.children]
                cur["order_sensitive"] += butterfly(ps) != sum(ps, 0.0)
            if i != plain:
                got, ref = node.children[i], node.children[plain]
                if got.N == 0 and ref.N > 0:
                    seen.add("unvisited_preferred")
                if got.N > 0 and ref.N == 0:
                    seen.add("unvisited_deferred")
                if node is root:
                    seen.add("root_differs")
            s.apply_action(node.actions[i])
            node = node.children[i]
            depth += 1
        for key in seen:
            eff[key] += 1
        if s.is_terminal() or (solver and node is not root and node.status != UNKNOWN):
            if solver and node.status != UNKNOWN:                       # the solver's rule 4
                node.update_recursive(SC.VALUE[node.status])
            else:
                x = -(-s.player_return(mover))
                node.update_recursive(x)
                if solver:                                              # rules 1 and 2
                    node.status = SC.status_of(x)
                    SC.propagate(node, [None] * (depth + 1), None)
            cnt["terminal_hits"] += 1
        else:
            priors, leaf_value = evaluate(s)
            node.expand(priors, s.legal_actions())
            node.update_recursive(-leaf_value)
        cnt["sims"] += 1
        cnt["sum_depth"] += depth
        cur["max_depth"] = max(cur["max_depth"], depth)

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
        kf = k if full else 0.0
        ran = 0
        for rnd in range(1 + again):
            cur["ply"], cur["ran"] = len(start) + ply, 0
            if use_dirichlet:                                           # mcts.py:182-190
                priors, _ = evaluate(state, PH_WAIT_ROOT)
                priors = [(1.0 - dirichlet_ratio) * p for p in priors]
                for i, a in enumerate(legal):
                    priors[a] = priors[a] + 0.25 * etas[ply][i]
                root.expand(priors, legal)
            ran = 0
            for _ in range(playouts):
                if solver and root.status != UNKNOWN:                   # rule 5
                    break
                cur["ran"] = ran
                playout(root, state.clone(), kf)
                ran += 1
            if trees is not None:
                trees.append(tree_dump(root))
        raw = [c.N for c in root.children]
        counts = list(raw)
        if solver and root.status != UNKNOWN:                           # rule 6
            if root.status == LOSS:
                counts = [n if c.status == WIN else 0 for n, c in zip(raw, root.children)]
            elif root.status == DRAW:
                counts = [0 if c.status == LOSS else n for n, c in zip(raw, root.children)]
        rec = dict(raw=raw, recorded=list(counts), actions=list(root.actions), ran=ran, status=root.status, full=bool(full))
        if kf > 0.0 and prune_targets:
            rec["recorded"] = FC.prune(root, c_puct, kf)[0]

        def visit_fractions(cs):                                        # mcts.py:155-162 + alphazerobot.py:7-18
            tot = sum(cs)
            nv = np.zeros(A, dtype=np.float64)
            for a, n in zip(root.actions, cs):
                nv[a] = float(n) / float(tot)
            return orc.remove_illegal_actions(nv, legal)

        nv = visit_fractions(counts)                                    # the move: raw counts, or the solver's adjusted ones
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
        rec["pi"] = visit_fractions(rec["recorded"]).tolist()
        if backup == "on-policy":
            rec["value"] = 0.0
        elif solver and root.status != UNKNOWN:
            rec["value"] = -SC.VALUE[root.status]
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
    if backup == "on-policy" and ret0 is not None:                      # game_utils.py:200-204
        reward = ret0 if len(start) % 2 == 0 else -ret0
        for rec in plies:
            rec["value"] = reward
            reward *= -1
    return {"plies": plies, "actions": hist, "ret0": ret0, "counters": cnt, "effects": eff, "mirrored": mirrored,
            "max_depth": cur["max_depth"], "order_sensitive": cur["order_sensitive"]}


def tree_dump(root):
    """The tree as the arrays of SelfPlayEngine.read_tree (breadth-first; parent, action, N, Q, P)."""
    return SC.tree_dump(root)


# ------------------------------------------------------------------------------------------------ the shared cases
C4, B66, B88 = "connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=8,columns=8)"

B88_MID = [180, 646, 148, 620, 110, 586, 204, 594, 124, 692, 266, 502, 362, 416, 132, 726, 172, 740, 156, 598]

# One search (two with again=1) on a manual_moves engine, no root noise: game, start, playouts, salt.  connect_four has 7
# children; breakthrough 6x6 opens with 16 and passes that, so more butterfly positions carry weight; B88_MID is a breakthrough 8x8
# middle game with 39 legal moves, where a visited child sits beyond lane 32; c4_deep: from a middle game with 20 empty cells the playouts descend to depth 10
# (test_fpu_host.py checks each of these properties on the model).
SEARCHES = {
    "c4": dict(game=C4, start=[], n_playouts=64, salt=11, again=0),
    "bt6": dict(game=B66, start=[], n_playouts=64, salt=5, again=0),
    "bt8": dict(game=B88, start=B88_MID, n_playouts=32, salt=9, again=0),
    "c4_deep": dict(game=C4, start=SC.c4_late_prefix(3, 20), n_playouts=96, salt=23, again=0),
    "c4_again": dict(game=C4, start=[3, 2], n_playouts=40, salt=7, again=1),
}

# Whole self-play games, 8 slots, 16 games, 48 playouts, kept trees, connect_four: name -> backup and the settings beside FPU.
# cap: (n_fast, p_full); forced: (k, prune); mirror: p; late: games start from SC.c4_late_prefix(seed, empties) and the engine runs
# with max_sims_per_tick large and no chain window, so that playouts chain on the register-cached root.
S, S_FAST, G, N, SEED = 48, 12, 8, 16, 977
GAMES = {
    "soft_z": dict(backup="soft-Z", salt=11),
    "off_policy": dict(backup="off-policy", salt=42),
    "cap": dict(backup="soft-Z", salt=3, cap=(S_FAST, 0.5)),
    "forced": dict(backup="soft-Z", salt=77, forced=(2.0, True)),
    "mirror": dict(backup="soft-Z", salt=5, mirror=0.5),
    "solver": dict(backup="soft-Z", salt=13, solver=True, late=(3, 14)),
    "chained": dict(backup="soft-Z", salt=29, late=(5, 12), eng=dict(max_sims_per_tick=1000, chain_window_us=-1)),
}

_MODEL = {}


def search_model(key, fpu=FPU):
    """The model's searches of SEARCHES[key] -> (game dict of the one ply, [tree_dump after each search]); computed once."""
    if (key, fpu) not in _MODEL:
        c = SEARCHES[key]
        trees = []
        w = play_game(c["game"], c["salt"], None, None, fpu=fpu, n_playouts=c["n_playouts"], use_dirichlet=False,
                      keep_search_tree=True, backup="soft-Z", num_probabilistic_actions=0, start=c["start"], trees=trees,
                      max_searches=1, again=c["again"])
        _MODEL[key, fpu] = (w, trees)
    return _MODEL[key, fpu]


def game_start(c):
    return SC.c4_late_prefix(*c["late"]) if "late" in c else []


def game_settings(key):
    """-> (schedules per game or None, mirrors per game or None) of GAMES[key], from the Python models of the cap's draw and of the
    mirror's coin (tests/test_playout_cap_host.py, tests/eval_mirror_cases.py)."""
    c = GAMES[key]
    p0 = len(game_start(c))
    schedules = mirrors = None
    if "cap" in c:
        from test_playout_cap_host import schedule
        _, mp, _, _ = FC.geometry(C4)
        sched = schedule(SEED, N, mp, c["cap"][1])                      # by game id and ABSOLUTE ply
        schedules = [[(S if sched[i, p0 + t] else c["cap"][0], bool(sched[i, p0 + t])) for t in range(mp - p0)] for i in range(N)]
    if "mirror" in c:
        import eval_mirror_cases as EM
        from alphazero_openspiel_amd import games
        from mirror_cases import action_mirror_table
        table = action_mirror_table(games.load_game(C4))
        mirrors = [((lambda ply, phase, sims, i=i: EM.coin(SEED, i, ply, phase, sims, c["mirror"])), table) for i in range(N)]
    return schedules, mirrors


def game_models(key, fpu=FPU):
    """The model's N games of GAMES[key]; computed once per (case, fpu)."""
    if ("game", key, fpu) not in _MODEL:
        c = GAMES[key]
        etas, us = FC.draws(SEED, C4, N)
        schedules, mirrors = game_settings(key)
        k, prune = c.get("forced", (0.0, False))
        _MODEL["game", key, fpu] = [
            play_game(C4, c["salt"], etas[i], us[i], fpu=fpu, k=k, prune_targets=prune, solver=c.get("solver", False),
                      schedule=None if schedules is None else schedules[i], n_playouts=S, keep_search_tree=True, backup=c["backup"],
                      start=game_start(c), mirror=None if mirrors is None else mirrors[i]) for i in range(N)]
    return _MODEL["game", key, fpu]
