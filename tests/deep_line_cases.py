"""Shared by test_deep_lines_host.py, test_deep_lines_gpu.py and oracle/gen_golden.py: a stand-in evaluator whose searches
run DEEP, and the cases that carry a select path across the lane/register boundaries of the tick kernel (depth 64, 128, and
the largest game the engine accepts).

oracle/fakepolicy.fake_eval is a softmax of hashed logits in [-2, 2]: PUCT spreads its playouts and the deepest one of a
60-190 playout search is 5-9 plies below the root.  line_eval instead puts (almost) all prior mass on ONE legal action a* of
every position, so every playout follows the chain of a* and expands one node more: depth grows by one per playout until the
line meets the end of the game, and from then on the +-1 of the terminal leaf is backed up the whole line.

    board (C+1,H,W) -> position, rebuilt from the planes alone with the cell-array rules of oracle/pygames.py
    a*     = by rule of the board (below), ties broken by fnv1a64(board) ^ salt
    logits = 0 at a*, -L elsewhere (illegal actions included); priors = softmax_f32(logits), float32 like Net.forward
    value  = float32(vs * (2 * u01(splitmix64(h ^ VSALT)) - 1))

L = 12: a* keeps 1 - (A - 1) e^-12 > 0.995 of the mass for A <= 768, and every other prior is e^-12 / sum ~ 6.1e-6, a normal
float32 (no prior of a legal move is 0, subnormal or NaN).

The rule for a*: breakthrough - any legal move, picked by the hash (the salt decides how long the line lasts: the cases' salts
are picked so that it ends inside the playout budget, past depth 64 / 128).  connect_four - a column of the lowest height,
which fills the board evenly; the cases' salt gives a line that ends in the ply-42 draw."""
import numpy as np

from oracle import binding as orc
from oracle import fakepolicy, pygames

L = 12.0

# key -> game, playouts of the one search, salt, value scale vs, and (one case) the root noise vector of the search.  The salts
# were picked on the CPU so that test_deep_lines_host.py's conditions hold (DESIGN_HISTORY.md has the measured depths).  No
# salt in 1..400 makes a ROOT branch on its own - the side that loses the line deviates a few plies above the terminal leaf,
# where N is small, long before the root's Q moves - so the connect_four case searches with root noise: a given vector that
# puts P = 0.025 on two other columns, which then get a visit or two beside the line's 55+.
CASES = {
    "bt26x2": dict(game="breakthrough(rows=26,columns=2)", n_playouts=190, salt=13, vs=0.01, eta=None),
    "bt12x5": dict(game="breakthrough(rows=12,columns=5)", n_playouts=120, salt=28, vs=0.0, eta=None),
    "bt8x8": dict(game="breakthrough(rows=8,columns=8)", n_playouts=90, salt=15, vs=0.01, eta=None),
    "c4": dict(game="connect_four", n_playouts=60, salt=17, vs=0.01, eta=[0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.1]),
}
SHORT_SALT = 9   # the flat policy's salt (policy(game, SHORT_SALT, 1.0, L=0)): the shallow games of the neighbouring-slots test


def _position(game, board):
    """(C+1,H,W) planes -> a pygames state with that position and side to move (history contents are not recoverable and not
    needed: the rules below read the cells and the parity of the ply only)."""
    b = np.asarray(board)
    st = game.new_initial_state()
    cells = np.argmax(b[:3], axis=0)                                   # the plane index IS the cell value (pygames.py)
    player = int(b[3, 0, 0]) & 1
    st._board = [[int(v) for v in row] for row in cells]
    st._history = [0] * player
    if isinstance(st, pygames.BreakthroughState):
        st._pieces = [int(b[0].sum()), int(b[1].sum())]
    return st, player


def choose(game, board, salt):
    """-> (a*, legal actions) of the position the planes show; (None, []) for planes that show no position with a move (the
    all-zero rows of an engine's request buffer before its first request)."""
    b = np.asarray(board)
    if not (b[:3].sum(axis=0) == 1).all():
        return None, []
    st, player = _position(game, b)
    legal = st.legal_actions()
    if not legal:
        return None, []
    h = fakepolicy._fnv1a64(fakepolicy.board_key(b)) ^ (salt & fakepolicy._M64)
    if isinstance(st, pygames.BreakthroughState):
        cand = legal
    else:
        height = [sum(1 for r in range(game.ROWS) if st._board[r][c] != 0) for c in range(game.COLS)]
        low = min(height[c] for c in legal)
        cand = [c for c in legal if height[c] == low]
    return cand[fakepolicy._splitmix64(h) % len(cand)], legal


def line_eval(game, board, num_actions, salt, vs, L=L):
    """-> (priors float32[A], value float32).  L = 0 is the flat policy: uniform priors, under which a search stays shallow."""
    a, _ = choose(game, board, salt) if L else (0, None)
    if a is None:
        return np.full(num_actions, np.float32(1.0 / num_actions), dtype=np.float32), np.float32(0.0)
    lg = np.full(num_actions, -L, dtype=np.float32)
    lg[a] = 0.0
    e = np.exp(lg - lg.max(), dtype=np.float32)
    pri = (e / e.sum(dtype=np.float32)).astype(np.float32)
    h = fakepolicy._fnv1a64(fakepolicy.board_key(board)) ^ (salt & fakepolicy._M64)
    val = np.float32(vs * (2.0 * fakepolicy._u01(fakepolicy._splitmix64(h ^ fakepolicy._VSALT)) - 1.0))
    return pri, val


_MEMO = {}


def policy(game_name, salt, vs, L=L):
    """board -> (priors, value), memoised by board key: the oracle's run and the engine's share their evaluations (and a
    HostPolicyEvaluator asks for every row again each tick)."""
    memo = _MEMO.setdefault((game_name, salt, vs, L), {})
    game = pygames.load_game(game_name)
    A = game.num_distinct_actions()
    shape = (4, game.ROWS, game.COLS)                                  # (the oracle hands its board over flat)

    def fn(board):
        key = fakepolicy.board_key(board)
        got = memo.get(key)
        if got is None:
            got = memo[key] = line_eval(game, np.asarray(board).reshape(shape), A, salt, vs, L)
        return got

    return fn


def case_policy(key):
    c = CASES[key]
    return policy(c["game"], c["salt"], c["vs"])


def principal_line(game_name, salt):
    """The chain of a* from the initial position to the end of the game -> list of actions."""
    game = pygames.load_game(game_name)
    shape = game.information_state_normalized_vector_shape()
    st, out = game.new_initial_state(), []
    while not st.is_terminal():
        planes = np.array(st.information_state_as_normalized_vector(), dtype=np.float64).reshape(shape)
        board = np.concatenate([planes, np.full((1,) + tuple(shape[1:]), float(st.current_player()))])
        a, legal = choose(game, board, salt)
        assert a in legal and legal == st.legal_actions()
        out.append(a)
        st.apply_action(a)
    return out


def oracle_search(key, use_puct=True):
    """The case's one search from the initial position with the C oracle, playout by playout -> (MCTS, state, depth of every
    playout, depths of those that ended on a terminal node)."""
    c = CASES[key]
    m = orc.MCTS(case_policy(key), c["game"], n_playouts=c["n_playouts"], use_dirichlet=c["eta"] is not None, use_puct=use_puct)
    s = orc.State(c["game"])
    if c["eta"] is not None:
        m.expand_root_dirichlet(s, c["eta"])
    depths, terminal = [], []
    prev = m.counters()
    for _ in range(c["n_playouts"]):
        m.playout(s)
        cur = m.counters()
        depths.append(cur["sum_depth"] - prev["sum_depth"])
        if cur["terminal_hits"] > prev["terminal_hits"]:
            terminal.append(depths[-1])
        prev = cur
    return m, s, depths, terminal


def most_visited(root):
    """The root child update_root descends to: the most visited one, the first maximum (None for a leaf root)."""
    return root["actions"][int(np.argmax(root["cN"]))] if root["actions"] else None


def oracle_descent(m):
    """Descend the principal line of a searched oracle tree with update_root -> [(action, root statistics after it)], down to
    and including the leaf root the line ends in."""
    out = []
    while True:
        a = most_visited(m.root_stats())
        if a is None:
            return out
        m.update_root(a)
        out.append((a, m.root_stats()))
