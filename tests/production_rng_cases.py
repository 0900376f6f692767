"""Shared pieces of the production-RNG tests (tests/test_production_rng_gpu.py, tests/test_production_rng_host.py); no GPU here.

Production mode (AZ_RNG_PHILOX) draws two things on the device: the move uniform - the first philox_u01 of the stream (seed,
game id, ply, purpose 1, index 0), which the Python Philox of tests/philox_cases.py models bit for bit - and the root
noise, gamma draws behind the stream (seed, game id, ply, purpose 0, index = child) made with hardware approximations, which no
host model reproduces.  So the noise is READ BACK (SelfPlayEngine.read_root_noise) and everything downstream of it is exact."""
import numpy as np

from philox_cases import cap_uniform   # the one Python Philox of the suite

from oracle import fakepolicy

ALPHA = 0.3   # the literal of mcts.py:187
N_LAW = 2048  # draws per law position: the same position under this many game ids


def move_uniform(seed, game_id, ply, purpose=1):
    """The uniform behind np.random.choice of game `game_id` at absolute ply `ply` (move_step, purpose 1)."""
    return cap_uniform(seed, game_id, ply, purpose=purpose)


def cached_policy(num_actions, salt):
    """oracle.fakepolicy.fake_eval of a board, memoised on the board's bytes: engine and oracle ask about the same positions."""
    memo = {}

    def fn(board):
        key = fakepolicy.board_key(board)
        if key not in memo:
            memo[key] = fakepolicy.fake_eval(board, num_actions, salt)
        return memo[key]
    return fn


def record_and_play(engine, evaluator, n_games, max_ticks=200000):
    """Play n_games on a reset Philox engine, tick by tick (advance + evaluator); after every tick the noise row of every slot
    in phase 3 is read back.  -> (etas, export, progress): etas[game_id][ply] = the LIST of rows read for that root (one each,
    which the caller asserts), rows float64 [max_children]."""
    obs, pri, val = engine.alloc_io()
    etas = {}
    for _ in range(max_ticks):
        engine.advance(pri, val, obs)
        for g in range(engine.G):
            info = engine.read_slot(g)
            if info["phase"] == 3:
                etas.setdefault(info["game_id"], {}).setdefault(info["ply"], []).append(engine.read_root_noise(g))
        evaluator(obs, pri, val)
        if engine.progress()["games_done"] >= n_games:
            break
    else:
        raise AssertionError("games did not finish")
    return etas, engine.export(), engine.progress()


# ------------------------------------------------------------------------------------------------ positions of the law tests
_C4_SIX = [0] * 6 + [1] * 6 + [4] + [2] * 6 + [3] * 6 + [4] * 5 + [5] * 6   # column pairs x o x o x o / o x o x o x: no four anywhere
BT54 = "breakthrough(rows=5,columns=4)"
BT66 = "breakthrough(rows=6,columns=6)"
# (label, game, prefix, number of legal moves): every prefix is replayed by the games module in the host test
LAW_POSITIONS = [
    ("c4_three_full_columns", "connect_four", [0] * 6 + [1] * 6 + [2] * 6, 4),
    ("c4_six_full_columns", "connect_four", _C4_SIX, 1),
    ("bt6_two_captures", BT66, [74, 308, 149, 299], 16),                      # one pawn of each side captured: lanes without a piece
    ("bt8_initial", "breakthrough(rows=8,columns=8)", [], 22),
    ("bt54_late_3", BT54, [86, 179, 72, 155, 60, 234, 98, 176, 16, 162, 77, 115, 24, 127, 38, 211], 3),
    ("bt54_late_2", BT54, [52, 178, 12, 162, 77, 202, 36, 107, 5, 155, 73, 210, 50, 163, 61, 186, 109, 226, 85], 2),
]
# keying: pairs of positions of the SAME ply with different numbers of legal moves
KEY_PAIRS = [
    ("connect_four", [0] * 6 + [1] * 6 + [2] * 6, 4, _C4_SIX[:18], 5),       # ply 18: children are columns 3.. / columns 2..
    (BT54, [76, 152, 62, 200, 26, 176], 6, [84, 188, 52, 162, 61, 139], 15),  # ply 6
]


def ks_components(n):
    """The components the KS test looks at: the first, a middle and the last one."""
    return sorted({0, n // 2, n - 1})


N_KS_TESTS = sum(len(ks_components(n)) for _, _, _, n in LAW_POSITIONS if n >= 2)
KS_P_BAR = 1e-3 / N_KS_TESTS   # the existing single test's bar, shared out over this file's KS tests


def check_dirichlet_law(etas, n_legal, alpha=ALPHA, p_bar=KS_P_BAR):
    """etas [N, >= n_legal]: are the first n_legal entries of the rows N draws of Dirichlet(alpha * ones(n_legal))?  Raises
    AssertionError naming the check.  Bars: the KS p-value bar above; variance 0.01 and covariance 0.004 absolute, those of
    test_philox_dirichlet_noise_has_the_right_law; and two this file derives -
      component means: each is a mean of N draws of variance v = (1/n)(1 - 1/n)/(n alpha + 1): within 5 sqrt(v / N) of 1/n
        (5 sigma per component, n <= 22 components: a false alarm in 1e5 runs);
      corr(e_0, e_1) = -1/(n - 1) exactly for a symmetric Dirichlet; a sample correlation of N = 2048 pairs has standard error
        about 1/sqrt(N) = 0.022 for normal data, more for these skewed ones: the bar is 0.2, nine such standard errors; two
        components that share a draw give +1."""
    from scipy import stats
    e = np.asarray(etas, dtype=np.float64)[:, :n_legal]
    N, n = e.shape
    assert n == n_legal and N >= 1000, e.shape
    assert np.isfinite(e).all(), "a component is not finite"
    assert (e > 0.0).all(), "a component is not positive"
    assert np.abs(e.sum(1) - 1.0).max() <= 1e-12, "rows do not sum to 1: %r" % np.abs(e.sum(1) - 1.0).max()
    if n == 1:   # nothing left to test: the row is its sum.  (np.random.dirichlet itself returns x * (1 / x), which is 1 - 2^-53 for
        return   # some x; the GPU test asks the engine for 1.0 exactly on its own account.)
    for comp in ks_components(n):
        d, pval = stats.kstest(e[:, comp], "beta", args=(alpha, alpha * (n - 1)))
        assert pval > p_bar, "KS of component %d against Beta(%g, %g): D = %.4f, p = %.3g" % (comp, alpha, alpha * (n - 1), d, pval)
    v = (1.0 / n) * (1.0 - 1.0 / n) / (n * alpha + 1.0)
    dev = np.abs(e.mean(0) - 1.0 / n).max()
    assert dev < 5.0 * np.sqrt(v / N), "a component's mean is %.4f from 1/n (bar %.4f)" % (dev, 5.0 * np.sqrt(v / N))
    assert abs(e.var(0).mean() - v) < 0.01, "variance %.5f, expected %.5f" % (e.var(0).mean(), v)
    cov = np.cov(e[:, 0], e[:, 1])[0, 1]
    assert abs(cov + (1.0 / n ** 2) / (n * alpha + 1.0)) < 0.004, "cov(e0, e1) = %.5f" % cov
    corr = np.corrcoef(e[:, 0], e[:, 1])[0, 1]
    assert abs(corr + 1.0 / (n - 1)) < 0.2, "corr(e0, e1) = %.3f, expected %.3f" % (corr, -1.0 / (n - 1))
