"""The cases of tests/test_forced_playouts_host.py and tests/test_forced_playouts_gpu.py: self-play under the two rules of
az_engine_set_forced_playouts (include/az_engine.h) - forced playouts at the root and policy target pruning - as
tests/search_model.py states them (forced, forced_budget, prune, and select's +infinity).  With k = 0 the model is play_game_self
itself, which tests/test_forced_playouts_host.py pins against the C oracle.  Also here: the geometry of a game string and the
injected draws (etas, us) that every model game of the suite takes, as in tests/test_fuzz_parity_gpu.py.  No test lives here."""
import functools

import numpy as np

import search_model as SM
from oracle import binding as orc

play_game = functools.partial(SM.play_game, fpu=None)


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
