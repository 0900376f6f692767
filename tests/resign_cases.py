"""The cases of tests/test_resign_host.py and tests/test_resign_gpu.py: self-play resignation (az_engine_set_resign,
include/az_engine.h) stated on the games of tests/search_model.py, which stays as it is - resignation does not change a search, it
cuts a game, so the expectation is read off the plain model's games:

  * the value target does not influence play, so play_game with backup="soft-Z" and with backup="A0C" plays the same moves, and
    their value columns are the two expressions of the criterion: crit[t] = max(softz[t], a0c[t]);
  * ply t qualifies when t - start >= min_ply and (under a playout cap) its search was a full one; the LAST ply of a game never
    counts: the move that ends the game lets its result stand, the criterion is not looked at;
  * the resign ply is the first qualifying t with crit[t] < -v; low[p] is the minimum of crit over player p's qualifying plies;
  * the game plays through iff the first uniform of the Philox stream (seed, game id, ply 0, purpose 6, index 0) is below
    p_playthrough (tests/philox_cases.py).

4 slots, 8 games, 24 playouts (6 for a fast move), the hashed policy of oracle.fakepolicy, injected draws.  V per case is a
constant chosen on the CPU from these very games; tests/test_resign_host.py asserts what the GPU tests rely on.  No test lives
here."""
import functools

import numpy as np

import search_model as SM
from forced_playouts_cases import draws
from philox_cases import cap_uniform, is_full

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
S, FAST, G, N = 24, 6, 4, 8
CAP = (FAST, 0.5)
INF = float("inf")

# seed: the engine's - the coins and the cap's schedule are drawn from it.  v: the hashed policy knows nothing, so its searches'
# values stay near 0 and the criterion - the larger of two estimates - rarely drops below -0.1: thresholds of a few hundredths
# split the eight games of a case as the tests need (tests/test_resign_host.py asserts it).
CASES = {
    "c4": dict(game=C4, salt=11, draws=31, seed=701, v=0.05, cap=None, kw=dict(keep_search_tree=True)),
    "b66": dict(game=B66, salt=5, draws=32, seed=701, v=0.035, cap=None, kw=dict(keep_search_tree=False)),
    "c4_cap": dict(game=C4, salt=42, draws=33, seed=705, v=0.03, cap=CAP, kw=dict(keep_search_tree=True)),
}


def schedules(case, starts=None):
    """Per game the per-ply-played list of (playouts, is_full) under the case's cap; None without one."""
    c = CASES[case]
    if c["cap"] is None:
        return None
    mp = len(draws(c["draws"], c["game"], 1)[1][0])
    out = []
    for i in range(N):
        p0 = 0 if starts is None else len(starts[i])
        kinds = [bool(is_full(c["seed"], i, t, c["cap"][1])) for t in range(p0, mp)]
        out.append([(S if f else c["cap"][0], f) for f in kinds])
    return out


@functools.lru_cache(maxsize=None)
def model_games(case, backup):
    """The plain model's N games of a case under one value target (computed once, shared)."""
    c = CASES[case]
    etas, us = draws(c["draws"], c["game"], N)
    sch = schedules(case)
    return [SM.play_game(c["game"], c["salt"], etas[i], us[i], n_playouts=S, backup=backup,
                         schedule=None if sch is None else sch[i], **c["kw"]) for i in range(N)]


def crit_of(softz, a0c):
    """Per game the criterion per ply played, from the two value columns."""
    return [[max(a, b) for a, b in zip(gs, ga)] for gs, ga in zip(softz, a0c)]


def model_crit(case):
    return crit_of([[p["value"] for p in g["plies"]] for g in model_games(case, "soft-Z")],
                   [[p["value"] for p in g["plies"]] for g in model_games(case, "A0C")])


def qualifying(n_plies, start=0, min_ply=0, full=None):
    """The plies played (0-based from the game's start) at which the criterion counts; full: per ply played, None = all."""
    return [j for j in range(n_plies - 1) if j >= min_ply and (full is None or full[j])]


def expect(crit, v, start=0, min_ply=0, full=None):
    """One game -> (resign ply as an ABSOLUTE ply or -1, low [2] by player)."""
    ply, low = -1, [INF, INF]
    for j in qualifying(len(crit), start, min_ply, full):
        t = start + j
        low[t & 1] = min(low[t & 1], crit[j])
        if ply < 0 and crit[j] < -v:
            ply = t
    return ply, low


def plays_through(seed, game_id, p):
    return cap_uniform(seed, game_id, 0, purpose=6, idx=0) < p


def resign_ret0(ply):
    """The result of a game resigned at absolute ply `ply`: a loss for the player to move there."""
    return -1.0 if ply % 2 == 0 else 1.0


def expected_games(case, v=None, p=0.0, min_ply=0):
    """Per game of the case: dict(ply, low, through, resigned, length, ret0) under threshold v (default the case's)."""
    c = CASES[case]
    v = c["v"] if v is None else v
    sch = schedules(case)
    games_ = model_games(case, "soft-Z")
    out = []
    for i, (g, cr) in enumerate(zip(games_, model_crit(case))):
        full = None if sch is None else [f for _, f in sch[i]]
        ply, low = expect(cr, v, 0, min_ply, full)
        through = ply >= 0 and plays_through(c["seed"], i, p)
        resigned = ply >= 0 and not through
        if resigned:                                  # the game is cut right there: later plies lower nothing
            _, low = expect(cr[:ply + 2], v, 0, min_ply, full)
        out.append(dict(ply=ply, low=low, through=through, resigned=resigned, length=ply + 1 if resigned else len(cr),
                        ret0=resign_ret0(ply) if resigned else g["ret0"]))
    return out
