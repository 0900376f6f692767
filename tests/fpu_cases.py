"""The cases of tests/test_fpu_host.py and tests/test_fpu_gpu.py: self-play under the rule of az_engine_set_fpu
(include/az_engine.h) as tests/search_model.py states it: an unvisited child enters the PUCT comparison with Q_eff = -X.Q - f *
sqrt(m), m the butterfly sum of the visited children's priors.  The cases compose the rule with each other setting - forced
playouts with pruning, the solver, a playout cap's schedule, the evaluation mirror, a start prefix.  With fpu=None the model is the
one the older host tests pin to the C oracle.  No test lives here."""
import functools

import forced_playouts_cases as FC
import search_model as SM
import solver_cases as SC
from philox_cases import schedule
from search_model import COUNTERS, UNKNOWN, butterfly   # (the tests read them here)
from search_model import FPU_EFFECTS as EFFECTS

FPU = (0.3, 0.1)                                       # reduction != reduction_root: a mix-up of the two shows
play_game = functools.partial(SM.play_game, fpu=None)


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
    """The model's searches of SEARCHES[key] -> (game dict of the one ply, [tree_dump after each search]); computed once.  The
    model's tree lives on through its searches, so the dump after search r is taken from a run that stops there (again=r)."""
    if (key, fpu) not in _MODEL:
        c = SEARCHES[key]
        runs = [play_game(c["game"], c["salt"], None, None, fpu=fpu, n_playouts=c["n_playouts"], use_dirichlet=False,
                          keep_search_tree=True, backup="soft-Z", num_probabilistic_actions=0, start=c["start"], dumps=True,
                          max_searches=1, again=r) for r in range(1 + c["again"])]
        _MODEL[key, fpu] = (runs[-1], [w["plies"][0]["tree"] for w in runs])
    return _MODEL[key, fpu]


def game_start(c):
    return SC.c4_late_prefix(*c["late"]) if "late" in c else []


def game_settings(key):
    """-> (schedules per game or None, mirrors per game or None) of GAMES[key], from the Python models of the cap's draw and of the
    mirror's coin (tests/philox_cases.py, tests/eval_mirror_cases.py)."""
    c = GAMES[key]
    p0 = len(game_start(c))
    schedules = mirrors = None
    if "cap" in c:
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
