"""The search model of tests/search_model.py against recorded results: tests/search_model_pins.json holds one sha256 per game (or
search) of every cached helper of the four case modules, recorded from the three separate models (forced_playouts_cases,
solver_cases, fpu_cases) and the arena agent as they stood before they were merged into search_model.py.  Where the C oracle
cannot speak - forcing and pruning on, the solver on, first-play urgency on, an arena agent under a setting - these digests are
what says that the one model still computes what the separate ones computed.  Floats enter a digest by their bit pattern."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import arena_match_cases as AM
import eval_mirror_cases as EM
import forced_playouts_cases as FC
import fpu_cases as F
import search_model as SM
import solver_cases as SC
from alphazero_openspiel_amd import games
from mirror_cases import action_mirror_table
from philox_cases import schedule

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "search_model_pins.json")) as _f:
    PINS = json.load(_f)

COUNTERS = ("sims", "evals", "terminal_hits", "sum_depth", "sum_children")
PLY_KEYS = ("raw", "recorded", "actions", "move", "ran", "status", "full")
STEP_KEYS = ("raw", "counts", "child_status", "ran", "move", "status", "kept_status")


def _feed(h, x):
    """x into the hash with its type: ints and None as text, floats as the eight bytes of the double, sequences by element."""
    if isinstance(x, (bool, np.bool_)):
        h.update(b"b%d" % int(x))
    elif isinstance(x, (int, np.integer)):
        h.update(b"i%d;" % int(x))
    elif isinstance(x, (float, np.floating)):
        h.update(b"f" + struct.pack("<d", float(x)))
    elif x is None:
        h.update(b"n")
    else:
        h.update(b"[")
        for y in x:
            _feed(h, y)
        h.update(b"]")


def _feed_game(h, w):
    _feed(h, w["actions"])
    _feed(h, w["ret0"])
    _feed(h, [w["counters"][k] for k in COUNTERS] if "counters" in w else None)   # (an arena game carries its agents' steps instead)
    for p in w.get("plies", ()):
        _feed(h, [p[k] for k in PLY_KEYS])
        _feed(h, p["pi"])
        _feed(h, p["value"])


def _feed_dump(h, d):
    for k in ("parent", "action", "N", "status", "Q", "P"):                     # the first four are integer arrays
        _feed(h, d[k].tolist())


def _feed_steps(h, agent):
    for s in agent.steps:
        _feed(h, [s[k] for k in STEP_KEYS])


def digest(w, dumps=(), agents=()):
    h = hashlib.sha256()
    _feed_game(h, w)
    for d in dumps:
        _feed_dump(h, d)
    for a in agents:
        _feed_steps(h, a)
    return h.hexdigest()


def _ply_dumps(w):
    return [p[k] for p in w["plies"] for k in ("tree", "kept") if p.get(k) is not None]


# ------------------------------------------------------------------------------------------------ what is pinned
def _forced_schedules(idx):
    """The playout cap of tests/test_forced_playouts_gpu.py, test_mixed_schedule_equals_the_model."""
    case = FC.CASES[idx]
    mp = FC.geometry(case["game"])[1]
    sched = schedule(701, case["n_games"], mp, 0.5)
    return [[(FC.S if sched[i, t] else FC.S_FAST, bool(sched[i, t])) for t in range(mp)] for i in range(case["n_games"])]


def _solver_settings(idx):
    """The cap and the mirror coins of tests/test_solver_gpu.py, test_with_a_playout_cap_and_eval_mirror_the_engine_equals_the_model."""
    case = SC.CASES[idx]
    n, p0 = case["n_games"], len(SC.case_start(case))
    mp = FC.geometry(case["game"])[1]
    sched = schedule(811, n, mp, 0.5)
    per_game = [[(SC.S if sched[i, p0 + t] else SC.S_FAST, bool(sched[i, p0 + t])) for t in range(mp - p0)] for i in range(n)]
    table = action_mirror_table(games.load_game(case["game"]))
    mirrors = [((lambda ply, phase, sims, i=i: EM.coin(811, i, ply, phase, sims, 0.5)), table) for i in range(n)]
    return per_game, mirrors


def _games(ws):
    return lambda: [digest(w) for w in ws()]


def _feeds(x):
    h = hashlib.sha256()
    _feed(h, x)
    return h.hexdigest()


def _forced_table():
    """The forcing rule on hand-made children, among them n * n == (k * P) * N exactly, which no game of the cases meets."""
    out = []
    for N, n, P, k in ((4, 2, 0.5, 2.0), (4, 1, 0.5, 2.0), (4, 3, 0.5, 2.0), (9, 3, 0.5, 2.0), (8, 0, 0.9, 2.0), (16, 4, 0.25, 4.0),
                       (16, 3, 0.25, 4.0), (16, 5, 0.25, 4.0), (100, 10, 0.5, 2.0), (100, 10, 0.1, 2.0)):
        parent = SM.Node(None, 0.0, True)
        parent.N = N
        child = SM.Node(parent, P, True)
        child.N = n
        out.append(bool(SM.forced(child, k)))
    return out


def _q_eff_table():
    """q_eff on hand-made nodes whose visited priors sum to another double left to right than through the butterfly: the games
    of the cases meet such sums, but a last-bit change of Q_eff flips no selection in them."""
    r = np.random.RandomState(11)
    out = []
    for priors in ([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], r.dirichlet(np.ones(20)).tolist(), r.dirichlet(0.3 * np.ones(48)).tolist()):
        node = SM.Node(None, 0.0, True)
        node.Q, node.N = 0.37, len(priors)
        for i, p in enumerate(priors):
            child = SM.Node(node, p, True)
            child.N = int(i % 5 != 3)                                            # every fifth child unvisited
            node.actions.append(i)
            node.children.append(child)
        out.extend(SM.q_eff(node, f) for f in (0.3, 0.1, 1.0))
    return out


def _groups():
    """name -> a function that returns the digests of that helper's games, in order."""
    g = {"rules/forced": lambda: [_feeds(_forced_table())], "rules/q_eff": lambda: [_feeds(_q_eff_table())]}
    for idx in range(len(FC.CASES)):
        for k in (0.0, FC.K):
            g["forced/%d/k%g" % (idx, k)] = _games(lambda idx=idx, k=k: FC.model_games(idx, k))
        g["forced/%d/cap" % idx] = _games(lambda idx=idx: FC.model_games(idx, FC.K, _forced_schedules(idx)))
    for idx in range(len(SC.CASES)):
        for solver in (False, True):
            g["solver/%d/%s" % (idx, "on" if solver else "off")] = _games(lambda idx=idx, solver=solver: SC.model_games(idx, solver))
        g["solver/%d/cap" % idx] = _games(lambda idx=idx: SC.model_games(idx, True, schedules=_solver_settings(idx)[0]))
        g["solver/%d/cap+mirror" % idx] = _games(lambda idx=idx: SC.model_games(idx, True, schedules=_solver_settings(idx)[0],
                                                                                mirrors=_solver_settings(idx)[1]))
    for solver in (False, True):
        on = "on" if solver else "off"
        for key in SC.SCALE_CASES:
            g["scale/%s/%s" % (key, on)] = lambda key=key, solver=solver: [
                digest(w, _ply_dumps(w)) for w in [SC.scale_model(key, solver)]]
        for key in SC.DEEP_CASES:
            g["deep/%s/%s" % (key, on)] = lambda key=key, solver=solver: [
                digest(w, _ply_dumps(w)) for w in [SC.deep_model(key, solver)]]
        g["deep_game/%s" % on] = _games(lambda solver=solver: [SC.deep_game_model(solver)])
    for key in SC.GAME_CASES:
        g["scale_games/%s" % key] = _games(lambda key=key: SC.game_models(key))
    for fpu in (F.FPU, None):
        on = "on" if fpu else "off"
        for key in F.SEARCHES:
            g["fpu_search/%s/%s" % (key, on)] = lambda key=key, fpu=fpu: [digest(F.search_model(key, fpu)[0], F.search_model(key, fpu)[1])]
        for key in F.GAMES:
            g["fpu_games/%s/%s" % (key, on)] = _games(lambda key=key, fpu=fpu: F.game_models(key, fpu))
    for key in AM.ARENA:
        for setting in AM.SETTINGS:
            g["arena/%s/%s" % (key, setting)] = lambda key=key, setting=setting: [
                digest(w, agents=[w["agent"]]) for w in AM.arena_models(key, setting)]
    g["arena_solver"] = lambda: [digest(w, agents=[w["agent"]]) for w in AM.solver_models()]
    for key in AM.DUEL:
        g["duel/%s" % key] = lambda key=key: [digest(w, agents=[w["a"], w["b"]]) for w in AM.duel_models(key)]
    return g


GROUPS = _groups()


def test_every_group_is_pinned_and_nothing_else():
    assert sorted(GROUPS) == sorted({name.rsplit("#", 1)[0] for name in PINS})
    assert all(isinstance(v, str) and len(v) == 64 for v in PINS.values())


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_the_model_computes_what_the_separate_models_computed(name):
    got = GROUPS[name]()
    want = [PINS["%s#%d" % (name, i)] for i in range(sum(1 for k in PINS if k.rsplit("#", 1)[0] == name))]
    assert len(got) == len(want), name
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s#%d" % (name, i)
