"""Evaluation in a random left-right orientation on the device (az_engine_set_eval_mirror, az_engine_read_request_mirror and
their Python facade).

The reference, bit for bit (there are no tolerances), is an engine WITHOUT the setting under a wrapping evaluator that mirrors
the rows itself (tests/eval_mirror_cases.py): all rows for p_mirror = 1, and for p_mirror = 0.5 the rows the pure-Python coin
model picks from read_slot() after each eager tick.  An engine with the setting runs under the bare net.  Comparisons cover the
valid part of a record: a game's own plies and children [0, n_children).

Every test here calls set_eval_mirror (or passes eval_mirror=), which the library lacks before this feature."""
import functools

import numpy as np
import pytest
import torch

import eval_mirror_cases as EM
from alphazero_openspiel_amd import games
from analysis_positions import random_positions
from eval_mirror_cases import B66, C4, G, N, S, SEED
from net_cases import drifted_net
from playout_cap_cases import same_game as _same_game

pytestmark = pytest.mark.gpu

AZ_E_INVALID, AZ_E_STATE = -1, -3
KEYS = ("game_len", "game_ret0", "states", "move", "n_children", "child_action", "child_visits", "value")
FAST, P_FULL, FORCED_K = 6, 0.5, 2.0


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _engine(name, n_slots=G, max_games=N, mirror=None, cap=None, forced=None, **kw):
    """use_dirichlet and keep_search_tree default to on; a pool that holds every search of a game (no compaction)."""
    from alphazero_openspiel_amd import engine as E
    game = games.load_game(name)
    kw.setdefault("nodes_per_slot", game.max_game_length() * (S + 1) * game.max_children() + 64)
    eng = E.SelfPlayEngine(name, n_slots, n_playouts=S, seed=SEED, max_games=max_games, device=0, **kw)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if forced is not None:
        eng.set_forced_playouts(forced)
    if mirror is not None:
        eng.set_eval_mirror(mirror)
    return eng


def _frozen(ex):
    for k in KEYS:
        ex[k].setflags(write=False)
    return ex


def _play(eng, ev, **kw):
    from alphazero_openspiel_amd import engine as E
    prog = E.run_selfplay(eng, ev, N, **kw)
    assert prog["games_done"] == N and prog["error_flags"] == 0
    return eng.export()


def _same_games(got, want, what, first=0):
    """Games [0, n) of `got` are games [first, first + n) of `want`."""
    n = len(got["game_len"])
    assert got["game_len"].tolist() == want["game_len"][first:first + n].tolist(), what
    for j in range(n):
        _same_game(got, j, want, first + j, 0, "%s: game %d" % (what, first + j))


@functools.lru_cache(maxsize=None)
def _bare(name, keep_tree=True):
    """The plain engine under the bare net.  Computed once; read-only."""
    eng, ev = _engine(name, keep_search_tree=keep_tree), _fused(name)
    ex = _play(eng, ev)
    eng.close()
    ev.close()
    return _frozen(ex)


@functools.lru_cache(maxsize=None)
def _reference(name, **setting):
    """Case 2's reference: the plain engine (with `setting`: a cap, forcing) under the model-driven wrapper, p_mirror = 0.5.
    Computed once per case; read-only."""
    eng, ev = _engine(name, **setting), _fused(name)
    ex = EM.play_model_driven(eng, EM.MirrorWrapper(ev, eng.game), N, SEED, 0.5)
    assert eng.progress()["error_flags"] == 0
    eng.close()
    ev.close()
    return _frozen(ex)


# ------------------------------------------------------------------------------------------------ 1. every request mirrored
@pytest.mark.parametrize("keep_tree", [False, True])
@pytest.mark.parametrize("name", [C4, B66])
def test_p_mirror_one_is_the_plain_engine_under_the_all_rows_wrapper(name, keep_tree):
    ev = _fused(name)
    eng = _engine(name, mirror=1.0, keep_search_tree=keep_tree)
    assert eng.eval_mirror == 1.0
    got = _play(eng, ev)
    eng.close()
    plain = _engine(name, keep_search_tree=keep_tree)
    want = _play(plain, EM.MirrorWrapper(ev, plain.game))                 # rows = None: every row
    plain.close()
    ev.close()
    _same_games(got, want, "p_mirror = 1")
    assert EM.exports_differ(got, _bare(name, keep_tree)), "the net is left-right symmetric on these games: the test shows nothing"


# ------------------------------------------------------------------------------------------------ 2. a coin per request
@pytest.mark.parametrize("name", [C4, B66])
def test_p_mirror_half_is_the_plain_engine_under_the_model_driven_wrapper(name):
    ev = _fused(name)
    eng = _engine(name, mirror=0.5)
    eng.reset(N)
    obs, pri, val = eng.alloc_io()
    seen, first_game_live = {0: 0, 1: 0}, True
    for tick in range(200000):
        eng.advance(pri, val, obs)
        if first_game_live:                                               # every tick of the first game: the read-back against the model
            infos = [eng.read_slot(g) for g in range(G)]
            for g, info in enumerate(infos):
                if info["phase"] in (EM.PH_WAIT_ROOT, EM.PH_WAIT_LEAF):
                    bit = eng.read_request_mirror(g)
                    assert bit == int(EM.slot_coin(SEED, info, 0.5)), (tick, g, info)
                    seen[bit] += 1
            first_game_live = any(info["game_id"] == 0 for info in infos)
        ev(obs, pri, val)
        if tick % 8 == 7 and eng.games_done() >= N:
            break
    got = eng.export()
    assert eng.progress()["error_flags"] == 0
    eng.close()
    ev.close()
    assert not first_game_live and seen[0] > S and seen[1] > S            # both orientations, many times over
    _same_games(got, _reference(name), "p_mirror = 0.5")
    assert EM.exports_differ(got, _bare(name))


# ------------------------------------------------------------------------------------------------ 3. cleared again
def test_p_mirror_zero_after_a_setting_is_an_engine_that_was_never_set():
    ev = _fused(C4)
    eng = _engine(C4, mirror=0.5)
    eng.set_eval_mirror(0.0)
    assert eng.eval_mirror is None
    got = _play(eng, ev)
    eng.reset(N)                                                          # (a request is outstanding after the first tick)
    obs, pri, val = eng.alloc_io()
    eng.advance(pri, val, obs)
    assert eng.read_slot(0)["phase"] == EM.PH_WAIT_ROOT and eng.read_request_mirror(0) == 0   # no setting in force: 0
    eng.close()
    ev.close()
    _same_games(got, _bare(C4), "p_mirror = 0 after 0.5")


# ------------------------------------------------------------------------------------------------ 4. tail rows and graphs
def _play_with_tail(eng, ev):
    """Eager ticks; once every game is handed out and a slot has gone idle, dense request rows (compact_rows / advance_rows)."""
    eng.reset(N)
    obs, pri, val = eng.alloc_io()
    rows, compactions = None, 0
    for tick in range(200000):
        if rows is None:
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        else:
            eng.advance_rows(rows, pri, val, obs)
            ev(obs[:rows], pri[:rows], val[:rows])
        if tick % 8 == 7:
            p = eng.progress()
            if p["games_done"] >= N:
                break
            if p["games_started"] >= N and p["slots_idle"] > (0 if rows is None else eng.G - rows):
                rows = eng.compact_rows()
                compactions += 1
    assert compactions >= 1 and rows < eng.G
    return eng.export()


@pytest.mark.parametrize("how", ["dense rows in the tail", "a 16-tick captured graph"])
def test_tail_rows_and_graph_replays_play_the_same_games(how):
    ev = _fused(C4)
    eng = _engine(C4, mirror=0.5)
    if how.startswith("dense"):
        got = _play_with_tail(eng, ev)
    else:
        got = _play(eng, ev, use_graph=True, ticks_per_graph=16, check_every=32)
    assert eng.progress()["error_flags"] == 0
    eng.close()
    ev.close()
    _same_games(got, _reference(C4), how)


# ------------------------------------------------------------------------------------------------ 5. stream
def test_stream_delivers_the_closed_generation_across_a_ring_wrap():
    from alphazero_openspiel_amd import engine as E
    ref = _reference(C4)
    ev = _fused(C4)
    eng = _engine(C4, max_games=6)                                        # a ring of 6 rows: ids 6 and 7 record into rows 0 and 1
    stream = E.SelfPlayStream(eng, ev, use_graph=False, eval_mirror=0.5)
    assert eng.eval_mirror == 0.5
    try:
        firsts = []
        for n in (3, 3, 2):
            buf, first = stream.take(n, max_ticks=200000)
            ex = E.unpack_device_export(buf.cpu().numpy(), n, eng.max_plies, eng.max_children)
            firsts.append(first)
            _same_games({k: ex[k].copy() for k in KEYS}, ref, "stream take at id %d" % first, first)
        assert firsts == [0, 3, 6] and eng.progress()["error_flags"] == 0
    finally:
        stream.close()
        E.close_all(eng, ev)


# ------------------------------------------------------------------------------------------------ 6. slot groups
def test_two_slot_groups_on_two_streams_play_the_same_games():
    groups = [(0, 2), (2, 2)]
    evs = [_fused(C4, 2), _fused(C4, 2)]
    eng = _engine(C4, mirror=0.5)
    eng.reset(N)
    obs, pri, val = eng.alloc_io()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream("cuda:0") for _ in groups]
    for tick in range(200000):
        for (first, n), st, ev in zip(groups, streams, evs):
            with torch.cuda.stream(st):
                eng.advance_slots(first, n, pri, val, obs)
                ev(obs[first:first + n], pri[first:first + n], val[first:first + n])
        if tick % 8 == 7:
            for st in streams:
                st.synchronize()
            if eng.games_done() >= N:
                break
    got = eng.export()
    assert eng.progress()["error_flags"] == 0
    eng.close()
    for ev in evs:
        ev.close()
    _same_games(got, _reference(C4), "two slot groups")


# ------------------------------------------------------------------------------------------------ 7. composition
def test_composes_with_a_playout_cap_and_forced_playouts():
    """The leaf coin's index is the sims_done read_slot reports, which counts a fast search from 0 too."""
    ev = _fused(C4)
    eng = _engine(C4, mirror=0.5, cap=(FAST, P_FULL), forced=FORCED_K)
    got = _play(eng, ev)
    mask = eng.full_moves_device().cpu().numpy()
    eng.close()
    ev.close()
    v = EM.valid(got)
    assert 0 < mask[v].sum() < v.sum()                                    # both kinds of search were played
    _same_games(got, _reference(C4, cap=(FAST, P_FULL), forced=FORCED_K), "cap + forced playouts + p_mirror = 0.5")
    assert EM.exports_differ(got, _reference(C4))                         # (and the cap and the forcing did act)


# ------------------------------------------------------------------------------------------------ 8. manual_moves
@pytest.mark.parametrize("name", [C4, B66])
def test_analysis_with_every_request_mirrored(name):
    from alphazero_openspiel_amd import analysis
    positions = random_positions(name, 8, seed=17, min_ply=2, max_ply=12)
    kw = dict(n_playouts=S, use_dirichlet=True, seed=SEED)
    got = analysis.analyze_positions(_net(name), name, positions, eval_mirror=1.0, **kw)
    bare = analysis.analyze_positions(_net(name), name, positions, **kw)
    ev = _fused(name, 8)
    an = analysis.Analyzer(None, name, 8, **kw)
    an.evaluator = EM.MirrorWrapper(ev, an.engine.game)                   # the plain analysis under the all-rows wrapper
    try:
        an.load(analysis.position_prefixes(name, positions), seed=SEED)
        an.search()
        want = an.results()
    finally:
        an.close()
        ev.close()
    for k in ("visits", "q", "priors", "root_q", "root_n", "best_action"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["progress"]["error_flags"] == 0 and int(got["root_n"].min()) >= S
    assert got["priors"].tobytes() != bare["priors"].tobytes() and got["visits"].tobytes() != bare["visits"].tobytes()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    arena = _engine(C4, arena_agent="zero", opponent="random")
    with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_eval_mirror.*refused for an arena engine" % AZ_E_INVALID):
        arena.set_eval_mirror(0.5)
    assert arena.eval_mirror is None
    arena.close()
    eng = _engine(C4)
    for p in (float("nan"), -0.01, 1.01, float("inf")):
        with pytest.raises(E.EngineError, match=r"\(%d\).*p_mirror must be finite and in \[0, 1\]" % AZ_E_INVALID):
            eng.set_eval_mirror(p)
    assert eng.eval_mirror is None
    eng.set_eval_mirror(1.0)
    eng.set_eval_mirror(0.5)
    obs, pri, val = eng.alloc_io()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):      # the caller resets after the setting
        eng.advance(pri, val, obs)
    with pytest.raises(E.EngineError, match=r"\(%d\).*before az_engine_reset" % AZ_E_STATE):
        eng.read_request_mirror(0)
    eng.reset(2)                                                          # slots 0 and 1 play, slots 2 and 3 stay idle
    for slot in (-1, G, 1 << 20):
        with pytest.raises(E.EngineError, match=r"\(%d\).*slot %d is outside \[0, n_slots = %d\)" % (AZ_E_INVALID, slot, G)):
            eng.read_request_mirror(slot)
    with pytest.raises(E.EngineError, match=r"\(%d\).*no request outstanding" % AZ_E_STATE):
        eng.read_request_mirror(0)                                        # before the first tick: no request yet
    eng.advance(pri, val, obs)
    assert eng.read_slot(0)["phase"] == EM.PH_WAIT_ROOT
    assert eng.read_request_mirror(0) == int(EM.coin(SEED, 0, 0, EM.PH_WAIT_ROOT, 0, 0.5))
    with pytest.raises(E.EngineError, match=r"\(%d\).*no request outstanding \(phase 0" % AZ_E_STATE):
        eng.read_request_mirror(G - 1)                                    # an idle slot
    prog = eng.progress()
    assert prog["error_flags"] == 0
    eng.close()
    manual = _engine(C4, manual_moves=True)                               # analysis and reanalyse engines take the setting
    manual.set_eval_mirror(0.5)
    assert manual.eval_mirror == 0.5
    manual.close()
