"""Stream mode of the self-play engine (az_engine_stream_begin / _ready / _take_device, engine.SelfPlayStream): continuous
self-play over a record store used as a ring.

A game depends on (seed, game id, network) alone, so what a stream hands over, in id order, must be the closed generation of
the same seed cut into pieces - bit for bit, whatever the ring's size, the drain schedule, or whether the ticks are replayed
from a captured graph.  The closed generation (az_engine_reset + az_engine_export, the code path that existed before stream
mode) is the reference throughout.  Comparisons cover the valid part of a record: plies [0, len) and children
[0, n_children); what lies beyond is unspecified on both paths."""
import functools

import numpy as np
import pytest
import torch

from alphazero_openspiel_amd import games
from net_cases import drifted_net

pytestmark = pytest.mark.gpu

S, G, SEED = 16, 64, 4242
KEYS = ("game_len", "game_ret0", "states", "move", "n_children", "child_action", "child_visits", "value")


@functools.lru_cache(maxsize=None)
def _net(which):
    return drifted_net([3, 6, 7], 7, 1, 50, seed={"A": 31, "B": 32}[which])


def _fused(which):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(which), "cuda:0", max_boards=G, precision="f32x")


def _engine(max_games, backup="on-policy", **kw):
    from alphazero_openspiel_amd import engine as E
    return E.SelfPlayEngine("connect_four", G, n_playouts=S, max_games=max_games, device=0, seed=SEED, backup=backup, **kw)


@functools.lru_cache(maxsize=None)
def _reference(which, backup, n_games):
    """A closed generation of n_games games, read back with az_engine_export.  Computed once per case; read-only."""
    from alphazero_openspiel_amd import engine as E
    eng, fn = _engine(n_games, backup), _fused(which)
    prog = E.run_selfplay(eng, fn, n_games, use_graph=True)
    assert prog["games_done"] == n_games and prog["error_flags"] == 0
    ex = eng.export()
    eng.close()
    fn.close()
    for k in KEYS:
        ex[k].setflags(write=False)
    return ex


def _unpack(eng, buf, n):
    from alphazero_openspiel_amd import engine as E
    ex = E.unpack_device_export(buf.cpu().numpy(), n, eng.max_plies, eng.max_children)
    return {k: ex[k].copy() for k in KEYS}


def _concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def _assert_games_equal(got, ref, first=0):
    """got's games equal ref's games [first, first + n) on the valid part of every array."""
    n = len(got["game_len"])
    sl = slice(first, first + n)
    assert n > 0 and first + n <= len(ref["game_len"])
    assert (got["game_len"] == ref["game_len"][sl]).all() and (got["game_len"] >= 7).all()
    assert (got["game_ret0"] == ref["game_ret0"][sl]).all()
    played = np.arange(got["move"].shape[1])[None, :] < got["game_len"][:, None]
    assert (got["n_children"][played] == ref["n_children"][sl][played]).all()
    kids = played[:, :, None] & (np.arange(got["child_action"].shape[2])[None, None, :] < got["n_children"][:, :, None])
    for k in ("states", "move", "value"):
        assert (got[k][played] == ref[k][sl][played]).all(), k
    for k in ("child_action", "child_visits"):
        assert (got[k][kids] == ref[k][sl][kids]).all(), k


def _drain(stream, chunk, total):
    """Take `total` games in chunks -> (list of unpacked chunks, list of first ids)."""
    parts, firsts = [], []
    for _ in range(total // chunk):
        buf, first = stream.take(chunk, max_ticks=200000)
        parts.append(_unpack(stream.engine, buf, chunk))
        firsts.append(first)
    return parts, firsts


def _open(which, max_games, backup="on-policy", **stream_kw):
    from alphazero_openspiel_amd import engine as E
    eng, fn = _engine(max_games, backup), _fused(which)
    stream_kw.setdefault("use_graph", False)
    return E.SelfPlayStream(eng, fn, **stream_kw), eng, fn


def _close(stream, eng, *evaluators):
    from alphazero_openspiel_amd import engine as E
    stream.close()
    E.close_all(eng, *evaluators)


@pytest.mark.parametrize("backup", ["on-policy", "soft-Z"])
def test_stream_equals_the_closed_generation_with_the_ring_wrapping_inside_takes(backup):
    """576 games through a ring of 128 rows in takes of 48 (128 is no multiple of 48: takes straddle the wrap, the ring is
    used more than four times over) equal the first 576 games of a closed generation of 600.  soft-Z: the value targets are
    written at move time, into the ring row; on-policy: they are formed by the take kernel."""
    ref = _reference("A", backup, 600)
    stream, eng, fn = _open("A", 128, backup)
    try:
        parts, firsts = _drain(stream, 48, 576)
        prog = eng.progress()
    finally:
        _close(stream, eng, fn)
    assert firsts == list(range(0, 576, 48))
    for part, first in zip(parts, firsts):
        _assert_games_equal(part, ref, first)
    assert prog["error_flags"] == 0 and prog["games_done"] >= 576 and prog["games_started"] <= 576 + 128


def test_full_stall_and_resume():
    """A ring as small as the slot count: every slot stalls once its first game is finished, nothing moves until the take, then
    the slots come back by themselves and play ids 64..127 - none skipped, none doubled."""
    ref = _reference("A", "on-policy", 600)
    stream, eng, fn = _open("A", G)
    try:
        for _ in range(400):
            stream.driver.run(32)
            if eng.stream_ready() == G:
                break
        assert eng.stream_ready() == G
        stalled = eng.progress()
        assert stalled["slots_idle"] == G and stalled["games_done"] == G and stalled["games_started"] == G
        stream.driver.run(64)
        assert eng.progress() == stalled and eng.stream_ready() == G
        buf, first = stream.take(G)
        assert first == 0
        _assert_games_equal(_unpack(eng, buf, G), ref, 0)
        buf, first = stream.take(G, max_ticks=200000)
        assert first == G
        _assert_games_equal(_unpack(eng, buf, G), ref, G)
        prog = eng.progress()
        assert prog["error_flags"] == 0 and prog["games_done"] == 2 * G and prog["games_started"] == 2 * G
    finally:
        _close(stream, eng, fn)


def test_drain_schedule_does_not_change_the_games():
    """The same 240 games taken as 5 x 48 and as 240 x 1 (ring of 256 rows)."""
    out = []
    for chunk in (48, 1):
        stream, eng, fn = _open("A", 256)
        try:
            parts, firsts = _drain(stream, chunk, 240)
        finally:
            _close(stream, eng, fn)
        assert firsts == list(range(0, 240, chunk))
        out.append(_concat(parts))
    _assert_games_equal(out[1], out[0])
    _assert_games_equal(out[0], _reference("A", "on-policy", 600))


def test_ticks_replayed_from_a_captured_graph():
    """The first 192 games with the ticks replayed from a graph of 16 (takes and limit raises run between replays) equal
    the eagerly ticked stream's."""
    out = []
    for use_graph in (False, True):
        stream, eng, fn = _open("A", 128, use_graph=use_graph, ticks_per_graph=16)
        try:
            assert (stream.driver.graph is not None) == use_graph
            parts, firsts = _drain(stream, 48, 192)
            assert eng.progress()["error_flags"] == 0
        finally:
            _close(stream, eng, fn)
        assert firsts == [0, 48, 96, 144]
        out.append(_concat(parts))
    _assert_games_equal(out[1], out[0])
    _assert_games_equal(out[1], _reference("A", "on-policy", 600))


def _assert_legal_and_visits_conserved(ex):
    """Every game replays through the host rules, and every recorded root holds the search's visits: S below the root of a
    game's first search, S + max(N_chosen - 1, 0) after a move into a child with N_chosen visits (the kept subtree) - the
    checks of tests/test_full_size_gpu.py, which hold whichever network answered the requests."""
    game = games.load_game("connect_four")
    for g in range(len(ex["game_len"])):
        n = int(ex["game_len"][g])
        assert 7 <= n <= 42
        s = game.new_initial_state()
        prev = None
        for i in range(n):
            assert [int(x) for x in ex["states"][g, i]] == list(s.bb)
            legal = s.legal_actions()
            nc = int(ex["n_children"][g, i])
            assert ex["child_action"][g, i, :nc].tolist() == legal
            visits = ex["child_visits"][g, i, :nc].astype(np.int64)
            assert int(visits.sum()) == (S if prev is None else S + max(prev - 1, 0))
            a = int(ex["move"][g, i])
            assert a in legal and visits[legal.index(a)] > 0
            prev = int(visits[legal.index(a)])
            s.apply_action(a)
        assert s.is_terminal()
        ret0 = s.returns()[0]
        assert float(ex["game_ret0"][g]) == ret0
        assert (ex["value"][g, :n] == np.where(np.arange(n) % 2 == 0, ret0, -ret0)).all()


def test_net_swap_between_takes():
    """Net A for the first 64 games, then set_evaluator(B): the games in flight go on under B with their trees (legal, visits
    conserved, no fault), and nothing of A is left in a stream that starts with B."""
    ref_a = _reference("A", "on-policy", 600)
    stream, eng, fn_a = _open("A", 256, use_graph=True)
    fn_b = None
    try:
        buf, first = stream.take(64, max_ticks=200000)
        assert first == 0
        _assert_games_equal(_unpack(eng, buf, 64), ref_a, 0)
        fn_b = _fused("B")
        stream.set_evaluator(fn_b)
        fn_a.close()
        buf, first = stream.take(192, max_ticks=200000)
        assert first == 64
        after = _unpack(eng, buf, 192)
        assert eng.progress()["error_flags"] == 0
    finally:
        _close(stream, eng, fn_b)
    _assert_legal_and_visits_conserved(after)
    stream, eng, fn = _open("B", 256, use_graph=True)
    try:
        buf, first = stream.take(64, max_ticks=200000)
        got = _unpack(eng, buf, 64)
    finally:
        _close(stream, eng, fn)
    assert first == 0
    _assert_games_equal(got, _reference("B", "on-policy", 64), 0)
    assert not (got["game_len"] == ref_a["game_len"][:64]).all() or not (got["move"][:, :7] == ref_a["move"][:64, :7]).all()


def test_refusals_name_their_reason_and_fault_nothing():
    from alphazero_openspiel_amd import engine as E, replay
    for kw, word in (({"arena_agent": "zero", "opponent": "random", "use_dirichlet": False}, "arena"),
                     ({"manual_moves": True}, "manual_moves"), ({"rng": "injected"}, "INJECTED")):
        eng = E.SelfPlayEngine("connect_four", 8, n_playouts=8, max_games=8, device=0, **kw)
        with pytest.raises(E.EngineError, match=word):
            eng.stream_begin()
        eng.close()
    eng = _engine(16)
    with pytest.raises(E.EngineError, match="max_games < n_slots"):
        eng.stream_begin()
    with pytest.raises(E.EngineError, match="az_engine_stream_begin first"):
        eng.stream_ready()
    eng.close()

    stream, eng, fn = _open("A", 128)
    rep = replay.DeviceReplay("connect_four", max_games=64, device=0)
    try:
        obs, pri, val = stream.obs, stream.pri, stream.val
        for call in (eng.export_device, eng.export, eng.compact_rows, lambda: eng.advance_slots(0, 32, pri, val, obs),
                     lambda: eng.advance_rows(G, pri, val, obs)):
            with pytest.raises(E.EngineError, match="stream mode"):
                call()
        with pytest.raises(RuntimeError, match="stream mode"):
            rep.append_engine(eng)
        assert eng.stream_ready() == 0
        with pytest.raises(E.EngineError, match="were ready"):
            eng.stream_take(5)
        for _ in range(400):
            stream.driver.run(32)
            if eng.stream_ready() >= 2:
                break
        ready = eng.stream_ready()
        assert ready >= 2
        with pytest.raises(E.EngineError, match="were ready"):
            eng.stream_take(ready + 1)
        with pytest.raises(E.EngineError, match="smaller than"):
            eng.stream_take(1, out=torch.empty(eng.stream_take_bytes(1) - 16, dtype=torch.uint8, device="cuda:0"))
        with pytest.raises(E.EngineError):
            eng.stream_take(129)
        assert eng.stream_ready() == ready and eng.progress()["error_flags"] == 0  # the refused takes took nothing
        # back to a closed generation on the same engine
        torch.cuda.synchronize()
        prog = E.run_selfplay(eng, fn, 64, seed=SEED, use_graph=False)
        assert prog["games_done"] == 64 and prog["error_flags"] == 0
        got = _unpack(eng, eng.export_device(), 64)
        with pytest.raises(E.EngineError, match="az_engine_stream_begin first"):
            eng.stream_take(1)
    finally:
        rep.close()
        _close(stream, eng, fn)
    _assert_games_equal(got, _reference("A", "on-policy", 600), 0)


def test_takes_go_into_the_replay_store_like_an_export():
    """Two consecutive takes of 48 appended with az_replay_append_device give the store that the closed generation's first 96
    games give through az_engine_export_device + az_replay_append_device."""
    from alphazero_openspiel_amd import engine as E, replay
    eng, fn = _engine(96), _fused("A")
    want = replay.DeviceReplay("connect_four", max_games=96, device=0)
    got = replay.DeviceReplay("connect_four", max_games=96, device=0)
    try:
        assert E.run_selfplay(eng, fn, 96, use_graph=False)["games_done"] == 96
        want.append_device(eng.export_device(), 96)
        torch.cuda.synchronize()
    finally:
        E.close_all(eng, fn)
    stream, eng, fn = _open("A", 128)
    try:
        for first_want in (0, 48):
            buf, first = stream.take(48, max_ticks=200000)
            assert first == first_want and buf.numel() == E.device_export_layout(48, eng.max_plies, eng.max_children)[1]
            got.append_device(buf, 48)
        torch.cuda.synchronize()
    finally:
        _close(stream, eng, fn)
    try:
        a, b = want.stats(), got.stats()
        assert a == b and a["n_games"] == 96 and a["n_examples"] == int(_reference("A", "on-policy", 600)["game_len"][:96].sum())
        for idx in (0, 1, 7, a["n_examples"] // 2, a["n_examples"] - 1):
            (pi_a, z_a), (pi_b, z_b) = want.read_example(idx), got.read_example(idx)
            assert (pi_a == pi_b).all() and z_a == z_b and abs(pi_a.sum() - 1) < 1e-12
    finally:
        want.close()
        got.close()
