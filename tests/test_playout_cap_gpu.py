"""Playout cap randomisation on the device (az_engine_set_playout_cap, az_engine_full_moves_device, az_replay_append_device_kept
and their Python facade).

References, all bit for bit (there are no tolerances):
  * the schedule: the pure-Python Philox restatement of tests/philox_cases.py;
  * the searches: plain engines (no cap) - with p_full = 1 / 0 the whole generation of a plain engine with n_playouts / n_fast
    playouts; with a mixed schedule and fresh trees, ply by ply, a plain engine whose n_playouts is that ply's count and whose
    game-start table puts game id i at game i's position (a fresh-tree search depends on state, ply, game id, seed and count);
  * the store: tests/replay_cases.FifoModel fed the same games with the fast plies removed.
Comparisons cover the valid part of a record: a game's own plies and children [0, n_children)."""
import functools

import numpy as np
import pytest
import torch

import replay_cases as RC
from alphazero_openspiel_amd import games
from net_cases import drifted_net
from playout_cap_cases import check_store as _check, expect as _expect, reference_games as _reference_games
from playout_cap_cases import same as _same, same_game as _same_game
from philox_cases import is_full, schedule

pytestmark = pytest.mark.gpu

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
S, FAST, G, N = 24, 6, 4, 8
SEED = 701          # both kinds of search within the first 7 plies of every game id below 12 (asserted from the model below)
AZ_E_INVALID, AZ_E_STATE = -1, -3


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _nodes(name, n_playouts=S):
    """A pool that holds every search of a game (no compaction), the same for every engine of a comparison."""
    game = games.load_game(name)
    return game.max_game_length() * (n_playouts + 1) * game.max_children() + 64


def _engine(name, n_slots=G, max_games=N, cap=None, **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", S)
    kw.setdefault("seed", SEED)
    kw.setdefault("nodes_per_slot", _nodes(name))
    eng = E.SelfPlayEngine(name, n_slots, max_games=max_games, device=0, **kw)
    if cap is not None:
        eng.set_playout_cap(*cap)
    return eng


def _play(eng, ev, n=N, **kw):
    from alphazero_openspiel_amd import engine as E
    prog = E.run_selfplay(eng, ev, n, **kw)
    return eng.export(), eng.full_moves_device().cpu().numpy(), prog


def _valid(ex):
    p0 = np.asarray(ex["start_ply"]).reshape(-1, 1)
    ply = np.arange(ex["move"].shape[1])[None, :]
    return (ply >= p0) & (ply < p0 + ex["game_len"].astype(np.int64)[:, None])


def _same_games(got, want, what):
    assert got["game_len"].tolist() == want["game_len"].tolist(), what
    p0 = np.broadcast_to(np.asarray(want["start_ply"]), (len(want["game_len"]),))
    for j in range(len(want["game_len"])):
        _same_game(got, j, want, j, int(p0[j]), "%s: game %d" % (what, j))


def _model_mask(ex, seed, p_full):
    """The schedule's model on the recorded plies of an export: 1 = full search."""
    return schedule(seed, len(ex["game_len"]), ex["move"].shape[1], p_full) * _valid(ex)


def _scheduled_sims(ex, seed, p_full):
    m = _model_mask(ex, seed, p_full)
    return int(m.sum()) * S + int((_valid(ex) & (m == 0)).sum()) * FAST


# ------------------------------------------------------------------------------------------------ 1. the extremes
@pytest.mark.parametrize("keep_tree", [False, True])
@pytest.mark.parametrize("name", [C4, B66])
def test_extremes_are_plain_engines(name, keep_tree):
    """p_full = 1: the generation of a plain engine (records, packed export, playout count), mask all ones on the recorded plies.
    p_full = 0: the generation of a plain engine created with n_playouts = n_fast, mask all zero.  Root noise on."""
    from alphazero_openspiel_amd.engine import unpack_device_export
    kw = dict(keep_search_tree=keep_tree, use_dirichlet=True)
    ev = _fused(name)
    plain = _engine(name, **kw)
    want, mask_plain, prog_plain = _play(plain, ev)
    want_dev = plain.export_device().cpu().numpy()
    plain.close()
    assert mask_plain.dtype == np.uint8 and (mask_plain == _valid(want)).all()        # no cap: every recorded ply gives 1
    full = _engine(name, cap=(FAST, 1.0), **kw)
    got, mask, prog = _play(full, ev)
    got_dev = full.export_device().cpu().numpy()
    full.close()
    _same_games(got, want, "p_full = 1")
    mp, mc = got["move"].shape[1], got["child_action"].shape[2]
    # The packed export: same size, the two whole-generation arrays byte for byte, and every record row of every game.  The rows
    # of plies that were never played are NOT compared: the record arrays come from the device allocator uninitialised and the
    # engine writes a row only when its ply is played, so those bytes are whatever each engine's allocation held (also on the
    # parent commit, between two plain engines).
    assert got_dev.shape == want_dev.shape and got_dev.dtype == np.uint8
    got_x, want_x = unpack_device_export(got_dev, N, mp, mc), unpack_device_export(want_dev, N, mp, mc)
    assert got_x["game_len"].tobytes() == want_x["game_len"].tobytes() and got_x["game_ret0"].tobytes() == want_x["game_ret0"].tobytes()
    _same_games(got_x, want_x, "p_full = 1, packed export")
    assert (mask == _valid(want)).all()
    assert prog["sims"] == prog_plain["sims"] and prog["moves"] == prog_plain["moves"] == int(want["game_len"].sum())
    small = _engine(name, n_playouts=FAST, **kw)
    want0, _, prog_small = _play(small, ev)
    small.close()
    fast = _engine(name, cap=(FAST, 0.0), **kw)
    got0, mask0, prog0 = _play(fast, ev)
    fast.close()
    ev.close()
    _same_games(got0, want0, "p_full = 0")
    assert not mask0.any()
    assert prog0["sims"] == prog_small["sims"] < prog["sims"]


# ------------------------------------------------------------------------------------------------ 2. mixed schedule, fresh trees
def _first_searches(ref, ev, histories):
    """Game id i of the plain engine `ref` (one slot per game) starts after histories[i]; tick until every game has made its first
    move -> the export (records at the games' start plies)."""
    n = len(histories)
    ref.set_game_starts(histories)
    ref.reset(n)
    obs, pri, val = ref.alloc_io()
    start = np.array([len(h) for h in histories])
    for tick in range(40 * S):
        ref.advance(pri, val, obs)
        ev(obs, pri, val)
        if tick >= 4:
            r = ref.read_roots()
            if ((r["ply"][:n] != start) | (r["game_id"][:n] != np.arange(n))).all():
                return ref.export()
    raise AssertionError("the first searches did not finish: %r" % (ref.progress(),))


@pytest.mark.parametrize("name,backup", [(C4, "on-policy"), (B66, "soft-Z")])
def test_mixed_schedule_ply_by_ply_against_plain_engines(name, backup):
    kw = dict(keep_search_tree=False, use_dirichlet=True, backup=backup)
    ev, ev8 = _fused(name), _fused(name, N)
    eng = _engine(name, cap=(FAST, 0.5), **kw)
    ex, mask, prog = _play(eng, ev)
    eng.close()
    model = _model_mask(ex, SEED, 0.5)
    lens = ex["game_len"].tolist()
    for i in range(N):                                                                 # the seed's schedule has both kinds in every game
        kinds = {bool(is_full(SEED, i, t, 0.5)) for t in range(lens[i])}
        assert kinds == {True, False}, "game %d of seed %d has one kind of search only: choose another seed" % (i, SEED)
    assert (mask == model).all()
    assert prog["sims"] == _scheduled_sims(ex, SEED, 0.5)
    checked = 0
    for count, kind in ((S, 1), (FAST, 0)):
        ref = _engine(name, n_slots=N, n_playouts=count, **kw)
        plies = [[t for t in range(lens[i]) if model[i, t] == kind] for i in range(N)]
        for r in range(max(len(p) for p in plies)):
            at = [p[min(r, len(p) - 1)] for p in plies]                                # (a game with fewer such plies repeats its last one)
            got = _first_searches(ref, ev8, [[int(a) for a in ex["move"][i, :at[i]]] for i in range(N)])
            for i, t in enumerate(at):
                what = "game %d, ply %d (%d playouts)" % (i, t, count)
                nc = int(ex["n_children"][i, t])
                assert nc > 0 and int(got["n_children"][i, t]) == nc and got["move"][i, t] == ex["move"][i, t], what
                _same(got["states"][i, t], ex["states"][i, t], what)
                _same(got["child_action"][i, t, :nc], ex["child_action"][i, t, :nc], what)
                _same(got["child_visits"][i, t, :nc], ex["child_visits"][i, t, :nc], what)
                if backup == "soft-Z":
                    assert got["value"][i, t] == ex["value"][i, t], what
                checked += r < len(plies[i])
        ref.close()
    assert checked == int(sum(lens))                                                   # every recorded ply of every game
    ev.close()
    ev8.close()


# ------------------------------------------------------------------------------------------------ 3. kept tree, mixed
def _play_with_tail(eng, ev, n=N):
    """Eager ticks; once every game is handed out and a slot has gone idle, dense request rows (compact_rows / advance_rows)."""
    eng.reset(n)
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
            if p["games_done"] >= n:
                break
            if p["games_started"] >= n and p["slots_idle"] > (0 if rows is None else eng.G - rows):
                rows = eng.compact_rows()
                compactions += 1
    assert compactions >= 1 and rows < eng.G
    return eng.export(), eng.full_moves_device().cpu().numpy(), eng.progress()


def test_kept_tree_schedule_counts_and_the_ways_to_tick():
    kw = dict(keep_search_tree=True, use_dirichlet=True, cap=(FAST, 0.5))
    ev, ev2 = _fused(C4), _fused(C4, 2)
    eng = _engine(C4, **kw)
    want, mask, prog = _play(eng, ev)
    eng.close()
    assert (mask == _model_mask(want, SEED, 0.5)).all() and 0 < mask.sum() < _valid(want).sum()
    assert prog["sims"] == _scheduled_sims(want, SEED, 0.5)                            # a kept tree: the count is what a search ADDS
    runs = {}
    eng = _engine(C4, **kw)
    runs["a 16-tick captured graph"] = _play(eng, ev, use_graph=True, ticks_per_graph=16, check_every=32)
    eng.close()
    eng = _engine(C4, n_slots=2, **kw)
    runs["2 slots"] = _play(eng, ev2)
    eng.close()
    eng = _engine(C4, **kw)
    runs["dense rows in the tail"] = _play_with_tail(eng, ev)
    eng.close()
    for what, (got, m, p) in runs.items():
        _same_games(got, want, what)
        assert (m == mask).all() and p["sims"] == prog["sims"], what
    ev.close()
    ev2.close()


def test_sims_done_counts_the_current_search_from_zero():
    ev = _fused(C4)
    eng = _engine(C4, keep_search_tree=True, use_dirichlet=True, cap=(FAST, 0.5))
    eng.reset(N)
    obs, pri, val = eng.alloc_io()
    seen = {True: 0, False: 0}
    for tick in range(150):
        eng.advance(pri, val, obs)
        ev(obs, pri, val)
        roots = eng.read_roots()
        for g in range(G):
            s = eng.read_slot(g)
            assert int(roots["sims_done"][g]) == s["sims_done"] and int(roots["ply"][g]) == s["ply"]
            if s["game_id"] < 0:
                assert s["sims_done"] == 0
                continue
            full = bool(is_full(SEED, s["game_id"], s["ply"], 0.5))
            count = S if full else FAST
            assert 0 <= s["sims_done"] <= count, (tick, g, s, count)
            if s["phase"] == 2:                                                        # move pending: the search is complete
                assert s["sims_done"] == count
            seen[full] += 0 < s["sims_done"] < count
    assert seen[True] > 0 and seen[False] > 0                                          # both kinds were read mid-search
    eng.close()
    ev.close()


# ------------------------------------------------------------------------------------------------ 4. the store
def _kept(ref_games, mask):
    return [[r for r in g if mask[i, r.ply]] for i, g in enumerate(ref_games)]


def test_store_holds_the_full_search_examples_only():
    """Two generations through append_engine and through export_device + full_moves_device + append_device(keep=).  The first
    starts every game at ply 0 (start_ply_dev == NULL); the second has a game-start table whose game 0 starts 36 plies in and -
    by the schedule of its seed - is searched fast on every ply it can have: a game with no kept ply."""
    from alphazero_openspiel_amd import replay
    game = games.load_game(C4)
    ev = _fused(C4)
    stores = [replay.DeviceReplay(C4, device=0, max_games=40), replay.DeviceReplay(C4, device=0, max_games=40)]
    model = RC.FifoModel(40, 40 * game.max_game_length())
    # generation 1
    eng = _engine(C4, cap=(FAST, 0.5), keep_search_tree=False)
    ex, mask, _ = _play(eng, ev)
    assert (mask == _model_mask(ex, SEED, 0.5)).all()
    stores[0].append_engine(eng)
    ply, keys = eng.game_starts_device()
    assert keys is None and ply.cpu().tolist() == [0] * N
    stores[1].append_device(eng.export_device(), N, start_ply=0, keep=eng.full_moves_device())
    eng.close()
    ref = _kept(RC.reference_games(game, ex), mask)
    assert 0 < sum(len(g) for g in ref) < int(ex["game_len"].sum())
    model.append(ref)
    e = _expect(model)                                                                  # (one pass: it writes the averages back)
    for rep in stores:
        _check(rep, e)
    # generation 2
    seed2 = 1033
    long_prefix = RC.ONE_MOVE_PREFIX[C4]
    assert not any(is_full(seed2, 0, t, 0.5) for t in range(len(long_prefix), game.max_game_length()))
    histories = [long_prefix, [], [3], [3, 2, 4], [4, 2, 3], [], [3, 3, 2, 4], [3]]
    eng = _engine(C4, cap=(FAST, 0.5), keep_search_tree=True, backup="soft-Z", seed=seed2)
    eng.set_game_starts(histories)
    ex, mask, _ = _play(eng, ev)
    assert ex["game_len"][0] >= 1 and not mask[0].any() and (mask == _model_mask(ex, seed2, 0.5)).all()
    stores[0].append_engine(eng)
    ply, keys = eng.game_starts_device()
    stores[1].append_device(eng.export_device(), N, start_ply=ply, keys=keys, keep=eng.full_moves_device())
    eng.close()
    ev.close()
    ref = _kept(_reference_games(game, ex, histories), mask)
    assert ref[0] == [] and sum(1 for g in ref if g) >= 1
    before = model.n_games
    model.append(ref)
    assert model.n_games == before + sum(1 for g in ref if g) < before + N             # a game with no kept ply is skipped
    e = _expect(model)
    for rep in stores:
        _check(rep, e)
    assert len(e["uidx"]) < len(e["flat_z"])                                           # (examples did merge: dedupe was exercised)
    u0, u1 = stores[0].read_unique(), stores[1].read_unique()
    assert all((u0[k] == u1[k]).all() for k in u0)                                     # the 64-bit keys too
    for rep in stores:
        rep.close()


def test_all_ones_mask_is_the_unmasked_append_and_stray_bytes_are_refused():
    from alphazero_openspiel_amd import replay
    game = games.load_game(C4)
    ex = RC.fake_export(game, n_games=6, seed=3, openings=RC.random_openings(game, 3, 3, 7, [3, 2]), start_history=[3, 2])
    buf = torch.from_numpy(RC.pack_device_export(ex)).cuda()
    mp = game.max_game_length()
    starts = torch.full((6,), 2, dtype=torch.int32, device="cuda")
    valid = torch.from_numpy(_valid(ex).astype(np.uint8)).cuda()
    a, b, c = (replay.DeviceReplay(C4, device=0, max_games=12) for _ in range(3))
    a.append_device(buf, 6, start_ply=starts)                                          # az_replay_append_device_starts
    b.append_device(buf, 6, start_ply=starts, keep=valid)                              # all ones on the games' rows
    c.append_device(buf, 6, start_ply=2, keep=valid)
    n = a.dedupe()
    assert b.dedupe() == n and c.dedupe() == n
    ua = a.read_unique()
    for rep in (b, c):
        u = rep.read_unique()
        assert all(u[k].dtype == ua[k].dtype and u[k].tobytes() == ua[k].tobytes() for k in ua)
        assert rep.stats() == a.stats()
        for i in range(a.stats()["n_examples"]):
            (pa, za), (pr, zr) = a.read_example(i), rep.read_example(i)
            assert pa.tobytes() == pr.tobytes() and za == zr
    # a keep byte outside a game's rows: refused before any kernel runs, the store is unchanged
    g = int(np.argmin(ex["game_len"]))
    for t in (1, 2 + int(ex["game_len"][g])):
        bad = valid.clone()
        bad[g, t] = 1
        before = b.stats()
        with pytest.raises(RuntimeError, match=r"\(%d\).*keep byte at game %d, ply %d" % (AZ_E_INVALID, g, t)):
            b.append_device(buf, 6, start_ply=starts, keep=bad)
        assert b.stats() == before
    with pytest.raises(RuntimeError, match="uint8"):
        b.append_device(buf, 6, start_ply=starts, keep=valid[:, :mp - 1].contiguous())
    for rep in (a, b, c):
        rep.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    for what, eng in (("arena", _engine(C4, arena_agent="zero", opponent="random")),
                      ("manual_moves", _engine(C4, manual_moves=True)),
                      ("stream", _engine(C4))):
        if what == "stream":
            eng.stream_begin()
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_playout_cap is for plain self-play.*%s" % (AZ_E_INVALID, what)):
            eng.set_playout_cap(FAST, 0.5)
        assert eng.playout_cap is None
        eng.close()
    eng = _engine(C4)
    for n_fast in (S + 1, -1, 1 << 20):
        with pytest.raises(E.EngineError, match=r"\(%d\).*n_fast must be in \[1, n_playouts = %d\]" % (AZ_E_INVALID, S)):
            eng.set_playout_cap(n_fast, 0.5)
    for p_full in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(E.EngineError, match=r"\(%d\).*p_full must be in \[0, 1\]" % AZ_E_INVALID):
            eng.set_playout_cap(FAST, p_full)
    eng.set_playout_cap(1, 0.0)                                                        # root Dirichlet expansion: one playout is enough
    eng.set_playout_cap(S, 1.0)
    assert eng.playout_cap == (S, 1.0)
    obs, pri, val = eng.alloc_io()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):                   # the caller resets after setting a cap
        eng.advance(pri, val, obs)
    with pytest.raises(E.EngineError, match=r"az_engine_stream_begin.*playout cap"):
        eng.stream_begin()
    eng.reset(4)
    assert eng.full_moves_device().shape == (4, eng.max_plies) and not eng.full_moves_device().any()   # nothing recorded yet
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_INVALID):
        eng.full_moves_device(N + 1)
    eng.set_playout_cap(0)                                                             # clears it
    assert eng.playout_cap is None
    eng.stream_begin()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):
        eng.full_moves_device(4)
    eng.close()
    bare = _engine(C4, use_dirichlet=False)
    with pytest.raises(E.EngineError, match=r"\(%d\).*>= 2 without root Dirichlet" % AZ_E_INVALID):
        bare.set_playout_cap(1, 0.5)
    bare.set_playout_cap(2, 0.5)
    bare.close()


# ------------------------------------------------------------------------------------------------ 6. facade
def test_example_generator_returns_the_full_search_examples():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd import replay
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", n_playouts=S, n_slots=G, seed=5, use_graph=False, playout_cap=(FAST, 0.5))
    out = gen.generate_examples(N)
    eng = E.SelfPlayEngine(C4, G, n_playouts=S, max_games=N, device=0, seed=5)         # the generator's first generation
    eng.set_playout_cap(FAST, 0.5)
    ev = _fused(C4)
    ex, mask, _ = _play(eng, ev)
    eng.close()
    ev.close()
    want = E.examples_from_export(eng.game, ex, keep=mask)
    assert len(out) == len(want) == N
    n_all = int(ex["game_len"].sum())
    assert 0 < sum(len(g) for g in out) == int(mask.sum()) < n_all
    for i, (got_g, want_g) in enumerate(zip(out, want)):
        assert len(got_g) == len(want_g)
        for a, b in zip(got_g, want_g):
            assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2] and a[3] == b[3]
            ply = len(a[0].split(", ")) if a[0] else 0
            assert is_full(5, i, ply, 0.5)                                             # a full-search example, by the model
    rep = replay.DeviceReplay(C4, 40, device=0)
    assert gen.generate_into(rep, N) == N                                              # the kept path (append_engine with the mask)
    st = rep.stats()
    assert 0 < st["n_examples"] < gen.last_progress["moves"] and st["n_games"] <= N and st["fault_flags"] == 0
    assert rep.dedupe() > 0 and rep.stats()["fault_flags"] == 0
    rep.close()
    gen.close()
