"""Self-play from per-game start positions (az_engine_set_game_starts / _device, az_engine_game_starts_device,
az_replay_gather_forks, az_replay_append_device_starts and their Python facade).

References: a game depends on (seed, game id, network) alone, so the single-prefix engine (az_engine_set_start_prefix, the code
path that existed before) is the reference for the games, bit for bit; tests/replay_cases.FifoModel - the Python restatement
of the reference buffer, keyed on history strings built as prefix + moves - is the reference for what the store must hold.
There are no tolerances.  Comparisons cover the valid part of a record: a game's own plies and children [0, n_children)."""
import functools

import numpy as np
import pytest
import torch

import reanalyse_cases as RA
import replay_cases as RC
from alphazero_openspiel_amd import games
from net_cases import drifted_net
from test_game_starts_host import _chain
from test_replay_store_gpu import _check, _expect, _same

pytestmark = pytest.mark.gpu

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
S, G, SEED = 16, 4, 777
KEYS = ("states", "move", "n_children", "value")
AZ_E_INVALID = -1


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _engine(name, n_slots=G, max_games=12, **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", S)
    kw.setdefault("seed", SEED)
    return E.SelfPlayEngine(name, n_slots, max_games=max_games, device=0, **kw)


def _replay(name, **kw):
    from alphazero_openspiel_amd import replay
    return replay.DeviceReplay(name, device=0, **kw)


def _prefixes(name):
    """Four prefixes of length 0, 1, 3, 4."""
    if name == C4:
        return [[], [3], [3, 2, 4], [3, 3, 2, 4]]
    game = games.load_game(name)
    return [[]] + [RC.random_openings(game, 1, d, 50 + d)[0] for d in (1, 3, 4)]


def _play(eng, ev, n):
    from alphazero_openspiel_amd import engine as E
    E.run_selfplay(eng, ev, n)
    return eng.export()


def _same_game(got, j, want, k, p0, what):
    """Game j of export `got` equals game k of export `want`: lengths, results, and every record row of the game's plies."""
    n = int(want["game_len"][k])
    assert n > 0 and int(got["game_len"][j]) == n, what
    assert got["game_ret0"][j] == want["game_ret0"][k], what
    rows = slice(p0, p0 + n)
    for key in KEYS:
        _same(got[key][j, rows], want[key][k, rows], "%s: %s" % (what, key))
    live = np.arange(got["child_action"].shape[2])[None, :] < want["n_children"][k, rows][:, None]
    for key in ("child_action", "child_visits"):
        _same(got[key][j, rows][live], want[key][k, rows][live], "%s: %s" % (what, key))


def _tensors(bb, ply):
    return torch.from_numpy(bb.view(np.int64)).cuda(), torch.from_numpy(ply).cuda()


# ------------------------------------------------------------------------------------------------ 1. identity, game for game
@pytest.mark.parametrize("search", ["dirichlet", "kept-uct-tree"])
@pytest.mark.parametrize("backup", ["on-policy", "soft-Z"])
@pytest.mark.parametrize("name", [C4, B66])
def test_every_game_is_the_game_of_the_single_prefix_engine(name, backup, search):
    """12 games on 4 slots (8 ids are taken mid-run), prefixes cycling over lengths 0, 1, 3, 4: game j is, bit for bit, game j of
    a plain engine started with set_start_prefix(prefix of j) and the same seed.  kept-uct-tree: the rule of a game's first
    tree depends on ITS start ply (PUCT at ply 0, select_rule from ply 1 on)."""
    kw = dict(backup=backup, use_dirichlet=True) if search == "dirichlet" else \
        dict(backup=backup, use_dirichlet=False, keep_search_tree=True, use_puct=False)
    prefixes, n = _prefixes(name), 12
    histories = [prefixes[j % 4] for j in range(n)]
    ev = _fused(name)
    eng = _engine(name, **kw)
    eng.set_game_starts(histories)
    got = _play(eng, ev, n)
    eng.close()
    assert got["start_ply"].dtype == np.int32 and got["start_ply"].tolist() == [len(h) for h in histories]
    for q, prefix in enumerate(prefixes):
        ref = _engine(name, **kw)
        ref.set_start_prefix(prefix)
        want = _play(ref, ev, n)
        ref.close()
        assert want["start_ply"] == len(prefix)
        for j in range(q, n, 4):
            _same_game(got, j, want, j, len(prefix), "game %d (prefix %r)" % (j, prefix))
    ev.close()


# ------------------------------------------------------------------------------------------------ 2. device form = prefix form
@pytest.mark.parametrize("name", [C4, B66])
def test_device_form_plays_the_games_of_the_prefix_form(name):
    game = games.load_game(name)
    prefixes, n = _prefixes(name), 12
    histories = [prefixes[(j + 1) % 4] for j in range(n)]
    ev = _fused(name)
    a = _engine(name)
    a.set_game_starts(histories)
    want = _play(a, ev, n)
    ply_a, keys_a = a.game_starts_device()
    b = _engine(name)
    bb, ply = RA.states_of(game, histories)
    b.set_game_starts_device(*_tensors(bb, ply), keys=None)
    got = _play(b, ev, n)
    ply_b, keys_b = b.game_starts_device()
    assert ply_a.dtype == ply_b.dtype == torch.int32
    assert ply_a.cpu().tolist() == ply_b.cpu().tolist() == ply.tolist() == got["start_ply"].tolist()
    assert keys_b is None and tuple(keys_a.shape) == (n, 2) and keys_a.dtype == torch.int64   # only the prefix form gives pairs
    k = keys_a.cpu().numpy()
    assert (k[0::4] == k[0]).all() and len({tuple(r) for r in k.tolist()}) == 4                # one pair per distinct prefix
    # the host replay of the prefix form: the pair of an ordinary game from the initial position after these moves (the Python
    # restatement of the chain in tests/test_game_starts_host.py, which that file pins to the shared header)
    assert [tuple(r) for r in k.view(np.uint64).tolist()] == [_chain(game, [], h)[1] for h in histories]
    for j in range(n):
        _same_game(got, j, want, j, len(histories[j]), "game %d" % j)
    # with no table: the uniform values of the engine's one start
    c = _engine(name)
    c.set_start_prefix(prefixes[2])
    c.reset(5)
    ply_c, keys_c = c.game_starts_device()
    assert ply_c.cpu().tolist() == [3] * 5 and keys_c is None
    for e in (a, b, c, ev):
        e.close()


# ------------------------------------------------------------------------------------------------ 3. store parity
def _reference_games(game, ex, histories):
    """examples_from_export with a history per game, every example carrying its bitboards and absolute ply (RC.reference_games)."""
    from alphazero_openspiel_amd.engine import examples_from_export
    out = []
    for g, plies in enumerate(examples_from_export(game, ex, histories)):
        p0, recs = len(histories[g]), []
        for i, item in enumerate(plies):
            r = RC.Rec(item)
            r.bb, r.ply = ex["states"][g, p0 + i].copy(), p0 + i
            recs.append(r)
        out.append(recs)
    return out


def test_store_holds_what_the_reference_buffer_holds():
    """16 connect_four games over a prefix set with a shared prefix (first examples merge), a transposing pair (same position
    and ply, different strings: two entries, no collision fault) and the empty prefix, through append_engine and through
    export_device + game_starts_device + append_device; a second generation on top covers the write-back aliasing."""
    game = games.load_game(C4)
    pool = [[3, 2, 4], [4, 2, 3], [], [3, 2, 4], [3], [3, 3, 2, 4], [], [4, 2, 3]]
    assert (RA.states_of(game, [pool[0]])[0] == RA.states_of(game, [pool[1]])[0]).all()       # a true transposition
    n = 16
    histories = [pool[j % len(pool)] for j in range(n)]
    ev = _fused(C4, 8)
    stores = [_replay(C4, max_games=40), _replay(C4, max_games=40)]
    model = RC.FifoModel(40, 40 * game.max_game_length())
    for gen in range(2):
        eng = _engine(C4, n_slots=8, max_games=n, seed=SEED + gen, backup="on-policy" if gen == 0 else "soft-Z")
        eng.set_game_starts(histories)
        ex = _play(eng, ev, n)
        stores[0].append_engine(eng)
        ply, keys = eng.game_starts_device()
        stores[1].append_device(eng.export_device(), n, start_ply=ply, keys=keys)
        eng.close()
        ref = _reference_games(game, ex, histories)
        assert [g[0][0] for g in ref] == [", ".join(map(str, h)) for h in histories]
        model.append(ref)
        e = _expect(model)
        for rep in stores:
            _check(rep, e)                                                                      # (fault_flags == 0 is part of it)
        firsts = [r for r in model.flat() if r[0] in ("3, 2, 4", "4, 2, 3")]
        uniq = [model.flat()[i][0] for i in e["uidx"]]
        assert len(firsts) >= 4 * (gen + 1) and uniq.count("3, 2, 4") == 1 and uniq.count("4, 2, 3") == 1
        assert len(e["uidx"]) < len(e["flat_z"])
    u0, u1 = stores[0].read_unique(), stores[1].read_unique()
    assert all((u0[k] == u1[k]).all() for k in u0)                                             # the 64-bit keys too
    for rep in stores:
        rep.close()
    ev.close()


# ------------------------------------------------------------------------------------------------ 4. fork loop
def test_forks_merge_with_their_parents_and_bring_fresh_outcomes():
    game = games.load_game(C4)
    n, n_fork = 16, 8
    ev = _fused(C4, 8)
    rep = _replay(C4, max_games=40)
    model = RC.FifoModel(40, 40 * game.max_game_length())
    eng = _engine(C4, n_slots=8, max_games=n)
    ex = _play(eng, ev, n)
    rep.append_engine(eng)
    model.append(RC.reference_games(game, ex))
    e = _expect(model)
    _check(rep, e)
    n_unique, n_before = len(e["uidx"]), len(e["flat_z"])
    flat = model.flat()
    odd = next(u for u in range(1, n_unique) if e["ply"][u] & 1)
    idx = sorted({0, odd} | set(np.random.RandomState(3).permutation(n_unique)[:n_fork].tolist()))[:n_fork]
    assert 0 in idx and odd in idx and len(idx) == n_fork
    # the parents' history strings, recovered on the host from read_unique's buffer_index and the model's flattened buffer
    bidx = rep.read_unique()["buffer_index"]
    parents = [flat[int(bidx[u])] for u in idx]
    histories = [[int(a) for a in r[0].split(", ")] if r[0] else [] for r in parents]
    assert [len(h) for h in histories] == [e["ply"][u] for u in idx]
    bb, ply, keys = rep.gather_forks(np.array(idx))
    assert ply.cpu().tolist() == [len(h) for h in histories]
    # the STORED pairs (device chain of the append) are the pairs the prefix form computes on the host for the same histories,
    # and the Python chain's: forking by history and forking by stored key are one thing
    by_history = _engine(C4, n_slots=8, max_games=n)
    by_history.set_game_starts(histories)
    by_history.reset(n_fork)
    assert (by_history.game_starts_device()[1].cpu().numpy() == keys.cpu().numpy()).all()
    by_history.close()
    assert [tuple(r) for r in keys.cpu().numpy().view(np.uint64).tolist()] == [_chain(game, [], h)[1] for h in histories]
    eng.set_game_starts_device(bb, ply, keys)
    ex2 = _play(eng, ev, n_fork)
    rep.append_engine(eng)
    eng.close()
    assert ex2["start_ply"].tolist() == [len(h) for h in histories]
    forks = _reference_games(game, ex2, histories)
    # on-policy z of the fork examples: the return of the player to move at the ABSOLUTE ply, by the Python rules
    for g, h in enumerate(histories):
        s = games.state_from_history(game, h)
        m = int(ex2["game_len"][g])
        for i in range(m):
            s.apply_action(int(ex2["move"][g, len(h) + i]))
        assert s.is_terminal() and m == len(forks[g])
        assert [r[3] for r in forks[g]] == [s.returns()[(len(h) + i) & 1] for i in range(m)]
    model.append(forks)
    e2 = _expect(model)
    _check(rep, e2)
    # every fork's first example merged with its parent (and the later ones with whatever shares their history)
    n_new = sum(len(g) for g in forks)
    new_strings = {r[0] for g in forks for r in g} - {r[0] for r in flat[:n_before]}
    assert len(e2["uidx"]) == n_unique + len(new_strings) and len(new_strings) <= n_new - n_fork
    assert e2["uidx"][:n_unique] == e["uidx"]                                                # the parents are still the first occurrences
    for u, parent in zip(idx, parents):
        pi, z = rep.read_example(int(bidx[u]))
        assert (pi == np.asarray(parent[2])).all() and z == parent[3]                          # = the model's average, written back
    rep.close()
    ev.close()


# ------------------------------------------------------------------------------------------------ 5. guards
def test_refusals_name_their_reason_and_leave_the_table_alone():
    from alphazero_openspiel_amd import engine as E
    game = games.load_game(C4)
    bb, ply = _tensors(*RA.states_of(game, [[3], [3, 2]]))
    for what, eng in (("arena", _engine(C4, arena_agent="zero", opponent="random")),
                      ("manual_moves", _engine(C4, manual_moves=True)),
                      ("stream", _engine(C4))):
        if what == "stream":
            eng.stream_begin()
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_game_starts is for plain self-play.*%s" % (AZ_E_INVALID, what)):
            eng.set_game_starts([[3], [3, 2]])
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_game_starts_device is for plain self-play.*%s" % (AZ_E_INVALID, what)):
            eng.set_game_starts_device(bb, ply)
        eng.close()
    eng = _engine(C4)
    eng.set_game_starts([[3], [3, 2], []])
    full_column = [3] * 6
    loses = [0, 1, 0, 1, 0, 1, 0]                                                             # the first player completes column 0
    with pytest.raises(E.EngineError, match=r"game 1: illegal prefix action"):
        eng.set_game_starts([[], full_column + [3]])
    with pytest.raises(E.EngineError, match=r"game 2: prefix ends the game"):
        eng.set_game_starts([[], [3], loses])
    bad_bb, bad_ply = _tensors(*RA.states_of(game, [[3], [3, 2]]))
    bad_ply[1] = 5
    with pytest.raises(E.EngineError, match=r"az_engine_set_game_starts_device: game 1: "):
        eng.set_game_starts_device(bad_bb, bad_ply)
    assert eng.game_starts.tolist() == [1, 2, 0]                                               # the earlier table is in force
    with pytest.raises(E.EngineError, match=r"\(%d\).*n_games exceeds" % AZ_E_INVALID):
        eng.reset(4)
    eng.reset(3)
    assert eng.game_starts_device()[0].cpu().tolist() == [1, 2, 0]
    assert [eng.read_slot(g)["ply"] for g in range(3)] == [1, 2, 0]
    with pytest.raises(E.EngineError, match=r"az_engine_stream_begin.*start-position table"):
        eng.stream_begin()
    eng.set_start_prefix([3])                                                                  # clears the table
    assert eng.game_starts is None
    eng.reset(12)
    assert eng.game_starts_device(12)[0].cpu().tolist() == [1] * 12 and eng.read_slot(2)["ply"] == 1
    eng.set_start_prefix([])
    eng.stream_begin()
    eng.close()


def test_setters_of_every_kind_replace_and_clear_one_another():
    """The transitions between the kinds of start (uniform, per position, per game; keyed or not; a table that grows; a refused
    call).  Neither engine is ticked."""
    from alphazero_openspiel_amd import engine as E
    game = games.load_game(C4)
    kw = dict(n_slots=8, n_playouts=4, max_games=8)
    man = _engine(C4, manual_moves=True, **kw)
    man.set_start_positions([[3], [3, 2], []])
    man.set_start_states_device(*_tensors(*RA.states_of(game, [[3, 2, 4], [3, 3, 2, 4]])))
    with pytest.raises(E.EngineError, match=r"\(%d\).*n_games exceeds" % AZ_E_INVALID):
        man.reset(3)
    man.reset(2)
    assert [man.read_slot(g)["ply"] for g in range(2)] == [3, 4]                                # the device states
    man.set_start_prefix([3])                                                                  # clears the table
    man.reset(8)
    assert [man.read_slot(g)["ply"] for g in range(8)] == [1] * 8
    man.close()

    def pairs(keys):
        return [tuple(r) for r in keys.cpu().numpy().view(np.uint64).tolist()]

    eng = _engine(C4, **kw)
    eng.set_game_starts([[3], [3, 2]])                                                          # keyed, 2 entries
    five = [[], [3], [3, 2], [3, 2, 4], [3, 3, 2, 4]]
    eng.set_game_starts_device(*_tensors(*RA.states_of(game, five)), keys=None)                 # not keyed, and the table grows
    ply, keys = eng.game_starts_device(5)
    assert keys is None and ply.cpu().tolist() == [0, 1, 2, 3, 4]
    three = [[3, 2, 4], [], [4, 2, 3]]
    eng.set_game_starts(three)                                                                  # keyed again
    ply, keys = eng.game_starts_device(3)
    assert ply.cpu().tolist() == [3, 0, 3] and pairs(keys) == [_chain(game, [], h)[1] for h in three]
    bad_bb, bad_ply = _tensors(*RA.states_of(game, five + [[0, 6]]))                            # more games than the table can hold
    bad_ply[4] = 9
    with pytest.raises(E.EngineError, match=r"az_engine_set_game_starts_device: game 4: "):
        eng.set_game_starts_device(bad_bb, bad_ply)
    ply, keys = eng.game_starts_device(3)                                                       # the keyed table of 3 is in force
    assert ply.cpu().tolist() == [3, 0, 3] and pairs(keys) == [_chain(game, [], h)[1] for h in three]
    assert eng.game_starts.tolist() == [3, 0, 3]
    with pytest.raises(E.EngineError, match=r"\(%d\).*n_games exceeds" % AZ_E_INVALID):
        eng.reset(4)
    eng.close()


def test_append_device_checks_the_start_plies_before_any_kernel():
    game = games.load_game(C4)
    ex = RC.fake_export(game, n_games=4, seed=1, start_history=[3, 2])
    buf = torch.from_numpy(RC.pack_device_export(ex)).cuda()
    rep = _replay(C4, max_games=8)
    ok = torch.full((4,), 2, dtype=torch.int32, device="cuda")
    g = int(np.argmax(ex["game_len"]))
    for bad_value, pattern in ((42 - int(ex["game_len"][g]) + 1, r"game_len\[%d\]" % g), (-1, r"start_ply\[%d\]" % g)):
        bad = ok.clone()
        bad[g] = bad_value
        with pytest.raises(RuntimeError, match=r"\(%d\).*%s" % (AZ_E_INVALID, pattern)):
            rep.append_device(buf, 4, start_ply=bad)
        st = rep.stats()
        assert (st["n_games"], st["n_examples"]) == (0, 0)
    with pytest.raises(ValueError):
        rep.append_device(buf, 4, start_ply=2, keys=torch.zeros((4, 2), dtype=torch.int64, device="cuda"))
    # keys=None: keyed from the start states, exactly as append_device(start_ply=2) keys the same games
    rep2 = _replay(C4, max_games=8)
    rep.append_device(buf, 4, start_ply=ok)
    rep2.append_device(buf, 4, start_ply=2)
    assert rep.dedupe() == rep2.dedupe()
    u, u2 = rep.read_unique(), rep2.read_unique()
    assert all((u[k] == u2[k]).all() for k in u)
    rep.close()
    rep2.close()


# ------------------------------------------------------------------------------------------------ 6. facade
def test_example_generator_plays_from_start_positions_and_forks(monkeypatch):
    from alphazero_openspiel_amd import replay
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    game = games.load_game(C4)
    histories = [[], [3], [3, 2, 4], [4, 2, 3], [3, 3, 2, 4], [0, 6]]
    kw = dict(n_playouts=S, n_slots=4, seed=5, use_graph=False)
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", **kw)
    out = gen.generate_examples(6, start_positions=histories)
    assert len(out) == 6
    for h, g in zip(histories, out):
        assert g[0][0] == ", ".join(map(str, h))
        s = games.state_from_history(game, h)
        assert (g[0][1] == games.boards_from_bitboards(game, np.array([s.bb], np.uint64), np.array([len(h)]))[0]).all()
        assert [len(r[0].split(", ")) if r[0] else 0 for r in g] == list(range(len(h), len(h) + len(g)))
    rep = replay.DeviceReplay(C4, 40, device=0)
    assert gen.generate_into(rep, 6, start_positions=histories) == 6
    n0 = rep.dedupe()
    idx = torch.tensor([0, n0 - 1, 1, 0], dtype=torch.int64)
    assert gen.generate_into(rep, 4, fork_from=idx) == 4
    st = rep.stats()
    assert st["n_games"] == 10 and st["fault_flags"] == 0
    assert rep.dedupe() > n0 and rep.stats()["fault_flags"] == 0                              # grew, without a collision fault
    with replay.Forker(rep, _net(C4), n_slots=4, n_playouts=S, seed=9) as fk:
        assert fk.fork(n=4) == 4
        assert rep.stats()["n_games"] == 14
        rep.dedupe()
        assert rep.stats()["fault_flags"] == 0
    rep.close()
    from alphazero_openspiel_amd import distributed as azdist
    for bad, pattern in ((dict(n_pools=2), "n_pools"), (dict(pool_devices=["cuda:0"]), "pool_devices"),
                         (dict(continuous=True), "continuous"), ("two ranks", "torch.distributed with world size 2")):
        if bad == "two ranks":                                                                 # a rank of a world of two
            monkeypatch.setattr(azdist, "world_size", lambda: 2)
            bad = {}
        g2 = ExampleGenerator(_net(C4), C4, "cuda:0", **kw, **bad)
        with pytest.raises(ValueError, match=pattern):
            g2.generate_examples(6, start_positions=histories)
        with pytest.raises(ValueError, match=pattern):
            g2.generate_into(None, 6, start_positions=histories)
        with pytest.raises(ValueError, match=pattern):
            g2.generate_into(None, 1, fork_from=[0])
        g2.close()
    gen.close()
