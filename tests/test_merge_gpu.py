"""az_replay_dedupe_positions and az_replay_unique_counts_device (csrc/az_replay.hip, replay.DeviceReplay.dedupe(by="position"),
unique_counts()) against the Python model of the rule (tests/merge_cases.py), bit for bit: there are no tolerances.

The generations (merge_cases.generation) hold a transposition, a mirrored pair, a self-symmetric position and equal histories by
construction; tests/test_merge_host.py checks on the model that each rule merges strictly more than the one before, that groups
of one, groups whose members alternate orientation and a group longer than one wave occur.  A = 7 (connect_four) and A = 240 /
432 (breakthrough: the lanes loop over the actions)."""
import ctypes as C

import numpy as np
import pytest
import torch

import merge_cases as MC
import mirror_cases as MIR
import replay_cases as RC
from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.engine import pi_from_visits, roots_export_layout
from test_game_starts_host import _chain
from test_replay_store_gpu import _check, _expect, _same

pytestmark = pytest.mark.gpu

AZ_OK, AZ_E_INVALID, AZ_E_STATE = 0, -1, -3
RULES = [("history", False), ("position", False), ("position", True)]


def _replay(name, **kw):
    from alphazero_openspiel_amd import replay
    return replay.DeviceReplay(name, device=0, **kw)


def _append(rep, ex, how):
    if how == "host":
        rep.append_export(ex)
    else:
        rep.append_device(torch.from_numpy(RC.pack_device_export(ex)).cuda(), len(ex["game_len"]))


def _model_pass(game, flat, by, mirror):
    return MC.by_history(flat) if by == "history" else MC.merged(game, flat, mirror)


def _check_pass(rep, game, flat, by, mirror):
    """One dedupe of the store and of the model (which mutates `flat`, the model's buffer): the count, read_unique, the counts
    and every stored example - first occurrences hold the written-back average, every other member what it held."""
    unique, flat = _model_pass(game, flat, by, mirror)
    assert rep.dedupe(by=by, mirror=mirror) == len(unique)
    st = rep.stats()
    assert (st["n_examples"], st["n_unique"], st["fault_flags"]) == (len(flat), len(unique), 0)
    u = rep.read_unique()
    assert u["buffer_index"].tolist() == [g["index"] for g in unique]
    _same(u["pi"], np.array([g["pi"] for g in unique]), "unique pi")
    _same(u["z"], np.array([g["z"] for g in unique]), "unique z")
    _same(u["bitboards"], np.array([flat[g["index"]].bb for g in unique], dtype=np.uint64), "unique bitboards")
    assert u["ply"].tolist() == [flat[g["index"]].ply for g in unique]
    counts = rep.unique_counts()
    assert counts.dtype == torch.int32 and counts.device == rep.device
    assert counts.cpu().tolist() == [g["count"] for g in unique]
    got = [rep.read_example(i) for i in range(len(flat))]
    _same(np.array([g[0] for g in got]), np.array([r[2] for r in flat]), "stored pi")
    _same(np.array([g[1] for g in got]), np.array([r[3] for r in flat]), "stored z")
    return unique


# ------------------------------------------------------------------------------------------------ a. the rule
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("name", MC.BOARDS)
def test_position_dedupe_equals_the_model(name, mirror):
    game = games.load_game(name)
    ex, ref = MC.generation(game, rounds=3, seed=7)
    flat = [r for g in ref for r in g]
    n_hist = len(MC.by_history(MC.copy_flat(flat))[0])
    for how in ("host", "device"):
        rep = _replay(name, max_games=len(ref))
        _append(rep, ex, how)
        mine = MC.copy_flat(flat)
        first = _check_pass(rep, game, mine, "position", mirror)
        assert len(first) < n_hist and 1 in [g["count"] for g in first]
        # a second pass: the written-back first occurrences are averaged with their members again, as in the reference
        second = _check_pass(rep, game, mine, "position", mirror)
        assert [g["index"] for g in second] == [g["index"] for g in first]
        assert [g["pi"] for g in second] != [g["pi"] for g in first]
        rep.close()


@pytest.mark.parametrize("name", [MC.C4, MC.B54])
def test_a_group_longer_than_one_wave(name):
    """The initial position of 84 / 70 games (cut to five plies each): a segment of more than 64 members."""
    game = games.load_game(name)
    ex, ref = MC.generation(game, rounds=14, seed=7, max_len=5)
    rep = _replay(name, max_games=len(ref))
    _append(rep, ex, "device")
    unique = _check_pass(rep, game, [r for g in ref for r in g], "position", True)
    assert unique[0]["count"] == len(ref) >= 65
    rep.close()


# ------------------------------------------------------------------------------------------------ b. ring wrap
@pytest.mark.parametrize("name", [MC.C4, MC.B54])
def test_groups_across_the_wrap_point_of_the_ring(name):
    game = games.load_game(name)
    gens = [MC.generation(game, rounds=3, seed=40 + gen) for gen in range(4)]
    sizes = [int(ex["game_len"].sum()) for ex, _ in gens]
    max_games, max_examples = 2 * len(gens[0][1]), max(sizes) + max(sizes) // 2
    rep = _replay(name, max_games=max_games, max_examples=max_examples)
    model = RC.FifoModel(max_games, max_examples)
    for gen, (ex, ref) in enumerate(gens):
        _append(rep, ex, "host" if gen & 1 else "device")
        model.append(ref)
        unique = _check_pass(rep, game, model.flat(), "position", True)       # (model.flat() holds the model's own records)
        assert unique[0]["count"] == model.n_games                            # the initial position: old games and new ones
        assert rep.stats()["games_dropped"] == model.games_dropped
    assert model.ring_evictions > 0 and model.appended > 2 * max_examples     # head != 0, and the ring has wrapped physically
    rep.close()


# ------------------------------------------------------------------------------------------------ c. mode changes
@pytest.mark.parametrize("name", [MC.C4, MC.B66])
def test_history_then_position_then_history(name):
    game = games.load_game(name)
    ex, ref = MC.generation(game, rounds=3, seed=9)
    flat = [r for g in ref for r in g]
    rep = _replay(name, max_games=len(ref))
    _append(rep, ex, "host")
    n = [len(_check_pass(rep, game, flat, by, mirror)) for by, mirror in (RULES[0], RULES[2], RULES[0], RULES[1], RULES[0])]
    assert n[0] == n[2] == n[4] and n[1] < n[3] < n[0]
    rep.close()


# ------------------------------------------------------------------------------------------------ d. the history pass
@pytest.mark.parametrize("name", MC.BOARDS)
def test_history_dedupe_is_what_it_was_and_fills_the_counts(name):
    game = games.load_game(name)
    rep = _replay(name, max_games=40)
    model = RC.FifoModel(40, 40 * game.max_game_length())
    for gen in range(2):
        ex, ref = MC.generation(game, rounds=3, seed=60 + gen)
        _append(rep, ex, "device")
        model.append(ref)
        counts = {}
        for r in model.flat():
            counts[r[0]] = counts.get(r[0], 0) + 1
        e = _expect(model)                                   # oracle.pyreplay, as tests/test_replay_store_gpu.py compares
        _check(rep, e)
        flat = model.flat()
        assert rep.unique_counts().cpu().tolist() == [counts[flat[i][0]] for i in e["uidx"]]
        assert max(counts.values()) == model.n_games and 1 in counts.values()
    rep.close()


# ------------------------------------------------------------------------------------------------ e. the readers
def _roots_buffer(game, states, visits, root_q):
    """A packed root export (engine.roots_export_layout) of finished searches: slot j = game j at states[j] = (bb, ply)."""
    G, mc = len(states), game.max_children()
    layout, total = roots_export_layout(G, mc)
    buf = np.zeros(total, dtype=np.uint8)
    arr = {name: buf[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape) for name, dt, shape, off in layout}
    arr["header"][:] = [G, G, mc, 0]
    arr["game_id"][:] = np.arange(G)
    arr["phase"][:] = 5
    for j, (bb, ply) in enumerate(states):
        la = games.legal_actions_from_bitboards(game, int(bb[0]), int(bb[1]), int(ply))
        arr["ply"][j], arr["n_children"][j] = ply, len(la)
        arr["child_action"][j, :len(la)] = la
        arr["child_n"][j, :len(la)] = visits[j][:len(la)]
        arr["root_n"][j] = 1 + int(np.sum(visits[j][:len(la)]))
        arr["sims_done"][j] = arr["root_n"][j]
        arr["root_q"][j] = root_q[j]
    return buf, arr


@pytest.mark.parametrize("name", [MC.C4, MC.B66])
def test_readers_of_the_unique_list_after_a_mirror_merge(name):
    game = games.load_game(name)
    ex, ref = MC.generation(game, rounds=3, seed=13)
    flat = [r for g in ref for r in g]
    rep = _replay(name, max_games=len(ref))
    _append(rep, ex, "device")
    unique = _check_pass(rep, game, flat, "position", True)
    n = len(unique)
    firsts = [flat[g["index"]] for g in unique]
    pi32 = np.array([g["pi"] for g in unique]).astype(np.float32)
    z32 = np.array([g["z"] for g in unique]).astype(np.float32)
    # sample: the first occurrences' own observations, the averaged targets
    plain = rep.sample(n, indices=np.arange(n))
    _same(plain[0].cpu().numpy(), np.stack([r[1] for r in firsts]).astype(np.float32), "sampled x")
    _same(plain[1].cpu().numpy(), pi32, "sampled pi")
    _same(plain[2].cpu().numpy(), z32, "sampled z")
    # sample with flips: the mirrored rows are the mirror images of those
    flips = np.random.RandomState(2).rand(n) < 0.5
    flips[:2] = [False, True]
    got = rep.sample(n, indices=np.arange(n), mirror=flips)
    want = MIR.mirrored(game, plain)
    sel = torch.as_tensor(flips, device=rep.device)
    assert bool(MIR.rows_equal(got, want)[sel].all()) and bool(MIR.rows_equal(got, plain)[~sel].all())
    # gather_forks: the first occurrences' positions and THEIR history key pairs
    bb, ply, keys = rep.gather_forks(np.arange(n))
    _same(bb.cpu().numpy().view(np.uint64), np.array([r.bb for r in firsts], dtype=np.uint64), "fork bitboards")
    assert ply.cpu().tolist() == [r.ply for r in firsts]
    histories = [[int(a) for a in r[0].split(", ")] if r[0] else [] for r in firsts]
    assert [tuple(k) for k in keys.cpu().numpy().view(np.uint64).tolist()] == [_chain(game, [], h)[1] for h in histories]
    # refresh_from_roots on a hand-built root buffer: the first occurrence is rewritten, the other members are left alone
    merged_u = [u for u, g in enumerate(unique) if g["count"] > 1]
    idx = np.array(merged_u[:6] + [u for u, g in enumerate(unique) if g["count"] == 1][:2])
    rng = np.random.RandomState(8)
    visits = rng.randint(1, 60, (len(idx), game.max_children())).astype(np.uint32)
    root_q = rng.uniform(-1, 1, len(idx))
    buf, arr = _roots_buffer(game, [(firsts[u].bb, firsts[u].ply) for u in idx], visits, root_q)
    gbb, gply = rep.gather_states(idx)
    assert gply.cpu().tolist() == [firsts[u].ply for u in idx]
    assert rep.refresh_from_roots(idx, torch.from_numpy(buf).cuda(), "soft-Z") == len(idx)
    for j, u in enumerate(idx):
        nc = int(arr["n_children"][j])
        r = flat[unique[u]["index"]]
        r[2], r[3] = pi_from_visits(arr["child_action"][j, :nc], arr["child_n"][j, :nc], rep.A), -root_q[j]
    got = [rep.read_example(i) for i in range(len(flat))]
    _same(np.array([g[0] for g in got]), np.array([r[2] for r in flat]), "stored pi after the refresh")
    _same(np.array([g[1] for g in got]), np.array([r[3] for r in flat]), "stored z after the refresh")
    assert rep.stats()["fault_flags"] == 0
    # ... and the next pass averages the refreshed first occurrences with their stale members, as the history pass does
    _check_pass(rep, game, flat, "position", True)
    rep.close()


# ------------------------------------------------------------------------------------------------ f. refusals
def _counts_rc(rep, n):
    out = torch.full((max(int(n), 1),), -5, dtype=torch.int32, device=rep.device)
    rc = rep.lib.az_replay_unique_counts_device(rep._h, C.c_void_p(out.data_ptr()), int(n), rep._stream())
    torch.cuda.synchronize()
    return rc, out


def test_refusals():
    game = games.load_game(MC.C4)
    rep = _replay(MC.C4, max_games=40)
    # an empty store: 0 and AZ_OK, for either rule, and its counts are an empty list
    assert _counts_rc(rep, 0)[0] == AZ_E_STATE                             # before any dedupe
    with pytest.raises(RuntimeError, match=r"\(%d\).*before any dedupe" % AZ_E_STATE):
        rep.unique_counts()
    for mirror in (0, 1):
        assert rep.lib.az_replay_dedupe_positions(rep._h, mirror, rep._stream()) == AZ_OK
        assert rep.stats()["n_unique"] == 0
    assert rep.dedupe(by="position", mirror=True) == 0 and rep.dedupe() == 0
    assert rep.unique_counts().shape == (0,)
    ex, ref = MC.generation(game, rounds=3, seed=1)
    rep.append_export(ex)
    assert _counts_rc(rep, 0)[0] == AZ_E_STATE                             # the append moved the epoch
    n = rep.dedupe(by="position", mirror=True)
    want = rep.unique_counts().cpu().tolist()
    assert len(want) == n and sum(want) == rep.stats()["n_examples"]
    # mirror = 2: refused, and nothing has moved - the list and its counts are still there
    assert rep.lib.az_replay_dedupe_positions(rep._h, 2, rep._stream()) == AZ_E_INVALID
    assert rep.lib.az_replay_dedupe_positions(rep._h, -1, rep._stream()) == AZ_E_INVALID
    assert b"mirror must be 0 or 1" in rep.lib.az_replay_last_error(rep._h)
    assert rep.stats()["n_unique"] == n and rep.unique_counts().cpu().tolist() == want
    # a wrong n
    for bad in (n - 1, n + 1, 0):
        rc, out = _counts_rc(rep, bad)
        assert rc == AZ_E_INVALID and (out == -5).all()
    rc, out = _counts_rc(rep, n)
    assert rc == AZ_OK and out.cpu().tolist() == want
    # an append, and a capacity change, move the epoch
    rep.append_export(ex)
    assert _counts_rc(rep, n)[0] == AZ_E_STATE
    with pytest.raises(RuntimeError, match=r"\(%d\).*the store has changed" % AZ_E_STATE):
        rep.unique_counts()
    n2 = rep.dedupe(by="position", mirror=False)
    assert _counts_rc(rep, n2)[0] == AZ_OK
    rep.set_capacity(30)
    assert _counts_rc(rep, n2)[0] == AZ_E_STATE
    # the facade's own refusal comes before the library is touched
    with pytest.raises(ValueError, match="no mirror key"):
        rep.dedupe(by="history", mirror=True)
    assert rep.stats()["fault_flags"] == 0
    rep.close()
