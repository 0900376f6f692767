"""The device replay store (csrc/az_replay.hip, replay.DeviceReplay) against the host reference, bit for bit, on every board
and on the paths the other replay tests never take: sample() on breakthrough, the example ring's eviction and physical wrap,
start_ply != 0, segments longer than one wave, the device-drawn indices and the refusals that come before any launch.

Reference: engine.examples_from_export + oracle/pyreplay.py (pinned to the reference Trainer by tests/golden/replay.json) on
synthetic games from the Python rules (tests/replay_cases.py); tests/test_replay_cases.py pins the reference on the visit-count
edges used here.  There are no tolerances."""
import numpy as np
import pytest
import torch

import replay_cases as RC
from alphazero_openspiel_amd import games

pytestmark = pytest.mark.gpu

C4, B54, B66, B88 = ("connect_four", "breakthrough(rows=5,columns=4)", "breakthrough(rows=6,columns=6)",
                     "breakthrough(rows=8,columns=8)")
AZ_E_INVALID, AZ_E_STATE = -1, -3


def _replay(name, **kw):
    from alphazero_openspiel_amd import replay
    return replay.DeviceReplay(name, device=0, **kw)


def _append_both(stores, ex, p0=0):
    """One generation into the first store as a host view and into the second as a packed device export."""
    stores[0].append_export(ex)
    stores[1].append_device(torch.from_numpy(RC.pack_device_export(ex)).cuda(), len(ex["game_len"]), start_ply=p0)


def _expect(model):
    """One remove_duplicates pass of the model -> what every store fed like the model must hold after ITS pass."""
    flat, unique, uidx = model.dedupe()
    return {"n_games": model.n_games, "games_dropped": model.games_dropped, "uidx": uidx,
            "flat_pi": np.array([r[2] for r in flat]), "flat_z": np.array([r[3] for r in flat]),
            "pi": np.array([r[2] for r in unique]), "z": np.array([r[3] for r in unique]),
            "bb": np.array([r.bb for r in unique], dtype=np.uint64), "ply": [r.ply for r in unique],
            "board": np.stack([r[1] for r in unique])}


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), "%s differs at %s: %r != %r (%d elements)" % (what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def _check_examples(rep, e):
    """Every stored example: first occurrences hold the written-back average, every other member its own pi / z."""
    got = [rep.read_example(i) for i in range(len(e["flat_z"]))]
    _same(np.array([g[0] for g in got]), e["flat_pi"], "stored pi")
    _same(np.array([g[1] for g in got]), e["flat_z"], "stored z")


def _check(rep, e):
    """dedupe() -> count, read_unique, read_example of the whole buffer, then sample() of every unique example."""
    n = len(e["uidx"])
    assert rep.dedupe() == n
    st = rep.stats()
    assert (st["n_games"], st["n_examples"], st["n_unique"], st["games_dropped"], st["fault_flags"]) == \
        (e["n_games"], len(e["flat_z"]), n, e["games_dropped"], 0)
    u = rep.read_unique()
    assert u["buffer_index"].tolist() == e["uidx"]
    _same(u["pi"], e["pi"], "unique pi")
    _same(u["z"], e["z"], "unique z")
    _same(u["bitboards"], e["bb"], "unique bitboards")
    assert u["ply"].tolist() == e["ply"]
    _check_examples(rep, e)
    perm = np.random.RandomState(n).permutation(n)
    x, pi, z = rep.sample(n, indices=perm)
    _same(x.cpu().numpy(), e["board"][perm].astype(np.float32), "sampled x")
    _same(pi.cpu().numpy(), e["pi"][perm].astype(np.float32), "sampled pi")
    _same(z.cpu().numpy(), e["z"][perm].astype(np.float32), "sampled z")
    assert x.dtype == pi.dtype == z.dtype == torch.float32
    assert rep.stats()["fault_flags"] == 0


def _generation(game, n_games, seed, start_history=(), one_move=True, depth=3):
    """Games with shared openings (so histories repeat below the start position too) and the visit-count edges."""
    openings = RC.random_openings(game, 4, depth, 1000 + len(start_history), start_history)
    if one_move and not start_history:
        openings.append(RC.ONE_MOVE_PREFIX[game.name])
    ex = RC.fake_export(game, n_games=n_games, seed=seed, openings=openings, start_history=start_history, visits="edges")
    return ex, RC.reference_games(game, ex, start_history)


# ------------------------------------------------------------------------------------------------ a. every board
@pytest.mark.parametrize("name,n_games", [(C4, 40), (B54, 40), (B66, 24), (B88, 12)])
def test_every_board_through_both_append_paths(name, n_games):
    game = games.load_game(name)
    max_games = 2 * n_games + n_games // 2                    # the third generation drops games
    stores = [_replay(name, max_games=max_games), _replay(name, max_games=max_games)]
    model = RC.FifoModel(max_games, max_games * game.max_game_length())
    for gen in range(3):
        ex, ref = _generation(game, n_games, 10 * gen + 1)
        _append_both(stores, ex)
        model.append(ref)
        e = _expect(model)
        for rep in stores:
            _check(rep, e)
        assert len(e["uidx"]) < len(e["flat_z"])                 # there ARE duplicates to average
    assert model.cap_evictions == n_games - n_games // 2 and model.ring_evictions == 0
    for rep in stores:
        rep.close()


# ------------------------------------------------------------------------------------------------ b. example ring
@pytest.mark.parametrize("name", [C4, B54])
def test_example_ring_evicts_wraps_and_refuses_an_oversized_generation(name):
    game = games.load_game(name)
    n_games = 20
    gens = [_generation(game, n_games, 100 + gen) for gen in range(6)]
    sizes = [int(ex["game_len"].sum()) for ex, _ in gens]
    max_examples = 3 * sum(sizes[:5]) // 10                  # about 1.5 generations
    max_games = 28                                            # the game cap trims too, but only after the ring has
    assert max(sizes) <= max_examples < 2 * min(sizes)
    stores = [_replay(name, max_games=max_games, max_examples=max_examples) for _ in range(2)]
    model = RC.FifoModel(max_games, max_examples)
    for gen in range(5):
        ex, ref = gens[gen]
        _append_both(stores, ex)
        model.append(ref)
        e = _expect(model)
        for rep in stores:
            _check(rep, e)
    assert model.events[0] == "ring" and "cap" in model.events    # the ring made room before the game cap trimmed anything
    assert model.appended > 2 * max_examples                  # the ring has wrapped physically, more than once
    # a generation that cannot fit: refused, and the store is what it was
    big = RC.fake_export(game, n_games=2 * n_games, seed=7, visits="edges")
    assert int(big["game_len"].sum()) > max_examples
    with pytest.raises(ValueError):
        model.append(RC.reference_games(game, big))
    with pytest.raises(RuntimeError, match=r"\(%d\).*more examples than max_examples" % AZ_E_INVALID):
        stores[0].append_export(big)
    with pytest.raises(RuntimeError, match=r"\(%d\).*more examples than max_examples" % AZ_E_INVALID):
        stores[1].append_device(torch.from_numpy(RC.pack_device_export(big)).cuda(), 2 * n_games)
    e = _expect(model)                                        # (a second pass over the same buffer, on the model and on the device)
    for rep in stores:
        _check(rep, e)
    ex, ref = gens[5]
    _append_both(stores, ex)
    model.append(ref)
    e = _expect(model)
    for rep in stores:
        _check(rep, e)
        rep.close()


# ------------------------------------------------------------------------------------------------ c. set_capacity
def test_set_capacity_takes_effect_at_the_next_append():
    game = games.load_game(C4)
    stores = [_replay(C4, max_games=30), _replay(C4, max_games=30)]
    model = RC.FifoModel(30, 30 * game.max_game_length())
    for gen, (capacity, before, after) in enumerate([(None, 0, 12), (8, 12, 8), (30, 8, 20)]):
        if capacity:
            model.set_capacity(capacity)
            for rep in stores:
                rep.set_capacity(capacity)
        assert [rep.stats()["n_games"] for rep in stores] == [before, before] == [model.n_games] * 2   # not at the call
        ex, ref = _generation(game, 12, 200 + gen, one_move=False)
        _append_both(stores, ex)
        model.append(ref)
        assert [rep.stats()["n_games"] for rep in stores] == [after, after] == [model.n_games] * 2      # at the append
        e = _expect(model)
        for rep in stores:
            _check(rep, e)
    assert model.games_dropped == 16
    for rep in stores:
        rep.close()


# ------------------------------------------------------------------------------------------------ d. start_ply
@pytest.mark.parametrize("name,start_history", [(C4, [3]), (C4, [3, 3, 2, 4]), (B66, "three plies")])
def test_generations_that_start_after_a_prefix(name, start_history):
    game = games.load_game(name)
    if isinstance(start_history, str):
        start_history = RC.random_openings(game, 1, 3, 5)[0]
    p0 = len(start_history)
    stores = [_replay(name, max_games=40), _replay(name, max_games=40)]
    model = RC.FifoModel(40, 40 * game.max_game_length())
    for gen in range(2):
        ex, ref = _generation(game, 16, 300 + gen, start_history)
        assert ex["start_ply"] == p0 and ref[0][0][0] == ", ".join(str(a) for a in start_history)
        _append_both(stores, ex, p0)
        model.append(ref)
        e = _expect(model)
        assert e["ply"][0] == p0 and set(np.array(e["ply"]) & 1) == {0, 1}     # the sampled player plane takes both values
        for rep in stores:
            _check(rep, e)
    for rep in stores:
        rep.close()


def test_engine_path_with_a_start_prefix_of_odd_length():
    """append_engine forms the on-policy z itself ((start_ply + i) & 1); the export paths trust the filled `value`."""
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.network import Net
    game = games.load_game(C4)
    prefix = [3, 2, 3]
    torch.manual_seed(2)
    ev = E.DeviceEvaluator(Net([3, 6, 7], 7, n_blocks=1, n_filters=16), "cuda:0")
    eng = E.SelfPlayEngine(C4, 8, n_playouts=4, max_games=8, backup="on-policy", seed=4)
    eng.set_start_prefix(prefix)
    E.run_selfplay(eng, ev, 8)
    rep_e, rep_h = _replay(C4, max_games=8), _replay(C4, max_games=8)
    rep_e.append_engine(eng)
    ex = eng.export()
    eng.close()
    assert ex["start_ply"] == 3
    rep_h.append_export(ex)
    # every stored z is the return of the player to move at that absolute ply, replayed with the Python rules
    want_z = []
    for g in range(8):
        s = games.state_from_history(game, prefix)
        n = int(ex["game_len"][g])
        for i in range(n):
            s.apply_action(int(ex["move"][g, 3 + i]))
        assert s.is_terminal()
        want_z += [s.returns()[(3 + i) & 1] for i in range(n)]
    assert {-1.0, 1.0} <= set(want_z)
    for rep in (rep_e, rep_h):
        assert rep.stats()["n_examples"] == len(want_z)
        assert [rep.read_example(i)[1] for i in range(len(want_z))] == want_z
    model = RC.FifoModel(8, 8 * 42)
    model.append(RC.reference_games(game, ex, prefix))
    e = _expect(model)
    _check(rep_e, e)
    _check(rep_h, e)
    ue, uh = rep_e.read_unique(), rep_h.read_unique()
    assert all((ue[k] == uh[k]).all() for k in ue) and e["ply"][0] == 3
    rep_e.close()
    rep_h.close()


# ------------------------------------------------------------------------------------------------ e. long segments
def test_segments_longer_than_a_wave_and_the_guard_beyond_lane_63():
    game = games.load_game(C4)
    ex, ref = _generation(game, 140, 400, one_move=False)
    rep = _replay(C4, max_games=140)
    model = RC.FifoModel(140, 140 * 42)
    rep.append_export(ex)
    model.append(ref)
    flat = model.flat()
    sizes = {}
    for r in flat:
        sizes[r[0]] = sizes.get(r[0], 0) + 1
    assert sizes[""] == 140 and sum(1 for c in sizes.values() if c > 64) >= 3
    e = _expect(model)
    _check(rep, e)
    n_unique = len(e["uidx"])
    u = rep.read_unique()
    key_of = {flat[i][0]: int(u["key"][k]) for k, i in enumerate(e["uidx"])}
    starts = np.concatenate([[0], np.cumsum(ex["game_len"])]).astype(int)
    for g in (64, 128):
        # ply 1 of game g sorts behind the starts of games 0..g: member position g + 1 of the start position's segment
        idx = int(starts[g]) + 1
        assert flat[idx][0] != "" and flat[idx].ply == 1
        before = rep.read_example(0)
        assert rep.lib.az_replay_debug_set_key(rep._h, idx, key_of[""]) == 0
        with pytest.raises(RuntimeError, match="different histories"):
            rep.dedupe()
        after = rep.read_example(0)
        assert (after[0] == before[0]).all() and after[1] == before[1]      # the segment's first record is untouched
        # what the refused pass did, on the model: the start position's segment and the re-keyed example were left alone,
        # every other segment was averaged (the re-keyed example missing from its own)
        saved = [(r, r[0]) for r in flat if r[0] == ""] + [(flat[idx], flat[idx][0])]
        for k, (r, _) in enumerate(saved):
            r[0] = ("left alone", k)
        model.dedupe()
        for r, key in saved:
            r[0] = key
        _check_examples(rep, {"flat_pi": np.array([r[2] for r in flat]), "flat_z": np.array([r[3] for r in flat])})
        # with the key restored the pass succeeds, with the reference's result
        assert rep.lib.az_replay_debug_set_key(rep._h, idx, key_of[flat[idx][0]]) == 0
        e = _expect(model)
        assert len(e["uidx"]) == n_unique
        _check(rep, e)
    rep.close()


# ------------------------------------------------------------------------------------------------ f. device-drawn indices
def test_device_drawn_indices_are_in_range_deterministic_and_uniform():
    game = games.load_game(C4)
    ex = RC.fake_export(game, n_games=6, seed=8, openings=RC.random_openings(game, 3, 2, 9))
    stores = [_replay(C4, max_games=6) for _ in range(3)]
    for rep in stores:
        rep.append_export(ex)
        U = rep.dedupe()

    def rows(x, pi, z):
        assert not torch.isnan(x).any() and not torch.isnan(pi).any() and not torch.isnan(z).any()
        m = np.concatenate([x.cpu().numpy().reshape(len(z), -1), pi.cpu().numpy(), z.cpu().numpy()[:, None]], axis=1)
        return [r.tobytes() for r in m]

    # all three stores make the same calls in the same order: the draw is keyed by (seed, call counter, row)
    every = [rows(*rep.sample(U, indices=np.arange(U))) for rep in stores]
    assert every[0] == every[1] == every[2]
    bucket = {}                                               # row content -> how many unique examples have it
    for r in every[0]:
        bucket[r] = bucket.get(r, 0) + 1
    assert bucket[every[0][0]] == 1 and bucket[every[0][-1]] == 1   # the first and the last example are recognisable
    B, calls, seed = 4096, 4, 12345
    drawn = [[rows(*rep.sample(B, seed=s)) for _ in range(calls)] for rep, s in zip(stores, (seed, seed, seed + 1))]
    assert drawn[0] == drawn[1]                               # same content, same seed: identical rows, call by call
    assert drawn[0][0] != drawn[2][0]                         # another seed
    assert len({tuple(c) for c in drawn[0]}) == calls         # the next call
    count = {r: 0 for r in bucket}
    for call in drawn[0]:
        for r in call:
            assert r in count                                 # every row is a row of the de-duplicated list
            count[r] += 1
    n = B * calls
    for r, k in bucket.items():
        p = k / U
        assert abs(count[r] - n * p) <= 6 * np.sqrt(n * p * (1 - p)) + 1, (count[r], n * p)
    assert count[every[0][0]] > 0 and count[every[0][-1]] > 0  # both ends of [0, U) are drawn
    for rep in stores:
        assert rep.stats()["fault_flags"] == 0
        rep.close()


# ------------------------------------------------------------------------------------------------ g. refusals
def test_sample_before_dedupe_is_a_state_error():
    game = games.load_game(C4)
    rep = _replay(C4, max_games=4)
    with pytest.raises(RuntimeError, match=r"\(%d\).*before az_replay_dedupe" % AZ_E_STATE):
        rep.sample(4, seed=1)
    rep.append_export(RC.fake_export(game, n_games=2, seed=1))
    with pytest.raises(RuntimeError, match=r"\(%d\).*before az_replay_dedupe" % AZ_E_STATE):
        rep.sample(4, indices=[0, 1, 2, 3])
    assert rep.dedupe() > 0
    rep.sample(4, indices=[0, 1, 2, 3])
    rep.append_export(RC.fake_export(game, n_games=1, seed=2))       # an append invalidates the de-duplicated list
    with pytest.raises(RuntimeError, match=r"\(%d\)" % AZ_E_STATE):
        rep.sample(4, seed=1)
    rep.close()


@pytest.mark.parametrize("start_history", [[], [3, 3, 2, 4]])
def test_bad_views_are_refused_before_any_launch(start_history):
    game = games.load_game(C4)
    p0, mp, mc = len(start_history), game.max_game_length(), game.max_children()
    stores = [_replay(C4, max_games=12), _replay(C4, max_games=12)]
    model = RC.FifoModel(12, 12 * mp)
    ex, ref = _generation(game, 4, 500, start_history)
    _append_both(stores, ex, p0)
    model.append(ref)
    held = _expect(model)
    for rep in stores:
        _check(rep, held)

    def variant(**change):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ex.items()}
        for k, (index, value) in change.items():
            bad[k][index] = value
        return bad

    def unchanged(rep):
        st = rep.stats()
        assert (st["n_games"], st["n_examples"], st["n_unique"], st["games_dropped"]) == \
            (held["n_games"], len(held["flat_z"]), len(held["uidx"]), held["games_dropped"])
        _check_examples(rep, held)

    too_long = mp - p0 + 1
    for bad, what in [(variant(game_len=(1, -1)), r"game_len\[1\] = -1"),
                      (variant(game_len=(2, too_long)), r"game_len\[2\] = %d" % too_long),
                      (variant(game_len=(3, 2 ** 31 - 1)), r"game_len\[3\]")]:
        with pytest.raises(RuntimeError, match=r"\(%d\).*%s" % (AZ_E_INVALID, what)):
            stores[0].append_export(bad)
        with pytest.raises(RuntimeError, match=r"\(%d\).*%s" % (AZ_E_INVALID, what)):
            stores[1].append_device(torch.from_numpy(RC.pack_device_export(bad)).cuda(), 4, start_ply=p0)
        for rep in stores:
            unchanged(rep)
    # host views only: the packed layout has no max_children of its own and its child counts stay on the device
    with pytest.raises(RuntimeError, match=r"\(%d\).*n_children = %d at game 1, ply %d" % (AZ_E_INVALID, mc + 1, p0 + 2)):
        stores[0].append_export(variant(n_children=((1, p0 + 2), mc + 1)))
    unchanged(stores[0])
    wide = dict(ex, child_action=np.zeros((4, mp, mc + 1), np.uint16), child_visits=np.ones((4, mp, mc + 1), np.uint32))
    with pytest.raises(RuntimeError, match=r"\(%d\).*max_children" % AZ_E_INVALID):
        stores[0].append_export(wide)
    unchanged(stores[0])
    with pytest.raises(RuntimeError, match="export buffer holds"):   # a buffer packed for fewer children is too short
        narrow = dict(ex, child_action=ex["child_action"][:, :, :mc - 1], child_visits=ex["child_visits"][:, :, :mc - 1])
        stores[1].append_device(torch.from_numpy(RC.pack_device_export(narrow)).cuda(), 4, start_ply=p0)
    unchanged(stores[1])
    # and the stores go on working
    ex2, ref2 = _generation(game, 4, 501, start_history)
    _append_both(stores, ex2, p0)
    model.append(ref2)
    e = _expect(model)
    for rep in stores:
        _check(rep, e)
        rep.close()
