"""Reanalyse on the GPU: stored positions -> az_replay_gather_states -> az_engine_set_start_states_device -> search ->
az_replay_refresh_from_roots, and analysis.Analyzer.load_states_device / replay.Reanalyser on top.

Bar: bit-exact.  No root noise enters a search and both sides of every comparison see the same float32 priors and values
(HostPolicyEvaluator over oracle.fakepolicy.fake_eval, or the fused net at f32x whose output bits do not depend on the batch),
so every comparison is `==`.  The one bound (pi rows sum to 1) is derived where it is used."""
import ctypes as C

import numpy as np
import pytest
import torch

import reanalyse_cases as RA
import replay_cases as RC
from analysis_positions import random_positions
from alphazero_openspiel_amd import _lib, games
from oracle import fakepolicy

pytestmark = pytest.mark.gpu

C4, B54, B66 = "connect_four", "breakthrough(rows=5,columns=4)", "breakthrough(rows=6,columns=6)"
AZ_E_INVALID, AZ_E_STATE, AZ_E_DEVICE = -1, -3, -4
SALT = 9


def _mods():
    from alphazero_openspiel_amd import analysis, engine, replay
    return engine, analysis, replay


def _board_fn(A, salt=SALT):
    return lambda board: fakepolicy.fake_eval(board, A, salt)


def _dev_states(bb, ply):
    """numpy (uint64 [n, 2], int32 [n]) -> the device tensors set_start_states_device takes."""
    return (torch.from_numpy(np.ascontiguousarray(bb, dtype=np.uint64).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(ply, dtype=np.int32)).cuda())


def _manual_engine(game, n, S):
    E, _, _ = _mods()
    eng = E.SelfPlayEngine(game, n, n_playouts=S, use_dirichlet=False, manual_moves=True, max_games=n)
    return eng, E.HostPolicyEvaluator(eng, _board_fn(eng.A))


def _search(eng, ev, buf=None):
    """advance + evaluate until the root export's header says every slot is done -> (read_roots(), the device buffer)."""
    obs, pri, val = eng.alloc_io()
    buf = eng.alloc_roots() if buf is None else buf
    for _ in range(4 * eng.cfg.n_playouts + 16):
        for _ in range(4):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        eng.export_roots_device(buf)
        if int(buf[:16].view(torch.int32)[0].item()) == eng.G:
            break
    else:
        pytest.fail("searches did not finish")
    return eng.read_roots(buf), buf


def _same_roots(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _store(name, ex_list, **kw):
    _, _, R = _mods()
    game = games.load_game(name)
    kw.setdefault("max_games", sum(len(ex["game_len"]) for ex in ex_list))
    rep = R.DeviceReplay(name, device=0, **kw)
    for ex in ex_list:
        rep.append_export(ex)
    return rep, rep.dedupe(), game


def _examples(rep):
    n = rep.stats()["n_examples"]
    got = [rep.read_example(i) for i in range(n)]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def _generation(name, n_games=6, seed=8):
    game = games.load_game(name)
    return RC.fake_export(game, n_games=n_games, seed=seed, openings=RC.random_openings(game, 3, 2, 9))


def _append_kernel_pi(name, bb, roots, slots):
    """The pi the APPEND kernel stores for these root visit counts: a one-ply-per-record export carrying exactly the child
    actions and visit counts of roots[slots], appended to a store of its own."""
    _, _, R = _mods()
    game = games.load_game(name)
    n, mp, mc = len(slots), game.max_game_length(), game.max_children()
    ex = {"game_len": np.ones(n, np.int32), "game_ret0": np.zeros(n, np.float32), "states": np.zeros((n, mp, 2), np.uint64),
          "move": np.zeros((n, mp), np.uint16), "n_children": np.zeros((n, mp), np.uint8),
          "child_action": np.zeros((n, mp, mc), np.uint16), "child_visits": np.zeros((n, mp, mc), np.uint32),
          "value": np.zeros((n, mp)), "start_ply": 0}
    for i, g in enumerate(slots):
        nc = int(roots["n_children"][g])
        ex["states"][i, 0] = bb[i]
        ex["n_children"][i, 0] = nc
        ex["child_action"][i, 0, :nc] = roots["child_action"][g, :nc]
        ex["child_visits"][i, 0, :nc] = roots["child_n"][g, :nc]
        ex["move"][i, 0] = roots["child_action"][g, 0]
    rep = R.DeviceReplay(name, max_games=n, device=0)
    rep.append_export(ex)
    pi = np.array([rep.read_example(i)[0] for i in range(n)])
    rep.close()
    return pi


def _a0c(roots, g):
    nc = int(roots["n_children"][g])
    return float(np.max(np.where(roots["child_n"][g, :nc] > 0, roots["child_q"][g, :nc], -99.0)))


# ------------------------------------------------------------------------------------------------ 1. device states = prefixes
@pytest.mark.parametrize("name,seed", [(C4, 21), (B66, 21)])
def test_device_states_search_as_the_same_positions_reached_by_prefixes(name, seed):
    n, S = 32, 32
    game = games.load_game(name)
    hist = random_positions(name, n, seed, 4, 30)
    assert len(set(map(tuple, hist))) == n
    eng_a, ev_a = _manual_engine(name, n, S)
    eng_a.set_start_positions(hist)
    eng_a.reset(n)
    want, _ = _search(eng_a, ev_a)
    eng_b, ev_b = _manual_engine(name, n, S)
    eng_b.set_start_states_device(*_dev_states(*RA.states_of(game, hist)))
    eng_b.reset(n)
    got, _ = _search(eng_b, ev_b)
    assert want["error_flags"] == 0 and want["n_finished"] == n and (want["phase"] == 5).all()
    assert want["ply"].tolist() == [len(h) for h in hist] and (want["root_n"] == S).all()
    _same_roots(got, want)
    # ... and it supersedes a prefix and an earlier table, as the host form does
    eng_b.set_start_prefix(hist[0][:2])
    eng_b.set_start_states_device(*_dev_states(*RA.states_of(game, hist[::-1])))
    eng_b.reset(n)
    assert eng_b.read_roots()["ply"].tolist() == [len(h) for h in hist[::-1]]
    eng_a.close()
    eng_b.close()


# ------------------------------------------------------------------------------------------------ 2. store round trip
@pytest.mark.parametrize("name", [C4, B54])
def test_store_round_trip_in_the_three_value_modes(name):
    G, S = 64, 24
    ex = _generation(name)
    modes = (None, "soft-Z", "A0C")
    stores = {}
    for m in modes:
        stores[m], U, game = _store(name, [ex])
    uniq = stores[None].read_unique()
    first = uniq["buffer_index"]
    old_pi, old_z = _examples(stores[None])
    assert U == len(first) < len(old_z)                          # there are duplicates that must stay untouched
    eng, ev = _manual_engine(name, G, S)
    buf = eng.alloc_roots()
    want_pi, want_z = {m: old_pi.copy() for m in modes}, {m: old_z.copy() for m in modes}
    refreshed = {m: 0 for m in modes}
    for lo in range(0, U, G):
        idx = np.arange(lo, min(lo + G, U))
        bb, ply = stores[None].gather_states(idx)
        assert np.array_equal(bb.cpu().numpy().view(np.uint64), uniq["bitboards"][idx])
        assert np.array_equal(ply.cpu().numpy(), uniq["ply"][idx])
        eng.set_start_states_device(bb, ply)
        eng.reset(len(idx))
        roots, _ = _search(eng, ev, buf)                         # one search per chunk, shared by the three stores
        assert roots["error_flags"] == 0 and (roots["phase"][:len(idx)] == 5).all()
        slots = list(range(len(idx)))
        pi = _append_kernel_pi(name, uniq["bitboards"][idx], roots, slots)
        for m in modes:
            if m is not None:
                stores[m].gather_states(idx)                    # (each store records its own epoch)
            refreshed[m] += stores[m].refresh_from_roots(idx, buf, m)
            want_pi[m][first[idx]] = pi
            if m == "soft-Z":
                want_z[m][first[idx]] = -roots["root_q"][:len(idx)]
            elif m == "A0C":
                want_z[m][first[idx]] = [_a0c(roots, g) for g in slots]
    changed = 0
    for m in modes:
        assert refreshed[m] == U, m
        got_pi, got_z = _examples(stores[m])
        assert np.array_equal(got_pi, want_pi[m]), m             # first occurrences refreshed, every other example untouched
        assert np.array_equal(got_z, want_z[m]), m
        changed += int((got_pi != old_pi).any()) + int((got_z != old_z).any())
        x, spi, sz = stores[m].sample(U, indices=np.arange(U))
        assert np.array_equal(spi.cpu().numpy(), want_pi[m][first].astype(np.float32)), m
        assert np.array_equal(sz.cpu().numpy(), want_z[m][first].astype(np.float32)), m
        assert stores[m].stats()["fault_flags"] == 0
        stores[m].close()
    assert changed == 5                                          # pi in all three, z in two: the refresh did write
    assert np.array_equal(want_z[None], old_z)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. visit edges
@pytest.mark.parametrize("S", [1, 2])
def test_roots_with_no_or_one_visited_child(S):
    n = 16
    E, _, _ = _mods()
    rep, U, game = _store(C4, [_generation(C4)])
    uniq = rep.read_unique()
    idx = np.arange(3, 3 + n)
    eng, ev = _manual_engine(C4, n, S)
    eng.set_start_states_device(*rep.gather_states(idx))
    eng.reset(n)
    roots, buf = _search(eng, ev)
    assert (roots["phase"] == 5).all() and (roots["child_n"].sum(axis=1) == S - 1).all()
    assert rep.refresh_from_roots(idx, buf, "A0C") == n
    for g, u in enumerate(idx):
        pi, z = rep.read_example(uniq["buffer_index"][u])
        nc = int(roots["n_children"][g])
        acts = roots["child_action"][g, :nc]
        if S == 1:                                               # no child has a visit: uniform over the children, -99.0
            want = np.zeros(7)
            want[acts] = 1.0 / nc
            assert pi.tolist() == want.tolist() and z == -99.0
        else:                                                    # one visit: the host arithmetic of the same counts
            assert pi.tolist() == E.pi_from_visits(acts, roots["child_n"][g, :nc], 7)
            assert z == _a0c(roots, g) and z != -99.0
    assert rep.stats()["fault_flags"] == 0
    rep.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. chunks and ring
def _wrapped_store():
    """An example ring that has wrapped, built as tests/test_replay_store_gpu.py builds one: max_examples of about 1.5
    generations, five generations appended."""
    game = games.load_game(C4)
    gens = [RC.fake_export(game, n_games=8, seed=100 + g, openings=RC.random_openings(game, 4, 3, 1000)) for g in range(5)]
    sizes = [int(ex["game_len"].sum()) for ex in gens]
    max_examples = 3 * sum(sizes) // 10
    assert max(sizes) <= max_examples < 2 * min(sizes) and sum(sizes) > 2 * max_examples
    rep, U, _ = _store(C4, gens, max_games=40, max_examples=max_examples)
    assert rep.stats()["games_dropped"] > 0
    return rep, U


def test_chunked_reanalysis_on_a_wrapped_ring_equals_one_pass():
    E, _, R = _mods()
    S = 24
    out = []
    for n_slots in (16, 40):
        rep, U = _wrapped_store()
        assert U >= 40
        idx = np.random.RandomState(5).permutation(U)[:40]
        before = _examples(rep)
        re = R.Reanalyser(rep, None, n_slots, S, value_target="soft-Z")
        re.analyzer.evaluator = E.HostPolicyEvaluator(re.analyzer.engine, _board_fn(7))
        assert re.reanalyse(indices=idx) == 40
        once = _examples(rep)
        assert (once[0] != before[0]).any() and (once[1] != before[1]).any()
        dup = np.concatenate([idx[:20], idx[10:30]])            # duplicates within a chunk and across chunks
        assert re.reanalyse(indices=dup) >= 30
        again = _examples(rep)
        assert re.analyzer.engine.progress()["error_flags"] == 0 and rep.stats()["fault_flags"] == 0
        out.append((once, again))
        re.close()
        rep.close()
    for k in range(2):                                           # chunks of 16 against one 40-slot pass
        assert np.array_equal(out[0][0][k], out[1][0][k]) and np.array_equal(out[0][1][k], out[1][1][k])
    for k in range(2):                                           # the same positions searched again: the same bits
        assert np.array_equal(out[0][1][k], out[0][0][k])


# ------------------------------------------------------------------------------------------------ 5. refusals
def _set_states_rc(eng, bb, ply):
    rc = eng.lib.az_engine_set_start_states_device(eng._h, C.c_void_p(bb.data_ptr()), C.c_void_p(ply.data_ptr()), int(ply.numel()),
                                                   None)
    torch.cuda.synchronize()
    return rc, eng.lib.az_last_error(eng._h).decode()


def test_self_play_and_arena_engines_are_refused():
    E, _, _ = _mods()
    from alphazero_openspiel_amd import arena
    game = games.load_game(C4)
    bb, ply = _dev_states(*RA.states_of(game, random_positions(C4, 12, 15, 0, 12)))
    sp = E.SelfPlayEngine(C4, 12, n_playouts=8, max_games=12)
    ar = arena.arena_engine(C4, 12, 12, "zero", "random", n_playouts=8)
    for other in (sp, ar):
        rc, msg = _set_states_rc(other, bb, ply)
        assert rc == AZ_E_INVALID and "manual_moves" in msg
        other.close()


@pytest.mark.parametrize("name", [C4, B66])
def test_a_bad_state_is_named_and_leaves_the_previous_table_in_force(name):
    E, _, _ = _mods()
    n, S = 16, 24
    game = games.load_game(name)
    hist = random_positions(name, n, 31, 2, 20)
    bb, ply = RA.states_of(game, hist)
    eng, ev = _manual_engine(name, n, S)
    eng.set_start_states_device(*_dev_states(bb, ply))
    eng.reset(n)
    want, _ = _search(eng, ev)
    other = RA.states_of(game, random_positions(name, n, 32, 2, 20))   # what a refused call must NOT leave behind
    for k, (what, b0, b1, p, rule) in enumerate(RA.bad_states(game)):
        at = 2 * k + 1
        bad_bb, bad_ply = other[0].copy(), other[1].copy()
        bad_bb[at], bad_ply[at] = (b0, b1), p
        bad_bb[at + 3:] = bad_bb[at]                             # further bad states above it: the LOWEST index is named
        bad_ply[at + 3:] = p
        rc, msg = _set_states_rc(eng, *_dev_states(bad_bb, bad_ply))
        assert rc == AZ_E_INVALID and ("game %d:" % at) in msg, (what, msg)
        with pytest.raises(E.EngineError, match="game %d:" % at):
            eng.set_start_states_device(*_dev_states(bad_bb, bad_ply))
    eng.reset(n)
    got, _ = _search(eng, ev)
    _same_roots(got, want)
    eng.close()


def _fault_flags(rep):
    s = _lib.AzReplayStats()
    rc = rep.lib.az_replay_stats_get(rep._h, C.byref(s))
    return rc, int(s.fault_flags)


def test_store_side_refusals():
    n, S = 16, 24
    rep, U, game = _store(C4, [_generation(C4)], max_games=12)
    uniq = rep.read_unique()
    eng, ev = _manual_engine(C4, n, S)
    # an index outside the de-duplicated list: a fault flag, and a state the engine refuses
    bb, ply = rep.gather_states([0, 1, U, 2])
    assert ply.cpu().tolist() == [int(uniq["ply"][0]), int(uniq["ply"][1]), -1, int(uniq["ply"][2])]
    assert _fault_flags(rep) == (AZ_E_DEVICE, 2) and _fault_flags(rep) == (0, 0)
    rc, msg = _set_states_rc(eng, bb, ply)
    assert rc == AZ_E_INVALID and "game 2:" in msg
    # roots of positions of ANOTHER ply at one slot: that example is skipped, the others are refreshed
    idx = np.arange(n)
    bb, ply = rep.gather_states(idx)
    odd = int(np.nonzero(uniq["ply"] != uniq["ply"][5])[0][-1])
    bb[5], ply[5] = rep.gather_states([odd])[0][0], int(uniq["ply"][odd])
    eng.set_start_states_device(bb, ply)
    eng.reset(n)
    roots, buf = _search(eng, ev)
    before = _examples(rep)
    rep.gather_states(idx)
    small = rep.lib.az_replay_refresh_from_roots(rep._h, C.c_void_p(rep._indices(idx).data_ptr()), n, C.c_void_p(buf.data_ptr()),
                                                 int(buf.numel()) - 1, 1, None)
    assert small == AZ_E_INVALID and "roots_bytes" in rep.lib.az_replay_last_error(rep._h).decode()
    assert all(np.array_equal(a, b) for a, b in zip(_examples(rep), before))
    assert rep.refresh_from_roots(idx, buf, "soft-Z") == n - 1
    assert _fault_flags(rep) == (AZ_E_DEVICE, 4)
    after = _examples(rep)
    skipped = int(uniq["buffer_index"][5])
    assert np.array_equal(after[0][skipped], before[0][skipped]) and after[1][skipped] == before[1][skipped]
    for g in (0, 4, 6, n - 1):
        assert after[1][uniq["buffer_index"][g]] == -roots["root_q"][g]
    # a refresh after an intervening append: the indices may name other records
    rep.append_export(_generation(C4, n_games=2, seed=3))
    with pytest.raises(RuntimeError, match=r"\(%d\)" % AZ_E_STATE):
        rep.refresh_from_roots(idx, buf, "soft-Z")
    rep.dedupe()
    with pytest.raises(RuntimeError, match=r"\(%d\)" % AZ_E_STATE):     # ... and a dedupe alone does not make them valid again
        rep.refresh_from_roots(idx, buf, "soft-Z")
    with pytest.raises(ValueError):
        rep.refresh_from_roots(idx, buf, "on-policy")
    rep.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. fused net end to end
def _c4_net(seed):
    from alphazero_openspiel_amd.network import Net
    torch.manual_seed(seed)
    return Net([3, 6, 7], 7, n_blocks=2, n_filters=50).eval()


def test_reanalyser_with_the_fused_net_end_to_end():
    _, _, R = _mods()
    rep, U, game = _store(C4, [_generation(C4, n_games=8)])
    assert U >= 64
    first = rep.read_unique()["buffer_index"]
    with R.Reanalyser(rep, _c4_net(3), n_slots=64, n_playouts=32, value_target="soft-Z", eval_precision="f32x") as re:
        idx = re.draw(64, seed=1).cpu().numpy()
        assert len(set(idx.tolist())) == 64 and idx.min() >= 0 and idx.max() < U
        before = _examples(rep)
        assert re.reanalyse(n=64, seed=1) == 64
        one = _examples(rep)
        rows = first[idx]
        assert (one[0][rows] != before[0][rows]).any(axis=1).sum() > 32 and (np.abs(one[1][rows]) <= 1.0).all()
        untouched = np.setdiff1d(np.arange(len(before[1])), rows)
        assert np.array_equal(one[0][untouched], before[0][untouched]) and np.array_equal(one[1][untouched], before[1][untouched])
        # pi_k = fl(nv_k / s), s = the float sum of the 7 nv_k (6 additions of partial sums <= s: off from the exact sum by at
        # most 6 * 2^-53 relative), one rounding per division (the weights nv_k / s sum to about 1: 2^-53 in all), and the sum
        # taken here (6 additions of partial sums <= 1: 6 * 2^-53): 13 * 2^-53, and one more for the second-order terms
        assert (np.abs(one[0][rows].sum(axis=1) - 1.0) <= 14 * 2.0 ** -53).all()
        assert (one[0][rows] >= 0).all()
        assert re.analyzer.engine.progress()["error_flags"] == 0 and rep.stats()["fault_flags"] == 0
        re.set_evaluator(_c4_net(4))
        assert re.reanalyse(n=64, seed=1) == 64
        two = _examples(rep)
        assert (two[0][rows] != one[0][rows]).any()
        assert np.array_equal(two[0][untouched], before[0][untouched])
        assert re.analyzer.engine.progress()["error_flags"] == 0 and rep.stats()["fault_flags"] == 0
    rep.close()
