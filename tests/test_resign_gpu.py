"""Self-play resignation on the device (az_engine_set_resign, az_engine_resign_info_device and their Python facade).

Every comparison is == (there are no tolerances).  References:
  * the criterion: two plain engines, soft-Z and A0C, whose rec_value columns are its two expressions - and, with injected draws
    and the hashed policy, the model's games of tests/resign_cases.py (which tests/test_resign_host.py shows to split as needed);
  * the games: the plain engine's own, which the suite pins to the oracle - a resigned game is their prefix;
  * the coin: the Python Philox of tests/philox_cases.py;
  * the store: tests/replay_cases.FifoModel fed the shortened games.
4 slots, 8 games, 24 playouts (6 for a fast move)."""
import functools

import numpy as np
import pytest
import torch

import replay_cases as RC
import resign_cases as R
from alphazero_openspiel_amd import games
from forced_playouts_cases import draws, geometry
from net_cases import drifted_net
from oracle import fakepolicy
from playout_cap_cases import check_store as _check, expect as _expect, same as _same, same_game as _same_game

pytestmark = pytest.mark.gpu

C4, B66, S, FAST, G, N = R.C4, R.B66, R.S, R.FAST, R.G, R.N
AZ_E_INVALID, AZ_E_STATE = -1, -3
INF = float("inf")


# ------------------------------------------------------------------------------------------------ engines
def _tick_until_done(eng, ev, n, rows_tail=False, groups=None):
    obs, pri, val = eng.alloc_io()
    rows = None
    for tick in range(400000):
        if groups is not None:
            for first, cnt in groups:
                eng.advance_slots(first, cnt, pri, val, obs)
            ev(obs, pri, val)
        elif rows is None:
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        else:
            eng.advance_rows(rows, pri, val, obs)
            ev(obs[:rows], pri[:rows], val[:rows])
        if tick % 8 == 7:
            p = eng.progress()
            if p["games_done"] >= n:
                return rows
            if rows_tail and p["games_started"] >= n and p["slots_idle"] > (0 if rows is None else eng.G - rows):
                rows = eng.compact_rows()
    raise AssertionError("games did not finish: %r" % (eng.progress(),))


def _injected(case, backup="soft-Z", resign=None, setup=None, starts=None, n_slots=G, **how):
    """The case's games on an engine with injected draws and the hashed policy -> (export, resign info or None)."""
    from alphazero_openspiel_amd import engine as E
    c = R.CASES[case]
    mc = geometry(c["game"])[2]
    etas, us = draws(c["draws"], c["game"], N)
    eng = E.SelfPlayEngine(c["game"], n_slots, n_playouts=S, rng="injected", max_games=N, device=0, seed=c["seed"], backup=backup,
                           **c["kw"])
    try:
        if starts is not None:
            eng.set_game_starts(starts)
        if c["cap"] is not None:
            eng.set_playout_cap(*c["cap"])
        if setup is not None:
            setup(eng)
        if resign is not None:
            eng.set_resign(*resign)
        eng.reset(N)
        eng.set_injected_rng([[row[:mc] for row in e] for e in etas], us, absolute_ply=True)
        A, salt = eng.A, c["salt"]
        ev = E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, A, salt))
        _tick_until_done(eng, ev, N, **how)
        prog = eng.progress()
        assert prog["games_done"] == N and prog["error_flags"] == 0
        ex = eng.export()
        ex["full"] = eng.full_moves_device().cpu().numpy()
        ex["packed"] = eng.export_device().cpu().numpy()
        return ex, (eng.resign_info() if resign is not None else None)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _plain(case, backup):
    """The plain engine's generation of a case (computed once, shared, never changed)."""
    return _injected(case, backup)[0]


def _device_crit(softz, a0c):
    """Per game the criterion per ply played, from the value columns of two plain exports of the same games."""
    assert softz["game_len"].tolist() == a0c["game_len"].tolist() and (softz["move"] == a0c["move"]).all()
    p0 = np.broadcast_to(np.asarray(softz["start_ply"]), (len(softz["game_len"]),))
    return R.crit_of([softz["value"][i, p0[i]:p0[i] + n].tolist() for i, n in enumerate(softz["game_len"])],
                     [a0c["value"][i, p0[i]:p0[i] + n].tolist() for i, n in enumerate(a0c["game_len"])])


def _expect_from(plain, crit, v, p, seed, min_ply=0, first_id=0):
    """What the rule makes of the plain engine's games (the expectation of tests/resign_cases.py, on the device's own figures)."""
    p0 = np.broadcast_to(np.asarray(plain["start_ply"]), (len(crit),))
    out = []
    for i, cr in enumerate(crit):
        s = int(p0[i])
        full = plain["full"][i, s:s + len(cr)].tolist() if "full" in plain else None
        ply, low = R.expect(cr, v, s, min_ply, full)
        through = ply >= 0 and R.plays_through(seed, first_id + i, p)
        resigned = ply >= 0 and not through
        if resigned:
            _, low = R.expect(cr[:ply - s + 2], v, s, min_ply, full)
        out.append(dict(ply=ply, low=low, through=through, resigned=resigned, start=s,
                        length=ply - s + 1 if resigned else len(cr),
                        ret0=R.resign_ret0(ply) if resigned else float(plain["game_ret0"][i])))
    return out


def _check_games(got, info, plain, want, what, j0=0):
    """Games j0.. of `got` are what `want` says of the plain games: a resigned game is the plain game's plies up to and including
    its resign ply, byte for byte, with the resigner's loss as its result; every other game is the plain game."""
    for i, w in enumerate(want):
        j, s, tag = j0 + i, w["start"], "%s: game %d" % (what, i)
        assert int(got["game_len"][j]) == w["length"] >= 1, (tag, int(got["game_len"][j]), w)
        assert float(got["game_ret0"][j]) == w["ret0"], tag
        rows = slice(s, s + w["length"])
        for key in ("states", "move", "n_children", "value") if got.get("on_policy") is None else ("states", "move", "n_children"):
            _same(got[key][j, rows], plain[key][i, rows], "%s: %s" % (tag, key))
        live = np.arange(got["child_action"].shape[2])[None, :] < plain["n_children"][i, rows][:, None]
        for key in ("child_action", "child_visits"):
            _same(got[key][j, rows][live], plain[key][i, rows][live], "%s: %s" % (tag, key))
        if info is not None:
            assert int(info["ply"][j]) == w["ply"], (tag, int(info["ply"][j]), w)
            assert bool(info["resigned"][j]) == w["resigned"] and bool(info["playthrough"][j]) == w["through"], tag
            assert info["low"][j].tolist() == w["low"], (tag, info["low"][j].tolist(), w["low"])


# ------------------------------------------------------------------------------------------------ 1. the criterion and the rule
@pytest.mark.parametrize("case", list(R.CASES))
def test_the_devices_criterion_is_the_models(case):
    softz, a0c = _plain(case, "soft-Z"), _plain(case, "A0C")
    crit = _device_crit(softz, a0c)
    assert crit == R.model_crit(case)
    assert [softz["move"][i, :n].tolist() for i, n in enumerate(softz["game_len"])] == \
        [g["actions"] for g in R.model_games(case, "soft-Z")]
    c = R.CASES[case]
    want = _expect_from(softz, crit, c["v"], 0.5, c["seed"])
    model = R.expected_games(case, p=0.5)
    assert [(w["ply"], w["low"], w["through"], w["length"], w["ret0"]) for w in want] == \
        [(m["ply"], m["low"], m["through"], m["length"], m["ret0"]) for m in model]


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("case", list(R.CASES))
def test_games_follow_the_rule_and_the_coin(case, p):
    """p = 0: every game with a resign ply is cut there.  p = 1: the plain generation, byte for byte, and the side information says
    where each game would have resigned.  p = 0.5: each game follows its own coin.  The cap case: only full plies resign."""
    c = R.CASES[case]
    softz, a0c = _plain(case, "soft-Z"), _plain(case, "A0C")
    want = _expect_from(softz, _device_crit(softz, a0c), c["v"], p, c["seed"])
    got, info = _injected(case, resign=(c["v"], p))
    _check_games(got, info, softz, want, "%s p = %g" % (case, p))
    assert sum(w["resigned"] for w in want) == (0 if p == 1.0 else sum(m["resigned"] for m in R.expected_games(case, p=p)))
    if p == 1.0:                                                                   # the packed export: the rows of every game's plies
        from alphazero_openspiel_amd.engine import unpack_device_export
        mp, mc = got["move"].shape[1], got["child_action"].shape[2]
        gx, wx = unpack_device_export(got["packed"], N, mp, mc), unpack_device_export(softz["packed"], N, mp, mc)
        assert gx["game_len"].tobytes() == wx["game_len"].tobytes() and gx["game_ret0"].tobytes() == wx["game_ret0"].tobytes()
        for j in range(N):
            _same_game(gx, j, wx, j, 0, "packed export: game %d" % j)
        assert info["playthrough"].tolist() == [w["ply"] >= 0 for w in want] and not info["resigned"].any()
    if c["cap"] is not None:
        for w, m in zip(want, got["full"]):
            assert w["ply"] < 0 or m[w["ply"]] == 1


def test_on_policy_targets_follow_from_the_new_result():
    case = "c4"
    c = R.CASES[case]
    softz, a0c = _plain(case, "soft-Z"), _plain(case, "A0C")
    want = _expect_from(softz, _device_crit(softz, a0c), c["v"], 0.0, c["seed"])
    got, info = _injected(case, backup="on-policy", resign=(c["v"], 0.0))
    got["on_policy"] = True
    _check_games(got, info, softz, want, "on-policy")
    for i, w in enumerate(want):
        z = [w["ret0"] if t % 2 == 0 else -w["ret0"] for t in range(w["length"])]
        assert got["value"][i, :w["length"]].tolist() == z, i
    assert any(w["resigned"] and w["ret0"] != float(softz["game_ret0"][i]) for i, w in enumerate(want))   # a result did change


# ------------------------------------------------------------------------------------------------ 2. min_ply and game starts
def test_min_ply_counts_from_the_games_own_start():
    case, min_ply = "c4", 4
    c = R.CASES[case]
    base = _plain(case, "soft-Z")
    starts = [base["move"][i, :3].tolist() if i % 2 == 0 else [] for i in range(N)]           # every other game forked 3 plies in
    softz, a0c = (_injected(case, b, starts=starts)[0] for b in ("soft-Z", "A0C"))
    assert softz["start_ply"].tolist() == [3, 0] * (N // 2)
    crit = _device_crit(softz, a0c)
    want = _expect_from(softz, crit, c["v"], 0.0, c["seed"], min_ply=min_ply)
    loose = _expect_from(softz, crit, c["v"], 0.0, c["seed"])
    assert [w["ply"] for w in want] != [w["ply"] for w in loose]                    # min_ply bites on these games
    assert all(w["ply"] < 0 or w["ply"] - w["start"] >= min_ply for w in want)
    got, info = _injected(case, resign=(c["v"], 0.0, min_ply), starts=starts)
    _check_games(got, info, softz, want, "min_ply")


# ------------------------------------------------------------------------------------------------ 3. composed, cleared, ways to tick
def test_composed_with_solver_fpu_and_mirror():
    case = "c4"
    c = R.CASES[case]

    def setup(eng):
        eng.set_solver(True)
        eng.set_fpu(0.2, 0.0)
        eng.set_eval_mirror(0.5)

    softz, a0c = (_injected(case, b, setup=setup)[0] for b in ("soft-Z", "A0C"))
    through, info1 = _injected(case, resign=(c["v"], 1.0), setup=setup)              # play-through: the plain games, and where they
    for j in range(N):                                                              # would have resigned, by the engine's own figures
        _same_game(through, j, softz, j, 0, "composed, play-through: game %d" % j)
    # Independently of the feature: under the solver rec_value holds the PROVEN value at a proven root (both targets then record
    # the same -1, 0 or +1) and the raw expressions everywhere else, so wherever the two plain engines' values are not such a
    # pair the criterion is max(soft-Z, A0C) as without the solver.  No such ply before a game's resign ply lies below -v, a
    # resign ply of that kind does, and a player all of whose plies are of that kind has exactly their minimum as `low`.
    crit, raw_resigns = _device_crit(softz, a0c), 0
    for i in range(N):
        n, ply = int(softz["game_len"][i]), int(info1["ply"][i])
        raw = [not (softz["value"][i, t] == a0c["value"][i, t] and softz["value"][i, t] in (-1.0, 0.0, 1.0)) for t in range(n)]
        for t in range(n - 1):                                                      # (the last ply never counts)
            if raw[t] and (ply < 0 or t < ply):
                assert crit[i][t] >= -c["v"], (i, t, crit[i][t])
        if ply >= 0 and raw[ply]:
            assert crit[i][ply] < -c["v"], (i, ply)
            raw_resigns += 1
        for pl in (0, 1):
            mine = [t for t in range(pl, n - 1, 2)]
            seen = [crit[i][t] for t in mine if raw[t]]
            if seen:
                assert info1["low"][i][pl] <= min(seen), (i, pl)
            if len(seen) == len(mine):
                assert info1["low"][i][pl] == (min(seen) if seen else INF), (i, pl)
    assert raw_resigns >= 1                                                         # the check bites on these games
    got, info = _injected(case, resign=(c["v"], 0.0), setup=setup)
    assert info["ply"].tolist() == info1["ply"].tolist() and (info["ply"] >= 0).sum() >= 1
    want = []
    for i in range(N):
        ply, n = int(info1["ply"][i]), int(softz["game_len"][i])
        assert ply < n - 1
        if ply >= 0:                                                                # (a proven root records the proven value: the raw
            assert min(info1["low"][i]) < -c["v"]                                   #  criterion is not in rec_value under the solver)
        want.append(dict(ply=ply, start=0, resigned=ply >= 0, through=False, length=ply + 1 if ply >= 0 else n,
                         ret0=R.resign_ret0(ply) if ply >= 0 else float(softz["game_ret0"][i]), low=info["low"][i].tolist()))
    _check_games(got, info, softz, want, "composed")


def test_set_then_cleared_is_never_set():
    from alphazero_openspiel_amd import engine as E
    case = "b66"
    c = R.CASES[case]
    softz = _plain(case, "soft-Z")

    def setup(eng):
        eng.set_resign(c["v"], 0.0)
        assert eng.resign == (c["v"], 0.0, 0)
        eng.clear_resign()
        assert eng.resign is None
        with pytest.raises(E.EngineError, match=r"\(%d\).*no resignation setting" % AZ_E_STATE):
            eng.resign_info_device(0, 1)

    got, _ = _injected(case, setup=setup)
    assert got["game_len"].tobytes() == softz["game_len"].tobytes() and got["game_ret0"].tobytes() == softz["game_ret0"].tobytes()
    for j in range(N):
        _same_game(got, j, softz, j, 0, "cleared: game %d" % j)


def test_dense_tail_rows_and_two_slot_groups_play_the_same_games():
    case = "c4"
    c = R.CASES[case]
    softz, a0c = _plain(case, "soft-Z"), _plain(case, "A0C")
    want = _expect_from(softz, _device_crit(softz, a0c), c["v"], 0.5, c["seed"])
    got, info = _injected(case, resign=(c["v"], 0.5), rows_tail=True)
    _check_games(got, info, softz, want, "dense rows in the tail")
    got, info = _injected(case, resign=(c["v"], 0.5), n_slots=16, groups=[(0, 8), (8, 8)])
    _check_games(got, info, softz, want, "two slot groups")


# ---- Philox and a network: a captured graph and the stream (neither takes injected draws or a host policy)
@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


SEED_NET, N_NET = 701, 9


def _philox_engine(backup="soft-Z", max_games=N_NET):
    from alphazero_openspiel_amd import engine as E
    return E.SelfPlayEngine(C4, G, n_playouts=S, max_games=max_games, device=0, seed=SEED_NET, backup=backup, keep_search_tree=True)


@functools.lru_cache(maxsize=None)
def _plain_net():
    """-> (soft-Z export, criterion, v): the plain closed generation of N_NET games under the network, and a threshold that lies
    between the third and the fourth lowest of the games' lowest criteria (so three games have a resign ply, the others none)."""
    from alphazero_openspiel_amd import engine as E
    ev, out = _fused(C4), []
    for backup in ("soft-Z", "A0C"):
        eng = _philox_engine(backup)
        prog = E.run_selfplay(eng, ev, N_NET)
        assert prog["games_done"] == N_NET and prog["error_flags"] == 0
        out.append(eng.export())
        eng.close()
    ev.close()
    crit = _device_crit(*out)
    lows = sorted(min(c[:-1]) for c in crit if len(c) > 1)
    assert len(lows) >= 4 and lows[2] < 0.0 and lows[2] < lows[3], lows              # the inputs this test needs
    v = -(lows[2] + min(lows[3], 0.0)) / 2.0
    assert 0.0 < v <= 1.0
    return out[0], crit, v


def test_a_captured_graph_plays_the_same_games():
    from alphazero_openspiel_amd import engine as E
    plain, crit, v = _plain_net()
    want = _expect_from(plain, crit, v, 0.5, SEED_NET)
    assert sum(w["ply"] >= 0 for w in want) == 3
    ev = _fused(C4)
    eng = _philox_engine()
    eng.set_resign(v, 0.5)
    prog = E.run_selfplay(eng, ev, N_NET, use_graph=True, ticks_per_graph=16, check_every=32)
    assert prog["games_done"] == N_NET and prog["error_flags"] == 0
    g = torch.cuda.CUDAGraph()                                                      # the read-back is capturable
    out = (torch.empty(N_NET, dtype=torch.int32, device="cuda"), torch.empty(N_NET, dtype=torch.uint8, device="cuda"),
           torch.empty((N_NET, 2), dtype=torch.float64, device="cuda"))
    eager = eng.resign_info_device()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            cap = eng.resign_info_device()
            for dst, src in zip(out, cap):
                dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    _check_games(eng.export(), E.unpack_resign_info(*eager), plain, want, "captured graph")
    eng.close()
    ev.close()


def test_a_stream_across_a_ring_wrap():
    """A ring of 6 rows, three takes of 3 games: ids 6..8 record into the rows of ids 0..2.  The information is read before each
    take (SelfPlayStream.last_resign_info); what the row's next game shows is its own, not the last game's."""
    from alphazero_openspiel_amd import engine as E
    plain, crit, v = _plain_net()
    want = _expect_from(plain, crit, v, 0.5, SEED_NET)
    ev = _fused(C4)
    eng = _philox_engine(max_games=6)
    stream = E.SelfPlayStream(eng, ev, seed=SEED_NET, use_graph=False, check_every=8, resign=(v, 0.5))
    assert eng.resign == (v, 0.5, 0)
    mp, mc = eng.max_plies, eng.max_children
    for k in range(3):
        with pytest.raises(E.EngineError, match=r"\(%d\).*outside the ring's window" % AZ_E_INVALID):
            eng.resign_info_device(3 * k + 1, 6)
        buf, first = stream.take(3)
        assert first == 3 * k
        got = E.unpack_device_export(buf.cpu().numpy(), 3, mp, mc)
        info = E.unpack_resign_info(*stream.last_resign_info)
        sub = {key: (val[3 * k:3 * k + 3] if isinstance(val, np.ndarray) else val) for key, val in plain.items()}
        _check_games(got, info, sub, want[3 * k:3 * k + 3], "take %d" % k)
        if k:
            with pytest.raises(E.EngineError, match=r"\(%d\).*outside the ring's window" % AZ_E_INVALID):
                eng.resign_info_device(3 * k - 1, 1)                                # taken: its row belongs to a later game
        if k == 0:
            # The rows of ids 0..2 are free: a slot that takes id 6, 7 or 8 clears the row's information (take_next_game).  Four
            # ticks hand ids out and finish no search of 24 playouts, so a started game shows the cleared state - not the finite
            # `low` its row's last game left (every finished game has one).
            assert np.isfinite(info["low"]).any(axis=1).all()
            stream.driver.run(4)
            started = eng.progress()["games_started"]
            assert 6 < started <= 9
            fresh = eng.resign_info(6, started - 6)
            assert fresh["ply"].tolist() == [-1] * (started - 6) and not fresh["resigned"].any() and not fresh["playthrough"].any()
            assert np.isinf(fresh["low"]).all() and (fresh["low"] > 0).all()
    stream.close()
    eng.close()
    ev.close()


# ------------------------------------------------------------------------------------------------ 4. the store
def test_the_store_holds_the_shortened_games():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd import replay
    case = "c4"
    c = R.CASES[case]
    game = games.load_game(C4)
    etas, us = draws(c["draws"], C4, N)
    eng = E.SelfPlayEngine(C4, G, n_playouts=S, rng="injected", max_games=N, device=0, seed=c["seed"], backup="soft-Z", **c["kw"])
    eng.set_resign(c["v"], 0.0)
    eng.reset(N)
    eng.set_injected_rng([[row[:7] for row in e] for e in etas], us, absolute_ply=True)
    ev = E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, 7, c["salt"]))
    _tick_until_done(eng, ev, N)
    ex = eng.export()
    want = R.expected_games(case, p=0.0)
    assert ex["game_len"].tolist() == [w["length"] for w in want] and sum(w["resigned"] for w in want) >= 3
    stores = [replay.DeviceReplay(C4, device=0, max_games=40), replay.DeviceReplay(C4, device=0, max_games=40)]
    stores[0].append_engine(eng)
    stores[1].append_device(eng.export_device(), N)
    eng.close()
    model = RC.FifoModel(40, 40 * game.max_game_length())
    model.append(RC.reference_games(game, ex))
    e = _expect(model)
    assert len(e["flat_z"]) == sum(w["length"] for w in want)
    for rep in stores:
        _check(rep, e)
        rep.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    for what, kw in (("arena", dict(arena_agent="zero", opponent="random")), ("manual_moves", dict(manual_moves=True))):
        eng = E.SelfPlayEngine(C4, G, n_playouts=S, max_games=N, device=0, **kw)
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_resign is for plain self-play engines.*%s" % (AZ_E_INVALID, what)):
            eng.set_resign(0.9)
        assert eng.resign is None
        eng.close()
    eng = E.SelfPlayEngine(C4, G, n_playouts=S, max_games=N, device=0)
    for bad in (dict(v=0.0), dict(v=-0.5), dict(v=1.01), dict(v=float("nan")), dict(v=0.5, playthrough=-0.1), dict(v=0.5, playthrough=1.5),
                dict(v=0.5, playthrough=float("nan")), dict(v=0.5, min_ply=-1)):
        with pytest.raises(E.EngineError, match=r"\(%d\).*v must be in \(0, 1\], p_playthrough in \[0, 1\] and min_ply >= 0" % AZ_E_INVALID):
            eng.set_resign(**bad)
        assert eng.resign is None
    eng.reset(4)
    with pytest.raises(E.EngineError, match=r"\(%d\).*no resignation setting" % AZ_E_STATE):
        eng.resign_info_device()
    eng.set_resign(1.0, 1.0, 3)
    obs, pri, val = eng.alloc_io()
    with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_STATE):                   # the caller resets after a setter
        eng.advance(pri, val, obs)
    with pytest.raises(E.EngineError, match=r"\(%d\).*before az_engine_reset" % AZ_E_STATE):
        eng.resign_info_device(0, 1)
    eng.reset(4)
    info = eng.resign_info()
    assert info["ply"].tolist() == [-1] * 4 and not info["resigned"].any() and np.isinf(info["low"]).all()
    for first, n in ((0, 5), (4, 1), (-1, 2), (3, 2), (0, 0)):
        with pytest.raises(E.EngineError, match=r"\(%d\)" % AZ_E_INVALID):
            eng.resign_info_device(first, n)
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. the facade
def _is_prefix(short, whole):
    return len(short) <= len(whole) and all(a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2] for a, b in zip(short, whole))


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_resign_stats_match_resign_info(p):
    """The generator's first closed generation is the engine's with the generator's seed: its statistics are that engine's
    resign_info(), counted here from the plain games' results (p = 1: every game with a resign ply plays through)."""
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    plain, crit, v = _plain_net()
    want = _expect_from(plain, crit, v, p, SEED_NET)[:N]
    ev = _fused(C4)
    eng = _philox_engine(max_games=N)
    eng.set_resign(v, p)
    prog = E.run_selfplay(eng, ev, N)
    assert prog["games_done"] == N and prog["error_flags"] == 0
    info, ex = eng.resign_info(), eng.export()
    eng.close()
    ev.close()
    _check_games(ex, info, plain, want, "the engine at p = %g" % p)
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", n_playouts=S, n_slots=G, seed=SEED_NET, use_graph=False, backup="soft-Z",
                           resign=(v, p))
    games_ = gen.generate_examples(N)
    gen.close()
    st = gen.resign_stats
    assert [len(g) for g in games_] == ex["game_len"].tolist()
    through = [w for w in want if w["through"]]
    wrong = [w for w in through if w["ret0"] != R.resign_ret0(w["ply"])]            # the resigner did not go on to lose
    assert st["games"] == N and st["resigned"] == int(info["resigned"].sum()) == sum(w["resigned"] for w in want)
    assert st["playthrough_would_resign"] == int((info["playthrough"] & (info["ply"] >= 0)).sum()) == len(through)
    assert st["playthrough_wrong"] == len(wrong)
    if p == 1.0:
        assert len(through) >= 2 and st["resigned"] == 0
    out = ~info["resigned"]
    assert st["low"].tolist() == info["low"][out].tolist() and st["ret0"].tolist() == ex["game_ret0"][out].astype(np.float64).tolist()
    assert st["weight"].tolist() == [1.0 / p if t >= 0 else 1.0 for t in info["ply"][out]]


@pytest.mark.parametrize("how", ["pools", "continuous"])
def test_example_generator_returns_the_prefix_games_and_counts_them(how):
    """A first generator under resign=(1.0, 1.0) never resigns and plays every game through: its games are the plain generator's,
    and its statistics give every game's lowest criterion - from which the threshold of the second generator is taken: halfway
    between the k-th lowest and the next (k = 3, or as many games as dip below 0 at all)."""
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    kw = dict(n_playouts=S, n_slots=G, seed=SEED_NET, use_graph=False, backup="soft-Z")
    kw.update(dict(pool_devices=["cuda:0", "cuda:0"]) if how == "pools" else dict(continuous=True))
    plain = ExampleGenerator(_net(C4), C4, "cuda:0", **kw)
    want = plain.generate_examples(N)
    plain.close()
    through = ExampleGenerator(_net(C4), C4, "cuda:0", resign=(1.0, 1.0), **kw)
    same = through.generate_examples(N)
    through.close()
    assert len(same) == len(want) == N
    for a, b in zip(same, want):
        assert len(a) == len(b) and _is_prefix(a, b) and [x[3] for x in a] == [x[3] for x in b]
    st = through.resign_stats
    assert st["games"] == N and st["resigned"] == 0 and st["playthrough_would_resign"] == 0 and st["low"].shape == (N, 2)
    lows = np.sort(st["low"].min(axis=1))
    k = min(3, int((lows < 0.0).sum()))                                             # the k games that dip lowest get a resign ply
    assert k >= 1 and lows[k - 1] < lows[k], lows                                   # (the inputs this test needs: one at least)
    v = -(lows[k - 1] + min(lows[k], 0.0)) / 2.0
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", resign=(v, 0.0), **kw)
    got = gen.generate_examples(N)
    gen.close()
    st = gen.resign_stats
    assert len(got) == N and st["games"] == N and st["resigned"] == k and st["playthrough_would_resign"] == 0
    assert st["low"].shape == (N - k, 2) and st["ret0"].shape == (N - k,)           # the games that were played out
    short = [i for i in range(N) if len(got[i]) < len(want[i])]
    assert len(short) == k
    for i in range(N):
        assert _is_prefix(got[i], want[i]), i
        if i not in short:
            assert [x[3] for x in got[i]] == [x[3] for x in want[i]]
