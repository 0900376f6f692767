"""Batched position analysis on the GPU: a start position per game (az_engine_set_start_positions), every root from one
kernel (az_engine_export_roots_device), and analysis.analyze_positions / Analyzer on top.

Bar: bit-exact, as in test_engine_parity.py.  Counts and actions are integers; Q and P are IEEE doubles compared with ==.
Both sides of every comparison see the same float32 priors and values, and no random draw enters a search (no root noise,
or an injected eta), so no tolerance is needed or used.

Positions: uniformly random legal moves from a fixed numpy seed to a random target ply, stopping before a move that would
end the game (analysis_positions.random_positions); every generated position is searched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from analysis_positions import random_positions
from conftest import load_golden
from oracle import fakepolicy

pytestmark = pytest.mark.gpu

ROOT_FIELDS = ("N", "Q", "actions", "cN", "cQ", "cP")


def _mods():
    from alphazero_openspiel_amd import analysis, engine
    return engine, analysis


def _board_fn(A, salt):
    return lambda board: fakepolicy.fake_eval(board, A, salt)


def _root_of(roots, g):
    """Slot g of read_roots() in the shape read_root() returns."""
    n = int(roots["n_children"][g])
    return {"N": int(roots["root_n"][g]), "Q": float(roots["root_q"][g]), "actions": roots["child_action"][g, :n].tolist(),
            "cN": roots["child_n"][g, :n].tolist(), "cQ": roots["child_q"][g, :n].tolist(),
            "cP": roots["child_p"][g, :n].tolist()}


def _search_all(eng, ev, S, check_every=4):
    """advance + evaluate until the root export's header says every slot is done -> read_roots()."""
    obs, pri, val = eng.alloc_io()
    buf = eng.alloc_roots()
    for _ in range(4 * S + 16):
        for _ in range(check_every):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
        eng.export_roots_device(buf)
        if int(buf[:16].view(torch.int32)[0].item()) == eng.G:
            break
    else:
        pytest.fail("searches did not finish")
    return eng.read_roots(buf)


def _search_single(eng1, ev1, io, history, S):
    """Today's single-position path: 1-slot engine, set_start_prefix, reset, tick to phase 5, read_root."""
    obs, pri, val = io
    eng1.set_start_prefix(history)
    eng1.reset(1)
    for _ in range(4 * S + 16):
        eng1.advance(pri, val, obs)
        info = eng1.read_slot(0)
        if info["phase"] == 5:
            break
        if info["phase"] in (3, 4):
            ev1(obs, pri, val)
    else:
        pytest.fail("single search did not finish")
    return eng1.read_root(0), info


@pytest.mark.parametrize("game,seed", [("connect_four", 11), ("breakthrough(rows=6,columns=6)", 11)])
def test_batched_roots_equal_the_single_position_path(game, seed):
    """64 distinct positions in one 64-slot engine against 64 runs of the 1-slot path: every field of every root."""
    E, _ = _mods()
    S, salt, n = 40, 9, 64
    hist = random_positions(game, n, seed, 4, 30)
    assert len(set(map(tuple, hist))) == n
    eng = E.SelfPlayEngine(game, n, n_playouts=S, use_dirichlet=False, manual_moves=True, max_games=n)
    eng.set_start_positions(hist)
    eng.reset(n)
    roots = _search_all(eng, E.HostPolicyEvaluator(eng, _board_fn(eng.A, salt)), S)
    prog = eng.progress()
    assert prog["error_flags"] == 0 and roots["error_flags"] == 0
    assert prog["sims"] == n * S and roots["n_finished"] == n
    eng1 = E.SelfPlayEngine(game, 1, n_playouts=S, use_dirichlet=False, manual_moves=True, max_games=1)
    ev1 = E.HostPolicyEvaluator(eng1, _board_fn(eng1.A, salt))
    io = eng1.alloc_io()
    for g in range(n):
        want, info = _search_single(eng1, ev1, io, hist[g], S)
        got = _root_of(roots, g)
        for k in ROOT_FIELDS:
            assert got[k] == want[k], (g, k)
        assert eng.read_root(g) == want, g  # the per-slot read of the same engine agrees with both
        assert (int(roots["game_id"][g]), int(roots["phase"][g]), int(roots["ply"][g]), int(roots["sims_done"][g])) == \
               (g, 5, len(hist[g]), info["sims_done"]), g
        assert info["ply"] == len(hist[g])
    assert eng1.progress()["error_flags"] == 0
    eng.close()
    eng1.close()


@pytest.mark.parametrize("idx", range(7))
def test_batched_root_equals_the_reference_fixture(idx):
    """The reference's own search results (tests/golden/mcts_trace.json): the case's prefix as game 5 of a 16-slot engine whose
    other slots search other positions of the same game, the case's eta injected for game 5."""
    E, _ = _mods()
    case = load_golden("mcts_trace.json")[idx]
    S, G, gid = case["n_playouts"], 16, 5
    hist = random_positions(case["game"], G, 100 + idx, 0, 24)
    hist[gid] = list(case["prefix"])
    eng = E.SelfPlayEngine(case["game"], G, n_playouts=S, c_puct=case["c_puct"], use_dirichlet=case["use_dirichlet"],
                           dirichlet_ratio=case["dirichlet_ratio"], manual_moves=True, rng="injected", max_games=G)
    eng.set_start_positions(hist)
    eng.reset(G)
    etas = [[] for _ in range(G)]
    etas[gid] = [[0.0]] * len(case["prefix"]) + [case["eta"] or [0.0]]
    eng.set_injected_rng(etas, [[0.0]] * G, absolute_ply=True)
    roots = _search_all(eng, E.HostPolicyEvaluator(eng, _board_fn(eng.A, case["salt"])), S)
    got = _root_of(roots, gid)
    assert int(roots["game_id"][gid]) == gid
    assert got == case["final"]
    pi = np.zeros(eng.A)  # MCTS.get_normalized_visit_counts (mcts.py:155-162): what the fixture's "pi" holds
    total = sum(got["cN"])
    for a, n in zip(got["actions"], got["cN"]):
        pi[a] = float(n) / total
    want_pi = np.zeros(eng.A)
    for a, p in case["pi"].items():
        want_pi[int(a)] = p
    assert pi.tolist() == want_pi.tolist()
    assert (roots["phase"] == 5).all() and (roots["root_n"] == S).all()
    assert eng.progress()["error_flags"] == 0
    eng.close()


def _c4_net(blocks=2):
    from alphazero_openspiel_amd.network import Net
    torch.manual_seed(3)
    return Net([3, 6, 7], 7, n_blocks=blocks, n_filters=50).eval()


RESULT_KEYS = ("visits", "q", "priors", "root_q", "root_n", "best_action")


def test_analyze_positions_does_not_depend_on_chunks_or_slot_count():
    """Fused net at f32x (output bits do not depend on the batch size), 300 positions, 32 playouts: one chunk of 300 slots,
    three chunks of 128 and 300 chunks of one slot give identical results."""
    _, A = _mods()
    net = _c4_net()
    hist = random_positions("connect_four", 300, 12, 0, 30)
    res = {k: A.analyze_positions(net, "connect_four", hist, n_playouts=32, n_slots=k, device="cuda:0") for k in (300, 128, 1)}
    for k, r in res.items():
        assert r["progress"]["error_flags"] == 0 and r["progress"]["sims"] == 300 * 32, k
        assert r["progress"]["chunks"] == {300: 1, 128: 3, 1: 300}[k]
        assert (r["root_n"] == 32).all() and (r["visits"].sum(axis=1) == 31).all(), k
        assert (r["best_action"] == np.argmax(r["visits"], axis=1)).all()
    for k in (128, 1):
        for f in RESULT_KEYS:
            assert np.array_equal(res[k][f], res[300][f]), (k, f)
    # the priors are the network's, not a constant: positions differ
    assert len({r.tobytes() for r in res[300]["priors"]}) > 200


def test_ticks_and_root_export_inside_a_captured_graph():
    """16 ticks + the root export captured with torch.cuda.graph leave the same buffer as the eager calls."""
    E, _ = _mods()
    from alphazero_openspiel_amd import fusednet
    net = _c4_net()
    n, S = 64, 24
    hist = random_positions("connect_four", n, 13, 0, 30)
    bufs = []
    for use_graph in (False, True):
        eng = E.SelfPlayEngine("connect_four", n, n_playouts=S, use_dirichlet=False, manual_moves=True, max_games=n)
        fn = fusednet.FusedNet(net, "cuda:0", max_boards=n, precision="f32x")
        eng.set_start_positions(hist)
        eng.reset(n)
        obs, pri, val = eng.alloc_io()
        buf = eng.alloc_roots()

        def ticks(k):
            for _ in range(k):
                eng.advance(pri, val, obs)
                fn(obs, pri, val)

        seen = []
        if use_graph:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ticks(2)
                eng.export_roots_device(buf)  # (first use outside the capture)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ticks(16)
                eng.export_roots_device(buf)
            for _ in range(2):
                graph.replay()
                torch.cuda.synchronize()
                seen.append(buf.cpu().numpy().copy())
        else:
            ticks(2)
            for _ in range(2):
                ticks(16)
                eng.export_roots_device(buf)
                torch.cuda.synchronize()
                seen.append(buf.cpu().numpy().copy())
        assert eng.progress()["error_flags"] == 0
        bufs.append(seen)
        fn.close()
        eng.close()
    mid = E.unpack_roots_export(bufs[0][0], n, 7)
    assert mid["sims_done"].max() > 0 and mid["n_finished"] < n  # the first snapshot is taken mid-search
    assert E.unpack_roots_export(bufs[0][1], n, 7)["n_finished"] == n
    for i in range(2):
        print("snapshot", i, "headers", bufs[0][i][:16].view(np.int32).tolist(), bufs[1][i][:16].view(np.int32).tolist())
        assert np.array_equal(bufs[0][i], bufs[1][i]), (i, np.nonzero(bufs[0][i] != bufs[1][i])[0][:16].tolist())


def test_continue_after_analysis():
    """update_root(best_action, keep_subtree=False) on all slots and another search = a fresh analysis of the histories
    extended by those actions.  connect_four positions of at most 4 plies: no single move can end the game (a win needs 7
    plies), so every slot continues."""
    _, A = _mods()
    net = _c4_net()
    n, S = 64, 32
    hist = random_positions("connect_four", n, 14, 0, 4)
    assert max(map(len, hist)) <= 4
    with A.Analyzer(net, "connect_four", n, n_playouts=S, device="cuda:0") as an:
        an.load(hist)
        an.search()
        first = an.results()
        best = first["best_action"]
        an.update_root(best, keep_subtree=False)
        an.search()
        second = an.results()
        assert an.engine.progress()["error_flags"] == 0
    assert (first["phase"] == 5).all() and (second["phase"] == 5).all()
    fresh0 = A.analyze_positions(net, "connect_four", hist, n_playouts=S, device="cuda:0")
    fresh1 = A.analyze_positions(net, "connect_four", [h + [int(a)] for h, a in zip(hist, best)], n_playouts=S, device="cuda:0")
    assert fresh0["progress"]["error_flags"] == 0 and fresh1["progress"]["error_flags"] == 0
    for f in RESULT_KEYS:
        assert np.array_equal(first[f], fresh0[f]), f
        assert np.array_equal(second[f], fresh1[f]), f


def _set_positions_rc(eng, hist):
    E, _ = _mods()
    actions, lengths, stride = E.pack_histories(hist)
    ip = C.POINTER(C.c_int32)
    rc = eng.lib.az_engine_set_start_positions(eng._h, actions.ctypes.data_as(ip), lengths.ctypes.data_as(ip), stride, len(hist))
    return rc, eng.lib.az_last_error(eng._h).decode()


def test_refusals():
    """Host-side argument checks: an illegal action (game 5), a prefix that ends the game (game 9), engines that keep one
    start ply, a root buffer that is too small."""
    E, _ = _mods()
    from alphazero_openspiel_amd import arena
    AZ_E_INVALID = -1
    hist = random_positions("connect_four", 12, 15, 0, 12)
    eng = E.SelfPlayEngine("connect_four", 12, n_playouts=8, use_dirichlet=False, manual_moves=True, max_games=12)
    assert _set_positions_rc(eng, hist)[0] == 0
    bad = [list(h) for h in hist]
    bad[5] = [0] * 7  # column 0 holds six stones
    rc, msg = _set_positions_rc(eng, bad)
    assert rc == AZ_E_INVALID and "game 5" in msg and "illegal" in msg
    bad = [list(h) for h in hist]
    bad[9] = [0, 1, 0, 1, 0, 1, 0]  # four in column 0
    rc, msg = _set_positions_rc(eng, bad)
    assert rc == AZ_E_INVALID and "game 9" in msg and "ends the game" in msg
    with pytest.raises(E.EngineError, match="game 9"):
        eng.set_start_positions(bad)
    # a refused table changes nothing: the accepted one is still in force
    eng.reset(12)
    buf = eng.alloc_roots()
    assert eng.read_roots(buf)["ply"].tolist() == [len(h) for h in hist]
    rc = eng.lib.az_engine_export_roots_device(eng._h, C.c_void_p(buf.data_ptr()), eng.roots_device_bytes() - 1, None)
    assert rc == AZ_E_INVALID and "smaller" in eng.lib.az_last_error(eng._h).decode()
    # set_start_prefix clears the table
    eng.set_start_prefix([3, 3])
    eng.reset(12)
    assert eng.read_roots(buf)["ply"].tolist() == [2] * 12
    eng.close()
    sp = E.SelfPlayEngine("connect_four", 12, n_playouts=8, max_games=12)
    ar = arena.arena_engine("connect_four", 12, 12, "zero", "random", n_playouts=8)
    for other in (sp, ar):
        rc, msg = _set_positions_rc(other, hist)
        assert rc == AZ_E_INVALID and "manual_moves" in msg
        other.close()
