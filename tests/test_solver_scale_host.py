"""What keeps test_solver_scale_gpu.py from passing vacuously, asserted without a GPU: the Python model of tests/solver_cases.py
is right at 400-1600 playouts and at depths 64-150 (whole trees against the C oracle with the solver off, every status of the late
connect_four case against a brute-force negamax), and the cases reach what they are for - proof climbs of 5 and more levels,
thousands of skipped lost children, playouts stopped at proven non-terminal nodes, kept trees with hundreds of proven nodes, proofs
that walk across depths 64 and 128 of the select path, searches ended early and kept proven roots.  The small pools of the
whole-game runs are sized here from the model's tree sizes.  Everything is compared with ==."""
import numpy as np
import pytest

import product_scale_cases as PS
import solver_cases as SC


def _same_tree(got, want, where):
    assert len(got["N"]) == len(want["N"]), where
    for f in ("parent", "action", "N"):
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), (where, f)
    for f in ("Q", "P"):                                                # bit patterns: -0.0 and NaN cannot hide
        assert np.array_equal(got[f].view(np.int64), want[f].view(np.int64)), (where, f)


# ------------------------------------------------------------------------------------------------ the model against the oracle
@pytest.mark.parametrize("key", sorted(SC.SCALE_CASES))
def test_model_without_the_solver_builds_the_oracles_trees(key):
    """solver=False: after every search of the sequence the model's whole tree is MCTS.dump_tree() of the C oracle on the same
    sequence (search, update_root(most visited child), search again) - node count, parent, action and N as integers, Q and P as
    bit patterns - and so are the five counters and the move."""
    got = SC.scale_model(key, solver=False)
    want = SC.oracle_sequence(key, len(got["plies"]))
    assert len(want) == len(got["plies"]) >= 3
    for k, (ply, row) in enumerate(zip(got["plies"], want)):
        _same_tree(ply["tree"], row["tree"], (key, "search", k))
        assert not ply["tree"]["status"].any()
        assert ply["counters"] == row["counters"] and ply["move"] == row["move"], (key, k)
        assert ply["nodes"] == len(row["tree"]["N"]) and ply["ran"] == SC.SCALE_CASES[key]["n_playouts"]
        if k:                                                           # what update_root kept, before it is searched again
            prev = want[k - 1]
            _same_tree(ply["kept"], PS.sub_bfs(prev["tree"], 1 + prev["root"]["actions"].index(prev["move"])), (key, "kept", k))
            assert ply["kept_nodes"] == len(ply["kept"]["N"])
    assert not any(got["solver_effects"].values()) and not got["events"]
    print(key, "searches", len(want), "largest tree", max(p["nodes"] for p in got["plies"]))


@pytest.mark.parametrize("key", sorted(SC.DEEP_CASES))
def test_model_without_the_solver_builds_the_oracles_deep_trees(key):
    """The same under the line policy, one search playout by playout: chains 90-150 plies deep."""
    got = SC.deep_model(key, solver=False)
    tree, counters = SC.oracle_deep(key)
    _same_tree(got["plies"][0]["tree"], tree, key)
    assert got["plies"][0]["counters"] == counters
    assert counters["terminal_hits"] > 0 and not got["events"]


# ------------------------------------------------------------------------------------------------ soundness
def test_every_status_of_the_late_case_is_the_negamax_value():
    """c4_3_14: 14 empty cells.  Every status the model assigns in the whole sequence (161 of them) equals the memo-free negamax
    value, searched to depth 14 - the full depth of the position, no cut (it takes 0.1 s: late positions have few open columns).
    No other scale case starts with at most 14 empty cells."""
    assert [k for k, c in SC.SCALE_CASES.items() if c["game"] == SC.C4 and 42 - len(c["start"]) <= 14] == ["c4_3_14"]
    seen = []

    def audit(state, status, mover):
        assert status in (SC.WIN, SC.DRAW, SC.LOSS)
        assert SC.check_status(state, status, mover, max_depth=14), (status, mover, state.board().tolist())
        seen.append(status)

    w = SC.scale_model("c4_3_14", audit=audit)
    want = SC.scale_model("c4_3_14")
    assert len(seen) >= 100 and {SC.WIN, SC.LOSS} <= set(seen)
    assert w["actions"] == want["actions"] and w["events"] == want["events"]     # (the audit changes nothing)
    assert [p["raw"] for p in w["plies"]] == [p["raw"] for p in want["plies"]]


# ------------------------------------------------------------------------------------------------ what the cases reach
def _summary(w):
    plies = w["plies"]
    return dict(SC.event_stats(w["events"]), loss_skipped=w["solver_effects"]["loss_skipped"],
                stopped_nonterminal=w["solver_effects"]["stopped_nonterminal"], ran=[p["ran"] for p in plies],
                kept_proven=[p["kept_proven"] for p in plies], largest_tree=max(p["nodes"] for p in plies))


@pytest.mark.parametrize("key", sorted(SC.SCALE_CASES))
def test_scale_cases_reach_what_they_are_for(key):
    c, w = SC.SCALE_CASES[key], SC.scale_model(key)
    s = _summary(w)
    print(key, s)
    plies = w["plies"]
    assert w["ret0"] is not None                                         # played to the end
    for p in plies:                                                      # only a proven root ends a search early
        assert p["ran"] == c["n_playouts"] or p["status"] != SC.UNKNOWN
    assert w["counters"]["sims"] == sum(s["ran"])
    if key not in SC.LATE_C4:
        assert s["loss_skipped"] >= 1000
    else:
        assert s["max_levels"] >= 5
    # a search that ends early at a proven root, and kept proven roots whose search runs no playout
    assert any(p["status"] != SC.UNKNOWN and p["ran"] < c["n_playouts"] for p in plies)
    kept_proven_roots = [p for p in plies[1:] if p["kept"]["status"][0] != SC.UNKNOWN]
    assert len(kept_proven_roots) >= 2 and all(p["ran"] == 0 for p in kept_proven_roots)
    assert len(kept_proven_roots) == w["solver_effects"]["kept_proven_root"]
    for p in plies[1:]:                                                  # the bookkeeping agrees with the dumps
        assert p["kept_proven"] == int((p["kept"]["status"] != SC.UNKNOWN).sum()) and p["kept_nodes"] == len(p["kept"]["N"])
    # the solver's sequence is not the plain one
    assert [p["raw"] for p in plies] != [p["raw"] for p in SC.scale_model(key, solver=False)["plies"]]


def test_scale_cases_reach_what_they_are_for_together():
    s = {key: _summary(SC.scale_model(key)) for key in SC.SCALE_CASES}
    n = {key: SC.SCALE_CASES[key]["n_playouts"] for key in s}
    assert max(s[k]["stopped_nonterminal"] for k in SC.LATE_C4) > 0
    assert any(0 < r < n[k] for k in s for r in s[k]["ran"])             # a search cut short after some playouts
    assert max(s["bt8_1600"]["kept_proven"]) >= 500                      # a kept tree with hundreds of proven nodes
    assert s["bt8_1600"]["largest_tree"] > 65536
    assert max(s[k]["max_depth"] for k in s) >= 17
    assert s["c4_late"]["events"] >= 200 and s["bt6_800"]["events"] >= 200 and s["bt8_1600"]["events"] >= 400


def test_deep_cases_walk_proofs_across_depths_64_and_128():
    ev = {key: SC.deep_model(key)["events"] for key in SC.DEEP_CASES}
    st = {key: SC.event_stats(e) for key, e in ev.items()}
    print(st)
    assert st["bt8x8"]["cross64"] >= 1
    assert any(d == 64 for _, d, _ in ev["bt8x8"])                       # a proven node in lane 0 of register 1
    assert st["bt26x2_128"]["cross128"] >= 1
    assert any(d - lv <= 127 and d >= 129 for _, d, lv in ev["bt26x2_128"])   # a walk that reads depth 128 AND depth 127
    assert any(d - lv >= 128 and lv >= 3 for _, d, lv in ev["bt26x2"]) and st["bt26x2"]["max_levels"] >= 5
    for key, c in SC.DEEP_CASES.items():
        ply = SC.deep_model(key)["plies"][0]
        assert ply["ran"] == c["n_playouts"] and ply["status"] == SC.UNKNOWN
        first = min(i for i, p in enumerate(_terminal_playouts(key)) if p)
        assert c["n_playouts"] - first >= 24                             # a few dozen playouts past the first terminal
        assert ply["tree"]["status"].any() and ply["tree"]["N"].tolist() != SC.deep_model(key, solver=False)["plies"][0]["tree"]["N"].tolist()
    first = min(d for _, d, _ in ev["bt26x2_128"])
    assert 128 <= first <= 131


def _terminal_playouts(key):
    """Per playout of the plain search: did it end on a terminal node?  (The oracle, playout by playout.)"""
    from oracle import binding as orc
    c = SC.DEEP_CASES[key]
    m, s = orc.MCTS(SC.deep_policy(c), c["game"], n_playouts=c["n_playouts"], use_dirichlet=False), orc.State(c["game"])
    out, prev = [], 0
    for _ in range(c["n_playouts"]):
        m.playout(s)
        cur = m.counters()["terminal_hits"]
        out.append(cur > prev)
        prev = cur
    return out


def test_the_deep_game_keeps_proven_chains_through_every_re_rooting():
    w = SC.deep_game_model()
    st = SC.event_stats(w["events"])
    print(len(w["plies"]), st, w["solver_effects"])
    assert st["cross64"] >= 10 and st["max_depth"] >= 90
    assert all(p["kept_proven"] > 0 for p in w["plies"][1:]) and max(p["kept_proven"] for p in w["plies"]) >= 1000
    assert w["solver_effects"]["kept_proven_root"] >= 1 and w["ret0"] is not None
    assert w["actions"] != SC.deep_game_model(solver=False)["actions"] or \
        [p["raw"] for p in w["plies"]] != [p["raw"] for p in SC.deep_game_model(solver=False)["plies"]]


# ------------------------------------------------------------------------------------------------ whole games and their pools
@pytest.mark.parametrize("key", sorted(SC.GAME_CASES))
def test_whole_games_and_the_small_pool_fit(key):
    """The self-play games (root noise, sampled moves) also end searches early and keep proven roots; and the pool of
    small_pool() - sized from the model's tree sizes - holds the kept subtree plus a search's room at every re-rooting (asserted
    inside small_pool), and makes at least one re-rooting compact."""
    c, games = SC.GAME_CASES[key], SC.game_models(key)
    cap, compactions = SC.small_pool(key)
    need = (c["n_playouts"] + 1) * PS.max_children(c["game"])
    print(key, "pool", cap, "compactions expected", compactions, [[p["ran"] for p in w["plies"]] for w in games])
    assert compactions >= 1
    assert cap >= need + max(p["kept_nodes"] for w in games for p in w["plies"])
    for w in games:
        assert w["solver_effects"]["kept_proven_root"] >= 1 and any(0 < p["ran"] < c["n_playouts"] or p["ran"] == 0 for p in w["plies"])
        assert any(p["raw"] != p["recorded"] for p in w["plies"])
    assert sum(w["solver_effects"]["loss_skipped"] for w in games) >= 500
