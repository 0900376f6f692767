"""First-play urgency on the device (az_engine_set_fpu and its Python facade).

References, all compared with == (there are no tolerances):
  * the rule: the Python model of tests/fpu_cases.py (pinned to the older models and the C oracle with the setting off, and shown to
    bite on these very inputs by tests/test_fpu_host.py) - same fake policy, same injected draws, reductions (0.3, 0.1);
  * clearing and the ways to tick: engines against engines."""
import functools
import types

import numpy as np
import pytest

import forced_playouts_cases as FC
import fpu_cases as F
from alphazero_openspiel_amd import games
from net_cases import drifted_net
from oracle import fakepolicy
from playout_cap_cases import same_game as _same_game

pytestmark = pytest.mark.gpu

C4 = F.C4
S, G, N, SEED = F.S, F.G, F.N, F.SEED
AZ_E_INVALID = -1
PH_SEARCH_DONE = 5


@functools.lru_cache(maxsize=None)
def _net(name):
    game = games.load_game(name)
    return drifted_net([3, game.rows, game.cols], game.num_distinct_actions(), 1, 16, seed=41)


def _fused(name, n_slots=G):
    from alphazero_openspiel_amd.fusednet import FusedNet
    return FusedNet(_net(name), "cuda:0", max_boards=n_slots, precision="f32x")


def _engine(name, fpu=None, n_slots=G, max_games=N, **kw):
    from alphazero_openspiel_amd import engine as E
    kw.setdefault("n_playouts", S)
    kw.setdefault("seed", SEED)
    eng = E.SelfPlayEngine(name, n_slots, max_games=max_games, device=0, **kw)
    if fpu is not None:
        eng.set_fpu(*fpu)
    return eng


def _play(eng, ev, n=N, **kw):
    from alphazero_openspiel_amd import engine as E
    prog = E.run_selfplay(eng, ev, n, **kw)
    assert prog["games_done"] == n and prog["error_flags"] == 0
    return eng.export(), prog


def _same_games(got, want, what, n=None):
    n = len(want["game_len"]) if n is None else n
    assert got["game_len"][:n].tolist() == want["game_len"][:n].tolist(), what
    for j in range(n):
        _same_game(got, j, want, j, 0, "%s: game %d" % (what, j))


def _differ(a, b):
    return a["game_len"].tolist() != b["game_len"].tolist() or (a["child_visits"] != b["child_visits"]).any()


# ------------------------------------------------------------------------------------------------ 1. trees against the model
def _search_manual(eng, ev_fn, max_ticks):
    from alphazero_openspiel_amd import engine as E
    ev = E.HostPolicyEvaluator(eng, ev_fn)
    obs, pri, val = eng.alloc_io()
    for tick in range(max_ticks):
        if eng.read_slot(0)["phase"] == PH_SEARCH_DONE:
            return tick
        eng.advance(pri, val, obs)
        ev(obs, pri, val)
    pytest.fail("the search did not finish")


def _same_tree(tree, want, what):
    assert tree["N"].tolist() == want["N"].tolist(), what                # exact
    assert tree["parent"].tolist() == want["parent"].tolist() and tree["action"].tolist() == want["action"].tolist(), what
    for key in ("Q", "P"):                                               # bit-equal doubles
        assert tree[key].dtype == np.float64 and tree[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize("key", list(F.SEARCHES))
def test_the_tree_of_a_search_equals_the_models(key):
    """az_engine_read_tree after every search of a manual_moves engine: 7 children, more than 16, children beyond lane 32, a
    descent past depth 8, and a root searched again (AZ_ACTION_SEARCH_AGAIN)."""
    from alphazero_openspiel_amd import _lib
    c = F.SEARCHES[key]
    w, dumps = F.search_model(key)
    eng = _engine(c["game"], fpu=F.FPU, n_slots=1, max_games=1, manual_moves=True, use_dirichlet=False, n_playouts=c["n_playouts"])
    try:
        assert eng.fpu == F.FPU
        eng.set_start_positions([c["start"]])
        eng.reset(1)
        A, salt = eng.A, c["salt"]
        fn = lambda b: fakepolicy.fake_eval(b, A, salt)
        for n, want in enumerate(dumps):
            if n:
                eng.update_root([_lib.ACTION_SEARCH_AGAIN])
            _search_manual(eng, fn, 2 * c["n_playouts"] + 64)
            assert eng.read_slot(0)["sims_done"] == c["n_playouts"]
            _same_tree(eng.read_tree(0), want, "%s, search %d" % (key, n))
            root = eng.read_root(0)
            assert root["N"] == int(want["N"][0]) and root["Q"] == float(want["Q"][0])   # the root's own Q: the v of depth 0
        prog = eng.progress()
        assert prog["error_flags"] == 0
        for k in F.COUNTERS:
            assert prog[k] == w["counters"][k], (key, k)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 2. whole games against the model
def _run_injected(key, fpu=F.FPU, per_slot=False):
    """The N games of F.GAMES[key] on G slots, injected draws, the fake policy on the host -> (export, progress, the largest
    number of playouts ONE slot ran in one tick: az_slot_info.sims_done before and after the tick, where the slot stayed in the same
    search - read only with per_slot, else 0)."""
    from alphazero_openspiel_amd import engine as E
    c = F.GAMES[key]
    start = F.game_start(c)
    _, _, mc, _ = FC.geometry(C4)
    etas, us = FC.draws(SEED, C4, N)
    eng = _engine(C4, fpu=fpu, rng="injected", keep_search_tree=True, backup=c["backup"], **c.get("eng", {}))
    try:
        if start:
            eng.set_start_prefix(start)
        if "forced" in c:
            eng.set_forced_playouts(*c["forced"])
        if c.get("solver"):
            eng.set_solver(True)
        if "cap" in c:
            eng.set_playout_cap(*c["cap"])
        if "mirror" in c:
            eng.set_eval_mirror(c["mirror"])
        eng.reset(N)
        left = eng.max_plies - len(start)
        eng.set_injected_rng([[row[:mc] for row in e[:left]] for e in etas], [u[:left] for u in us])
        A, salt = eng.A, c["salt"]
        ev = E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, A, salt))
        obs, pri, val = eng.alloc_io()
        most = 0
        slots = lambda: [eng.read_slot(g) for g in range(eng.G)] if per_slot else []
        before = slots()
        for _ in range(200000):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
            p = eng.progress()
            after = slots()
            for a, b in zip(before, after):
                if (a["game_id"], a["ply"]) == (b["game_id"], b["ply"]):   # the same search: its counter only grew
                    most = max(most, b["sims_done"] - a["sims_done"])
            before = after
            if p["games_done"] >= N:
                break
        else:
            pytest.fail("games did not finish")
        return eng.export(), eng.progress(), most
    finally:
        eng.close()


def _assert_equals_model(ex, prog, want, p0, what):
    assert prog["error_flags"] == 0, what
    for i, w in enumerate(want):
        n = len(w["actions"])
        assert int(ex["game_len"][i]) == n and ex["move"][i, p0:p0 + n].tolist() == w["actions"], (what, i)
        assert float(ex["game_ret0"][i]) == w["ret0"], (what, i)
        for j, ply in enumerate(w["plies"]):
            nc = int(ex["n_children"][i, p0 + j])
            assert ex["child_action"][i, p0 + j, :nc].tolist() == ply["actions"], (what, i, j)
            assert ex["child_visits"][i, p0 + j, :nc].tolist() == ply["recorded"], (what, i, j, ply["raw"], ply["recorded"])
            assert float(ex["value"][i, p0 + j]) == ply["value"], (what, i, j)
    for key in F.COUNTERS:
        assert prog[key] == sum(w["counters"][key] for w in want), (what, key)


@pytest.mark.parametrize("key", list(F.GAMES))
def test_self_play_equals_the_model(key):
    """8 slots, 16 games, 48 playouts, kept trees: every move, recorded visit vector, value target (soft-Z and off-policy read the
    tree), result and counter.  Composed with a playout cap (12, 0.5), forced playouts with pruning, the evaluation mirror p = 0.5,
    the solver; and late connect_four starts with max_sims_per_tick large and no chain window, where playouts chain on the
    register-cached root with the setting on."""
    c = F.GAMES[key]
    ex, prog, most = _run_injected(key, per_slot=key == "chained")
    _assert_equals_model(ex, prog, F.game_models(key), len(F.game_start(c)), key)
    if key == "chained":
        assert prog["terminal_hits"] > 0 and most > 1                    # a slot ran more than one playout in a tick: a chained one


# ------------------------------------------------------------------------------------------------ 3. the ways to tick
def test_a_stream_delivers_the_games_of_the_closed_generation():
    from alphazero_openspiel_amd import engine as E
    kw = dict(keep_search_tree=True, use_dirichlet=True)
    ev = _fused(C4)
    eng = _engine(C4, fpu=F.FPU, **kw)
    want, _ = _play(eng, ev)
    eng.close()
    eng = _engine(C4, max_games=N // 2, **kw)                            # a ring of 8 rows: 16 games wrap it
    stream = E.SelfPlayStream(eng, ev, seed=SEED, use_graph=False, fpu=F.FPU)
    try:
        assert eng.fpu == F.FPU
        for first_want in (0, N // 2):
            buf, first = stream.take(N // 2, max_ticks=200000)
            assert first == first_want
            got = E.unpack_device_export(buf.cpu().numpy(), N // 2, eng.max_plies, eng.max_children)
            for j in range(N // 2):
                _same_game(got, j, want, first + j, 0, "a stream: game %d" % (first + j))
    finally:
        stream.close()
        E.close_all(eng, ev)


def test_dense_rows_play_the_same_games():
    """16 slots, 40 games, 16 playouts (the shape of tests/test_tail_rows_gpu.py): the generation ticked whole, and with the tail
    on dense request rows (az_engine_compact_rows / az_engine_advance_rows)."""
    from alphazero_openspiel_amd import engine as E
    slots, n, playouts = 16, 40, 16

    def run(switch_when, fpu=F.FPU):
        eng = _engine(C4, fpu=fpu, n_slots=slots, max_games=n, n_playouts=playouts, seed=5)
        eng.reset(n)
        A = eng.A
        ev = E.HostPolicyEvaluator(eng, lambda b: fakepolicy.fake_eval(b, A, 9))
        obs, pri, val = eng.alloc_io()
        rows, switches, switched = None, list(switch_when), 0
        for _ in range(200000):
            if rows is None:
                eng.advance(pri, val, obs)
                ev(obs, pri, val)
            else:
                eng.advance_rows(rows, pri, val, obs)
                ev(obs[:rows], pri[:rows], val[:rows])
            done = eng.games_done()
            if done >= n:
                break
            if switches and min(n, slots + done) >= n and n - done <= switches[0]:
                switches.pop(0)
                rows = eng.compact_rows()
                assert rows == n - done
                switched += 1
        else:
            pytest.fail("games did not finish")
        prog, ex = eng.progress(), eng.export()
        eng.close()
        assert prog["error_flags"] == 0 and prog["games_done"] == n and switched == len(switch_when)
        return ex

    whole = run([])
    _same_games(run([slots - 2, slots // 4]), whole, "dense rows in the tail")
    assert _differ(whole, run([], fpu=None))                             # (the setting was in force)


# ------------------------------------------------------------------------------------------------ 4. off means off; refusals
def test_a_cleared_setting_is_the_plain_engine():
    ev = _fused(C4)
    kw = dict(keep_search_tree=True, use_dirichlet=True)
    eng = _engine(C4, **kw)
    assert eng.fpu is None
    want, prog_want = _play(eng, ev)
    packed = eng.export_device().cpu().numpy().tobytes()
    eng.set_fpu(0.3, 0.1)
    assert eng.fpu == (0.3, 0.1)
    eng.clear_fpu()
    assert eng.fpu is None
    got, prog = _play(eng, ev)                                           # the same generation again
    assert eng.export_device().cpu().numpy().tobytes() == packed
    assert sorted(got) == sorted(want)
    for key in want:                                                     # byte for byte, every array of the export
        assert np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    for key in F.COUNTERS:
        assert prog[key] == prog_want[key], key
    eng.set_fpu(0.3, 0.1)                                                # (and the setting, in force, plays other games)
    with_fpu, _ = _play(eng, ev)
    eng.close()
    ev.close()
    assert _differ(with_fpu, want)


def test_refusals_name_their_reason():
    from alphazero_openspiel_amd import engine as E
    for what, eng in (("arena", _engine(C4, arena_agent="zero", opponent="random")), ("AZ_SELECT_UCT", _engine(C4, use_puct=False))):
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_fpu is for PUCT self-play and manual_moves.*%s" % (AZ_E_INVALID, what)):
            eng.set_fpu(0.3)
        assert eng.fpu is None
        eng.close()
    eng = _engine(C4)
    for bad in ((-0.1, 0.0), (0.3, -1.0), (float("nan"), 0.0), (0.3, float("inf")), (float("-inf"), 0.0)):
        with pytest.raises(E.EngineError, match=r"\(%d\).*az_engine_set_fpu: reduction and reduction_root must be finite" % AZ_E_INVALID):
            eng.set_fpu(*bad)
        assert eng.fpu is None
    assert eng.lib.az_engine_set_fpu(eng._h, 0, float("nan"), -1.0) == 0  # on == 0: the other two arguments are ignored
    eng.set_fpu(0.0, 0.0)                                                # zero reductions are a setting
    assert eng.fpu == (0.0, 0.0)
    eng.set_forced_playouts(2.0)                                         # composes with forcing, a cap and the mirror
    eng.set_playout_cap(12, 0.5)
    eng.set_eval_mirror(0.5)
    eng.reset(4)
    obs, pri, val = eng.alloc_io()
    eng.advance(pri, val, obs)
    eng.close()
    eng = _engine(C4, fpu=F.FPU)
    eng.set_solver(True)                                                 # ... and with the solver
    eng.reset(4)
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. the facade
def _flat(games_):
    return [(r[0], r[2], r[3]) for g in games_ for r in g]


def test_example_generator_passes_the_setting_to_its_engines():
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    kw = dict(n_playouts=S, n_slots=G, seed=5, use_graph=False)
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", fpu=F.FPU, **kw)
    out = gen.generate_examples(N)
    gen.close()
    gen = ExampleGenerator(_net(C4), C4, "cuda:0", **kw)
    plain = gen.generate_examples(N)
    gen.close()
    assert _flat(out) != _flat(plain)
    eng = _engine(C4, fpu=F.FPU, seed=5)                                 # the generator's first generation
    ev = _fused(C4)
    ex, _ = _play(eng, ev)
    eng.close()
    ev.close()
    assert _flat(out) == _flat(E.examples_from_export(eng.game, ex))


def test_analyze_positions_equals_the_one_position_path():
    """analyze_positions(fpu=...) on three positions side by side against the model's one-position searches (which
    test_the_tree_of_a_search_equals_the_models pins to an engine of one slot), and against the same call without the setting."""
    from alphazero_openspiel_amd import analysis
    from alphazero_openspiel_amd import engine as E
    A, salt, n_playouts = 7, 11, 64
    positions = [[], [3, 2], F.SEARCHES["c4_deep"]["start"]]
    ev = E.HostPolicyEvaluator(types.SimpleNamespace(A=A), lambda b: fakepolicy.fake_eval(b, A, salt))
    res = analysis.analyze_positions(ev, C4, positions, n_playouts=n_playouts, fpu=F.FPU, seed=SEED)
    assert res["progress"]["error_flags"] == 0
    for i, h in enumerate(positions):
        w = F.play_game(C4, salt, None, None, fpu=F.FPU, n_playouts=n_playouts, use_dirichlet=False, backup="soft-Z",
                        num_probabilistic_actions=0, start=h, max_searches=1)
        ply = w["plies"][0]
        assert res["visits"][i, ply["actions"]].tolist() == ply["raw"] and int(res["visits"][i].sum()) == sum(ply["raw"]), i
    plain = analysis.analyze_positions(ev, C4, positions, n_playouts=n_playouts, seed=SEED)
    assert (plain["visits"] != res["visits"]).any()


def test_reanalyser_and_forker_take_the_setting():
    import replay_cases as RC
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd import replay as R
    ex = RC.fake_export(games.load_game(C4), n_games=4, seed=3)
    targets = []
    for fpu in (None, F.FPU):
        rep = R.DeviceReplay(C4, max_games=4, device=0)
        rep.append_export(ex)
        U = rep.dedupe()
        re = R.Reanalyser(rep, None, U, S, value_target="soft-Z", fpu=fpu)
        try:
            assert re.analyzer.engine.fpu == fpu
            re.analyzer.evaluator = E.HostPolicyEvaluator(re.analyzer.engine, lambda b: fakepolicy.fake_eval(b, 7, 9))
            assert re.reanalyse() == U
            assert re.analyzer.engine.progress()["error_flags"] == 0 and rep.stats()["fault_flags"] == 0
            targets.append(np.array([rep.read_example(i)[0] for i in range(rep.stats()["n_examples"])]))
        finally:
            re.close()
            rep.close()
    assert (targets[0] != targets[1]).any()
    rep = R.DeviceReplay(C4, max_games=8, device=0)
    rep.append_export(ex)
    rep.dedupe()
    fk = R.Forker(rep, _net(C4), 2, S, max_games=2, fpu=0.3)
    try:
        assert fk.engine.fpu == (0.3, 0.0)
    finally:
        fk.close()
        rep.close()
