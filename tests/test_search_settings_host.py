"""The one parser of the search settings (alphazero_openspiel_amd/search_settings.py) behind every facade that takes the keywords
playout_cap=, forced_playouts=, eval_mirror=, solver= and fpu=: the same bad value raises the same ValueError from each of them, the
same good value lands as the same normalised tuple on the engine, and each facade keeps its own meaning of "absent".  No device is
touched: the facades are built on a stand-in engine that records the setter calls."""
import types

import pytest
import torch

from alphazero_openspiel_amd import analysis, arena, replay
from alphazero_openspiel_amd import engine as E
from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
from alphazero_openspiel_amd.search_settings import KEYS, SearchSettings

NAN, INF = float("nan"), float("inf")
BAD = {  # keyword -> (bad value, the text of its ValueError)
    "fpu": [((0.3, NAN), "fpu reductions must be finite and >= 0"), (-1.0, "fpu reductions must be finite and >= 0"),
            ((0.1, 0.2, 0.3), "fpu must be a reduction r or a pair"), ("x", "fpu must be a reduction r or a pair"),
            (True, "fpu must be a reduction r or a pair")],
    "eval_mirror": [(1.5, r"eval_mirror must be a probability in \[0, 1\]"), (-0.1, r"eval_mirror must be a probability in \[0, 1\]"),
                    (NAN, r"eval_mirror must be a probability in \[0, 1\]"), ("x", r"eval_mirror must be a probability in \[0, 1\]")],
    "forced_playouts": [(-1.0, "forced_playouts needs a finite k >= 0"), (INF, "forced_playouts needs a finite k >= 0"),
                        ((2.0, 2), "forced_playouts needs a finite k >= 0 and prune False / True"),
                        ("x", "forced_playouts must be k or a pair"), ((1.0, True, 0), "forced_playouts must be k or a pair")],
    "playout_cap": [(6, "playout_cap must be a pair"), ((6,), "playout_cap must be a pair"), (("a", 0.5), "playout_cap must be a pair")],
}
GOOD = {  # keyword -> (value as given, the normalised form every facade hands to the setter)
    "fpu": [(0.3, (0.3, 0.0)), ((0.3, 0.1), (0.3, 0.1)), ([0, 1], (0.0, 1.0))],
    "eval_mirror": [(0.5, 0.5), (1, 1.0)],
    "forced_playouts": [(2, (2.0, True)), ((2.0, 0), (2.0, False)), ([1.5, True], (1.5, True))],
    "solver": [(True, True), (1, True)],
}


class Stop(Exception):
    pass


class FakeEngine:
    """Records the setter calls in order; stands in for SelfPlayEngine where a facade builds or is handed one."""
    made = []

    def __init__(self, *args, **kw):
        self.calls, self.kw, self.device, self.G, self.max_plies = [], kw, torch.device("cpu"), 4, 42
        FakeEngine.made.append(self)

    def set_forced_playouts(self, k, prune=True):
        self.calls.append(("forced_playouts", (k, prune)))

    def set_eval_mirror(self, p):
        self.calls.append(("eval_mirror", p))

    def set_solver(self, on=True):
        self.calls.append(("solver", on))

    def set_fpu(self, reduction, root=0.0):
        self.calls.append(("fpu", (reduction, root)))

    def set_arena_search(self, **kw):
        self.calls.append(("arena", kw))

    def stream_begin(self, seed):
        raise Stop  # (SelfPlayStream: the settings have been applied by now)

    def alloc_io(self):
        return None, None, None

    def alloc_roots(self):
        raise Stop  # (Analyzer: the settings have been applied by now; pinned host memory comes next)

    def close(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    FakeEngine.made = []
    for mod in (analysis, arena, E):
        monkeypatch.setattr(mod, "SelfPlayEngine", FakeEngine)
    monkeypatch.setattr(E, "make_evaluator", lambda *a, **k: None)
    return FakeEngine


def _generator(**kw):
    g = ExampleGenerator(torch.nn.Identity(), "connect_four", "cuda:0", n_playouts=24, **kw)   # (no device before a generation)
    eng = FakeEngine()
    g.settings.apply(eng)                                                 # what _new_engine does to every engine it builds
    return eng.calls


def _stream(**kw):
    eng = FakeEngine()
    with pytest.raises(Stop):
        E.SelfPlayStream(eng, None, **kw)
    return eng.calls


def _analyzer(**kw):
    with pytest.raises(Stop):
        analysis.Analyzer(None, "connect_four", 4, n_playouts=8, device="cpu", **kw)
    return FakeEngine.made[-1].calls


def _reanalyser(**kw):
    store = types.SimpleNamespace(game="connect_four", device=torch.device("cpu"))
    with pytest.raises(Stop):
        replay.Reanalyser(store, None, 4, 8, **kw)
    return FakeEngine.made[-1].calls


def _forker(**kw):
    store = types.SimpleNamespace(game="connect_four", device=torch.device("cpu"))
    return replay.Forker(store, None, 4, 8, **kw).engine.calls


def _arena(**kw):
    return arena.arena_engine("connect_four", 4, 8, "zero", "random", device=0, **kw).calls


FACADES = {  # facade -> (builder, the keywords its constructor takes)
    "ExampleGenerator": (_generator, ("fpu", "eval_mirror", "forced_playouts", "solver", "playout_cap")),
    "SelfPlayStream": (_stream, ("fpu", "eval_mirror", "forced_playouts", "solver")),
    "Analyzer": (_analyzer, ("fpu", "eval_mirror", "solver")),
    "Reanalyser": (_reanalyser, ("fpu", "eval_mirror", "solver")),
    "Forker": (_forker, ("fpu",)),
    "arena_engine": (_arena, ("fpu", "eval_mirror", "solver")),
}


@pytest.mark.parametrize("facade", list(FACADES))
def test_a_bad_value_raises_the_same_error_from_every_facade(facade, fake):
    build, keys = FACADES[facade]
    for key in keys:
        for bad, text in BAD.get(key, []):
            with pytest.raises(ValueError, match=text):
                build(**{key: bad})
            with pytest.raises(ValueError, match=text):                  # ... the text of the one parser
                SearchSettings.from_kwargs({key: bad})
    assert all(not e.calls for e in fake.made)                            # a refusal called no setter


@pytest.mark.parametrize("facade", list(FACADES))
def test_a_good_value_lands_as_the_same_normalised_tuple(facade, fake):
    build, keys = FACADES[facade]
    for key in keys:
        for given, want in GOOD.get(key, []):
            calls = build(**{key: given})
            if facade == "arena_engine":
                assert calls == [("arena", dict(dict(fpu=None, solver=False, eval_mirror=0.0), **{key: want}))], (key, given)
            else:
                assert calls == [(key, want)] and type(calls[0][1]) is type(want), (key, given, calls)
    if "playout_cap" in keys:
        g = ExampleGenerator(torch.nn.Identity(), "connect_four", "cuda:0", n_playouts=24, playout_cap=[6, 1])
        assert g.playout_cap == (6, 1.0) and type(g.playout_cap[1]) is float


def test_the_setters_are_called_in_one_order(fake):
    every = dict(fpu=0.3, solver=True, eval_mirror=0.5)
    order = ["eval_mirror", "solver", "fpu"]
    assert [c[0] for c in _stream(**every)] == order and [c[0] for c in _analyzer(**every)] == order
    assert [c[0] for c in _generator(**every)] == order
    assert [c[0] for c in _stream(fpu=0.3, forced_playouts=2.0, eval_mirror=0.5)] == ["forced_playouts", "eval_mirror", "fpu"]
    eng = FakeEngine()
    SearchSettings.from_kwargs(dict(forced_playouts=2.0, eval_mirror=0.5, fpu=0.3, playout_cap=(6, 0.5))).apply(eng)
    assert [c[0] for c in eng.calls] == ["forced_playouts", "eval_mirror", "fpu"]      # (the cap: set by the path that reads its mask)


def test_every_facade_keeps_its_meaning_of_absent(fake):
    # SelfPlayStream is handed an engine: None leaves its setting alone, an off value calls the setter, which clears
    assert _stream() == [] and _stream(forced_playouts=None, eval_mirror=None, solver=None, fpu=None) == []
    assert _stream(forced_playouts=0, eval_mirror=0.0, solver=False) == [("forced_playouts", (0.0, True)), ("eval_mirror", 0.0),
                                                                         ("solver", False)]
    # Analyzer: eval_mirror=0 calls the setter and clears; solver=False (its default) and fpu=None call nothing
    assert _analyzer() == [] and _analyzer(eval_mirror=0) == [("eval_mirror", 0.0)] and _analyzer(solver=False, fpu=None) == []
    # ExampleGenerator: 0 is normalised to None, and nothing is called
    g = ExampleGenerator(torch.nn.Identity(), "connect_four", "cuda:0", forced_playouts=0, eval_mirror=0.0, solver=False)
    assert (g.forced_playouts, g.eval_mirror, g.solver, g.fpu, g.playout_cap) == (None, None, False, None, None)
    assert _generator(forced_playouts=(0.0, True), eval_mirror=0) == [] and _generator() == []
    # the arena: nothing on, nothing called
    assert _arena() == [] and _arena(solver=False, eval_mirror=0.0, fpu=None) == []
    # the two forms, stated once
    off = dict(forced_playouts=0, eval_mirror=0, solver=False)
    clear, absent = SearchSettings.from_kwargs(off, off="clear"), SearchSettings.from_kwargs(off, off="absent")
    assert (clear.forced_playouts, clear.eval_mirror, clear.solver) == ((0.0, True), 0.0, False)
    assert all(getattr(absent, k) is None for k in KEYS) and absent == SearchSettings()
    with pytest.raises(ValueError, match="off must be"):
        SearchSettings.from_kwargs({}, off="keep")


def test_the_engine_parses_arena_settings_through_the_same_parser():
    eng = object.__new__(E.SelfPlayEngine)                               # (no handle: a refusal comes before the library is asked)
    for key in ("fpu", "eval_mirror"):
        for bad, text in BAD[key]:
            with pytest.raises(ValueError, match=text):
                E.SelfPlayEngine.set_arena_search(eng, **{key: bad})
    assert E.fpu_pair is __import__("alphazero_openspiel_amd.search_settings", fromlist=["fpu_pair"]).fpu_pair


def test_check_states_the_generators_rules():
    s = SearchSettings.from_kwargs(dict(fpu=0.3, solver=True, forced_playouts=2.0))
    with pytest.raises(ValueError, match="forced_playouts.*is_test=True"):
        s.check(is_test=True)
    with pytest.raises(ValueError, match="forced_playouts.*use_puct=False"):
        s.check(use_puct=False)
    with pytest.raises(ValueError, match="solver is not supported together with forced_playouts"):
        s.check()
    with pytest.raises(ValueError, match="fpu.*is_test=True"):
        SearchSettings.from_kwargs(dict(fpu=0.3)).check(is_test=True)
    cap = SearchSettings.from_kwargs(dict(playout_cap=(6, 0.5)))
    assert cap.check(n_playouts=24) is cap
    with pytest.raises(ValueError, match=r"needs 1 <= n_fast <= n_playouts = 4 .* got \(6, 0.5\)"):
        cap.check(n_playouts=4)
    with pytest.raises(ValueError, match="playout_cap is not supported with overlap > 1"):
        cap.check(n_playouts=24, overlap=2)
    asked = []
    cap.check(asked.append, n_playouts=24)
    assert asked == ["playout_cap"]
