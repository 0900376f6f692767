"""Self-play resignation, host side: the conditions tests/test_resign_gpu.py relies on, asserted on the model's games
(tests/resign_cases.py); the calibration arithmetic of alphazero_openspiel_amd/resign.py; the C ABI's two entries; the refusals
the facades state before an engine exists.  No device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import resign_cases as R
from alphazero_openspiel_amd import _lib, resign
from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
from alphazero_openspiel_amd.search_settings import ARENA_KEYS, KEYS, SearchSettings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the model's games
@pytest.mark.parametrize("case", list(R.CASES))
def test_the_two_value_targets_play_the_same_moves(case):
    a, b = R.model_games(case, "soft-Z"), R.model_games(case, "A0C")
    assert [g["actions"] for g in a] == [g["actions"] for g in b] and [g["ret0"] for g in a] == [g["ret0"] for g in b]
    for ga, gb in zip(a, b):
        assert [p["raw"] for p in ga["plies"]] == [p["raw"] for p in gb["plies"]]
    assert any(x != y for ga, gb in zip(a, b) for x, y in zip([p["value"] for p in ga["plies"]], [p["value"] for p in gb["plies"]]))


@pytest.mark.parametrize("case", list(R.CASES))
def test_the_cases_split_their_games_as_the_device_tests_need(case):
    ex = R.expected_games(case, p=0.5)
    lens = [len(g["actions"]) for g in R.model_games(case, "soft-Z")]
    with_ply = [i for i, e in enumerate(ex) if e["ply"] >= 0]
    assert sum(1 for i in with_ply if ex[i]["ply"] < lens[i] - 1) >= 3            # (a resign ply is never the last one, by the rule)
    assert len(ex) - len(with_ply) >= 2
    assert {ex[i]["through"] for i in with_ply} == {True, False}                   # both coin values at p = 0.5
    cut = R.expected_games(case, p=0.0)
    for i, (e, c) in enumerate(zip(ex, cut)):
        assert c["ply"] == e["ply"] and c["resigned"] == (e["ply"] >= 0)
        if c["resigned"]:
            assert 1 <= c["length"] == c["ply"] + 1 < lens[i] and c["ret0"] == (-1.0 if c["ply"] % 2 == 0 else 1.0)
        else:
            assert c["length"] == lens[i] and c["low"] == e["low"]
    assert all(not e["through"] and not e["resigned"] for e in R.expected_games(case, v=1.0, p=0.5))    # crit >= -1: never


def test_a_fast_ply_below_the_threshold_is_skipped():
    case = "c4_cap"
    v, sch, crit = R.CASES[case]["v"], R.schedules(case), R.model_crit(case)
    skipped = [(i, j) for i, c in enumerate(crit) for j, x in enumerate(c[:-1]) if x < -v and not sch[i][j][1]]
    assert skipped
    uncapped = [R.expect(c, v)[0] for c in crit]
    capped = [e["ply"] for e in R.expected_games(case)]
    assert uncapped != capped                                                      # the cap's rule moves at least one resign ply
    for i, j in skipped:
        assert capped[i] != j


def test_min_ply_and_the_start_shift_the_qualifying_plies():
    crit = [0.1, -0.5, 0.2, -0.6, -0.7, 0.0, 1.0]
    assert R.expect(crit, 0.3) == (1, [-0.7, -0.6])
    assert R.expect(crit, 0.3, min_ply=2) == (3, [-0.7, -0.6])
    assert R.expect(crit, 0.3, start=3, min_ply=2) == (6, [-0.6, -0.7]) and R.expect(crit, 0.3, start=3) == (4, [-0.6, -0.7])
    assert R.expect(crit, 0.65) == (4, [-0.7, -0.6]) and R.expect(crit[:5], 0.65) == (-1, [0.1, -0.6])   # the last ply never counts
    assert R.expect(crit, 0.3, full=[1, 0, 1, 0, 1, 1, 1]) == (4, [-0.7, 0.0])
    assert R.plays_through(701, 3, 1.0) and not R.plays_through(701, 3, 0.0)


# ------------------------------------------------------------------------------------------------ calibration
LOW = np.array([[-0.95, INF]] * 10 + [[INF, -0.9]] * 10 + [[-0.5, 0.2]] * 5)
RET0 = np.array([-1.0] * 9 + [1.0] + [1.0] * 10 + [1.0] * 5)


def test_false_positive_rate_counts_the_players_who_would_have_resigned():
    assert resign.false_positive_rate(LOW, RET0, 0.9) == (0.1, 10)                  # -0.9 < -0.9 is false: ten players, one won
    assert resign.false_positive_rate(LOW, RET0, 0.89) == (0.05, 20)
    assert resign.false_positive_rate(LOW, RET0, 0.4) == (6 / 25, 25)               # player 0 of the last five won all five
    assert resign.false_positive_rate(LOW, RET0, 0.95) == (0.0, 0) and resign.false_positive_rate(LOW, RET0, 1.0) == (0.0, 0)
    draw = resign.false_positive_rate([[-0.8, INF]], [0.0], 0.5)
    assert draw == (1.0, 1)                                                         # a draw was given away too
    counts = [resign.false_positive_rate(LOW, RET0, v)[1] for v in np.linspace(0.05, 1.0, 96)]
    assert counts == sorted(counts, reverse=True)                                   # a more cautious threshold resigns no more players
    nested_low = np.array([[-0.9, INF], [-0.7, INF], [-0.5, INF], [-0.3, INF]])     # the surer the resigner, the likelier the loss:
    nested_ret = np.array([-1.0, -1.0, 1.0, 1.0])                                   # then the rate itself falls as v rises
    rates = [resign.false_positive_rate(nested_low, nested_ret, v)[0] for v in (0.2, 0.4, 0.6, 0.8, 0.95)]
    assert rates == [0.5, 1 / 3, 0.0, 0.0, 0.0] and rates == sorted(rates, reverse=True)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"threshold lies in \(0, 1\]"):
            resign.false_positive_rate(LOW, RET0, bad)
    with pytest.raises(ValueError, match="low holds 25 games, ret0 3"):
        resign.false_positive_rate(LOW, RET0[:3], 0.5)


def test_calibrate_returns_the_most_eager_threshold_that_holds():
    assert resign.calibrate(LOW, RET0, target=0.05) == 0.95                         # at 0.9 one of ten resigners won: 10 %
    assert resign.calibrate(LOW, RET0, target=0.1) == 0.5
    assert resign.calibrate(LOW, RET0, target=0.25) == 0.05                         # every threshold down to the floor holds
    assert resign.calibrate(LOW, RET0, target=0.25, floor=0.2) == 0.2
    assert resign.calibrate(LOW, RET0, target=0.0) == 0.95
    v = resign.calibrate(LOW, RET0, target=0.05)
    assert resign.false_positive_rate(LOW, RET0, v)[0] <= 0.05
    with pytest.raises(ValueError, match="at least 20 play-through games.*got 19"):
        resign.calibrate(LOW[:19], RET0[:19])
    assert resign.calibrate(LOW[:3], RET0[:3], min_games=3) == 0.05
    with pytest.raises(ValueError, match="floor must lie"):
        resign.calibrate(LOW, RET0, floor=0.0)


def test_weights_undo_the_sampling_of_the_played_out_games():
    """A run under (v0 = 0.6, playthrough = 0.25): of 8 games with a resign ply 2 were played out (weight 4), all 4 without one
    were (weight 1).  At or above v0 only the first kind counts and the weights cancel; below it they restore the proportions."""
    low = np.array([[-0.9, INF], [-0.7, INF]] + [[-0.5, INF]] * 4)
    ret0 = np.array([-1.0, 1.0] + [-1.0, -1.0, -1.0, 1.0])
    w = resign.played_out_weights([True, True, False, False, False, False], 0.25)
    assert w.tolist() == [4.0, 4.0, 1.0, 1.0, 1.0, 1.0]
    assert resign.false_positive_rate(low, ret0, 0.6, w) == resign.false_positive_rate(low, ret0, 0.6) == (0.5, 2)
    assert resign.false_positive_rate(low, ret0, 0.4) == (2 / 6, 6)
    assert resign.false_positive_rate(low, ret0, 0.4, w) == (5.0 / 12.0, 6)          # (4 + 1) wrong of (8 + 4) by weight
    low2, ret2 = np.array([[-0.9, INF]] * 2 + [[-0.5, INF]] * 4), np.array([-1.0, -1.0, -1.0, -1.0, 1.0, 1.0])
    assert resign.calibrate(low2, ret2, target=0.4, min_games=6) == 0.05            # 2 wrong of 6 at the floor: passes unweighted,
    assert resign.calibrate(low2, ret2, target=0.4, min_games=6, weights=w) == 0.05  # and 2 of 12 by weight
    assert resign.calibrate(low2[1:], ret2[[0, 2, 3, 4, 5]], target=0.35, min_games=5) == 0.5    # 2 of 5 = 0.4 fails unweighted ...
    assert resign.calibrate(low2[1:], ret2[[0, 2, 3, 4, 5]], target=0.35, min_games=5, weights=w[1:]) == 0.05   # ... 2 of 8 holds
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"playthrough share in \(0, 1\]"):
            resign.played_out_weights([True], bad)
    with pytest.raises(ValueError, match="one positive number per game"):
        resign.false_positive_rate(low, ret0, 0.4, w[:3])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_abi_has_the_two_entries_with_these_signatures():
    import ctypes as C
    lib = _lib.load()
    protos = {n: (r, a) for n, r, a in _lib.PROTOTYPES}
    vp = C.c_void_p
    assert protos["az_engine_set_resign"] == (C.c_int, [vp, C.c_int32, C.c_double, C.c_double, C.c_int32])
    assert protos["az_engine_resign_info_device"] == (C.c_int, [vp, C.c_int64, C.c_int64, vp, vp, vp, vp])
    assert hasattr(lib, "az_engine_set_resign") and hasattr(lib, "az_engine_resign_info_device")
    assert lib.az_engine_set_resign(None, 1, 0.5, 0.1, 0) == -1 and lib.az_engine_resign_info_device(None, 0, 1, None, None, None, None) == -1
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int az_engine_set_resign(az_engine *e, int32_t on, double v, double p_playthrough, int32_t min_ply);" in flat
    assert ("int az_engine_resign_info_device(az_engine *e, int64_t first_game, int64_t n_games, int32_t *ply_out_dev, "
            "uint8_t *flags_out_dev, double *low_out_dev, void *stream);") in flat
    doc = flat[flat.index("Self-play resignation"):flat.index("int az_engine_set_resign(")]
    for words in ("az_engine_set_resign:", "az_engine_resign_info_device:", "purpose 6", "crit = max(r, b)", "-99.0", "min_ply",
                  "play-through", "bit 0", "bit 1", "+infinity", "BEFORE az_engine_stream_take_device", "AZ_E_INVALID", "AZ_E_STATE"):
        assert words in doc, words
    internal = open(os.path.join(ROOT, "alphazero-openspiel_amd", "csrc", "az_engine_internal.h")).read()
    assert "sizeof(Params) == 992" in internal and "const ResDev *resdev;" in internal


# ------------------------------------------------------------------------------------------------ the facades' refusals
def test_search_settings_parse_and_refuse_resign():
    assert "resign" in KEYS and "resign" not in ARENA_KEYS
    for given, want in ((0.9, (0.9, 0.1, 0)), ((0.9, 0.5), (0.9, 0.5, 0)), ([1, 0, 4], (1.0, 0.0, 4)), ((0.5, 1, 0), (0.5, 1.0, 0))):
        got = SearchSettings.from_kwargs(dict(resign=given)).resign
        assert got == want and [type(x) for x in got] == [float, float, int]
    for bad in ("x", (), (0.9, 0.1, 0, 1), (0.9, "p"), (0.9, 0.1, 2.5), True, (0.9, True)):
        with pytest.raises(ValueError, match="resign must be v, "):
            SearchSettings.from_kwargs(dict(resign=bad))
    for bad in (0.0, -0.5, 1.01, float("nan"), (0.9, -0.1), (0.9, 1.5), (0.9, 0.1, -1)):
        with pytest.raises(ValueError, match=r"resign needs v in \(0, 1\], playthrough in \[0, 1\] and min_ply >= 0"):
            SearchSettings.from_kwargs(dict(resign=bad))
    assert SearchSettings.from_kwargs(dict(resign=None)).resign is None and SearchSettings.from_kwargs({}) == SearchSettings()
    with pytest.raises(ValueError, match="resign is a self-play setting.*is_test=True"):
        SearchSettings.from_kwargs(dict(resign=0.9)).check(is_test=True)
    with pytest.raises(ValueError, match="resign is a self-play setting: an arena engine"):
        SearchSettings.from_kwargs(dict(resign=0.9)).apply_arena(object())
    calls = []

    class Eng:
        def set_fpu(self, *a):
            calls.append(("fpu", a))

        def set_resign(self, *a):
            calls.append(("resign", a))

    SearchSettings.from_kwargs(dict(resign=(0.9, 0.5), fpu=0.3)).apply(Eng())
    assert calls == [("fpu", (0.3, 0.0)), ("resign", (0.9, 0.5, 0))]                # after the search's own settings


def test_example_generator_takes_and_refuses_resign():
    net = torch.nn.Identity()
    g = ExampleGenerator(net, "connect_four", "cuda:0", n_playouts=24, resign=(0.9, 0.25))   # (no device before a generation)
    assert g.resign == (0.9, 0.25, 0) and g.settings.resign == g.resign
    assert g.resign_stats["games"] == 0 and g.resign_stats["low"].shape == (0, 2)
    assert g.resign_stats["weight"].shape == (0,)
    assert ExampleGenerator(net, "connect_four", "cuda:0").resign is None
    with pytest.raises(ValueError, match="resign is a self-play setting.*is_test=True"):
        ExampleGenerator(net, "connect_four", "cuda:0", is_test=True, resign=0.9)
    with pytest.raises(ValueError, match=r"resign needs v in \(0, 1\]"):
        ExampleGenerator(net, "connect_four", "cuda:0", resign=2.0)
    ok = ExampleGenerator(net, "connect_four", "cuda:0", resign=0.9, continuous=True)          # pools, ranks and the stream take it
    assert ok.resign == (0.9, 0.1, 0)
    assert ExampleGenerator(net, "connect_four", "cuda:0", resign=0.9, n_pools=2).resign == (0.9, 0.1, 0)
