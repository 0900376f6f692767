"""Merging transpositions and mirror images at dedupe (include/az_replay.h: az_replay_dedupe_positions,
az_replay_unique_counts_device) - what can be checked without a GPU: the Python model of the rule (tests/merge_cases.py) against
the Python rules and against the history model where the two must agree, the condition that keeps the GPU tests from passing
vacuously, the header, the binding list and the facade's argument check."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merge_cases as MC
import replay_cases as RC
from conftest import ROOT
from alphazero_openspiel_amd import _lib, games, replay
from mirror_cases import mirror_action_py

ENTRIES = ("az_replay_dedupe_positions", "az_replay_unique_counts_device")


def _same_unique(a, b):
    assert [(u["index"], u["count"]) for u in a] == [(u["index"], u["count"]) for u in b]
    assert [u["pi"] for u in a] == [u["pi"] for u in b] and [u["z"] for u in a] == [u["z"] for u in b]


def _same_flat(a, b):
    assert [r[2] for r in a] == [r[2] for r in b] and [r[3] for r in a] == [r[3] for r in b]


# ------------------------------------------------------------------------------------------------ the model's pieces
@pytest.mark.parametrize("name", MC.BOARDS + ["breakthrough(rows=6,columns=5)"])
def test_python_bitboard_mirror_commutes_with_the_rules(name):
    """Playing the mirrored actions reaches the mirrored position, ply by ply; the mirror is an involution."""
    game = games.load_game(name)
    rng = np.random.RandomState(4)
    for _ in range(6):
        s, m = game.new_initial_state(), game.new_initial_state()
        while not s.is_terminal():
            la = s.legal_actions()
            a = la[rng.randint(len(la))]
            s.apply_action(a)
            m.apply_action(mirror_action_py(game, a))
            assert [MC.mirror_bits_py(game, b) for b in s.bb] == [int(b) for b in m.bb]
            assert [MC.mirror_bits_py(game, b) for b in m.bb] == [int(b) for b in s.bb]
        assert m.is_terminal() and m.returns() == s.returns()
    stray = (1 << 63) | (1 << 62)      # bits that are no cell stay where they are
    if game.rows * game.cols < 62:
        assert MC.mirror_bits_py(game, stray | 1) & stray == stray


@pytest.mark.parametrize("name", MC.BOARDS)
def test_openings_are_what_their_comment_says(name):
    game = games.load_game(name)
    ops = MC.OPENINGS[name]
    st = [games.state_from_history(game, h) for h in ops]
    assert not any(s.is_terminal() for s in st)
    assert st[0].bb == st[1].bb and ops[0] != ops[1] and sorted(ops[0]) == sorted(ops[1])           # a transposition
    assert ops[3] == [mirror_action_py(game, a) for a in ops[2]] and st[2].bb != st[3].bb           # a mirrored pair
    assert MC.canonical(game, st[2].bb, 2, True)[:3] == MC.canonical(game, st[3].bb, 2, True)[:3]
    assert MC.canonical(game, st[2].bb, 2, False)[:3] != MC.canonical(game, st[3].bb, 2, False)[:3]
    assert ops[-1] == ops[0]                                                                        # equal histories


@pytest.mark.parametrize("name", MC.BOARDS)
def test_a_self_symmetric_position_keeps_flip_0(name):
    game = games.load_game(name)
    sym = [game.new_initial_state()] + ([games.state_from_history(game, [3])] if name == MC.C4 else [])
    for s in sym:
        assert [MC.mirror_bits_py(game, b) for b in s.bb] == [int(b) for b in s.bb]
        assert MC.canonical(game, s.bb, len(s.history()), True) == (int(s.bb[0]), int(s.bb[1]), len(s.history()) & 1, 0)
    # ... as a first occurrence: every game starts with one, so the first group's average is in the stored orientation of
    # record 0 and every member of that group has flip 0 (nothing of it is mapped)
    _, ref = MC.generation(game, rounds=2, seed=3)
    flat = [r for g in ref for r in g]
    plain, _ = MC.merged(game, MC.copy_flat(flat), False)
    both, _ = MC.merged(game, MC.copy_flat(flat), True)
    assert plain[0]["index"] == both[0]["index"] == 0 and plain[0]["count"] == both[0]["count"] == len(ref)
    assert plain[0]["pi"] == both[0]["pi"] and plain[0]["z"] == both[0]["z"]
    # a pair of unsigned words is compared, bb0 first: a canonical key is never above its mirror image
    for r in flat:
        c0, c1, _, flip = MC.canonical(game, r.bb, r.ply, True)
        m = (MC.mirror_bits_py(game, r.bb[0]), MC.mirror_bits_py(game, r.bb[1]))
        s = (int(r.bb[0]), int(r.bb[1]))
        assert (c0, c1) == min(s, m) and flip == (1 if m < s else 0)


# ------------------------------------------------------------------------------------------------ model against model
def test_with_no_two_equal_positions_the_model_is_the_history_dedupe():
    """Nothing to merge: one game never repeats a position, so all three rules give the buffer back."""
    for name in MC.BOARDS:
        game = games.load_game(name)
        ref = RC.reference_games(game, RC.fake_export(game, n_games=1, seed=11))
        flat = ref[0]
        assert len({MC.canonical(game, r.bb, r.ply, True)[:3] for r in flat}) == len(flat) > 5
        want, want_flat = MC.by_history(MC.copy_flat(flat))
        for mirror in (False, True):
            got, got_flat = MC.merged(game, MC.copy_flat(flat), mirror)
            _same_unique(got, want)
            _same_flat(got_flat, want_flat)
            _same_flat(got_flat, flat)
            assert [u["count"] for u in got] == [1] * len(flat)


def test_where_equal_positions_come_from_equal_histories_only_the_plain_rule_is_the_history_dedupe():
    """Games that share one opening and are cut one ply after it: two records hold one position exactly when they hold one
    history, so grouping by position (no mirror) must reproduce oracle.pyreplay bit for bit, counts included."""
    game = games.load_game(MC.B66)
    _, ref = MC.generation(game, rounds=12, seed=21, max_len=4, openings=[MC.OPENINGS[MC.B66][0]])
    flat = [r for g in ref for r in g]
    by_pos, by_hist = {}, {}
    for r in flat:
        by_pos.setdefault(MC.canonical(game, r.bb, r.ply, False)[:3], set()).add(r[0])
        by_hist.setdefault(r[0], set()).add(MC.canonical(game, r.bb, r.ply, False)[:3])
    assert all(len(v) == 1 for v in by_pos.values()) and all(len(v) == 1 for v in by_hist.values())
    want, want_flat = MC.by_history(MC.copy_flat(flat))
    got, got_flat = MC.merged(game, MC.copy_flat(flat), False)
    assert len(want) < len(flat) and max(u["count"] for u in want) == 12
    _same_unique(got, want)
    _same_flat(got_flat, want_flat)


@pytest.mark.parametrize("name", MC.BOARDS)
def test_each_rule_merges_strictly_more_than_the_one_before(name):
    """The condition that keeps the GPU tests from passing vacuously, on the generations they use."""
    game = games.load_game(name)
    for rounds, max_len in ((3, None), (4, None), (14, 5)):
        _, ref = MC.generation(game, rounds=rounds, seed=7, max_len=max_len)
        flat = [r for g in ref for r in g]
        n_hist = len(MC.by_history(MC.copy_flat(flat))[0])
        plain = MC.merged(game, MC.copy_flat(flat), False)[0]
        both = MC.merged(game, MC.copy_flat(flat), True)[0]
        assert len(both) < len(plain) < n_hist < len(flat)
        assert sum(u["count"] for u in plain) == sum(u["count"] for u in both) == len(flat)
        # the shapes the GPU tests rely on: a group of one, and a group whose members alternate orientation
        assert min(u["count"] for u in both) == 1
        flips = {}                                               # key -> the members' flip bits, in buffer order
        for r in flat:
            c = MC.canonical(game, r.bb, r.ply, True)
            flips.setdefault(c[:3], []).append(c[3])
        assert any(sum(a != b for a, b in zip(f, f[1:])) >= 3 for f in flips.values())
    assert max(u["count"] for u in both) >= 65                  # (the last generation: longer than one wave)


@pytest.mark.parametrize("name", MC.BOARDS)
def test_mirroring_a_buffer_twice_is_the_identity_and_once_mirrors_the_result(name):
    game = games.load_game(name)
    _, ref = MC.generation(game, rounds=3, seed=5)
    flat = [r for g in ref for r in g]
    twice = MC.mirrored_flat(game, MC.mirrored_flat(game, flat))
    _same_flat(twice, flat)
    assert all((a.bb == b.bb).all() for a, b in zip(twice, flat))
    # the mirror image of the buffer merges into the mirror image of the result, bit for bit: the members keep their order
    # and their orientation relative to the first, which is all the rule looks at
    got, got_flat = MC.merged(game, MC.copy_flat(flat), True)
    mgot, mgot_flat = MC.merged(game, MC.mirrored_flat(game, flat), True)
    assert [(u["index"], u["count"]) for u in got] == [(u["index"], u["count"]) for u in mgot]
    _same_flat(MC.mirrored_flat(game, mgot_flat), got_flat)
    assert any(u["count"] > 1 for u in got)


# ------------------------------------------------------------------------------------------------ header, binding, facade
def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "az_replay.h")).read(), flags=re.S)
    return {name: (ret, [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in re.findall(r"\b(int|int64_t)\s+(az_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_entries():
    decl = _declarations()
    assert decl["az_replay_dedupe_positions"] == ("int", ["az_replay *r", "int32_t mirror", "void *stream"])
    assert decl["az_replay_unique_counts_device"] == ("int", ["az_replay *r", "int32_t *counts_out_dev", "int64_t n", "void *stream"])
    assert decl["az_replay_dedupe"] == ("int", ["az_replay *r", "void *stream"])       # the reference's rule keeps its entry


def test_lib_binds_the_entries():
    proto = {n: (res, args) for n, res, args in _lib.PROTOTYPES}
    decl = _declarations()
    for name in ENTRIES:
        assert name in proto and proto[name][0] is C.c_int and len(proto[name][1]) == len(decl[name][1]), name
    assert proto["az_replay_dedupe_positions"][1][1] is C.c_int32
    assert proto["az_replay_unique_counts_device"][1][2] is C.c_int64
    lib = _lib.load()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == proto[name][1]


def test_dedupe_arguments_are_checked_without_a_device():
    assert replay.dedupe_mode() is None and replay.dedupe_mode("history", False) is None
    assert replay.dedupe_mode("position") == 0 and replay.dedupe_mode("position", True) == 1
    with pytest.raises(ValueError, match="no mirror key"):
        replay.dedupe_mode("history", True)
    with pytest.raises(ValueError, match="by must be"):
        replay.dedupe_mode("positions")

    class _NoStore:
        """dedupe() must refuse before it touches the library."""
    with pytest.raises(ValueError, match="no mirror key"):
        replay.DeviceReplay.dedupe(_NoStore(), by="history", mirror=True)
