"""CPU-only checks of self-play from per-game start positions: the C ABI surface of its five entries, the scalar / array forms
of examples_from_export and unpack_device_export, the HOST build of the shared key-chain header (csrc/az_keychain.h)
against a Python restatement of the chain written here, and the host replay of an action prefix (csrc/az_starts.h) against
games.py and that chain.

The headers are checked through small stand-alone C++ programs compiled at test time (g++, where AZ_KEY_HD is plain `inline`):
the library's entries need a device, the shared headers do not."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import replay_cases as RC
from conftest import ROOT
from alphazero_openspiel_amd import _lib, games
from alphazero_openspiel_amd.engine import examples_from_export, unpack_device_export

ENTRIES = ("az_engine_set_game_starts", "az_engine_set_game_starts_device", "az_engine_game_starts_device",
           "az_replay_gather_forks", "az_replay_append_device_starts")
M64 = (1 << 64) - 1


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declarations():
    """{entry: (return type, [parameter declarations])} from the headers, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _header("az_engine.h") + _header("az_replay.h"), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|int64_t)\s+(az_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = (ret, [" ".join(p.split()) for p in params.split(",")])
    return out


def test_headers_declare_the_entries():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl and decl[name][0] == "int", name
    assert decl["az_engine_set_game_starts"][1] == decl["az_engine_set_start_positions"][1]
    assert decl["az_engine_set_game_starts_device"][1][1:4] == ["const uint64_t *bb_dev", "const int32_t *ply_dev",
                                                                "const uint64_t *keys_dev"]
    assert decl["az_engine_game_starts_device"][1][1:3] == ["int32_t *ply_out_dev", "uint64_t *keys_out_dev"]
    assert decl["az_replay_gather_forks"][1][:5] == decl["az_replay_gather_states"][1][:5]
    assert decl["az_replay_gather_forks"][1][5] == "uint64_t *keys_out"
    assert decl["az_replay_append_device_starts"][1][3:5] == ["const int32_t *start_ply_dev", "const uint64_t *keys_dev"]
    # the entries whose behaviour must not change keep their argument lists
    assert len(decl["az_engine_set_start_states_device"][1]) == 5 and len(decl["az_replay_append_device"][1]) == 5
    assert len(decl["az_engine_export_device"][1]) == 4


def test_lib_binds_the_entries_with_matching_argument_lists():
    decl = _declarations()
    proto = {n: (res, args) for n, res, args in _lib.PROTOTYPES}
    lib = _lib.load()
    for name in ENTRIES:
        res, args = proto[name]
        assert len(args) == len(decl[name][1]), name
        assert res is C.c_int, name
        for i, (a, d) in enumerate(zip(args, decl[name][1])):
            if name == "az_engine_set_game_starts" and i in (1, 2):
                want = C.POINTER(C.c_int32)           # host arrays, as az_engine_set_start_positions binds them
            else:
                want = C.c_void_p if "*" in d else {"int64_t": C.c_int64, "int32_t": C.c_int32}[d.split()[0]]
            assert a is want, (name, d)
        assert hasattr(lib, name)
    assert proto["az_engine_set_game_starts"][1] == proto["az_engine_set_start_positions"][1]


# ------------------------------------------------------------------------------------------------ export forms
def _concat(exs, plies):
    out = {k: np.concatenate([ex[k] for ex in exs]) for k in exs[0] if k != "start_ply"}
    out["start_ply"] = np.concatenate([np.full(len(ex["game_len"]), p, np.int32) for ex, p in zip(exs, plies)])
    return out


@pytest.mark.parametrize("name", ["connect_four", "breakthrough(rows=5,columns=4)"])
def test_scalar_and_array_forms_of_examples_from_export_agree(name):
    game = games.load_game(name)
    hists = [[], RC.random_openings(game, 1, 1, 3)[0], RC.random_openings(game, 1, 4, 4)[0]]
    exs = [RC.fake_export(game, n_games=3, seed=10 + i, start_history=h) for i, h in enumerate(hists)]
    want = [g for ex, h in zip(exs, hists) for g in examples_from_export(game, ex, h)]
    both = _concat(exs, [len(h) for h in hists])
    per_game = [h for h in hists for _ in range(3)]
    got = examples_from_export(game, both, per_game)
    assert len(got) == len(want) == 9
    for a, b in zip(got, want):
        assert len(a) == len(b) > 0
        for x, y in zip(a, b):
            assert x[0] == y[0] and (x[1] == y[1]).all() and x[2] == y[2] and x[3] == y[3]
    assert [g[0][0] for g in got] == [", ".join(map(str, h)) for h in per_game]
    # one shared prefix given in either form
    one = examples_from_export(game, exs[2], hists[2])
    ex = dict(exs[2], start_ply=np.full(3, len(hists[2]), np.int32))
    two = examples_from_export(game, ex, [hists[2]] * 3)
    assert [[r[0] for r in g] for g in one] == [[r[0] for r in g] for g in two]
    with pytest.raises(ValueError):
        examples_from_export(game, both, per_game[:4])
    for flat_history in ((), hists[2]):              # a start ply per game without a history per game: no key strings to build
        with pytest.raises(ValueError, match="start history per game"):
            examples_from_export(game, both, flat_history)
    # unpack_device_export: the same two forms
    buf = RC.pack_device_export(both)
    n, mp = both["move"].shape
    mc = both["child_action"].shape[2]
    arr = unpack_device_export(buf, n, mp, mc, start_ply=both["start_ply"])
    assert arr["start_ply"].dtype == np.int32 and arr["start_ply"].tolist() == both["start_ply"].tolist()
    assert unpack_device_export(buf, n, mp, mc, start_ply=2)["start_ply"] == 2
    again = examples_from_export(game, arr, per_game)
    assert [[r[0] for r in g] for g in again] == [[r[0] for r in g] for g in got]


# ------------------------------------------------------------------------------------------------ the key chain
def _mix64(h, v):
    z = (h + 0x9E3779B97F4A7C15 * ((v + 1) & M64)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _seed(ply, bb0, bb1):
    key = _mix64(_mix64(_mix64(0x243F6A8885A308D3, ply), bb0), bb1)
    key2 = _mix64(0x13198A2E03707344 ^ ply, (bb0 + 0x9E3779B97F4A7C15 * bb1) & M64)
    return key, key2


def _step(pair, move, index):
    return _mix64(pair[0], move), _mix64(pair[1] ^ 0xA4093822299F31D0, (move << 20) | index)


def _chain(game, start_history, moves, given=None):
    """The pairs of a game's examples: seeded from its start state (index 1, 2, ...), or continuing `given` by absolute ply."""
    s = games.state_from_history(game, start_history)
    p0 = len(start_history)
    pair, base = (given, p0) if given is not None else (_seed(p0, int(s.bb[0]), int(s.bb[1])), 0)
    out = []
    for i, m in enumerate(moves):
        out.append(pair)
        pair = _step(pair, int(m), base + i + 1)
    return out, pair


_PROGRAM = r"""
#include <cstdio>
#include "az_keychain.h"
int main() { // per line: ply bb0 bb1 given(0/1) key key2 n m_1 .. m_n  ->  the pair after every move
    int ply, given, n;
    unsigned long long b0, b1, k1, k2;
    while (scanf("%d %llu %llu %d %llu %llu %d", &ply, &b0, &b1, &given, &k1, &k2, &n) == 7) {
        AzKeyPair k = az_key_seed(ply, b0, b1);
        if (given) k.key = k1, k.key2 = k2;
        printf("%llu %llu", (unsigned long long)k.key, (unsigned long long)k.key2);
        for (int i = 0; i < n; i++) {
            unsigned m;
            if (scanf("%u", &m) != 1) return 1;
            k = az_key_step(k, m, (given ? ply : 0) + i + 1);
            printf(" %llu %llu", (unsigned long long)k.key, (unsigned long long)k.key2);
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_chain(tmp_path_factory):
    d = tmp_path_factory.mktemp("keychain")
    src, exe = d / "chain.cpp", d / "chain"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(cases):
        text = "".join("%d %d %d %d %d %d %d %s\n" % (ply, b0, b1, int(given is not None), *(given or (0, 0)), len(moves),
                                                       " ".join(map(str, moves))) for ply, b0, b1, given, moves in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [[(int(w[i]), int(w[i + 1])) for i in range(0, len(w), 2)] for w in (line.split() for line in out)]

    return run


@pytest.mark.parametrize("name", ["connect_four", "breakthrough(rows=6,columns=6)"])
def test_header_chain_is_the_python_chain_and_obeys_the_key_rule(name, header_chain):
    game = games.load_game(name)
    ex = RC.fake_export(game, n_games=4, seed=21)
    cases, want = [], []
    for g in range(4):
        moves = ex["move"][g, :int(ex["game_len"][g])].tolist()
        whole, last = _chain(game, [], moves)
        s0 = games.state_from_history(game, [])
        cases.append((0, int(s0.bb[0]), int(s0.bb[1]), None, moves))
        want.append(whole + [last])
        for cut in (1, 3, len(moves) - 1):
            # THE KEY RULE: a game given the pair of the prefix moves[:cut] carries, from there on, the pairs of the whole game
            forked, flast = _chain(game, moves[:cut], moves[cut:], given=whole[cut])
            assert forked + [flast] == (whole + [last])[cut:]
            s = games.state_from_history(game, moves[:cut])
            cases.append((cut, int(s.bb[0]), int(s.bb[1]), whole[cut], moves[cut:]))
            want.append(forked + [flast])
            # ... while a game merely STARTED there (one shared prefix, no given pair) keeps the keys of such games: other ones
            plain, plast = _chain(game, moves[:cut], moves[cut:])
            assert plain[0] != whole[cut]
            cases.append((cut, int(s.bb[0]), int(s.bb[1]), None, moves[cut:]))
            want.append(plain + [plast])
    got = header_chain(cases)
    assert got == want
    # transposing prefixes: one position, two strings, two pairs
    if name == "connect_four":
        a, b = _chain(game, [], [3, 2, 4])[1], _chain(game, [], [4, 2, 3])[1]
        assert games.state_from_history(game, [3, 2, 4]).bb == games.state_from_history(game, [4, 2, 3]).bb
        assert a[0] != b[0] and a[1] != b[1]


# ------------------------------------------------------------------------------------------------ the host replay of a prefix
# csrc/az_starts.h: the position and key pair of an action prefix, and the game's legality check of every action id, against
# games.py and the Python chain above.  Every comparison is exact.
_STARTS_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "az_starts.h"
int main() { // per line: game rows cols n a_1 .. a_n  ->  code bb0 bb1 ply key key2
    int game, rows, cols, n;
    while (scanf("%d %d %d %d", &game, &rows, &cols, &n) == 4) {
        std::vector<int32_t> a((size_t)n + 1);
        for (int i = 0; i < n; i++)
            if (scanf("%d", &a[(size_t)i]) != 1) return 1;
        const AzGeom g = az_make_geom(game, rows, cols);
        AzState s;
        AzKeyPair k;
        const int code = az_replay_prefix(game, g, az_num_actions(game, rows, cols), a.data(), n, s, k);
        printf("%d %llu %llu %d %llu %llu\n", code, (unsigned long long)s.bb0, (unsigned long long)s.bb1, s.ply,
               (unsigned long long)k.key, (unsigned long long)k.key2);
    }
    return 0;
}
"""
STARTS_GAMES = ["connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=5,columns=4)"]


@pytest.fixture(scope="module")
def header_replay(tmp_path_factory):
    d = tmp_path_factory.mktemp("starts")
    src, exe = d / "starts.cpp", d / "starts"
    src.write_text(_STARTS_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(game, prefixes):
        """[(code, bb0, bb1, ply, key, key2)] of the header's replay, one per prefix."""
        head = "%d %d %d " % (game.game_id, game.rows, game.cols)
        text = "".join(head + " ".join(map(str, [len(p)] + list(p))) + "\n" for p in prefixes)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(prefixes)
        return [tuple(int(w) for w in line.split()) for line in out]

    return run


@functools.lru_cache(maxsize=None)
def _played_games(name):
    game = games.load_game(name)
    ex = RC.fake_export(game, n_games=3, seed=33)
    return game, [ex["move"][g, :int(ex["game_len"][g])].tolist() for g in range(3)]


def test_starts_header_compiles_without_warnings(header_replay):
    """The fixture builds with -Wall -Werror; the empty prefix is the initial position with its seed pair."""
    for name in STARTS_GAMES:
        game = games.load_game(name)
        s0 = games.state_from_history(game, [])
        assert header_replay(game, [[]]) == [(0, int(s0.bb[0]), int(s0.bb[1]), 0) + _seed(0, int(s0.bb[0]), int(s0.bb[1]))]


@pytest.mark.parametrize("name", STARTS_GAMES)
def test_header_replay_gives_the_state_and_key_pair_of_every_prefix(name, header_replay):
    game, played = _played_games(name)
    prefixes = [moves[:n] for moves in played for n in range(len(moves))]
    want = []
    for p in prefixes:
        s = games.state_from_history(game, p)
        want.append((0, int(s.bb[0]), int(s.bb[1]), len(p)) + _chain(game, [], p)[1])
    assert header_replay(game, prefixes) == want


@pytest.mark.parametrize("name", STARTS_GAMES)
def test_header_replay_judges_every_action_id_as_the_python_rules_do(name, header_replay):
    """At every position along the games, every id in [-1, A]: code 1 exactly for the ids games.py does not list (-1 and A among
    them, and a breakthrough move whose capture bit says the wrong thing), 2 exactly when the move ends the game, 0 otherwise."""
    game, played = _played_games(name)
    A = game.num_distinct_actions()
    cases, want = [], []
    seen = {"capture": 0, "plain": 0, "ends": 0}
    for moves in played:
        for n in range(len(moves)):
            s = games.state_from_history(game, moves[:n])
            legal = set(s.legal_actions())
            assert moves[n] in legal
            for a in range(-1, A + 1):
                cases.append(moves[:n] + [a])
                if a not in legal:
                    want.append(1)
                    continue
                t = s.clone()
                t.apply_action(a)
                want.append(2 if t.is_terminal() else 0)
                seen["ends"] += t.is_terminal()
                if game.game_id == 1:                      # the twin with the other capture bit is no move
                    assert a ^ 1 not in legal
                    seen["capture" if a & 1 else "plain"] += 1
        # the whole game ends with its last move, and moves after the end do not change that - legal-looking ones or not
        cases += [moves, moves + [moves[0]], moves + [A]]
        want += [2, 2, 2]
    got = header_replay(game, cases)
    assert [r[0] for r in got] == want
    assert seen["ends"] >= len(played) and (game.game_id == 0 or (seen["capture"] > 0 and seen["plain"] > 0))
    if game.game_id == 0:
        column = [0, 1, 0, 1, 0, 1]                        # four in column 0 for the first player
        assert [r[0] for r in header_replay(game, [column, column + [0], column + [0, 3], [3] * 6, [3] * 7])] == [0, 2, 2, 0, 1]
    else:
        # a move onto the last rank: one of the random games ends that way (not by capturing the last piece)
        ends = [games.state_from_history(game, moves) for moves in played]
        last_ranks = ((1 << game.cols) - 1) << ((game.rows - 1) * game.cols), (1 << game.cols) - 1
        assert any(s.bb[0] & last_ranks[0] or s.bb[1] & last_ranks[1] for s in ends)
