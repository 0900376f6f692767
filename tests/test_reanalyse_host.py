"""CPU-only checks of the reanalyse route: the C ABI surface of its three entries, and the HOST build of the state validity
function az_check_state (csrc/az_games.h) that az_engine_set_start_states_device runs on the device.

The validity function is checked through a small stand-alone C++ program compiled at test time (g++ over az_games.h, where
AZ_HD is plain `inline`): the library's entry needs a device, the shared header does not."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reanalyse_cases as RA
from conftest import ROOT, load_golden
from alphazero_openspiel_amd import _lib, games

ENTRIES = ("az_engine_set_start_states_device", "az_replay_gather_states", "az_replay_refresh_from_roots")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declarations():
    """{entry: (return type, [parameter declarations])} from the headers, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _header("az_engine.h") + _header("az_replay.h"), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|int64_t)\s+(az_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = (ret, [p.strip() for p in params.split(",")])
    return out


def test_headers_declare_the_entries_and_constants():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, name
    assert decl["az_replay_refresh_from_roots"][0] == "int64_t"
    assert decl["az_engine_set_start_states_device"][1][1:3] == ["const uint64_t *bb_dev", "const int32_t *ply_dev"]
    defines = dict(re.findall(r"#define\s+(AZ_[A-Z_0-9]+)\s+(\d+)u?\b", _header("az_replay.h")))
    assert (defines["AZ_REFRESH_KEEP_Z"], defines["AZ_REFRESH_SOFT_Z"], defines["AZ_REFRESH_A0C"]) == ("0", "1", "2")
    assert defines["AZ_REPLAY_FAULT_ROOT_MISMATCH"] == "4"
    assert (_lib.REFRESH_KEEP_Z, _lib.REFRESH_SOFT_Z, _lib.REFRESH_A0C) == (0, 1, 2)
    assert _lib.REFRESH_MODES == {None: 0, "soft-Z": 1, "A0C": 2}
    assert _lib.REPLAY_FAULTS[4] == "ROOT_MISMATCH"


def test_lib_binds_the_entries_with_matching_argument_counts():
    decl = _declarations()
    proto = {n: (res, args) for n, res, args in _lib.PROTOTYPES}
    lib = _lib.load()
    for name in ENTRIES:
        res, args = proto[name]
        assert len(args) == len(decl[name][1]), name
        assert res is {"int": C.c_int, "int64_t": C.c_int64}[decl[name][0]], name
        for a, d in zip(args, decl[name][1]):  # pointers are void*, the counts are 64-bit, value_mode is 32-bit
            want = C.c_void_p if "*" in d else {"int64_t": C.c_int64, "int32_t": C.c_int32}[d.split()[0]]
            assert a is want, (name, d)
        assert hasattr(lib, name)


_PROGRAM = r"""
#include <cstdio>
#include "az_games.h"
int main() {
    int game, rows, cols, ply;
    unsigned long long b0, b1;
    while (scanf("%d %d %d %llu %llu %d", &game, &rows, &cols, &b0, &b1, &ply) == 6) {
        AzGeom g = az_make_geom(game, rows, cols);
        AzState s;
        s.bb0 = b0, s.bb1 = b1, s.ply = ply;
        int mp = az_max_plies(game, rows, cols);
        int r = game == AZG_CONNECT_FOUR ? az_check_state<AZG_CONNECT_FOUR>(s, g, mp) : az_check_state<AZG_BREAKTHROUGH>(s, g, mp);
        printf("%d|%s\n", r, az_state_rule_name(r));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def check_states(tmp_path_factory):
    d = tmp_path_factory.mktemp("check_state")
    src, exe = d / "check.cpp", d / "check"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(game, states):
        text = "".join("%d %d %d %d %d %d\n" % (game.game_id, game.rows, game.cols, b0, b1, ply) for b0, b1, ply in states)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(states)
        return [(int(line.split("|")[0]), line.split("|")[1]) for line in out]

    return run


@pytest.mark.parametrize("tag", ["connect_four", "breakthrough6", "breakthrough8", "breakthrough5x4"])
def test_validity_function_accepts_every_non_terminal_fixture_position(tag, check_states):
    blob = load_golden("rules_%s.json" % tag)
    game = games.load_game(blob["game"])
    states = []
    for g in blob["games"]:
        s = game.new_initial_state()
        for ply in g["plies"]:
            assert not s.is_terminal()
            states.append((int(s.bb[0]), int(s.bb[1]), len(s.history())))
            s.apply_action(ply["action"])
        assert s.is_terminal()
    assert len(states) > 20
    got = check_states(game, states)
    assert [r for r, _ in got] == [RA.OK] * len(states), [(i, m) for i, (r, m) in enumerate(got) if r][:4]


@pytest.mark.parametrize("name", ["connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=5,columns=4)"])
def test_validity_function_rejects_the_hand_made_bad_states(name, check_states):
    game = games.load_game(name)
    cases = RA.bad_states(game)
    assert len(cases) == (6 if name == "connect_four" else 3)
    got = check_states(game, [(b0, b1, ply) for _, b0, b1, ply, _ in cases])
    for (what, _, _, _, rule), (r, msg) in zip(cases, got):
        assert r == rule, (what, r, msg)
    # and the states they were made from are fine: the initial position, and a position a few plies in
    start = game.new_initial_state()
    bb, ply = RA.states_of(game, [[], [start.legal_actions()[0]]])
    assert [r for r, _ in check_states(game, [(int(b[0]), int(b[1]), int(p)) for b, p in zip(bb, ply)])] == [RA.OK, RA.OK]
