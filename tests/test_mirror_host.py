"""CPU-only checks of the left-right mirror (csrc/az_games.h: az_mirror_state, az_mirror_action) and of the C ABI surface of
az_replay_sample_sym.

The two helpers are host + device code; here their HOST build runs in a small stand-alone C++ program compiled at test time
(g++ over az_games.h, as tests/test_reanalyse_host.py does for az_check_state) over every position of the rules fixtures,
random playouts, and a few invalid states.  The symmetry is checked against the dynamics themselves (az_check_state, the legal
actions, az_apply) and against the Python rules and observation planes of alphazero_openspiel_amd.games."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reanalyse_cases as RA
from conftest import ROOT, load_golden
from mirror_cases import mirror_action_py
from alphazero_openspiel_amd import _lib, games

# board -> its rules fixture (None: random playouts only).  6 rows x 5 columns and 5 x 4 are not square: mixing rows up with
# columns hides on the square boards.
BOARDS = {"connect_four": "connect_four", "breakthrough(rows=6,columns=6)": "breakthrough6",
          "breakthrough(rows=8,columns=8)": "breakthrough8", "breakthrough(rows=6,columns=5)": None,
          "breakthrough(rows=5,columns=4)": "breakthrough5x4"}


_PROGRAM = r"""
#include <cstdio>
#include "az_games.h"
template <int GAME> static void state_line(AzState s, const AzGeom &g, int mp) {
    AzState m = az_mirror_state<GAME>(s, g), mm = az_mirror_state<GAME>(m, g);
    int ok = az_check_state<GAME>(s, g, mp), okm = az_check_state<GAME>(m, g, mp);
    printf("%llu %llu %d %llu %llu %d %d %d", (unsigned long long)m.bb0, (unsigned long long)m.bb1, m.ply,
           (unsigned long long)mm.bb0, (unsigned long long)mm.bb1, mm.ply, ok, okm);
    if (ok == AZ_STATE_OK && okm == AZ_STATE_OK) {
        int n = az_count_legal<GAME>(s, g), nm = az_count_legal<GAME>(m, g);
        printf(" | %d", n);
        for (int k = 0; k < n; k++) printf(" %d", az_nth_legal<GAME>(s, g, k));
        printf(" | %d", nm);
        for (int k = 0; k < nm; k++) printf(" %d", az_nth_legal<GAME>(m, g, k));
        printf(" |");
        for (int k = 0; k < n; k++) { // mirror(apply(s, a)) next to apply(mirror(s), mirror(a))
            int a = az_nth_legal<GAME>(s, g, k), ma = az_mirror_action<GAME>(a, g);
            AzState t = s, tm = m;
            float r = 0.f, rm = 0.f;
            int term = az_apply<GAME>(t, g, a, &r), termm = az_apply<GAME>(tm, g, ma, &rm);
            t = az_mirror_state<GAME>(t, g);
            printf(" %d %llu %llu %d %d %g %llu %llu %d %d %g", ma, (unsigned long long)t.bb0, (unsigned long long)t.bb1, t.ply, term,
                   term ? r : 0.f, (unsigned long long)tm.bb0, (unsigned long long)tm.bb1, tm.ply, termm, termm ? rm : 0.f);
        }
    }
    printf("\n");
}
int main() {
    int game, rows, cols, ply;
    unsigned long long b0, b1;
    if (scanf("%d %d %d", &game, &rows, &cols) != 3) return 1;
    AzGeom g = az_make_geom(game, rows, cols);
    int mp = az_max_plies(game, rows, cols), A = az_num_actions(game, rows, cols);
    for (int a = 0; a < A; a++) { // first line: the action mirror and its square over [0, A)
        int m = game == AZG_CONNECT_FOUR ? az_mirror_action<AZG_CONNECT_FOUR>(a, g) : az_mirror_action<AZG_BREAKTHROUGH>(a, g);
        int mm = game == AZG_CONNECT_FOUR ? az_mirror_action<AZG_CONNECT_FOUR>(m, g) : az_mirror_action<AZG_BREAKTHROUGH>(m, g);
        printf("%d %d ", m, mm);
    }
    printf("\n");
    while (scanf("%llu %llu %d", &b0, &b1, &ply) == 3) {
        AzState s;
        s.bb0 = b0, s.bb1 = b1, s.ply = ply;
        if (game == AZG_CONNECT_FOUR) state_line<AZG_CONNECT_FOUR>(s, g, mp);
        else state_line<AZG_BREAKTHROUGH>(s, g, mp);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def mirror_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mirror")
    src, exe = d / "mirror.cpp", d / "mirror"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(game, states):
        """-> (action mirror [A], its square [A], one parsed record per state)"""
        text = "%d %d %d\n" % (game.game_id, game.rows, game.cols)
        text += "".join("%d %d %d\n" % s for s in states)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(states) + 1
        first = [int(v) for v in out[0].split()]
        recs = []
        for line in out[1:]:
            parts = [[v for v in p.split()] for p in line.split("|")]
            h = [int(v) for v in parts[0]]
            rec = {"m": tuple(h[0:3]), "mm": tuple(h[3:6]), "ok": h[6], "okm": h[7], "legal": None}
            if len(parts) > 1:
                rec["legal"] = [int(v) for v in parts[1][1:]]
                rec["legal_m"] = [int(v) for v in parts[2][1:]]
                assert len(rec["legal"]) == int(parts[1][0]) and len(rec["legal_m"]) == int(parts[2][0])
                f = parts[3]
                assert len(f) == 11 * len(rec["legal"])
                rec["moves"] = [(int(f[i]), (int(f[i + 1]), int(f[i + 2]), int(f[i + 3]), int(f[i + 4]), float(f[i + 5])),
                                 (int(f[i + 6]), int(f[i + 7]), int(f[i + 8]), int(f[i + 9]), float(f[i + 10])))
                                for i in range(0, len(f), 11)]
            recs.append(rec)
        return first[0::2], first[1::2], recs

    return run


def _positions(game, tag, seed):
    """(live, final): every non-terminal position of the board's rules fixture and of random playouts of a few hundred plies
    in all, as (bb0, bb1, ply); and the terminal positions the games end in."""
    histories = []
    if tag is not None:
        blob = load_golden("rules_%s.json" % tag)
        assert games.load_game(blob["game"]).name == game.name
        histories += [[p["action"] for p in g["plies"]] for g in blob["games"]]
    rng = np.random.RandomState(seed)
    plies = 0
    while plies < 300:
        s, h = game.new_initial_state(), []
        while not s.is_terminal():
            la = s.legal_actions()
            h.append(la[rng.randint(len(la))])
            s.apply_action(h[-1])
        histories.append(h)
        plies += len(h)
    live, final = [], []
    for h in histories:
        s = game.new_initial_state()
        for a in h:
            live.append((int(s.bb[0]), int(s.bb[1]), len(s.history())))
            s.apply_action(a)
        assert s.is_terminal()
        final.append((int(s.bb[0]), int(s.bb[1]), len(s.history())))
    return live, final


@pytest.mark.parametrize("name", list(BOARDS))
def test_mirror_is_a_symmetry_of_the_dynamics(name, mirror_program):
    game = games.load_game(name)
    A = game.num_distinct_actions()
    live, final = _positions(game, BOARDS[name], seed=len(name))
    assert len(live) >= 300
    bad = [(b0, b1, ply) for _, b0, b1, ply, _ in RA.bad_states(game)] if game.rows * game.cols < 60 or game.game_id == 0 else []
    states = live + final + bad
    m, mm, recs = mirror_program(game, states)
    # the action mirror: an involution of [0, A), the independent restatement, and no fixed point beyond a centre column
    assert mm == list(range(A)) and sorted(m) == list(range(A))
    assert m == [mirror_action_py(game, a) for a in range(A)]
    if game.cols % 2 == 0:
        assert all(m[a] != a for a in range(A))
    n_asym = 0
    for (b0, b1, ply), rec in zip(states, recs):
        assert rec["mm"] == (b0, b1, ply)                                    # mirror o mirror = identity
        assert rec["m"][2] == ply
        assert rec["ok"] == rec["okm"], (b0, b1, ply)                        # accepted together, refused for the same rule
        # the mirrored state IS the column-reversed board: compare the observation planes of the Python rules
        planes = games.observation_planes(game, np.array([[b0, b1], rec["m"][:2]], dtype=np.uint64))
        assert (planes[1] == planes[0][:, :, ::-1]).all()
        n_asym += rec["m"][:2] != (b0, b1)
    for (b0, b1, ply), rec in zip(live, recs):                               # every non-terminal position
        assert rec["ok"] == RA.OK and rec["legal"] is not None
        legal = games.legal_actions_from_bitboards(game, b0, b1, ply)
        assert rec["legal"] == legal                                         # (the C helpers agree with the Python rules)
        assert rec["legal_m"] == sorted(m[a] for a in legal)                 # legal(mirror s) = mirror(legal s)
        assert rec["legal_m"] == games.legal_actions_from_bitboards(game, rec["m"][0], rec["m"][1], ply)
        for a, (ma, mirrored_after, after_mirrored) in zip(legal, rec["moves"]):
            assert ma == m[a]
            assert mirrored_after == after_mirrored, (b0, b1, ply, a)        # state, terminal flag and ret0
    for rec in recs[len(live):]:
        assert rec["ok"] != RA.OK and rec["legal"] is None                   # terminal and invalid states: refused both ways
    assert n_asym > len(states) // 2                                         # (the positions are not all their own mirror image)


# ------------------------------------------------------------------------------------------------ the C ABI surface
def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "az_replay.h")).read(), flags=re.S)
    return {name: (ret, [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in re.findall(r"\b(int|int64_t)\s+(az_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}


def test_abi_declares_and_exports_az_replay_sample_sym():
    decl = _declarations()
    assert decl["az_replay_sample_sym"] == ("int", [
        "az_replay *r", "const int64_t *indices", "const uint8_t *flips", "int32_t batch", "uint64_t seed", "float *x", "float *pi",
        "float *z", "void *stream"])
    # az_replay_sample plus the flips, in the documented place
    plain = decl["az_replay_sample"][1]
    assert plain[:2] + ["const uint8_t *flips"] + plain[2:] == decl["az_replay_sample_sym"][1]
    proto = {n: (res, args) for n, res, args in _lib.PROTOTYPES}
    res, args = proto["az_replay_sample_sym"]
    vp = C.c_void_p
    assert res is C.c_int and args == [vp, vp, vp, C.c_int32, C.c_uint64, vp, vp, vp, vp]
    lib = _lib.load()
    assert hasattr(lib, "az_replay_sample_sym")
    header = open(os.path.join(ROOT, "include", "az_replay.h")).read()
    doc = header[:header.index("int az_replay_sample_sym(")].rsplit("/*", 1)[1]
    assert "flips" in doc and "AZ_REPLAY_FAULT_BAD_INDEX" in doc and "AZ_E_STATE" in doc  # documented next to its neighbours
