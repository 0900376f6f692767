"""Evaluation in a random left-right orientation (az_engine_set_eval_mirror), the parts that need no GPU: the ABI surface, the
coin model of tests/eval_mirror_cases.py at the seed the GPU tests use, the observation of a mirrored state (the HOST build of
csrc/az_games.h in a small stand-alone program, as tests/test_mirror_host.py does), and the ExampleGenerator refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import eval_mirror_cases as EM
from conftest import ROOT
from alphazero_openspiel_amd import _lib, games
from philox_cases import cap_uniform


# ------------------------------------------------------------------------------------------------ 1. ABI surface
def test_header_declares_both_entries():
    header = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"^int az_engine_set_eval_mirror\(az_engine \*e, double p_mirror\);$", header, flags=re.M)
    assert re.search(r"^int az_engine_read_request_mirror\(az_engine \*e, int32_t slot\);$", header, flags=re.M)
    doc = header[:header.index("int az_engine_set_eval_mirror(")].rsplit("/*", 1)[1]
    for word in ("purpose 4", "purpose 5", "AZ_ACTION_SEARCH_AGAIN", "az_mirror_state", "az_mirror_action", "leaf_bb", "AZ_E_STATE"):
        assert word in doc, word                                          # documented next to its neighbours
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    vp = C.c_void_p
    assert protos["az_engine_set_eval_mirror"] == (C.c_int, [vp, C.c_double])
    assert protos["az_engine_read_request_mirror"] == (C.c_int, [vp, C.c_int32])
    lib = _lib.load()                                                     # (raises if the library lacks a declared symbol)
    for name in ("az_engine_set_eval_mirror", "az_engine_read_request_mirror"):
        assert getattr(lib, name).argtypes == protos[name][1]
    assert C.sizeof(_lib.AzConfig) == 152                                 # az_config keeps its layout: it is an engine SETTING


# ------------------------------------------------------------------------------------------------ 2. the coin model
def test_coin_model_gives_both_values_early_in_every_game():
    for g in range(EM.N):
        assert set(EM.first_requests(EM.SEED, g, 0.5)) == {True, False}, \
            "game %d of seed %d has one orientation only in its first six requests: choose another seed" % (g, EM.SEED)
    # the streams: purposes 4 and 5 beside the taken 0..3, keyed by game id, root ply and (leaves) the playout index
    u = cap_uniform(EM.SEED, 3, 5, purpose=4, idx=7)
    assert len({u, cap_uniform(EM.SEED, 3, 5, purpose=4, idx=8), cap_uniform(EM.SEED, 3, 6, purpose=4, idx=7),
                cap_uniform(EM.SEED, 4, 5, purpose=4, idx=7), cap_uniform(EM.SEED + 1, 3, 5, purpose=4, idx=7),
                cap_uniform(EM.SEED, 3, 5, purpose=5, idx=7), cap_uniform(EM.SEED, 3, 5, purpose=3, idx=7)}) == 7
    assert EM.coin(EM.SEED, 3, 5, EM.PH_WAIT_LEAF, 7, 0.5) == (u < 0.5)
    assert EM.coin(EM.SEED, 3, 5, EM.PH_WAIT_ROOT, 7, 0.5) == (cap_uniform(EM.SEED, 3, 5, purpose=5, idx=0) < 0.5)   # a root: index 0
    for phase in (0, 1, 2, 5):
        assert EM.coin(EM.SEED, 3, 5, phase, 7, 1.0) is False             # no request outstanding
    for g in range(EM.N):
        assert all(EM.first_requests(EM.SEED, g, 1.0)) and not any(EM.first_requests(EM.SEED, g, 0.0))


# ------------------------------------------------------------------------------------------------ 3. the mirrored observation
_PROGRAM = r"""
#include <cstdio>
#include "az_games.h"
template <int GAME> static void obs_lines(const AzState &s, const AzGeom &g, int n) {
    const AzState m = az_mirror_state<GAME>(s, g);
    for (int i = 0; i < n; i++) printf("%d ", (int)az_obs_elem<GAME>(s, g, i));
    printf("\n");
    for (int i = 0; i < n; i++) printf("%d ", (int)az_obs_elem<GAME>(m, g, i));
    printf("\n");
}
int main() {
    int game, rows, cols, ply;
    unsigned long long b0, b1;
    if (scanf("%d %d %d", &game, &rows, &cols) != 3) return 1;
    const AzGeom g = az_make_geom(game, rows, cols);
    while (scanf("%llu %llu %d", &b0, &b1, &ply) == 3) {
        AzState s;
        s.bb0 = b0, s.bb1 = b1, s.ply = ply;
        if (game == AZG_CONNECT_FOUR) obs_lines<AZG_CONNECT_FOUR>(s, g, 4 * rows * cols);
        else obs_lines<AZG_BREAKTHROUGH>(s, g, 4 * rows * cols);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def obs_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_mirror")
    src, exe = d / "obs.cpp", d / "obs"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])
    return str(exe)


def _reachable_states(game, seed, n_plies=200):
    """Non-terminal positions of random playouts as (bb0, bb1, ply)."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n_plies:
        s = game.new_initial_state()
        while not s.is_terminal():
            out.append((int(s.bb[0]), int(s.bb[1]), len(s.history())))
            la = s.legal_actions()
            s.apply_action(la[rng.randint(len(la))])
    return out


@pytest.mark.parametrize("name", [EM.C4, EM.B66, "breakthrough(rows=6,columns=5)"])
def test_observation_of_the_mirrored_state_is_the_w_flip(name, obs_program):
    game = games.load_game(name)
    states = _reachable_states(game, seed=len(name))
    text = "%d %d %d\n" % (game.game_id, game.rows, game.cols) + "".join("%d %d %d\n" % s for s in states)
    out = subprocess.run([obs_program], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(states)
    shape = (4, game.rows, game.cols)
    n_asym = 0
    for i, (b0, b1, ply) in enumerate(states):
        plain = np.array(out[2 * i].split(), dtype=np.float32).reshape(shape)
        mirrored = np.array(out[2 * i + 1].split(), dtype=np.float32).reshape(shape)
        assert (mirrored == plain[:, :, ::-1]).all(), (b0, b1, ply)       # what the reference wrapper's obs.flip(-1) gives
        # ... and the plain observation is the one the Python rules give (planes 0..2; plane 3 = the player to move)
        assert (plain[:3] == games.observation_planes(game, np.array([[b0, b1]], dtype=np.uint64))[0]).all()
        assert (plain[3] == float(ply & 1)).all()
        n_asym += bool((mirrored != plain).any())
    assert n_asym > len(states) // 2                                       # (the positions are not all their own mirror image)


# ------------------------------------------------------------------------------------------------ 4. facade refusals
def test_example_generator_refusals_need_no_device():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    net = torch.nn.Identity()
    g = ExampleGenerator(net, "connect_four", "cuda:0", n_playouts=24, eval_mirror=0.5)   # (no device is touched before a generation)
    assert g.eval_mirror == 0.5
    assert ExampleGenerator(net, "connect_four", "cuda:0", eval_mirror=0.0).eval_mirror is None
    assert ExampleGenerator(net, "connect_four", "cuda:0", eval_mirror=1).eval_mirror == 1.0
    assert ExampleGenerator(net, "connect_four", "cuda:0").eval_mirror is None
    # every way of building engines takes it: pools, pool_devices, overlap, the stream of continuous=True, and the other settings
    for kw in (dict(n_pools=2), dict(pool_devices=["cuda:0", "cuda:0"]), dict(overlap=2), dict(continuous=True),
               dict(playout_cap=(6, 0.5)), dict(forced_playouts=2.0)):
        assert ExampleGenerator(net, "connect_four", "cuda:0", n_playouts=24, eval_mirror=0.25, **kw).eval_mirror == 0.25
    with pytest.raises(ValueError, match="eval_mirror.*is_test=True"):
        ExampleGenerator(net, "connect_four", "cuda:0", eval_mirror=0.5, is_test=True)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "half", (0.5,)):
        with pytest.raises(ValueError, match=r"eval_mirror must be a probability in \[0, 1\]"):
            ExampleGenerator(net, "connect_four", "cuda:0", eval_mirror=bad)
