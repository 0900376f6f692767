"""Forced playouts and policy target pruning (az_engine_set_forced_playouts), the parts that need no GPU: the Python model of
tests/forced_playouts_cases.py is pinned against the C oracle at k = 0, its games on the inputs of the GPU test show every effect
the two rules must have, and the ABI / facade surfaces exist."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import forced_playouts_cases as FC
from alphazero_openspiel_amd import _lib
from oracle import binding as orc
from oracle import fakepolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=5,columns=4)"]
BACKUPS = ["on-policy", "soft-Z", "A0C", "off-policy"]


def _config(seed):
    """Drawn like _config of tests/test_fuzz_parity_gpu.py; game, value target, tree reuse and root noise cycle with the seed so
    that 12 seeds cover them all."""
    r = np.random.RandomState(3000 + seed)
    use_dirichlet = seed % 4 != 3
    kw = dict(n_playouts=int(r.randint(8, 41)), use_dirichlet=use_dirichlet, backup=BACKUPS[(seed // 3) % 4],
              temperature=[1.0, 1.0, 0.5, 2.0][r.randint(4)], keep_search_tree=seed % 5 != 2,
              c_puct=float(r.choice([0.5, 1.0, 2.5, 4.0])), dirichlet_ratio=float(r.choice([0.1, 0.25, 0.5])),
              num_probabilistic_actions=int(r.choice([1000, 1000, 0, 3, 7])), use_puct=bool(r.rand() < 0.8))
    return GAMES[seed % 3], int(r.randint(100)), kw, r


CONFIGS = range(14)


def test_the_configurations_cover_the_option_space():
    seen = [(_config(s)[0], _config(s)[2]) for s in CONFIGS]
    assert {g for g, _ in seen} == set(GAMES) and {kw["backup"] for _, kw in seen} == set(BACKUPS)
    assert {kw["keep_search_tree"] for _, kw in seen} == {False, True} == {kw["use_dirichlet"] for _, kw in seen}
    assert all(8 <= kw["n_playouts"] <= 40 for _, kw in seen) and len(seen) >= 12


@pytest.mark.parametrize("seed", CONFIGS)
def test_model_without_forcing_is_play_game_self(seed):
    game, salt, kw, r = _config(seed)
    A, mp, _, cells = FC.geometry(game)
    etas = [r.dirichlet(0.3 * np.ones(3 * cells)).tolist() for _ in range(mp)]
    us = r.random_sample(mp).tolist()
    want = orc.play_game_self(lambda b: fakepolicy.fake_eval(b, A, salt), game, etas=etas, us=us, **kw)
    got = FC.play_game(game, salt, etas, us, k=0.0, prune_targets=True, **kw)
    assert got["actions"] == want["actions"] and got["ret0"] == want["ret0"], (seed, game, kw)
    assert got["counters"] == want["counters"], (seed, game, kw)
    for j, ply in enumerate(got["plies"]):
        assert ply["raw"] == ply["recorded"] == want["root_cN"][j], (seed, j)
        assert ply["move"] == want["actions"][j]
        assert ply["pi"] == ply["pi_raw"] == want["examples"][j][2], (seed, j)
        assert ply["value"] == want["examples"][j][3], (seed, j, kw["backup"])


def test_the_rules_bite_on_the_inputs_of_the_gpu_test():
    differs = pruned = singles = by_puct = 0
    for idx, case in enumerate(FC.CASES):
        assert FC.S <= 40
        plain, forced = FC.model_games(idx, 0.0), FC.model_games(idx, FC.K)
        for a, b in zip(plain, forced):
            differs += sum(1 for pa, pb in zip(a["plies"], b["plies"]) if pa["raw"] != pb["raw"])
            for j, ply in enumerate(b["plies"]):
                raw, rec, F = ply["raw"], ply["recorded"], ply["budgets"]
                best = raw.index(max(raw))
                assert rec[best] == raw[best] and ply["full"]
                # a child gives back at most its budget F - and, where that leaves it a single playout, that one too (the
                # single-playout rule acts after the bound lo = n - F: the only way past F, and by exactly one)
                for i, (n, m, f) in enumerate(zip(raw, rec, F)):
                    assert 0 <= n - m <= f or (i in ply["singles"] and m == 0 and n - 1 <= f), (idx, j, i)
                # what the search added: with root noise every playout passes a root child (a fresh tree starts from none)
                assert sum(raw) == ply["carried"] + FC.S and (case["kw"]["keep_search_tree"] or ply["carried"] == 0), (idx, j)
                pruned += rec != raw
                singles += sum(1 for i in ply["singles"] if raw[i] > 1 and rec[i] == 0)
                by_puct += len(ply["by_puct"])
            assert b["counters"]["sims"] == FC.S * len(b["plies"])
    assert differs > 0 and pruned > 0 and singles > 0 and by_puct > 0, (differs, pruned, singles, by_puct)


def test_abi_surface():
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    assert protos["az_engine_set_forced_playouts"] == (C.c_int, [C.c_void_p, C.c_double, C.c_int32])
    header = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"int az_engine_set_forced_playouts\(az_engine \*e, double k, int32_t prune\);", header)
    lib = _lib.load()                                                    # (raises if the library lacks a declared symbol)
    assert lib.az_engine_set_forced_playouts.argtypes == protos["az_engine_set_forced_playouts"][1]
    # az_config and az_progress keep their layout
    assert C.sizeof(_lib.AzConfig) == 152 and _lib.AzConfig.seed.offset == 104 and _lib.AzConfig.spare_pools.offset == 148


def test_example_generator_takes_and_refuses_the_setting():
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    net = torch.nn.Identity()
    kw = dict(n_playouts=24)                                             # (no device is touched before a generation is asked for)
    assert ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=2.0, **kw).forced_playouts == (2.0, True)
    assert ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=(1.5, False), **kw).forced_playouts == (1.5, False)
    assert ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=0, **kw).forced_playouts is None
    assert ExampleGenerator(net, "connect_four", "cuda:0", **kw).forced_playouts is None
    # unlike a playout cap, the setting goes with every way of building engines
    for ok in (dict(continuous=True), dict(n_pools=2), dict(pool_devices=["cuda:0"]), dict(overlap=2), dict(playout_cap=(6, 0.5))):
        assert ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=2.0, **kw, **ok).forced_playouts == (2.0, True)
    with pytest.raises(ValueError, match="forced_playouts.*is_test=True"):
        ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=2.0, is_test=True, **kw)
    with pytest.raises(ValueError, match="forced_playouts.*use_puct=False"):
        ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=2.0, use_puct=False, **kw)
    for bad in (-1.0, float("nan"), float("inf"), "a", (2.0, 2), (2.0, True, 1), (None, True)):
        with pytest.raises(ValueError, match="forced_playouts"):
            ExampleGenerator(net, "connect_four", "cuda:0", forced_playouts=bad, **kw)
