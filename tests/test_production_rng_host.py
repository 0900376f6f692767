"""The production-RNG tests' own tools, checked without a GPU: the law check accepts numpy's Dirichlet draws and rejects wrong
samplers, the move-uniform model is keyed by everything it should be, the positions are what production_rng_cases.py says, and
the ABI line of the read-back entry is in the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import production_rng_cases as PC
from alphazero_openspiel_amd import _lib, games
from philox_cases import cap_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = sorted({n for _, _, _, n in PC.LAW_POSITIONS})          # every number of legal moves the GPU law test meets
N = PC.N_LAW


def _numpy_draws(n, alpha=PC.ALPHA):
    return np.random.RandomState(20000 + n).dirichlet(alpha * np.ones(n), size=N)   # the fixed seeds of this file


@pytest.mark.parametrize("n", NS)
def test_the_reference_sampler_passes_the_bars(n):
    PC.check_dirichlet_law(_numpy_draws(n), n)


@pytest.mark.parametrize("n", [n for n in NS if n >= 2])
def test_the_bars_see_a_wrong_sampler(n):
    r = np.random.RandomState(30000 + n)
    for alpha in (0.2, 0.45):
        with pytest.raises(AssertionError):
            PC.check_dirichlet_law(_numpy_draws(n, alpha), n)
    unboosted = r.gamma(PC.ALPHA + 1.0, size=(N, n))         # Marsaglia-Tsang at alpha + 1 without the U^(1/alpha) factor
    with pytest.raises(AssertionError):
        PC.check_dirichlet_law(unboosted / unboosted.sum(1, keepdims=True), n)
    shared = r.gamma(PC.ALPHA, size=(N, n))
    shared[:, 1] = shared[:, 0]                               # the first two children read the same gamma draw
    with pytest.raises(AssertionError):
        PC.check_dirichlet_law(shared / shared.sum(1, keepdims=True), n)
    bad = _numpy_draws(n)
    bad[7, n - 1] = np.nan
    with pytest.raises(AssertionError, match="finite"):
        PC.check_dirichlet_law(bad, n)


def test_single_move_rows():
    PC.check_dirichlet_law(np.ones((N, 3)), 1)                # (entries beyond n_legal are not looked at)
    one = _numpy_draws(1)                                     # numpy's own draw is x * (1 / x): within an ulp of 1, not always 1.0
    assert np.abs(one - 1.0).max() <= 2.0 ** -53
    with pytest.raises(AssertionError):
        PC.check_dirichlet_law(np.full((N, 1), 1.0 - 1e-9), 1)


def test_ks_bar_is_the_existing_bar_shared_out():
    assert PC.N_KS_TESTS == sum(len({0, n // 2, n - 1}) for _, _, _, n in PC.LAW_POSITIONS if n >= 2) == 14
    assert PC.KS_P_BAR == 1e-3 / 14


def test_move_uniform_is_keyed_by_seed_halves_game_ply_and_purpose():
    base = PC.move_uniform(777, 3, 5)
    others = [PC.move_uniform(778, 3, 5), PC.move_uniform(777 + (1 << 32), 3, 5), PC.move_uniform(777, 4, 5),
              PC.move_uniform(777, 3, 6), PC.move_uniform(777, 3, 5, purpose=3), PC.move_uniform(777, 3, 5, purpose=0),
              PC.move_uniform(777, 5, 3)]
    assert 0.0 <= base < 1.0 and base not in others and len(set(others)) == len(others)
    assert base == cap_uniform(777, 3, 5, purpose=1) != cap_uniform(777, 3, 5)


def test_positions_are_legal_and_have_the_stated_moves():
    for label, name, prefix, n in PC.LAW_POSITIONS:
        s = games.state_from_history(games.load_game(name), prefix)          # raises on an illegal action
        assert not s.is_terminal() and len(s.legal_actions()) == n, label
    full = [c for c in range(7) if c not in games.state_from_history(games.load_game("connect_four"), PC.LAW_POSITIONS[0][2]).legal_actions()]
    assert len(full) == 3
    bt6 = games.state_from_history(games.load_game(PC.BT66), PC.LAW_POSITIONS[2][2])
    assert sum(a & 1 for a in PC.LAW_POSITIONS[2][2]) >= 2 and bin(bt6.bb[0]).count("1") == 11 and bin(bt6.bb[1]).count("1") == 11
    for name, pa, na, pb, nb in PC.KEY_PAIRS:
        g = games.load_game(name)
        sa, sb = games.state_from_history(g, pa), games.state_from_history(g, pb)
        assert len(pa) == len(pb) and sa.bb != sb.bb and na != nb
        assert (len(sa.legal_actions()), len(sb.legal_actions())) == (na, nb) and not sa.is_terminal() and not sb.is_terminal()


def test_abi_line_of_the_noise_read_back():
    protos = {name: (res, args) for name, res, args in _lib.PROTOTYPES}
    assert protos["az_engine_read_root_noise"] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)])
    hdr = open(os.path.join(ROOT, "include", "az_engine.h")).read()
    assert re.search(r"int az_engine_read_root_noise\(az_engine \*e, int32_t slot, double \*eta_out\);", hdr)
    assert _lib.load().az_engine_read_root_noise.argtypes == protos["az_engine_read_root_noise"][1]
