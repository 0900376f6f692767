"""Every combination of the search settings that selects its own tick kernel, played against the model.

launch_tick (csrc/az_engine.hip) maps (forced playouts, evaluation mirror, solver, first-play urgency) to one instantiation of
az_advance_kernel: 16 combinations less the four with forced playouts and the solver together, which the setters refuse.  The older
modules play each setting alone and each paired with FPU; here all 12 are played, connect_four self-play with injected draws and
the fake policy on the host exactly as tests/test_fpu_gpu.py does (its _run_injected and _assert_equals_model, the model of
tests/fpu_cases.py), at that module's sizes: 8 slots, 16 games, 48 playouts, kept trees, soft-Z.  Everything is compared with ==.

A combination whose branch fell back to a kernel without one of its features would still pass on inputs where that feature
happens to change nothing, so every case also asserts ON THE MODEL that each of its features acted: a pruned visit vector
(forced), a request evaluated mirrored and one evaluated as it is (mirror), a proven root (solver; the games start late so that
proofs occur), a selection that differs from the rule without FPU (fpu)."""
import itertools

import pytest

import fpu_cases as F
from test_fpu_gpu import _assert_equals_model, _run_injected

pytestmark = pytest.mark.gpu

FORCED, MIRROR, LATE, SALT = (2.0, True), 0.5, (3, 14), 13   # (chosen on the model: with this salt every feature acts in every case)
COMBOS = [c for c in itertools.product((False, True), repeat=4) if not (c[0] and c[2])]   # (forced, mirror, solver, fpu)


def _name(combo):
    return "+".join(n for n, on in zip(("forced", "mirror", "solver", "fpu"), combo) if on) or "plain"


def _case(combo):
    forced, mirror, solver, _ = combo
    c = dict(backup="soft-Z", salt=SALT)
    if forced:
        c["forced"] = FORCED
    if mirror:
        c["mirror"] = MIRROR
    if solver:
        c.update(solver=True, late=LATE)
    return c


def acted(combo, want):
    """-> the names of the features of `combo` that changed nothing in the model's games `want` (empty: every one acted)."""
    forced, mirror, solver, fpu = combo
    plies = [ply for w in want for ply in w["plies"]]
    idle = []
    if forced and not any(ply["recorded"] != ply["raw"] for ply in plies):
        idle.append("forced")
    if mirror and not (sum(w["mirrored"][0] for w in want) and sum(w["mirrored"][1] for w in want)):
        idle.append("mirror")
    if solver and not any(ply["status"] != F.UNKNOWN for ply in plies):
        idle.append("solver")
    if fpu and not sum(sum(w["fpu_effects"].values()) for w in want):
        idle.append("fpu")
    return idle


def test_the_matrix_is_the_twelve_kernels():
    assert len(COMBOS) == 12 and len(set(COMBOS)) == 12
    assert sorted(_name(c) for c in COMBOS) == sorted(set(_name(c) for c in COMBOS))


@pytest.mark.parametrize("combo", COMBOS, ids=_name)
def test_self_play_equals_the_model(combo, monkeypatch):
    key = "matrix:" + _name(combo)
    case = _case(combo)
    monkeypatch.setitem(F.GAMES, key, case)            # the key _run_injected and game_models look the case up by
    fpu = F.FPU if combo[3] else None
    want = F.game_models(key, fpu=fpu)
    assert acted(combo, want) == [], key               # (the model alone: the inputs exercise every feature of the combination)
    ex, prog, _ = _run_injected(key, fpu=fpu)
    _assert_equals_model(ex, prog, want, len(F.game_start(case)), key)
    if combo[2]:
        assert prog["terminal_hits"] > 0
