"""The production RNG path (rng="philox": move_step draws the root noise and the move uniform on the device), pinned.

Exact part: the move uniform is modelled on the host (production_rng_cases.move_uniform, the suite's Python Philox at purpose 1)
and the root noise is read back while it is staged (SelfPlayEngine.read_root_noise); the C oracle replayed with those draws must
play the device's games - moves, child visits, pi, value target, ret0 and the five counters compared with ==, as in
test_fuzz_parity_gpu.py.  Law and keying part: the noise at chosen positions, 2048 game ids each, against Dirichlet(0.3) by
production_rng_cases.check_dirichlet_law, and the raw gamma of child k as a function of (seed, game id, ply, k) alone."""
import functools

import numpy as np
import pytest
import torch

import production_rng_cases as PC
from oracle import binding as orc

pytestmark = pytest.mark.gpu

SEED_LO, SEED_HI = 0x5EED1234, 0x5EED1234 + (0x9E37 << 32)   # the same low half; the second has a non-zero high half
SALT = 31
FIELDS = ("sims", "evals", "sum_depth", "terminal_hits", "sum_children")


def _E():
    from alphazero_openspiel_amd import engine
    return engine


def _dims(game):
    gid, rows, cols = orc.parse_game(game)
    return orc.lib().orc_num_actions(gid, rows, cols), orc.max_plies(gid, rows, cols)


def _play(game, n_slots, n_games, seed, record, **kw):
    """-> dict(etas, ex, games, prog, policy): n_games of a Philox engine under the fake policy."""
    E = _E()
    A, _ = _dims(game)
    policy = PC.cached_policy(A, SALT)
    eng = E.SelfPlayEngine(game, n_slots, rng="philox", seed=seed, max_games=n_games, **kw)
    eng.reset(n_games)
    ev = E.HostPolicyEvaluator(eng, policy)
    if record:
        etas, ex, prog = PC.record_and_play(eng, ev, n_games)
    else:
        etas = None
        obs, pri, val = eng.alloc_io()
        for _ in range(200000):
            eng.advance(pri, val, obs)
            ev(obs, pri, val)
            if eng.progress()["games_done"] >= n_games:
                break
        else:
            pytest.fail("games did not finish")
        ex, prog = eng.export(), eng.progress()
    games = E.examples_from_export(eng.game, ex)
    eng.close()
    assert prog["error_flags"] == 0
    return dict(etas=etas, ex=ex, games=games, prog=prog, policy=policy)


def _rows_of(run, i):
    """The recorded noise rows of game i by ply, each cut to the ply's number of children."""
    n = int(run["ex"]["game_len"][i])
    return [run["etas"][i][t][0][:int(run["ex"]["n_children"][i, t])].tolist() for t in range(n)]


def _oracle(run, game, i, seed, kw, etas=None, purpose=1):
    _, mp = _dims(game)
    us = [PC.move_uniform(seed, i, t, purpose=purpose) for t in range(mp)]
    return orc.play_game_self(run["policy"], game, etas=etas, us=us, **kw)


def _difference(run, i, want):
    """None when game i of the run equals the oracle's game `want` in every compared field, else the first difference."""
    ex, games = run["ex"], run["games"]
    n = len(want["actions"])
    if int(ex["game_len"][i]) != n:
        return "length %d != %d" % (int(ex["game_len"][i]), n)
    if ex["move"][i, :n].tolist() != want["actions"]:
        return "moves %s != %s" % (ex["move"][i, :n].tolist(), want["actions"])
    if float(ex["game_ret0"][i]) != want["ret0"]:
        return "ret0"
    for j in range(n):
        nc = int(ex["n_children"][i, j])
        if ex["child_visits"][i, j, :nc].tolist() != want["root_cN"][j]:
            return "child visits at ply %d" % j
        if games[i][j][2] != want["examples"][j][2]:
            return "pi at ply %d" % j
        if games[i][j][3] != want["examples"][j][3]:
            return "value target at ply %d" % j
        if not (games[i][j][1] == want["examples"][j][1]).all():
            return "board at ply %d" % j
    return None


def _assert_run_equals(run, game, n_games, seed, kw, with_noise):
    wants = [_oracle(run, game, i, seed, kw, etas=_rows_of(run, i) if with_noise else None) for i in range(n_games)]
    for i, w in enumerate(wants):
        d = _difference(run, i, w)
        assert d is None, (game, seed, kw, "game %d: %s" % (i, d))
    for key in FIELDS:
        assert run["prog"][key] == sum(w["counters"][key] for w in wants), (game, seed, kw, key)
    return wants


# ------------------------------------------------------------------------------------------------ the move stream alone
MOVE_CASES = [("connect_four", 3, 7, 12), (PC.BT54, 2, 5, 8)]


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "fresh"])
@pytest.mark.parametrize("game,n_slots,n_games,S", MOVE_CASES, ids=["c4", "bt54"])
def test_move_stream_equals_the_oracle_under_the_philox_model(game, n_slots, n_games, S, keep):
    kw = dict(n_playouts=S, use_dirichlet=False, keep_search_tree=keep)
    moves = {}
    for seed in (SEED_LO, SEED_HI):
        run = _play(game, n_slots, n_games, seed, False, **kw)
        _assert_run_equals(run, game, n_games, seed, kw, with_noise=False)
        moves[seed] = [run["ex"]["move"][i, :int(run["ex"]["game_len"][i])].tolist() for i in range(n_games)]
    assert moves[SEED_LO] != moves[SEED_HI], "the high half of the seed does not reach the move uniform"


# ------------------------------------------------------------------------------------------------ noise plus moves
NOISE_CASES = {
    "c4-on-policy": ("connect_four", 4, 6, dict(n_playouts=12, backup="on-policy")),
    "c4-soft-Z": ("connect_four", 4, 6, dict(n_playouts=12, backup="soft-Z", keep_search_tree=False)),
    "c4-A0C": ("connect_four", 4, 6, dict(n_playouts=12, backup="A0C")),
    "c4-off-policy": ("connect_four", 4, 6, dict(n_playouts=12, backup="off-policy")),
    "bt66-A0C": (PC.BT66, 2, 3, dict(n_playouts=8, backup="A0C")),
    "bt54-off-policy": (PC.BT54, 1, 3, dict(n_playouts=10, backup="off-policy")),
    "c4-T0.7": ("connect_four", 4, 6, dict(n_playouts=12, backup="soft-Z", temperature=0.7)),
    "c4-T1.5": ("connect_four", 4, 6, dict(n_playouts=12, backup="on-policy", temperature=1.5)),
}


@functools.lru_cache(maxsize=None)
def _noise_run(name):
    game, n_slots, n_games, kw = NOISE_CASES[name]
    return _play(game, n_slots, n_games, SEED_HI, True, use_dirichlet=True, **kw)


@pytest.mark.parametrize("name", sorted(NOISE_CASES))
def test_games_equal_the_oracle_replayed_with_the_recorded_noise(name):
    game, n_slots, n_games, kw = NOISE_CASES[name]
    run = _noise_run(name)
    ex, etas = run["ex"], run["etas"]
    rows = []
    for i in range(n_games):   # every recorded ply has exactly one noise row, and no row belongs to a ply that was not played
        n = int(ex["game_len"][i])
        assert sorted(etas[i]) == list(range(n)), (name, i)
        for t in range(n):
            assert len(etas[i][t]) == 1, (name, i, t)
            nc = int(ex["n_children"][i, t])
            row = etas[i][t][0][:nc]
            assert np.isfinite(row).all() and (row > 0.0).all() and abs(row.sum() - 1.0) <= 1e-12, (name, i, t, row)
            if nc > 1:          # (a single legal move takes all the noise: such rows coincide by definition)
                rows.append(tuple(row))
    assert sorted(etas) == list(range(n_games))
    assert len(set(rows)) == len(rows), "two roots drew the same noise"
    _assert_run_equals(run, game, n_games, SEED_HI, dict(use_dirichlet=True, **kw), with_noise=True)


def test_the_exact_test_looks_at_what_it_claims():
    """Host arithmetic on the connect_four run above: each wrong keying of the replay must change at least one game."""
    name = "c4-on-policy"
    game, n_slots, n_games, kw = NOISE_CASES[name]
    kw = dict(use_dirichlet=True, **kw)
    run = _noise_run(name)
    own = [_rows_of(run, i) for i in range(n_games)]

    def changed(etas_of, purpose=1):
        return sum(_difference(run, i, _oracle(run, game, i, SEED_HI, kw, etas=etas_of(i), purpose=purpose)) is not None
                   for i in range(n_games))

    assert changed(lambda i: own[i]) == 0
    swapped = changed(lambda i: [own[i][1], own[i][0]] + own[i][2:])
    purpose3 = changed(lambda i: own[i], purpose=3)
    nxt = changed(lambda i: [(own[(i + 1) % n_games] + own[i][len(own[(i + 1) % n_games]):])[t] for t in range(len(own[i]))])
    print("sensitivity (games changed of %d): plies 0/1 swapped %d, us from purpose 3 %d, rows of game i+1 %d"
          % (n_games, swapped, purpose3, nxt))
    assert swapped >= 1 and purpose3 >= 1 and nxt >= 1, (swapped, purpose3, nxt)


@pytest.mark.parametrize("temperature", [0.7, 1.5])
def test_move_stream_at_a_generic_temperature(temperature):
    """np_pow's pow() branch (temperatures outside {1, 2, 0.5, -1}): pi and the targets do not pass through it; a move differs
    from the oracle's libm pow only if u lies within an ulp of a cdf edge."""
    kw = dict(n_playouts=12, use_dirichlet=False, temperature=temperature)
    run = _play("connect_four", 3, 7, SEED_LO, False, **kw)
    _assert_run_equals(run, "connect_four", 7, SEED_LO, kw, with_noise=False)


# ------------------------------------------------------------------------------------------------ law and keying
LAW_SEED = 0xD1A1C0DE + (3 << 32)


@functools.lru_cache(maxsize=None)
def _staged_rows(game, prefix=None, state=None, seed=LAW_SEED):
    """[N_LAW, max_children]: the noise N_LAW game ids staged for the same position (a prefix, or (bb0, bb1, ply) given to the
    device form), and the root priors the next tick made of it under uniform network priors."""
    E = _E()
    G = PC.N_LAW
    eng = E.SelfPlayEngine(game, G, n_playouts=2, rng="philox", seed=seed, max_games=G, manual_moves=True)
    if state is None:
        eng.set_start_positions([list(prefix)] * G)
    else:
        bb = torch.tensor([[state[0], state[1]]] * G, dtype=torch.int64, device=eng.device)
        eng.set_start_states_device(bb, torch.full((G,), state[2], dtype=torch.int32, device=eng.device))
    eng.reset(G)
    obs, pri, val = eng.alloc_io()
    eng.advance(pri, val, obs)                       # the root requests: every slot stages its row (phase 3)
    rows = np.stack([eng.read_root_noise(g) for g in range(G)])
    eng.advance(pri, val, obs)                       # ... and consumes it
    roots = eng.read_roots()
    with pytest.raises(E.EngineError):               # (the row is stale now: refused)
        eng.read_root_noise(0)
    assert eng.progress()["error_flags"] == 0
    A = eng.A
    eng.close()
    assert (roots["game_id"] == np.arange(G)).all()
    return rows, roots["child_p"], roots["n_children"], A


@pytest.mark.parametrize("label,game,prefix,n_legal", PC.LAW_POSITIONS, ids=[p[0] for p in PC.LAW_POSITIONS])
def test_noise_law_at_chosen_positions(label, game, prefix, n_legal):
    rows, child_p, n_children, A = _staged_rows(game, tuple(prefix))
    assert (n_children == n_legal).all()
    PC.check_dirichlet_law(rows, n_legal)
    if n_legal == 1:
        assert (rows[:, 0] == 1.0).all(), "a single legal move: eta must be exactly 1.0; off by %r in %d rows" % (
            np.abs(rows[:, 0] - 1.0).max(), int((rows[:, 0] != 1.0).sum()))
    assert len({tuple(r) for r in rows[:, :n_legal]}) == (PC.N_LAW if n_legal > 1 else 1)
    # the row read for slot g is the row slot g consumed: P = 0.75 * prior + 0.25 * eta (mcts.py:189), uniform float32 priors
    assert (child_p[:, :n_legal] == 0.75 * float(np.float32(1.0 / A)) + 0.25 * rows[:, :n_legal]).all()


@pytest.mark.parametrize("game,pa,na,pb,nb", PC.KEY_PAIRS, ids=["c4_ply18", "bt54_ply6"])
def test_gamma_of_child_k_depends_on_seed_game_ply_and_k_alone(game, pa, na, pb, nb):
    ra, rb = _staged_rows(game, tuple(pa))[0], _staged_rows(game, tuple(pb))[0]
    m = min(na, nb)
    qa, qb = ra[:, 1:m] / ra[:, :1], rb[:, 1:m] / rb[:, :1]    # the normaliser cancels: raw gamma k / raw gamma 0
    assert (np.abs(qa - qb) <= 1e-12 * np.abs(qb)).all(), np.abs(qa / qb - 1.0).max()
    assert (ra[:, 0] != rb[:, 0]).any()                        # (different normalisers: the rows themselves differ)


def test_the_same_position_at_another_ply_draws_unrelated_noise():
    """A breakthrough board under two ply numbers of the same side (the device form of the start table takes board and ply
    apart): rows of the same game id share nothing.  The sample correlation of 2048 independent pairs has standard error about
    0.022 (more for skewed data); the bar 0.2 is the one of check_dirichlet_law; a draw that ignored the ply would give 1."""
    bb0, bb1 = 0xFF, 0xFF << 12                                # the 5x4 initial position
    r0, r2 = _staged_rows(PC.BT54, state=(bb0, bb1, 0))[0], _staged_rows(PC.BT54, state=(bb0, bb1, 2))[0]
    rp = _staged_rows(PC.BT54, ())[0]
    assert (r0[:, :10] == rp[:, :10]).all()                      # the device form at ply 0 is the prefix form
    assert (r0[:, :10] != r2[:, :10]).any(1).all()
    q0, q2 = r0[:, 1:10] / r0[:, :1], r2[:, 1:10] / r2[:, :1]
    assert (q0 != q2).any(1).all()
    for k in range(10):                                        # (10 legal moves)
        assert abs(np.corrcoef(r0[:, k], r2[:, k])[0, 1]) < 0.2, k


def test_read_root_noise_refusals():
    E = _E()
    for kw in (dict(rng="injected"), dict(rng="philox", use_dirichlet=False)):
        eng = E.SelfPlayEngine("connect_four", 2, n_playouts=4, max_games=2, **kw)
        eng.reset(2)
        with pytest.raises(E.EngineError, match="root noise"):
            eng.read_root_noise(0)
        eng.close()
    eng = E.SelfPlayEngine("connect_four", 2, n_playouts=4, max_games=2)
    with pytest.raises(E.EngineError):                          # before reset
        eng.read_root_noise(0)
    eng.reset(2)
    for slot in (-1, 2):
        with pytest.raises(E.EngineError):
            eng.read_root_noise(slot)
    with pytest.raises(E.EngineError, match="phase 3"):         # nothing staged yet
        eng.read_root_noise(0)
    obs, pri, val = eng.alloc_io()
    eng.advance(pri, val, obs)
    assert eng.read_root_noise(1).shape == (7,)
    eng.close()
