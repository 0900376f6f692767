"""Shared by tests/test_eval_mirror_host.py and tests/test_eval_mirror_gpu.py: the pure-Python model of the engine's coin
(include/az_engine.h, az_engine_set_eval_mirror) and the reference construction - a PLAIN engine (no setting) under a wrapping
evaluator that mirrors the chosen rows itself.  No test lives here.

The coin: every network request is mirrored iff u < p_mirror, u = the first philox_u01 of the Philox stream
  leaf request (phase 4):  (seed, game id, absolute ply of the slot's root, purpose 4, index = sims_done of the waiting slot)
  root request (phase 3):  (seed, game id, root ply, purpose 5, index 0)
restated with the Philox model of tests/philox_cases.py.

The wrapper: for each row whose coin is set it evaluates obs.flip(-1) and writes the priors permuted by
mirror_cases.action_mirror_table(game), so that the plain engine, which reads priors[row][a], finds net(flip(obs))[mirror(a)]
there - what an engine with the setting reads from the bare net's answer."""
import numpy as np
import torch

from mirror_cases import action_mirror_table
from philox_cases import cap_uniform

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
S, G, N = 24, 4, 8
SEED = 900           # both coin values within the first six requests of every game id below N (test_eval_mirror_host asserts it)
PH_WAIT_ROOT, PH_WAIT_LEAF = 3, 4
PURPOSE_LEAF, PURPOSE_ROOT = 4, 5


def coin(seed, game_id, root_ply, phase, sims_done, p_mirror):
    """The bit of the request a slot in `phase` (3 or 4) has outstanding; a slot without a request has none (False)."""
    if phase == PH_WAIT_LEAF:
        return cap_uniform(seed, game_id, root_ply, purpose=PURPOSE_LEAF, idx=sims_done) < p_mirror
    if phase == PH_WAIT_ROOT:
        return cap_uniform(seed, game_id, root_ply, purpose=PURPOSE_ROOT, idx=0) < p_mirror
    return False


def first_requests(seed, game_id, p_mirror, n=6):
    """The coins of the first n requests of a game that starts at ply 0 with root noise on: the root expansion, then the leaves of
    playouts 0 .. n - 2 (none of them can end on a terminal state that early)."""
    return [coin(seed, game_id, 0, PH_WAIT_ROOT, 0, p_mirror)] + \
           [coin(seed, game_id, 0, PH_WAIT_LEAF, i, p_mirror) for i in range(n - 1)]


def slot_coin(seed, info, p_mirror):
    """coin() of an engine.read_slot() dict."""
    return coin(seed, info["game_id"], info["ply"], info["phase"], info["sims_done"], p_mirror)


class MirrorWrapper:
    """evaluator(obs, priors_out, values_out) of engine.py around `inner`: rows whose entry of `rows` (a bool device tensor of
    at least obs.shape[0] entries; None = every row) is set are evaluated mirrored and mapped back; the value is left alone."""

    def __init__(self, inner, game, device="cuda:0"):
        self.inner = inner
        self.perm = torch.as_tensor(action_mirror_table(game), dtype=torch.int64, device=device)
        self.rows = None

    def __call__(self, obs, priors_out, values_out):
        n = obs.shape[0]
        rows = torch.ones(n, dtype=torch.bool, device=obs.device) if self.rows is None else self.rows[:n]
        x = torch.where(rows[:, None, None, None], obs.flip(-1), obs).contiguous()
        self.inner(x, priors_out, values_out)
        priors_out.copy_(torch.where(rows[:, None], priors_out[:, self.perm], priors_out))


def play_model_driven(eng, wrapper, n_games, seed, p_mirror, max_ticks=200000):
    """A closed generation of the plain engine `eng` in eager ticks; after each tick the coin model, applied to read_slot(g),
    says which rows the wrapper mirrors.  -> the export."""
    eng.reset(n_games, seed)
    obs, pri, val = eng.alloc_io()
    for tick in range(max_ticks):
        eng.advance(pri, val, obs)
        bits = [slot_coin(seed, eng.read_slot(g), p_mirror) for g in range(eng.G)]
        wrapper.rows = torch.as_tensor(bits, dtype=torch.bool, device=obs.device)
        wrapper(obs, pri, val)
        if tick % 8 == 7 and eng.games_done() >= n_games:
            return eng.export()
    raise AssertionError("the generation did not finish: %r" % (eng.progress(),))


def valid(ex):
    p0 = np.asarray(ex["start_ply"]).reshape(-1, 1)
    ply = np.arange(ex["move"].shape[1])[None, :]
    return (ply >= p0) & (ply < p0 + ex["game_len"].astype(np.int64)[:, None])


def exports_differ(a, b):
    """Do two exports of the same generation differ anywhere on their recorded moves or child visits?"""
    if a["game_len"].tolist() != b["game_len"].tolist():
        return True
    v = valid(a)
    if (a["move"][v] != b["move"][v]).any():
        return True
    live = v[:, :, None] & (np.arange(a["child_visits"].shape[2])[None, None, :] < a["n_children"][:, :, None])
    return bool((a["child_visits"][live] != b["child_visits"][live]).any())
