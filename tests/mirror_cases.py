"""Shared by the mirror tests: the boards, a pure-Python restatement of the action mirror and of the store's index draw, and
small stores filled through az_replay_append_host from games played with the Python rules (replay_cases.fake_export).  No
engine and no net is needed."""
import ctypes as C

import numpy as np
import torch

import replay_cases as RC
from alphazero_openspiel_amd import games

# 6 rows x 5 columns is not square: mixing rows up with columns hides on the square boards
BOARDS = ["connect_four", "breakthrough(rows=6,columns=6)", "breakthrough(rows=8,columns=8)", "breakthrough(rows=6,columns=5)"]

E_INVALID, E_STATE, E_DEVICE = -1, -3, -4  # include/az_engine.h


def mirror_action_py(game, a):
    """The action mirror restated from the codec comment of az_games.h (action = ((cell*6) + dir)*2 + capture, cell = row*C +
    col, dir 0..2 black / 3..5 white with dc = -1, 0, +1), with divisions, independently of the C helper."""
    if game.game_id == 0:
        return 6 - a
    capture, dir_, cell = a % 2, (a // 2) % 6, (a // 2) // 6
    row, col = divmod(cell, game.cols)
    side, dc = dir_ // 3, dir_ % 3 - 1
    return (((row * game.cols + game.cols - 1 - col) * 6) + side * 3 + (-dc + 1)) * 2 + capture


def action_mirror_table(game):
    return [mirror_action_py(game, a) for a in range(game.num_distinct_actions())]


_M64 = (1 << 64) - 1


def _mix64(h, v):
    z = (h + 0x9E3779B97F4A7C15 * (v + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def drawn_indices(seed, call, batch, n_unique):
    """The rows az_replay_sample picks for indices == NULL (include/az_replay.h: one splitmix64 draw per row over (seed, call
    counter, row), scaled by the high half of a 64x64-bit product).  The tests check it against the entry before they use it."""
    return np.array([(_mix64(_mix64(seed, call), b) * n_unique) >> 64 for b in range(batch)], dtype=np.int64)


def small_export(name, seed=0):
    """Three random games cut to their first 14 plies: about 40 unique positions (the shared start is stored once), every one
    with an uneven pi and a z of its own."""
    game = games.load_game(name)
    ex = RC.fake_export(game, n_games=3, seed=seed)
    ex["game_len"] = np.minimum(ex["game_len"], 14).astype(np.int32)
    ex["value"] = np.random.RandomState(seed + 1).uniform(-1, 1, ex["value"].shape)
    return game, ex


def make_store(name, seed=0, dedupe=True):
    """A fresh store (call counter 0) holding small_export(name, seed) -> (store, n_unique)."""
    from alphazero_openspiel_amd import replay
    _, ex = small_export(name, seed)
    rep = replay.DeviceReplay(name, max_games=8, device=0)
    rep.append_export(ex)
    return rep, (rep.dedupe() if dedupe else 0)


def outputs(rep, batch):
    dev = rep.device
    return (torch.full((batch,) + rep.obs_shape, -7.0, dtype=torch.float32, device=dev),
            torch.full((batch, rep.A), -7.0, dtype=torch.float32, device=dev), torch.full((batch,), -7.0, dtype=torch.float32, device=dev))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call_plain(rep, batch, indices=None, seed=0):
    """az_replay_sample through the C ABI (indices: device int64 tensor or None) -> (x, pi, z)."""
    x, pi, z = outputs(rep, batch)
    rc = rep.lib.az_replay_sample(rep._h, _ptr(indices), batch, seed, _ptr(x), _ptr(pi), _ptr(z), rep._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return x, pi, z


def call_sym(rep, batch, indices=None, flips=None, seed=0):
    """az_replay_sample_sym through the C ABI (indices: device int64, flips: device uint8, or None) -> (x, pi, z)."""
    x, pi, z = outputs(rep, batch)
    rc = rep.lib.az_replay_sample_sym(rep._h, _ptr(indices), _ptr(flips), batch, seed, _ptr(x), _ptr(pi), _ptr(z), rep._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return x, pi, z


def mirrored(game, plain):
    """What a mirrored row must hold, from the plain rows: x with its columns reversed, pi_out[mirror(a)] = pi[a], z."""
    x, pi, z = plain
    m = torch.as_tensor(action_mirror_table(game), device=pi.device)
    pim = torch.empty_like(pi)
    pim[:, m] = pi
    return torch.flip(x, dims=[3]), pim, z


def bits(t):
    """float32 tensor -> its bit patterns (so that comparisons are on bytes: NaN equals NaN, -0 differs from 0)."""
    return t.contiguous().view(torch.int32)


def rows_equal(a, b):
    """[batch] bool: row b of the three tensors of `a` holds the same bytes as row b of `b`."""
    ok = torch.ones(a[0].shape[0], dtype=torch.bool, device=a[0].device)
    for s, t in zip(a, b):
        ok &= (bits(s) == bits(t)).reshape(s.shape[0], -1).all(dim=1)
    return ok


def recover_flips(game, plain, got):
    """Which rows of `got` are the mirror image of the plain rows -> bool [batch]; every row must be one of the two, and the
    stores' examples are all uneven, so none is both."""
    as_plain, as_mirror = rows_equal(got, plain), rows_equal(got, mirrored(game, plain))
    assert bool((as_plain ^ as_mirror).all()), "a row is neither the stored example nor its mirror image (or both)"
    return as_mirror.cpu().numpy()
