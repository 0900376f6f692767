"""Every append route of the device replay store (csrc/az_replay.hip) must store the same thing for the same games: the host
view (az_replay_append_host) and the three device entries az_replay_append_device / _starts / _kept, which share one body
(append_packed) and one record layout (csrc/az_records.h).  No search and no net: the games are tests/replay_cases.py's.

The stores are compared with each other, bit for bit; what a store must hold against the host reference is
tests/test_replay_store_gpu.py's subject."""
import numpy as np
import pytest
import torch

import replay_cases as RC
from alphazero_openspiel_amd import games

pytestmark = pytest.mark.gpu

C4, B54 = "connect_four", "breakthrough(rows=5,columns=4)"
AZ_E_INVALID = -1
N = 6


def _replay(name):
    from alphazero_openspiel_amd import replay
    return replay.DeviceReplay(name, device=0, max_games=2 * N)


def _snapshot(rep):
    """Everything the read-backs show of a store, as plain values: stats, read_unique, read_example over every index."""
    st = rep.stats()
    uniq = {k: (str(v.dtype), v.shape, v.tobytes()) for k, v in rep.read_unique().items()}
    examples = [(pi.tobytes(), z) for pi, z in (rep.read_example(i) for i in range(st["n_examples"]))]
    return st, uniq, examples


def _games(name, prefix_plies):
    """(game, export of N games of which game 2 has no recorded ply, start ply, packed device buffer, mask of the recorded plies)"""
    game = games.load_game(name)
    history = RC.random_openings(game, 1, prefix_plies, 5)[0] if prefix_plies else []
    ex = RC.fake_export(game, n_games=N, seed=7, openings=RC.random_openings(game, 3, 2, 9, history), start_history=history)
    ex["game_len"][2] = 0
    p0 = len(history)
    mask = np.zeros((N, game.max_game_length()), np.uint8)
    for g in range(N):
        mask[g, p0:p0 + int(ex["game_len"][g])] = 1
    return game, ex, p0, torch.from_numpy(RC.pack_device_export(ex)).cuda(), torch.from_numpy(mask).cuda()


@pytest.mark.parametrize("prefix_plies", [0, 3])
@pytest.mark.parametrize("name", [C4, B54])
def test_all_routes_store_the_same(name, prefix_plies):
    game, ex, p0, buf, mask = _games(name, prefix_plies)
    assert ex["start_ply"] == p0 == prefix_plies and (ex["game_len"] > 0).sum() == N - 1
    plies = torch.full((N,), p0, dtype=torch.int32, device="cuda")
    routes = {
        "host view": lambda rep: rep.append_export(ex),
        "device, one ply": lambda rep: rep.append_device(buf, N, start_ply=p0),
        "device, ply per game": lambda rep: rep.append_device(buf, N, start_ply=plies),
        "kept, one ply": lambda rep: rep.append_device(buf, N, start_ply=p0, keep=mask),
        "kept, ply per game": lambda rep: rep.append_device(buf, N, start_ply=plies, keep=mask),
    }
    shots = {}
    for what, append in routes.items():
        rep = _replay(name)
        append(rep)
        n_unique = rep.dedupe()
        shots[what] = _snapshot(rep)
        rep.close()
        st = shots[what][0]
        assert (st["n_games"], st["n_examples"], st["n_unique"], st["fault_flags"]) == \
            (N - 1, int(ex["game_len"].sum()), n_unique, 0), what
        assert 0 < n_unique < st["n_examples"], what                 # the shared openings did merge
    for what, shot in shots.items():
        assert shot == shots["host view"], what
    # GIVEN history keys (one pair for all: the games share their start): only the two entries that take a ply per game have the
    # form, and a host view has none - they are compared with each other, and differ from the above in their keys alone
    keys = torch.tensor([[0x243F6A8885A308D3, -0x5A5A5A5A12345678]] * N, dtype=torch.int64, device="cuda")
    keyed = []
    for keep in (None, mask):
        rep = _replay(name)
        rep.append_device(buf, N, start_ply=plies, keys=keys, keep=keep)
        rep.dedupe()
        keyed.append(_snapshot(rep))
        rep.close()
    assert keyed[0] == keyed[1]
    plain = shots["host view"]
    assert keyed[0][0] == plain[0] and keyed[0][2] == plain[2]
    assert {k: v for k, v in keyed[0][1].items() if k != "key"} == {k: v for k, v in plain[1].items() if k != "key"}
    assert keyed[0][1]["key"] != plain[1]["key"]


def test_bad_lengths_and_start_plies_are_refused_by_every_device_entry():
    """None of these inputs reaches a kernel: the host loop of append_packed (or its argument check) refuses them.  The error
    text names the entry that was called: DeviceReplay.append_device picks the narrowest one for its arguments."""
    game, ex, p0, buf, mask = _games(C4, 0)
    mp = game.max_game_length()
    long_game = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ex.items()}
    long_game["game_len"][4] = mp + 1
    long_buf = torch.from_numpy(RC.pack_device_export(long_game)).cuda()
    zeros = torch.zeros((N,), dtype=torch.int32, device="cuda")
    no_keep = torch.zeros_like(mask)

    def ply_tensor(value):                                           # game 3 alone starts at `value`
        t = zeros.clone()
        t[3] = value
        return t

    entries = {
        "az_replay_append_device": [lambda rep, b, ply: rep.append_device(b, N, start_ply=ply)],
        "az_replay_append_device_starts": [lambda rep, b, ply: rep.append_device(b, N, start_ply=ply_tensor(ply))],
        "az_replay_append_device_kept": [lambda rep, b, ply: rep.append_device(b, N, start_ply=ply, keep=no_keep),
                                         lambda rep, b, ply: rep.append_device(b, N, start_ply=ply_tensor(ply), keep=no_keep)],
    }
    for entry, forms in entries.items():
        rep = _replay(C4)
        rep.append_device(buf, N, start_ply=0)
        rep.dedupe()
        held = _snapshot(rep)
        assert held[0]["n_examples"] > 0
        for form in forms:
            for b, ply, text in ((long_buf, 0, r"game_len\[4\] = %d is outside" % (mp + 1)), (buf, -1, "outside"),
                                 (buf, mp + 1, "outside")):
                with pytest.raises(RuntimeError, match=r"\(%d\): %s: .*%s" % (AZ_E_INVALID, entry, text)):
                    form(rep, b, ply)
                assert _snapshot(rep) == held, (entry, ply)
        rep.append_device(buf, N, start_ply=0)                       # and the store goes on working
        assert rep.stats()["n_examples"] == 2 * held[0]["n_examples"]
        rep.close()
