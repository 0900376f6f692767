"""Helpers of tests/test_playout_cap_gpu.py: bit-for-bit comparison of engine exports, the reference-format games of a generation
with a history per game, and the check of a DeviceReplay against tests/replay_cases.FifoModel.  No test lives here."""
import numpy as np
import torch

import replay_cases as RC
from alphazero_openspiel_amd.engine import examples_from_export

RECORD_KEYS = ("states", "move", "n_children", "value")


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), "%s differs at %s: %r != %r (%d elements)" % (what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def same_game(got, j, want, k, p0, what):
    """Game j of export `got` equals game k of export `want`: length, result, and every record row of the game's plies
    [p0, p0 + len) with the children [0, n_children)."""
    n = int(want["game_len"][k])
    assert n > 0 and int(got["game_len"][j]) == n, what
    assert got["game_ret0"][j] == want["game_ret0"][k], what
    rows = slice(p0, p0 + n)
    for key in RECORD_KEYS:
        same(got[key][j, rows], want[key][k, rows], "%s: %s" % (what, key))
    live = np.arange(got["child_action"].shape[2])[None, :] < want["n_children"][k, rows][:, None]
    for key in ("child_action", "child_visits"):
        same(got[key][j, rows][live], want[key][k, rows][live], "%s: %s" % (what, key))


def reference_games(game, ex, histories):
    """examples_from_export with a history per game, every example carrying its bitboards and absolute ply (RC.Rec)."""
    out = []
    for g, plies in enumerate(examples_from_export(game, ex, histories)):
        p0, recs = len(histories[g]), []
        for i, item in enumerate(plies):
            r = RC.Rec(item)
            r.bb, r.ply = ex["states"][g, p0 + i].copy(), p0 + i
            recs.append(r)
        out.append(recs)
    return out


def expect(model):
    """One remove_duplicates pass of the FifoModel (it writes the averages back: once per append) -> what a store fed like the
    model must hold after ITS pass."""
    flat, unique, uidx = model.dedupe()
    return {"n_games": model.n_games, "games_dropped": model.games_dropped, "uidx": uidx,
            "flat_pi": np.array([r[2] for r in flat]), "flat_z": np.array([r[3] for r in flat]),
            "pi": np.array([r[2] for r in unique]), "z": np.array([r[3] for r in unique]),
            "bb": np.array([r.bb for r in unique], dtype=np.uint64), "ply": [r.ply for r in unique],
            "board": np.stack([r[1] for r in unique])}


def check_store(rep, e):
    """dedupe() -> count and stats, read_unique, read_example of the whole buffer, then sample() of every unique example."""
    n = len(e["uidx"])
    assert rep.dedupe() == n
    st = rep.stats()
    assert (st["n_games"], st["n_examples"], st["n_unique"], st["games_dropped"], st["fault_flags"]) == \
        (e["n_games"], len(e["flat_z"]), n, e["games_dropped"], 0)
    u = rep.read_unique()
    assert u["buffer_index"].tolist() == e["uidx"]
    same(u["pi"], e["pi"], "unique pi")
    same(u["z"], e["z"], "unique z")
    same(u["bitboards"], e["bb"], "unique bitboards")
    assert u["ply"].tolist() == e["ply"]
    got = [rep.read_example(i) for i in range(len(e["flat_z"]))]
    same(np.array([g[0] for g in got]), e["flat_pi"], "stored pi")
    same(np.array([g[1] for g in got]), e["flat_z"], "stored z")
    perm = np.random.RandomState(n).permutation(n)
    x, pi, z = rep.sample(n, indices=perm)
    same(x.cpu().numpy(), e["board"][perm].astype(np.float32), "sampled x")
    same(pi.cpu().numpy(), e["pi"][perm].astype(np.float32), "sampled pi")
    same(z.cpu().numpy(), e["z"][perm].astype(np.float32), "sampled z")
    assert x.dtype == pi.dtype == z.dtype == torch.float32
    assert rep.stats()["fault_flags"] == 0
