"""Shared by test_merge_host.py and test_merge_gpu.py: a plain-Python model of az_replay_dedupe_positions (include/az_replay.h:
the group, order and average rules) and the generations the tests feed it and the store with.

The model restates the rule, not the kernels: the bitboard mirror is written from the layout comment of csrc/az_games.h (and
checked against the Python rules in test_merge_host.py), the action mirror is mirror_cases.mirror_action_py, and the sums run
over Python floats (IEEE float64, one rounding per operation) in buffer order."""
import numpy as np

import replay_cases as RC
from mirror_cases import action_mirror_table

C4, B54, B66 = "connect_four", "breakthrough(rows=5,columns=4)", "breakthrough(rows=6,columns=6)"
BOARDS = [C4, B54, B66]

# Openings that make every kind of merge occur (breakthrough: found with the Python rules, replayed by test_merge_host.py):
#   [0] / [1]  one side's two independent moves in either order: a transposition (equal position, different histories)
#   [2] / [3]  a line and its mirror image
#   [4]        connect_four: the centre column, a position that is its own mirror image (breakthrough: the initial one is)
#   the last   [0] once more: equal histories
# [2] is a prefix of [0] in connect_four, so the position after two plies collects members of both orientations.
OPENINGS = {
    C4: [[0, 1, 2], [2, 1, 0], [0, 1], [6, 5], [3], [0, 1, 2]],
    B54: [[50, 166, 62], [62, 166, 50], [52, 188], [84, 152], [50, 166, 62]],
    B66: [[74, 296, 86], [86, 296, 74], [76, 356], [132, 296], [74, 296, 86]],
}

_ARRAYS = ("game_len", "game_ret0", "states", "move", "n_children", "child_action", "child_visits", "value")


def mirror_bits_py(game, b):
    """Column c <-> cols-1-c of one bitboard.  connect_four: bit = col*7 + row, the 7-bit column groups swap; breakthrough:
    bit = row*C + col, every row of C bits is reversed.  Bits that are no cell stay where they are."""
    b = int(b)
    if game.game_id == 0:
        out = b >> 49 << 49
        for col in range(7):
            out |= ((b >> (7 * col)) & 0x7F) << (7 * (6 - col))
        return out
    cells = game.rows * game.cols
    out = b >> cells << cells
    for cell in range(cells):
        if b >> cell & 1:
            row, col = divmod(cell, game.cols)
            out |= 1 << (row * game.cols + game.cols - 1 - col)
    return out


def canonical(game, bb, ply, mirror):
    """-> (c0, c1, parity, flip): the sort key of an example and whether it is stored as the mirror image of that key."""
    s = (int(bb[0]), int(bb[1]))
    flip = 0
    if mirror:
        m = (mirror_bits_py(game, s[0]), mirror_bits_py(game, s[1]))
        if m < s:                       # unsigned pairs, bb0 the major word; a self-symmetric position has m == s
            s, flip = m, 1
    return s[0], s[1], int(ply) & 1, flip


def merged(game, flat, mirror):
    """One az_replay_dedupe_positions pass over the flattened buffer `flat` (replay_cases.Rec: [key, board, pi, z] with .bb and
    .ply).  The first occurrence of every group is MUTATED (the write-back), every other record is left alone.
    -> (unique, flat): unique = [{"index", "count", "pi", "z"}] in first-occurrence order, flat = the buffer after write-back."""
    table = action_mirror_table(game)
    groups = {}
    for i, r in enumerate(flat):
        c0, c1, par, flip = canonical(game, r.bb, r.ply, mirror)
        g = groups.get((c0, c1, par))
        if g is None:
            groups[(c0, c1, par)] = {"index": i, "flip": flip, "count": 1, "pi": [float(x) for x in r[2]], "z": float(r[3])}
            continue
        pi = [float(x) for x in r[2]]
        if flip != g["flip"]:
            pi = [pi[table[a]] for a in range(len(pi))]
        g["pi"] = [x + y for x, y in zip(g["pi"], pi)]
        g["z"] = g["z"] + float(r[3])
        g["count"] += 1
    unique = list(groups.values())      # dict order = first-occurrence order
    for g in unique:
        if g["count"] > 1:
            g["pi"] = [x / float(g["count"]) for x in g["pi"]]
            g["z"] = g["z"] / float(g["count"])
            flat[g["index"]][2] = list(g["pi"])
            flat[g["index"]][3] = g["z"]
    return unique, flat


def by_history(flat):
    """One az_replay_dedupe pass of the model (oracle.pyreplay, which mutates the first occurrences) in the form merged() gives."""
    from oracle import pyreplay
    counts = {}
    for r in flat:
        counts[r[0]] = counts.get(r[0], 0) + 1
    index = {id(r): i for i, r in enumerate(flat)}
    return [{"index": index[id(r)], "count": counts[r[0]], "pi": list(r[2]), "z": r[3]} for r in pyreplay.remove_duplicates(flat)], flat


def mirrored_flat(game, flat):
    """Every record as its mirror image: the mirrored position, pi_out[mirror(a)] = pi[a], the same z.  New records."""
    table = action_mirror_table(game)
    out = []
    for r in flat:
        pi = [0.0] * len(r[2])
        for a, x in enumerate(r[2]):
            pi[table[a]] = x
        m = RC.Rec([r[0], r[1], pi, r[3]])
        m.bb, m.ply = np.array([mirror_bits_py(game, r.bb[0]), mirror_bits_py(game, r.bb[1])], dtype=np.uint64), r.ply
        out.append(m)
    return out


def copy_flat(flat):
    out = []
    for r in flat:
        c = RC.Rec([r[0], r[1], list(r[2]), r[3]])
        c.bb, c.ply = r.bb.copy(), r.ply
        out.append(c)
    return out


def generation(game, rounds=3, seed=0, max_len=None, openings=None):
    """`rounds` games per opening of OPENINGS, interleaved (so the members of a group alternate between the openings, and with
    them between the two orientations), each continued by random play; z of every example drawn from (-1, 1), so that the order
    of the additions shows in the sums.  max_len cuts every game to its first plies.  -> (export, reference games)."""
    pool = (OPENINGS[game.name] if openings is None else openings) * rounds
    parts = [RC.fake_export(game, n_games=1, seed=seed + 97 * k, openings=[op]) for k, op in enumerate(pool)]
    ex = {k: np.concatenate([p[k] for p in parts]) for k in _ARRAYS}
    ex["start_ply"] = 0
    ex["value"] = np.random.RandomState(seed + 1).uniform(-1, 1, ex["value"].shape)
    if max_len is not None:
        ex["game_len"] = np.minimum(ex["game_len"], max_len).astype(np.int32)
    return ex, RC.reference_games(game, ex)
