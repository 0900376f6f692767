"""Synthetic generations for the replay-store tests: games played with the Python rules and written in the engine's export
layout, the packed device export built from them, and a Python model of the store's FIFO.  No engine and no net is needed.

The reference for what the store must hold is `engine.examples_from_export` + `oracle/pyreplay.py`, both pinned to the
reference Trainer by tests/golden/replay.json."""
import numpy as np

from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.engine import device_export_layout, examples_from_export
from oracle import pyreplay

# Action prefixes from the initial position that end in a position with exactly ONE legal move (found by random play with the
# Python rules; tests/test_replay_cases.py replays them).  Used as an opening, every game that follows one records such a ply.
ONE_MOVE_PREFIX = {
    "connect_four": [5, 2, 6, 4, 2, 6, 0, 1, 2, 0, 1, 1, 0, 5, 5, 6, 5, 6, 6, 5, 5, 4, 6, 1, 4, 2, 2, 2, 1, 4, 0, 1, 4, 0, 4, 0],
    "breakthrough(rows=5,columns=4)": [76, 179, 52, 155, 60, 163, 84, 187, 12, 115, 28, 131, 4, 107],
    "breakthrough(rows=6,columns=6)": [100, 346, 88, 354, 185, 296, 265, 415, 124, 330, 50, 426, 120, 251, 76, 227, 112, 283, 14,
                                       203, 26, 167, 37, 187, 170, 311, 86, 247, 2, 163, 206, 347],
    "breakthrough(rows=8,columns=8)": [136, 630, 144, 606, 230, 658, 324, 503, 98, 594, 2, 738, 60, 666, 148, 642, 242, 754, 40,
                                       536, 110, 572, 340, 559, 256, 455, 196, 415, 158, 367, 144, 263, 85, 694, 14, 488, 170,
                                       666, 50, 608, 108, 307, 232, 730, 336, 515, 208, 427, 266, 475, 146, 622, 240, 439, 24,
                                       203, 122, 331, 72, 634, 182, 371, 98, 702, 194, 718, 158, 538, 256, 455],
}

BIG = 2 ** 31  # the largest visit count the edge mode writes: three of them in one ply sum past 2^32


def _edge_visits(rng, n):
    """Visit counts of one ply with the edges a converter can get wrong: children with 0 visits (never all of them), and
    counts up to 2^31 whose total exceeds 2^32 (a 32-bit total wraps; a float32 total rounds)."""
    v = rng.randint(1, 50, n).astype(np.int64)
    kind = rng.randint(4)
    if kind == 1 and n > 1:  # some children were never visited
        v[rng.rand(n) < 0.5] = 0
        if not v.any():
            v[rng.randint(n)] = 1 + rng.randint(50)
    elif kind == 2:  # huge counts next to small ones
        big = rng.rand(n) < 0.6
        big[rng.permutation(n)[:3]] = True  # at least three (all, when the ply has fewer children)
        v[big] = BIG - rng.randint(0, 2 ** 20, int(big.sum()))
        v[rng.randint(n)] = BIG
    return v.astype(np.uint32)


def fake_export(game, n_games=3, seed=0, openings=None, start_history=(), visits="plain"):
    """n_games random games in the layout of engine.export().

    openings: a pool of legal action prefixes (after start_history); each game follows one of them for its first plies and then
        plays randomly, so histories repeat at plies 1..d and not only at the start.
    start_history: every game starts after these actions: records sit in rows p0 .. p0+len-1 (p0 = len(start_history)),
        "start_ply" = p0, and `value` carries the sign of the player to move at the ABSOLUTE ply.
    visits: "plain" (1..49 per child) or "edges" (see _edge_visits)."""
    rng = np.random.RandomState(seed)
    mp, mc = game.max_game_length(), game.max_children()
    p0 = len(start_history)
    ex = {"game_len": np.zeros(n_games, np.int32), "game_ret0": np.zeros(n_games, np.float32),
          "states": np.zeros((n_games, mp, 2), np.uint64), "move": np.zeros((n_games, mp), np.uint16),
          "n_children": np.zeros((n_games, mp), np.uint8), "child_action": np.zeros((n_games, mp, mc), np.uint16),
          "child_visits": np.zeros((n_games, mp, mc), np.uint32), "value": np.zeros((n_games, mp)), "start_ply": p0}
    for g in range(n_games):
        s = games.state_from_history(game, start_history)
        forced = list(openings[rng.randint(len(openings))]) if openings else []
        i = p0
        while not s.is_terminal():
            la = s.legal_actions()
            ex["states"][g, i] = s.bb
            ex["n_children"][g, i] = len(la)
            ex["child_action"][g, i, :len(la)] = la
            ex["child_visits"][g, i, :len(la)] = rng.randint(1, 50, len(la)) if visits == "plain" else _edge_visits(rng, len(la))
            a = la[rng.randint(len(la))]
            if i - p0 < len(forced):
                a = forced[i - p0]
            ex["move"][g, i] = a
            s.apply_action(a)
            i += 1
        ex["game_len"][g], ex["game_ret0"][g] = i - p0, s.returns()[0]
        z = s.returns()[0] * (-1.0 if p0 & 1 else 1.0)
        for j in range(p0, i):
            ex["value"][g, j] = z
            z = -z
    return ex


def random_openings(game, n, depth, seed, start_history=()):
    """n legal action prefixes of `depth` plies after start_history, drawn so that they share their first moves."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        s = games.state_from_history(game, start_history)
        h = []
        for d in range(depth):
            la = s.legal_actions()
            a = la[rng.randint(min(2, len(la)))]  # two choices per ply: prefixes collide often
            h.append(a)
            s.apply_action(a)
            assert not s.is_terminal()
        out.append(h)
    return out


def pack_device_export(ex):
    """The bytes of az_engine_export_device for these games (uint8 array): the inverse of engine.unpack_device_export."""
    n, mp = ex["move"].shape
    layout, total = device_export_layout(n, mp, ex["child_action"].shape[2])
    buf = np.zeros(total, dtype=np.uint8)
    for name, dt, shape, off in layout:
        a = np.ascontiguousarray(ex[name], dtype=dt)
        assert a.shape == shape, name
        raw = a.reshape(-1).view(np.uint8)
        buf[off:off + raw.size] = raw
    return buf


class Rec(list):
    """One example in the reference's format `[key, board, pi, z]`, remembering the record it was made from."""
    bb = ply = None


def reference_games(game, ex, start_history=()):
    """examples_from_export (the host reference), every example carrying its bitboards and absolute ply."""
    p0 = int(ex["start_ply"])
    assert p0 == len(start_history)
    out = []
    for g, plies in enumerate(examples_from_export(game, ex, start_history)):
        recs = []
        for i, item in enumerate(plies):
            r = Rec(item)
            r.bb, r.ply = ex["states"][g, p0 + i].copy(), p0 + i
            recs.append(r)
        out.append(recs)
    return out


class FifoModel:
    """The store's FIFO of games with both limits, as include/az_replay.h and append_common state it: a generation with
    more examples than max_examples is refused; the oldest games leave until the generation fits the example ring; the
    generation is appended; then the oldest games leave until at most `capacity` games remain (train.py:233-236)."""

    def __init__(self, max_games, max_examples):
        self.max_games, self.max_examples, self.capacity = max_games, max_examples, max_games
        self.buffer, self.games_dropped, self.ring_evictions, self.cap_evictions, self.appended = [], 0, 0, 0, 0
        self.events = []  # "ring" / "cap" per evicted game, in order

    n_games = property(lambda self: len(self.buffer))
    n_examples = property(lambda self: sum(len(g) for g in self.buffer))

    def set_capacity(self, n_games):
        assert 1 <= n_games <= self.max_games
        self.capacity = n_games  # takes effect at the next append

    def append(self, generation):
        """-> (buffer, n_games, n_examples, games_dropped); ValueError when the store refuses the generation."""
        generation = [g for g in generation if len(g)]
        add = sum(len(g) for g in generation)
        if add > self.max_examples:
            raise ValueError("one generation holds more examples than max_examples")
        while self.n_examples + add > self.max_examples and self.buffer:
            del self.buffer[0]
            self.games_dropped += 1
            self.ring_evictions += 1
            self.events.append("ring")
        self.buffer.extend(generation)
        self.appended += add
        while len(self.buffer) > self.capacity:
            del self.buffer[0]
            self.games_dropped += 1
            self.cap_evictions += 1
            self.events.append("cap")
        return self.buffer, self.n_games, self.n_examples, self.games_dropped

    def flat(self):
        return [r for g in self.buffer for r in g]

    def dedupe(self):
        """Trainer.remove_duplicates over the flattened buffer (mutates the first occurrences, as the reference does)
        -> (flat, unique records, their indices in flat)."""
        flat = self.flat()
        unique = pyreplay.remove_duplicates(flat)
        index = {id(r): i for i, r in enumerate(flat)}
        return flat, unique, [index[id(r)] for r in unique]
