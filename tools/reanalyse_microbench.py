#!/usr/bin/env python3
"""Times one Reanalyse pass over stored positions (replay.Reanalyser: gather -> load -> search -> refresh, all on the device)
and, in the same process on the same engine and evaluator, the host route to the same searches (analysis.Analyzer.load of the
positions' action histories -> search -> read-back of all roots: what tools/analysis_microbench.py times), on one GPU.
    python tools/reanalyse_microbench.py [--positions 4096] [--playouts 400] [--blocks 10] [--filters 50] [--repeat 3]
                                         [--out profiles/<name>.json]
Positions: distinct connect_four positions from uniformly random legal moves (fixed seed, stopping before a move that would
end the game), stored as one-ply records so that the de-duplicated list holds exactly them.  Each route runs once untimed, then
--repeat times between device synchronisations; the medians are reported.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_openspiel_amd import games, replay  # noqa: E402
from alphazero_openspiel_amd.network import Net  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=4096)
ap.add_argument("--playouts", type=int, default=400)
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--filters", type=int, default=50)
ap.add_argument("--slots", type=int, default=0, help="engine slots (default: min(positions, 4096))")
ap.add_argument("--precision", default="f32x", choices=["f16", "f32x"])
ap.add_argument("--min-ply", type=int, default=6)
ap.add_argument("--max-ply", type=int, default=30)
ap.add_argument("--value-target", default="soft-Z", choices=["soft-Z", "A0C", "off-policy", "none"])
ap.add_argument("--check-every", type=int, default=16)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
a = ap.parse_args()

game = games.load_game("connect_four")
rng = np.random.RandomState(a.seed)
seen, by_ply = set(), {}
while len(seen) < a.positions:
    target, st = int(rng.randint(a.min_ply, a.max_ply + 1)), game.new_initial_state()
    while len(st.history()) < target:
        legal = st.legal_actions()
        nxt = st.clone()
        nxt.apply_action(int(legal[rng.randint(len(legal))]))
        if nxt.is_terminal():
            break
        st = nxt
    key = (int(st.bb[0]), int(st.bb[1]), len(st.history()))
    if key not in seen:
        seen.add(key)
        by_ply.setdefault(key[2], []).append(st)

# one append per ply: a generation of one-ply games that all start at that ply; the unique list is in this order
mp, mc = game.max_game_length(), game.max_children()
store = replay.DeviceReplay(game, max_games=a.positions, device=0)
hist = []
for ply in sorted(by_ply):
    sts = by_ply[ply]
    n = len(sts)
    ex = {"game_len": np.ones(n, np.int32), "game_ret0": np.zeros(n, np.float32), "states": np.zeros((n, mp, 2), np.uint64),
          "move": np.zeros((n, mp), np.uint16), "n_children": np.zeros((n, mp), np.uint8),
          "child_action": np.zeros((n, mp, mc), np.uint16), "child_visits": np.zeros((n, mp, mc), np.uint32),
          "value": np.zeros((n, mp)), "start_ply": ply}
    for g, st in enumerate(sts):
        la = st.legal_actions()
        ex["states"][g, ply] = st.bb
        ex["n_children"][g, ply] = len(la)
        ex["child_action"][g, ply, :len(la)] = la
        ex["child_visits"][g, ply, :len(la)] = 1
        ex["move"][g, ply] = la[0]
        hist.append(st.history())
    store.append_export(ex)
assert store.dedupe() == a.positions

torch.manual_seed(0)
net = Net(game.information_state_normalized_vector_shape(), game.num_distinct_actions(), n_blocks=a.blocks, n_filters=a.filters).eval()
n_slots = a.slots or min(a.positions, 4096)
target = None if a.value_target == "none" else a.value_target


def timed(fn):
    fn()  # untimed: kernels loaded, clocks up
    torch.cuda.synchronize()
    walls = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    return out, walls


with replay.Reanalyser(store, net, n_slots, a.playouts, value_target=target, eval_precision=a.precision,
                       check_every=a.check_every) as re:
    an = re.analyzer
    everything = torch.arange(a.positions, dtype=torch.int64, device=store.device)

    def device_route():
        return re.reanalyse(indices=everything)

    def host_route():
        parts = []
        for first in range(0, len(hist), n_slots):
            an.load(hist[first:first + n_slots])
            an.search()
            parts.append(an.results()["visits"])
        return np.concatenate(parts)

    refreshed, walls_dev = timed(device_route)
    visits, walls_host = timed(host_route)
    assert refreshed == a.positions and an.engine.progress()["error_flags"] == 0 and store.stats()["fault_flags"] == 0
    # both routes searched the same positions: the stored pi is the baseline's visit distribution
    _, pi, _ = store.sample(a.positions, indices=np.arange(a.positions))
    want = visits / visits.sum(axis=1, keepdims=True)
    assert np.allclose(pi.cpu().numpy(), want, rtol=0, atol=1e-6)

dev, host = float(np.median(walls_dev)), float(np.median(walls_host))
out = {"tool": "reanalyse_microbench", "game": game.name, "positions": a.positions, "playouts": a.playouts, "n_slots": n_slots,
       "net": "%d-block x %d, fused %s, random-init" % (a.blocks, a.filters, a.precision), "check_every": a.check_every,
       "value_target": a.value_target, "mean_ply": float(np.mean([len(h) for h in hist])),
       "device_route": {"what": "Reanalyser.reanalyse: gather_states + load_states_device + search_device + refresh_from_roots",
                        "wall_s": dev, "wall_s_all": walls_dev, "positions_per_s": a.positions / dev},
       "host_route": {"what": "Analyzer.load(histories) + search + results on the same engine and evaluator",
                      "wall_s": host, "wall_s_all": walls_host, "positions_per_s": a.positions / host},
       "device_over_host": dev / host}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
