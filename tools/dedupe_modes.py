#!/usr/bin/env python3
"""What the three dedupe rules make of one self-play generation, and what each costs, on one GPU.
    python tools/dedupe_modes.py [--games 4096] [--playouts 100] [--repeat 5] [--out profiles/<name>.json]
One generation of connect_four self-play (5-block x 50 net, random-init, fused f16) is appended to a store; then, for
history (az_replay_dedupe), position and position+mirror (az_replay_dedupe_positions), the tool prints n_examples, n_unique, the
largest group (unique_counts) and the wall time of the dedupe call between HIP events, median of --repeat.  Every timed call
runs on the same stored generation: a dedupe writes its averages back into the first occurrences, which changes the targets the
next call averages and nothing about the grouping or the work.  The comparison is the history pass of the same build on the
same store.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_openspiel_amd import engine as E, games, replay  # noqa: E402
from alphazero_openspiel_amd.fusednet import FusedNet  # noqa: E402
from alphazero_openspiel_amd.network import Net  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--playouts", type=int, default=100)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

game = games.load_game("connect_four")
torch.manual_seed(0)
net = Net([3, 6, 7], 7).eval()
slots = min(a.games, 4096)
eng = E.SelfPlayEngine(game, slots, n_playouts=a.playouts, max_games=a.games, seed=1)
ev = FusedNet(net, "cuda:0", max_boards=eng.G, precision="f16")
E.run_selfplay(eng, ev, a.games, use_graph=True)
store = replay.DeviceReplay(game, max_games=a.games)
store.append_engine(eng)
eng.close()
ev.close()

rows = {}
for label, kw in (("history", dict()), ("position", dict(by="position")), ("position+mirror", dict(by="position", mirror=True))):
    n_unique = store.dedupe(**kw)  # untimed: kernels loaded
    largest = int(store.unique_counts().max())
    ms = []
    for _ in range(a.repeat):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        assert store.dedupe(**kw) == n_unique
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    st = store.stats()
    assert st["fault_flags"] == 0
    rows[label] = {"n_examples": st["n_examples"], "n_unique": n_unique, "largest_group": largest,
                   "dedupe_ms": round(statistics.median(ms), 3), "dedupe_ms_all": [round(m, 3) for m in ms]}
    print("%-16s n_examples %d  n_unique %d  largest group %d  dedupe %.3f ms" %
          (label, st["n_examples"], n_unique, largest, rows[label]["dedupe_ms"]), flush=True)
line = json.dumps({"tool": "dedupe_modes", "game": game.name, "games": a.games, "playouts": a.playouts, "net": "5-block x 50, fused f16, random-init",
                   "repeat": a.repeat, "device": torch.cuda.get_device_name(0), "rows": rows})
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
