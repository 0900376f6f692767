#!/usr/bin/env python3
"""Times batched position analysis (analysis.Analyzer: one engine slot per position) and, on a sample of the same positions,
the one-position-at-a-time route (mcts.MCTS.search on its 1-slot engine), on one GPU.
    python tools/analysis_microbench.py [--positions 4096] [--playouts 400] [--blocks 10] [--filters 50] [--slots N]
                                        [--repeat 3] [--single-sample 64] [--out profiles/<name>.json]
Positions: uniformly random legal moves from a fixed seed to a random target ply (stopping before a move that would end the
game).  Wall time spans load (host replay of the prefixes + table upload + reset), every tick, and the read-back of all roots,
between device synchronisations, after one untimed warm-up run.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_openspiel_amd import games  # noqa: E402
from alphazero_openspiel_amd.analysis import Analyzer  # noqa: E402
from alphazero_openspiel_amd.mcts import MCTS  # noqa: E402
from alphazero_openspiel_amd.network import Net  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=4096)
ap.add_argument("--playouts", type=int, default=400)
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--filters", type=int, default=50)
ap.add_argument("--slots", type=int, default=0, help="engine slots (default: min(positions, 4096))")
ap.add_argument("--game", default="connect_four")
ap.add_argument("--precision", default="f32x", choices=["f16", "f32x"])
ap.add_argument("--max-ply", type=int, default=30)
ap.add_argument("--check-every", type=int, default=16)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--single-sample", type=int, default=64, help="positions searched one at a time through mcts.MCTS (0 = skip)")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
a = ap.parse_args()

game = games.load_game(a.game)
rng = np.random.RandomState(a.seed)
hist = []
for _ in range(a.positions):
    target, st = int(rng.randint(0, a.max_ply + 1)), game.new_initial_state()
    while len(st.history()) < target:
        legal = st.legal_actions()
        nxt = st.clone()
        nxt.apply_action(int(legal[rng.randint(len(legal))]))
        if nxt.is_terminal():
            break
        st = nxt
    hist.append(st.history())
torch.manual_seed(0)
net = Net(game.information_state_normalized_vector_shape(), game.num_distinct_actions(), n_blocks=a.blocks, n_filters=a.filters).eval()
n_slots = a.slots or min(a.positions, 4096)


def batched(an):
    parts = []
    for first in range(0, len(hist), n_slots):
        an.load(hist[first:first + n_slots])
        an.search()
        parts.append(an.results()["visits"])
    return np.concatenate(parts)


walls = []
with Analyzer(net, game, n_slots, n_playouts=a.playouts, device="cuda:0", eval_precision=a.precision, seed=1,
              check_every=a.check_every) as an:
    visits = batched(an)  # warm-up: kernels loaded, clocks up
    torch.cuda.synchronize()
    t_ticks = an.ticks
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        v = batched(an)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        assert np.array_equal(v, visits)
    prog = an.engine.progress()
    ticks_per_run = (an.ticks - t_ticks) // a.repeat
assert prog["error_flags"] == 0
wall = float(np.median(walls))
out = {"tool": "analysis_microbench", "game": game.name, "positions": a.positions, "playouts": a.playouts, "n_slots": n_slots,
       "net": "%d-block x %d, fused %s, random-init" % (a.blocks, a.filters, a.precision), "check_every": a.check_every,
       "batched": {"wall_s": wall, "wall_s_all": walls, "positions_per_s": a.positions / wall,
                   "sims_per_s": a.positions * a.playouts / wall, "ticks": int(ticks_per_run),
                   "mean_ply": float(np.mean([len(h) for h in hist]))}}
if a.single_sample > 0:
    pick = np.random.RandomState(a.seed + 1).choice(len(hist), size=min(a.single_sample, len(hist)), replace=False)
    m = MCTS(net, game.num_distinct_actions(), n_playouts=a.playouts, use_dirichlet=False, device=torch.device("cuda:0"))
    m.search(games.state_from_history(game, hist[int(pick[0])]))  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in pick:
        m.search(games.state_from_history(game, hist[int(i)]))
    torch.cuda.synchronize()
    w1 = time.perf_counter() - t0
    out["one_at_a_time"] = {"route": "mcts.MCTS.search (1-slot engine, torch fp32 forward per playout)", "sample": int(len(pick)),
                            "wall_s_sample": w1, "positions_per_s": len(pick) / w1, "sims_per_s": len(pick) * a.playouts / w1,
                            "wall_s_scaled_to_all": w1 * a.positions / len(pick), "scaled": True}
    out["speedup_scaled"] = out["one_at_a_time"]["wall_s_scaled_to_all"] / wall
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
