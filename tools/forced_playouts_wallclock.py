#!/usr/bin/env python3
"""Wall clock of one closed self-play generation without and with forced playouts and policy target pruning
(az_engine_set_forced_playouts), same process, same build, same net: games/s and plies per game.  One untimed pass per leg, then
the median of --runs timed generations.  There is no threshold: forcing is a different search, this records what it costs.

    python tools/forced_playouts_wallclock.py [--games 4096] [--slots 4096] [--playouts 400] [--k 2] [--blocks 10]
                                              [--out profiles/forced_playouts_wallclock_c4_4096x400.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=50)
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--runs", type=int, default=3, help="timed generations per leg (after one untimed one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.fusednet import FusedNet
    from alphazero_openspiel_amd.network import Net
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = Net([3, 6, 7], 7, n_blocks=a.blocks, n_filters=a.filters).eval()
    out = {"game": "connect_four", "games": a.games, "n_slots": a.slots, "n_playouts": a.playouts, "k": a.k, "prune": 1,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "timed_runs": a.runs,
           "device": torch.cuda.get_device_name(0)}
    ev = FusedNet(net, dev, max_boards=a.slots, precision=a.precision)
    for leg, k in (("plain", 0.0), ("forced", a.k)):
        eng = E.SelfPlayEngine("connect_four", a.slots, n_playouts=a.playouts, max_games=a.games, device=dev, seed=1)
        E.SearchSettings.from_kwargs(dict(forced_playouts=(k, True))).apply(eng)
        rows = []
        for run in range(a.runs + 1):  # (the first one is untimed: library load, kernel first use, graph capture)
            torch.cuda.synchronize()
            t = time.perf_counter()
            prog = E.run_selfplay(eng, ev, a.games, seed=1 + run, use_graph=True)
            torch.cuda.synchronize()
            s = time.perf_counter() - t
            if run:
                rows.append({"seconds": round(s, 3), "games_per_s": a.games / s, "plies_per_game": prog["moves"] / a.games,
                             "playouts_per_move": prog["sims"] / prog["moves"]})
        eng.close()
        out[leg] = {"runs": rows, **{key: round(statistics.median(r[key] for r in rows), 2)
                                     for key in ("games_per_s", "plies_per_game", "playouts_per_move")}}
        print("%s: %s" % (leg, json.dumps(out[leg])), flush=True)
    ev.close()
    out["forced_over_plain_games_per_s"] = round(out["forced"]["games_per_s"] / out["plain"]["games_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
