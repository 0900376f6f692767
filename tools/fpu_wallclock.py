#!/usr/bin/env python3
"""Wall clock of one closed self-play generation without and with first-play urgency (az_engine_set_fpu), same process, same build,
same net: games/s, plies per game, sum_depth / sims (the mean depth of a playout) and evals / sims (the share of playouts that ask
the network).  One untimed pass per leg, then the median of --runs timed generations.  There is no threshold: the rule changes the
shape of the trees, so playouts per second move for reasons other than its arithmetic; this records the values.

    python tools/fpu_wallclock.py [--games 4096] [--slots 4096] [--playouts 400] [--blocks 10] [--fpu 0.3:0.0] [--legs plain,fpu]
                                  [--out profiles/fpu_wallclock_c4_4096x400.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("games_per_s", "sims_per_s", "plies_per_game", "depth_per_sim", "evals_per_sim")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=50)
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--fpu", default="0.3:0.0", metavar="R:R_ROOT")
    ap.add_argument("--legs", default="plain,fpu", help="which legs to run (a profiler run takes one)")
    ap.add_argument("--runs", type=int, default=3, help="timed generations per leg (after one untimed one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.fusednet import FusedNet
    from alphazero_openspiel_amd.network import Net
    settings = E.SearchSettings.from_kwargs(dict(fpu=tuple(float(x) for x in a.fpu.split(":"))))
    fpu = settings.fpu
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = Net([3, 6, 7], 7, n_blocks=a.blocks, n_filters=a.filters).eval()
    out = {"game": "connect_four", "games": a.games, "n_slots": a.slots, "n_playouts": a.playouts,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "timed_runs": a.runs, "fpu": list(fpu),
           "device": torch.cuda.get_device_name(0)}
    ev = FusedNet(net, dev, max_boards=a.slots, precision=a.precision)
    for leg in a.legs.split(","):
        eng = E.SelfPlayEngine("connect_four", a.slots, n_playouts=a.playouts, max_games=a.games, device=dev, seed=1)
        if leg == "fpu":
            settings.apply(eng)
        rows = []
        for run in range(a.runs + 1):  # (the first one is untimed: library load, kernel first use, graph capture)
            torch.cuda.synchronize()
            t = time.perf_counter()
            prog = E.run_selfplay(eng, ev, a.games, seed=1 + run, use_graph=True)
            torch.cuda.synchronize()
            s = time.perf_counter() - t
            if run:
                rows.append({"seconds": round(s, 3), "games_per_s": a.games / s, "sims_per_s": prog["sims"] / s,
                             "plies_per_game": prog["moves"] / a.games, "depth_per_sim": prog["sum_depth"] / prog["sims"],
                             "evals_per_sim": prog["evals"] / prog["sims"]})
        out[leg] = {"runs": rows, **{key: round(statistics.median(r[key] for r in rows), 4) for key in KEYS}}
        eng.close()
        print("%s: %s" % (leg, json.dumps(out[leg])), flush=True)
    ev.close()
    if "plain" in out and "fpu" in out:
        out["fpu_over_plain_games_per_s"] = round(out["fpu"]["games_per_s"] / out["plain"]["games_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
