#!/usr/bin/env python3
"""Wall clock of one closed self-play generation without and with playout cap randomisation (az_engine_set_playout_cap), same
process, same build, same net: games/s, kept (full-search) examples/s and playouts per move.  One untimed pass per leg, then
the median of --runs timed generations.  There is no threshold: it records what the cap buys on this box.

    python tools/playout_cap_wallclock.py [--games 4096] [--slots 4096] [--playouts 400] [--cap 100:0.25] [--blocks 10]
                                          [--out profiles/playout_cap_wallclock_c4_4096x400.json]
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
    ap.add_argument("--cap", default="100:0.25", metavar="N_FAST:P_FULL")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=50)
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--runs", type=int, default=3, help="timed generations per leg (after one untimed one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_fast, p_full = int(a.cap.split(":")[0]), float(a.cap.split(":")[1])

    import torch
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.fusednet import FusedNet
    from alphazero_openspiel_amd.network import Net
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = Net([3, 6, 7], 7, n_blocks=a.blocks, n_filters=a.filters).eval()
    out = {"game": "connect_four", "games": a.games, "n_slots": a.slots, "n_playouts": a.playouts, "n_fast": n_fast, "p_full": p_full,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "timed_runs": a.runs,
           "device": torch.cuda.get_device_name(0)}
    ev = FusedNet(net, dev, max_boards=a.slots, precision=a.precision)
    for leg, cap in (("no_cap", None), ("cap", (n_fast, p_full))):
        eng = E.SelfPlayEngine("connect_four", a.slots, n_playouts=a.playouts, max_games=a.games, device=dev, seed=1)
        if cap is not None:
            eng.set_playout_cap(*E.SearchSettings.from_kwargs(dict(playout_cap=cap)).check(n_playouts=a.playouts).playout_cap)
        rows = []
        for run in range(a.runs + 1):  # (the first one is untimed: library load, kernel first use, graph capture)
            torch.cuda.synchronize()
            t = time.perf_counter()
            prog = E.run_selfplay(eng, ev, a.games, seed=1 + run, use_graph=True)
            torch.cuda.synchronize()
            s = time.perf_counter() - t
            kept = int(eng.full_moves_device().sum().item())  # (after the clock: the mask is not self-play)
            if run:
                rows.append({"seconds": round(s, 3), "games_per_s": a.games / s, "kept_examples_per_s": kept / s,
                             "playouts_per_move": prog["sims"] / prog["moves"], "moves": prog["moves"], "kept_examples": kept})
        eng.close()
        out[leg] = {"runs": rows, **{k: round(statistics.median(r[k] for r in rows), 2)
                                     for k in ("games_per_s", "kept_examples_per_s", "playouts_per_move")}}
        print("%s: %s" % (leg, json.dumps(out[leg])), flush=True)
    ev.close()
    out["cap_over_no_cap_games_per_s"] = round(out["cap"]["games_per_s"] / out["no_cap"]["games_per_s"], 3)
    out["cap_over_no_cap_kept_examples_per_s"] = round(out["cap"]["kept_examples_per_s"] / out["no_cap"]["kept_examples_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
