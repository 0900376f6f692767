#!/usr/bin/env python3
"""Wall clock of one closed self-play generation without and with MCTS-Solver (az_engine_set_solver), same process, same build,
same net: games/s, plies per game, playouts actually run per move, evaluations per game, terminal_hits and - for the solver - the
share of moves made at a proven root.  One untimed pass per leg, then the median of --runs timed generations.  There is no
threshold: the solver is a different search, this records what it costs and what it saves.

The share of moves made at a proven root is counted in a pass of its own (untimed, eager ticks): after every tick the root export
and the proof export say which slots stand on a proven root, and every (game id, ply) seen so is one such move - a search ends at
once at a proven root, and the move is made there.  The pass plays the games of the first timed run (the games do not depend on how
the ticks are driven); its move and playout counts are checked against that run's.

    python tools/solver_wallclock.py [--games 4096] [--slots 4096] [--playouts 400] [--blocks 10]
                                     [--out profiles/solver_wallclock_c4_4096x400.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("games_per_s", "plies_per_game", "playouts_per_move", "evals_per_game", "terminal_hits")


def proven_root_census(E, eng, ev, n_games, seed):
    """One eager generation -> (moves made at a proven root, the progress dict).  Everything per tick stays on the device."""
    import numpy as np
    import torch
    G, mp = eng.G, eng.max_plies
    off = {name: (o, int(np.prod(shape))) for name, _, shape, o in E.roots_export_layout(G, eng.max_children)[0]}
    roots = eng.alloc_roots()
    proofs = torch.empty((G, 1 + eng.max_children), dtype=torch.uint8, device=roots.device)
    seen = torch.zeros(n_games * mp + 1, dtype=torch.bool, device=roots.device)   # (the last entry takes the slots that do not count)

    def field(name):
        o, n = off[name]
        return roots[o:o + 4 * n].view(torch.int32)

    def on_tick(engine, ticks):
        engine.export_roots_device(roots)
        engine.export_proofs_device(proofs)
        gid, ply = field("game_id").long(), field("ply").long()
        hit = (proofs[:, 0] != 0) & (field("phase") != 0) & (gid >= 0) & (gid < n_games)
        seen[torch.where(hit, gid * mp + ply, torch.full_like(gid, n_games * mp))] = True

    prog = E.run_selfplay(eng, ev, n_games, seed=seed, on_tick=on_tick)
    return int(seen[:-1].sum().item()), prog


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=400)
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
    out = {"game": "connect_four", "games": a.games, "n_slots": a.slots, "n_playouts": a.playouts,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "timed_runs": a.runs,
           "device": torch.cuda.get_device_name(0)}
    ev = FusedNet(net, dev, max_boards=a.slots, precision=a.precision)
    for leg, solver in (("plain", False), ("solver", True)):
        eng = E.SelfPlayEngine("connect_four", a.slots, n_playouts=a.playouts, max_games=a.games, device=dev, seed=1)
        E.SearchSettings.from_kwargs(dict(solver=solver)).apply(eng)
        rows, counts = [], []
        for run in range(a.runs + 1):  # (the first one is untimed: library load, kernel first use, graph capture)
            torch.cuda.synchronize()
            t = time.perf_counter()
            prog = E.run_selfplay(eng, ev, a.games, seed=1 + run, use_graph=True)
            torch.cuda.synchronize()
            s = time.perf_counter() - t
            if run:
                counts.append((prog["moves"], prog["sims"]))
                rows.append({"seconds": round(s, 3), "games_per_s": a.games / s, "plies_per_game": prog["moves"] / a.games,
                             "playouts_per_move": prog["sims"] / prog["moves"], "evals_per_game": prog["evals"] / a.games,
                             "terminal_hits": prog["terminal_hits"]})
        out[leg] = {"runs": rows, **{key: round(statistics.median(r[key] for r in rows), 2) for key in KEYS}}
        if solver:
            proven, prog = proven_root_census(E, eng, ev, a.games, seed=2)  # the games of the first timed run
            if (prog["moves"], prog["sims"]) != counts[0]:
                raise SystemExit("the census pass played other games than the timed run: %r against %r"
                                 % ((prog["moves"], prog["sims"]), counts[0]))
            out[leg]["moves_at_a_proven_root"] = proven
            out[leg]["proven_root_share"] = round(proven / prog["moves"], 4)
        eng.close()
        print("%s: %s" % (leg, json.dumps(out[leg])), flush=True)
    ev.close()
    out["solver_over_plain_games_per_s"] = round(out["solver"]["games_per_s"] / out["plain"]["games_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
