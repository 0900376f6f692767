#!/usr/bin/env python3
"""Games/s of bench.py's headline configuration without and with evaluation in a random left-right orientation
(az_engine_set_eval_mirror), measured the way bench.py measures: one engine with games to spare, ticks replayed from a captured
graph of 16, --warmup steps untimed, then --steps steps of n_slots finished games timed.  Same process, same build, same net.
There is no threshold: this records what the setting costs.

    python tools/eval_mirror_wallclock.py [--slots 4096] [--playouts 400] [--p 0.5] [--steps 2] [--warmup 1] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=50)
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check-every", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from alphazero_openspiel_amd import engine as E
    from alphazero_openspiel_amd.fusednet import FusedNet
    from alphazero_openspiel_amd.network import Net
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = Net([3, 6, 7], 7, n_blocks=a.blocks, n_filters=a.filters).eval()
    G, tpg = a.slots, 16
    out = {"game": "connect_four", "n_slots": G, "n_playouts": a.playouts, "p_mirror": a.p, "steps": a.steps, "warmup": a.warmup,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "device": torch.cuda.get_device_name(0)}
    ev = FusedNet(net, dev, max_boards=G, precision=a.precision)
    for leg, p in (("plain", 0.0), ("eval_mirror", a.p)):
        eng = E.SelfPlayEngine("connect_four", G, n_playouts=a.playouts, max_games=(a.warmup + a.steps + 2) * G, device=dev, seed=1)
        E.SearchSettings.from_kwargs(dict(eval_mirror=p)).apply(eng)
        eng.reset((a.warmup + a.steps + 2) * G)
        obs, pri, val = eng.alloc_io()

        def tick():
            eng.advance(pri, val, obs)
            ev(obs, pri, val)

        drv = E.TickDriver(dev, tick)
        drv.capture(tpg)

        def run_until(n_done):
            while eng.games_done() < n_done:
                drv.run(a.check_every)
            return eng.progress()

        p0 = run_until(a.warmup * G)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        p1 = run_until((a.warmup + a.steps) * G)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        games = p1["games_done"] - p0["games_done"]
        out[leg] = {"games_per_s": round(games / dt, 1), "seconds": round(dt, 3), "games_timed": games,
                    "plies_per_game": round((p1["moves"] - p0["moves"]) / games, 2), "error_flags": p1["error_flags"]}
        print("%s: %s" % (leg, json.dumps(out[leg])), flush=True)
        eng.close()
    ev.close()
    out["eval_mirror_over_plain_games_per_s"] = round(out["eval_mirror"]["games_per_s"] / out["plain"]["games_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
