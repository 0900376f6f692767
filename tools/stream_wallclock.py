#!/usr/bin/env python3
"""Wall clock of the reference-facing per-generation call, closed generations next to continuous self-play:
ExampleGenerator.generate_into(replay, n) with continuous=False (an engine per call, a closed generation played to its last
game) and with continuous=True (one engine in stream mode across the calls, a call takes its n games off the stream), same
process, same net, same box.  For the stream: games/s, ticks per call, the mean number of stalled slots per check, graph
captures, the cost of a call that swaps the net, over a sweep of the record ring's capacity (n + G, n + 2G, n + 4G).

With --parent-tree DIR (a built checkout of the parent commit) it first runs bench.py's headline there and here, alternating,
--bench-runs times each, and compares the --dump-outputs arrays of the two builds: the tick kernel gained a stream-mode branch,
the headline has to stay inside the parent's own run-to-run spread.

    python tools/stream_wallclock.py [--games 4096] [--slots 4096] [--playouts 400] [--blocks 10] [--calls 5]
                                     [--parent-tree DIR] [--out profiles/stream_wallclock_c4_4096x400.json]
"""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(tree, steps, warmup, dump=None, timeout=900):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    if dump:
        cmd += ["--dump-outputs", dump]
    env = {k: v for k, v in os.environ.items() if k != "AZ_ENGINE_LIB"}
    out = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise SystemExit("bench.py in %s failed:\n%s" % (tree, (out.stdout + out.stderr)[-3000:]))
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def headline(parent_tree, runs, steps, warmup):
    """bench.py in the parent's tree and in this one, alternating (before this process touches the GPU)."""
    import numpy as np
    res = {"parent": [], "this": []}
    with tempfile.TemporaryDirectory() as tmp:
        dumps = {"parent": os.path.join(tmp, "parent"), "this": os.path.join(tmp, "this")}
        for i in range(runs):
            for name, tree in (("parent", parent_tree), ("this", ROOT)):
                line = _bench(tree, steps, warmup, dump=dumps[name] if i == runs - 1 else None)
                res[name].append(round(float(line["value"]), 1))
                print("bench %s run %d: %.1f %s" % (name, i, line["value"], line.get("unit", "")), flush=True)
        names = sorted(f for f in os.listdir(dumps["parent"]) if f.endswith(".npy"))
        same = names == sorted(f for f in os.listdir(dumps["this"]) if f.endswith(".npy")) and len(names) > 0
        differing = []
        for f in names if same else []:
            a, b = np.load(os.path.join(dumps["parent"], f)), np.load(os.path.join(dumps["this"], f))
            if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b):
                differing.append(f)
    p, t = res["parent"], res["this"]
    return {"command": "bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), "parent_games_per_s": p, "this_games_per_s": t,
            "parent_spread_pct": round(100.0 * (max(p) - min(p)) / (sum(p) / len(p)), 2),
            "this_over_parent_mean": round((sum(t) / len(t)) / (sum(p) / len(p)), 4),
            "dump_outputs_arrays": names, "dump_outputs_equal": bool(same and not differing), "dump_outputs_differing": differing}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--playouts", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=50)
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--calls", type=int, default=5, help="timed generate_into calls per leg (after one untimed call)")
    ap.add_argument("--capacity-slots", default="1,2,4", help="ring capacities to sweep, as n_games + k * n_slots")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: run bench.py there and here")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=2)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"game": "connect_four", "games_per_call": a.games, "n_slots": a.slots, "n_playouts": a.playouts,
           "net": "%d blocks x %d filters" % (a.blocks, a.filters), "precision": a.precision, "timed_calls": a.calls}
    if a.parent_tree:
        out["bench_headline"] = headline(os.path.abspath(a.parent_tree), a.bench_runs, a.bench_steps, a.bench_warmup)

    import torch
    from alphazero_openspiel_amd import replay
    from alphazero_openspiel_amd.examplegenerator import ExampleGenerator
    from alphazero_openspiel_amd.network import Net
    dev = torch.device("cuda:0")
    out["device"] = torch.cuda.get_device_name(0)
    torch.manual_seed(0)
    net = Net([3, 6, 7], 7, n_blocks=a.blocks, n_filters=a.filters).eval()
    kw = dict(n_slots=a.slots, n_playouts=a.playouts, eval_precision=a.precision, seed=1)

    def timed_calls(gen, store, n_calls):
        secs = []
        for _ in range(n_calls):
            torch.cuda.synchronize()
            t = time.perf_counter()
            gen.generate_into(store, a.games)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t)
        return secs

    def summary(secs):
        return {"call_s": [round(s, 3) for s in secs], "games_per_s": round(a.games * len(secs) / sum(secs), 1)}

    store = replay.DeviceReplay("connect_four", max_games=2 * a.games, device=dev)
    gen = ExampleGenerator(net, "connect_four", dev, **kw)
    gen.generate_into(store, a.games)  # untimed: library load, kernel first use
    secs = timed_calls(gen, store, a.calls)
    out["closed"] = dict(summary(secs), ticks_per_call=gen.last_progress["ticks"],
                         tail_compactions_last_call=gen.last_progress.get("tail_compactions"))
    print("closed generations: %s" % json.dumps(out["closed"]), flush=True)

    out["continuous"] = []
    for k in [int(x) for x in a.capacity_slots.split(",")]:
        cap = a.games + k * a.slots
        gen = ExampleGenerator(net, "connect_four", dev, continuous=True, stream_capacity=cap, **kw)
        try:
            gen.generate_into(store, a.games)  # untimed: builds engine, evaluator and stream; fills the pipeline
            stream = gen._stream
            t0, c0 = stream.ticks, stream.captures
            secs = timed_calls(gen, store, a.calls)
            leg = dict(summary(secs), capacity=cap, capacity_rule="n + %dG" % k, ticks_per_call=round((stream.ticks - t0) / a.calls, 1),
                       graph_captures_in_timed_calls=stream.captures - c0)
            # stalled slots per check: a full progress() at every check, so on calls of their own
            stream.count_idle, stream.idle_sum, stream.checks = True, 0, 0
            timed_calls(gen, store, 2)
            leg["mean_slots_idle_per_check"] = round(stream.idle_sum / max(1, stream.checks), 2)
            leg["checks_in_those_calls"] = stream.checks
            stream.count_idle = False
            # a call that finds new weights: new evaluator (fold + pack), device synchronisation, graph capture
            other = copy.deepcopy(net)
            with torch.no_grad():
                for p in other.parameters():
                    p.add_(1e-3 * torch.randn_like(p))
            gen.net = other
            leg["call_with_net_swap_s"] = round(timed_calls(gen, store, 1)[0], 3)
            leg["error_flags"] = gen.last_progress["error_flags"]
            leg["engine_device_bytes"] = int(gen._stream_engine.sizes.device_bytes)
        finally:
            gen.close()
        out["continuous"].append(leg)
        print("continuous, capacity %d: %s" % (cap, json.dumps(leg)), flush=True)
    store.close()
    best = max(leg["games_per_s"] for leg in out["continuous"])
    out["continuous_over_closed"] = round(best / out["closed"]["games_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
