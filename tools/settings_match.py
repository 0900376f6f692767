#!/usr/bin/env python3
"""A match between two search settings on one checkpoint (arena.play_match): engine A plays --a, engine B plays --b, over --pairs
random openings of --plies moves, each played twice with the colours swapped and scored per pair.  Prints the result (wins / draws /
losses, score, standard error and Elo with its 95 % interval, all seen from A) and games/s as one JSON line.  There is no threshold:
whether a setting gains strength is what the match is run to find out.

A settings string is a comma-separated list of  plain | solver | fpu=R[:R_ROOT] | eval_mirror=P | n_playouts=N | c_puct=X |
temperature=X;  e.g.  --a fpu=0.3:0.0,solver --b plain.

    python tools/settings_match.py [--game connect_four] [--checkpoint tests/golden/checkpoint_connect_four.npz] [--pairs 1024]
                                   [--plies 4] [--playouts 100] [--a fpu=0.3:0.0] [--b plain] [--seed 1] [--runs 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHECKPOINTS = {"connect_four": "checkpoint_connect_four.npz", "breakthrough(rows=6,columns=6)": "checkpoint_breakthrough6.npz"}


def parse_settings(text, playouts):
    """'fpu=0.3:0.0,solver' -> dict(n_playouts=playouts, fpu=(0.3, 0.0), solver=True)."""
    out = {"n_playouts": int(playouts)}
    for item in filter(None, (s.strip() for s in text.split(","))):
        key, _, val = item.partition("=")
        if key == "plain" and not val:
            continue
        if key == "solver" and val in ("", "1", "true", "True"):
            out["solver"] = True
        elif key == "fpu" and val:
            out["fpu"] = tuple(float(x) for x in val.split(":")) if ":" in val else float(val)  # (read by SearchSettings)
        elif key == "eval_mirror" and val:
            out["eval_mirror"] = float(val)
        elif key == "n_playouts" and val:
            out["n_playouts"] = int(val)
        elif key in ("c_puct", "temperature") and val:
            out[key] = float(val)
        else:
            raise ValueError("cannot read the setting %r" % item)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="connect_four", choices=sorted(CHECKPOINTS))
    ap.add_argument("--checkpoint", default=None, help="an .npz checkpoint (default: the game's one under tests/golden/)")
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=4, help="length of the random openings; 0 = every game from the initial position")
    ap.add_argument("--playouts", type=int, default=100)
    ap.add_argument("--a", default="fpu=0.3:0.0", help="settings of engine A")
    ap.add_argument("--b", default="plain", help="settings of engine B")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=1, help="timed matches (the same match again: the result is that of the first)")
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from alphazero_openspiel_amd import arena, games
    from alphazero_openspiel_amd.network import load_npz_checkpoint
    game = games.load_game(a.game)
    path = a.checkpoint or os.path.join(ROOT, "tests", "golden", CHECKPOINTS[a.game])
    net = load_npz_checkpoint(path, [3, game.rows, game.cols], game.num_distinct_actions())
    sa, sb = parse_settings(a.a, a.playouts), parse_settings(a.b, a.playouts)
    openings = arena.random_openings(a.game, a.pairs, a.plies, a.seed) if a.plies > 0 else None
    rows, first = [], None
    for run in range(a.runs + 1):  # (the first one is untimed: library load, kernel first use, graph capture)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = arena.play_match(net, None, a.game, a.pairs, settings_a=sa, settings_b=sb, openings=openings, device="cuda:0", seed=a.seed,
                               eval_precision=a.precision)
        torch.cuda.synchronize()
        s = time.perf_counter() - t
        if first is None:
            first = res
        if run:
            rows.append({"seconds": round(s, 3), "games_per_s": round(2 * a.pairs / s, 1)})
    out = {"game": a.game, "checkpoint": os.path.basename(path), "a": a.a, "b": a.b, "pairs": a.pairs, "plies": a.plies,
           "playouts": a.playouts, "seed": a.seed, "device": torch.cuda.get_device_name(0),
           "wins": first["wins"], "draws": first["draws"], "losses": first["losses"], "score": round(first["score"], 5),
           "stderr": round(first["stderr"], 5), "elo": round(first["elo"], 1), "elo_lo": round(first["elo_lo"], 1),
           "elo_hi": round(first["elo_hi"], 1), "ticks": first["progress"]["ticks"], "error_flags": first["progress"]["error_flags"],
           "games_per_s": max(r["games_per_s"] for r in rows), "runs": rows}
    text = json.dumps(out)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
