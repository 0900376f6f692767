#!/usr/bin/env python3
"""The reference's Trainer.run loop (train.py:272-293) with every stage on the GPU:

    generation:  self-play (HIP search + fused net)  ->  device replay store (FIFO, remove_duplicates)
                 ->  n_batches x (gather 256 + net_step, replayed as one HIP graph)
                 ->  every --eval-every generations: Trainer.test_agent (train.py:238-270) on the device arena

    python examples/train_connect_four.py --generations 3 --games 512 --playouts 100

Hyper-parameters default to the reference's (train.py:24-49): 100 playouts/move, c_puct 2.5, temperature 1,
Dirichlet ratio 0.25, 500 batches of 256 per generation, Adam lr 1e-3 wd 1e-4, buffer of 4 generations growing to 40.
Checkpoints are written in the reference's .pth format.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_openspiel_amd import arena, engine as E, games, replay, resign  # noqa: E402
from alphazero_openspiel_amd.examplegenerator import ExampleGenerator  # noqa: E402
from alphazero_openspiel_amd.fusednet import FusedNet  # noqa: E402
from alphazero_openspiel_amd.network import Net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="connect_four")
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--games", type=int, default=500, help="n_games_per_generation (train.py:36)")
    ap.add_argument("--playouts", type=int, default=100, help="n_playouts_train (train.py:46)")
    ap.add_argument("--batches", type=int, default=500, help="n_batches_per_generation (train.py:37)")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--backup", default="on-policy", choices=["on-policy", "soft-Z", "A0C", "off-policy"])
    ap.add_argument("--save", default=None, help="directory for <generation>.pth checkpoints")
    ap.add_argument("--precision", default="f32x", choices=["f32x", "f16"], help="fused-net arithmetic (f32x = fp32-grade)")
    ap.add_argument("--eval-every", type=int, default=0, help="run test_agent every N generations (0 = never)")
    ap.add_argument("--tests", type=int, default=200, help="n_tests (train.py:30)")
    ap.add_argument("--continuous", action="store_true",
                    help="self-play as ONE stream across the generations (ExampleGenerator(continuous=True)): the slots never wait "
                         "for a generation's longest game, and games in flight go on under each updated net")
    ap.add_argument("--reanalyse", type=int, default=0,
                    help="before training, search N sampled positions of the de-duplicated buffer again with the current net and "
                         "overwrite their pi (and z, when --backup is soft-Z, A0C or off-policy: the targets a search gives)")
    ap.add_argument("--fork", type=int, default=0,
                    help="after each generation, fork N more games from uniformly drawn stored positions (played to the end "
                         "with the current net) and append them: fresh outcomes under old positions, lines the policy left early")
    ap.add_argument("--mirror", action="store_true",
                    help="train on left-right mirrored batches: every sampled position is flipped or not by a coin drawn on the "
                         "device (both games are symmetric under it; the policy is mirrored with the board)")
    ap.add_argument("--playout-cap", default=None, metavar="N_FAST:P_FULL",
                    help="playout cap randomisation: every move is searched with --playouts playouts with probability P_FULL and "
                         "with N_FAST otherwise, and only the full-search moves are trained on (e.g. 25:0.25; not with --continuous)")
    ap.add_argument("--forced-playouts", type=float, default=0.0, metavar="K",
                    help="forced playouts at the root and policy target pruning (KataGo, section 3.2) in every full search: a tried "
                         "root child gets at least sqrt(K P N) visits, and the visits it did not earn leave the recorded pi (e.g. 2)")
    ap.add_argument("--eval-mirror", type=float, default=0.0, metavar="P",
                    help="evaluate every network request of a search (self-play, and the searches of --reanalyse) left-right mirrored "
                         "with probability P and map the answer back, as AlphaGo Zero and KataGo do: a left/right bias of the net "
                         "averages out of the visit counts instead of being trained back in (e.g. 0.5)")
    ap.add_argument("--solver", action="store_true",
                    help="MCTS-Solver: prove wins, losses and draws inside the search tree (self-play, and the searches of "
                         "--reanalyse): never select a move proven lost, end a search whose root is proven, play a proven win and "
                         "record exact targets there; not together with --forced-playouts")
    ap.add_argument("--fpu", default="", metavar="R[:R_ROOT]",
                    help="first-play urgency reduction, as Lc0 and KataGo select: an unvisited child is valued at its parent's value "
                         "minus R * sqrt(explored prior mass) (R_ROOT at the root, default 0) in place of the reference's 0, in "
                         "self-play and in the searches of --reanalyse and --fork (e.g. 0.3)")
    ap.add_argument("--merge-positions", default="off", choices=["off", "plain", "mirror"],
                    help="what the dedupe before training merges: off = examples with equal action histories, as the reference; "
                         "plain = examples of one position (bitboards and side to move) whatever the move order that led there; "
                         "mirror = also a position and its left-right mirror image, the policy mapped with the board")
    ap.add_argument("--resign", default=None, metavar="V[:P[:MIN_PLY]]",
                    help="self-play resignation, as AlphaGo Zero and KataGo: a game ends with a loss for the side to move once its "
                         "search values the position below -V (after MIN_PLY plies, default 0); a share P of the games (default 0.1) "
                         "plays through all the same, which measures the false positives (e.g. 0.9:0.1)")
    ap.add_argument("--resign-auto", type=float, default=None, metavar="FP",
                    help="with --resign: between generations, set V to the most eager threshold whose false-positive rate on the "
                         "played-out games so far stays at or below FP (e.g. 0.05), and print it with the measured rate (not with "
                         "--continuous: a stream keeps the threshold it began with)")
    a = ap.parse_args()
    dedupe = {"off": dict(), "plain": dict(by="position"), "mirror": dict(by="position", mirror=True)}[a.merge_positions]
    if a.playout_cap and a.continuous:
        ap.error("--playout-cap is not available with --continuous (the mask of full-search moves does not travel with a take)")
    if a.resign_auto is not None and (a.resign is None or a.continuous):
        ap.error("--resign-auto needs --resign and is not available with --continuous")
    if a.resign_auto is not None and ":" in a.resign and float(a.resign.split(":")[1]) <= 0.0:
        ap.error("--resign-auto needs a play-through share P > 0: without play-through games no false positive is ever seen")
    try:  # one parser and one set of rules for the six settings (alphazero_openspiel_amd/search_settings.py)
        settings = E.SearchSettings.from_kwargs(dict(
            forced_playouts=a.forced_playouts or None, eval_mirror=a.eval_mirror or None, solver=a.solver,
            fpu=(tuple(float(x) for x in a.fpu.split(":")) if ":" in a.fpu else float(a.fpu)) if a.fpu else None,
            playout_cap=tuple(a.playout_cap.split(":")) if a.playout_cap else None,
            resign=tuple(float(x) if i < 2 else int(x) for i, x in enumerate(a.resign.split(":"))) if a.resign else None,
        )).check(n_playouts=a.playouts)
    except ValueError as err:
        ap.error("%s (--fpu takes R or R:R_ROOT, --playout-cap N_FAST:P_FULL, --resign V[:P[:MIN_PLY]])" % err)
    fpu, cap = settings.fpu, settings.playout_cap
    seen_low, seen_ret0, seen_w = np.zeros((0, 2)), np.zeros((0,)), np.zeros((0,))   # --resign: the played-out games so far, each
    #                                                                        with its sampling weight (resign.played_out_weights)

    dev = torch.device("cuda:0")
    game = games.load_game(a.game)
    torch.manual_seed(0)
    net = Net(game.information_state_normalized_vector_shape(), game.num_distinct_actions()).to(dev)
    n_buffer, n_buffer_max = 4 * a.games, 40 * a.games                     # train.py:38-41
    store = replay.DeviceReplay(game, max_games=n_buffer_max, device=dev)
    trainer = reanalyser = forker = None
    generator, before = None, {"moves": 0, "sims": 0}
    if a.continuous:
        generator = ExampleGenerator(net, a.game, dev, continuous=True, n_slots=min(a.games, 4096), n_playouts=a.playouts,
                                     backup=a.backup, eval_precision=a.precision, seed=1,
                                     forced_playouts=a.forced_playouts or None, eval_mirror=a.eval_mirror or None, solver=a.solver,
                                     fpu=fpu, resign=settings.resign)
    for gen in range(1, a.generations + 1):
        t0 = time.perf_counter()
        net.eval()
        if generator is not None:
            generator.net = net                                            # read again at every call: the stream takes the new weights over
            generator.generate_into(store, a.games)
            total = generator.last_progress                                # (counters since the stream began, games in flight included)
            prog = {k: total[k] - before[k] for k in before}
            before = {k: total[k] for k in before}
        else:
            eng = E.SelfPlayEngine(game, min(a.games, 4096), n_playouts=a.playouts, backup=a.backup, max_games=a.games,
                                   device=dev, seed=gen)
            settings.apply(eng)                                            # (under forced playouts the records hold the pruned counts)
            if cap is not None:
                eng.set_playout_cap(*cap)                                  # append_engine below keeps the full-search moves only
            prog = E.run_selfplay(eng, FusedNet(net, dev, max_boards=eng.G, precision=a.precision), a.games, use_graph=True)
        t_play = time.perf_counter() - t0
        if generator is None:
            store.append_engine(eng)
            if settings.resign is not None:                                # what the threshold did, and - auto - the next one
                info = eng.resign_info()
                ret0 = E.unpack_device_export(eng.export_device().cpu().numpy(), a.games, eng.max_plies, eng.max_children)["game_ret0"]
                out = ~info["resigned"]
                seen_low, seen_ret0 = np.concatenate([seen_low, info["low"][out]]), np.concatenate([seen_ret0, ret0[out]])
                if settings.resign[1] > 0.0:                               # a game with a resign ply is played out with probability P
                    seen_w = np.concatenate([seen_w, resign.played_out_weights(info["ply"][out] >= 0, settings.resign[1])])
                else:
                    seen_w = np.concatenate([seen_w, np.ones(int(out.sum()))])
                v = settings.resign[0]
                rate, n_below = resign.false_positive_rate(seen_low, seen_ret0, v, seen_w)
                print("gen %d: resign v %.3f: %d of %d games resigned | false-positive rate %.3f at that v, over the %d players below it "
                      "in the %d played-out games so far (play-through games and games without a resign ply, weighted by how often "
                      "each kind is played out)" % (gen, v, int(info["resigned"].sum()), a.games, rate, n_below, len(seen_ret0)), flush=True)
                if a.resign_auto is not None:
                    try:
                        v = resign.calibrate(seen_low, seen_ret0, target=a.resign_auto, weights=seen_w)
                        settings.resign = (v,) + settings.resign[1:]
                        print("gen %d: resign-auto: v -> %.3f (rate %.3f on the same weighted games, target %.3f)"
                              % (gen, v, resign.false_positive_rate(seen_low, seen_ret0, v, seen_w)[0], a.resign_auto), flush=True)
                    except ValueError as err:
                        print("gen %d: resign-auto: %s" % (gen, err), flush=True)
            eng.close()
        if gen % 2 == 0 and n_buffer < n_buffer_max:                       # Trainer.update_buffer_size
            n_buffer += a.games
        store.set_capacity(n_buffer)
        n_unique = store.dedupe(**dedupe)
        if a.fork:                                                         # store -> engine -> store, on the device
            t_fk = time.perf_counter()
            if forker is None:
                forker = replay.Forker(store, net, min(a.fork, 4096), a.playouts, eval_precision=a.precision, use_graph=True,
                                       max_games=a.fork, backup=a.backup, seed=1000, fpu=fpu)
            else:
                forker.set_net(net)
            forker.fork(n=a.fork, seed=gen)
            n_before, n_unique = n_unique, store.dedupe(**dedupe)
            print("gen %d: forked %d games from %d unique positions in %.2f s -> %d unique" %
                  (gen, a.fork, n_before, time.perf_counter() - t_fk, n_unique), flush=True)
        t_re = time.perf_counter()
        if a.reanalyse:                                                    # stale targets of older generations -> the current net's
            if reanalyser is None:
                reanalyser = replay.Reanalyser(store, net, min(a.reanalyse, 4096), a.playouts,
                                               value_target=a.backup if a.backup in ("soft-Z", "A0C", "off-policy") else None,
                                               eval_precision=a.precision, eval_mirror=a.eval_mirror or None, solver=a.solver, fpu=fpu)
            else:
                reanalyser.set_evaluator(net)
            n_re = reanalyser.reanalyse(n=a.reanalyse, seed=gen)
            print("gen %d: reanalysed %d of %d unique positions in %.2f s" % (gen, n_re, n_unique, time.perf_counter() - t_re),
                  flush=True)
        net.train()
        if trainer is None:
            trainer = replay.GraphedNetStep(net, a.batch_size, store, mirror=a.mirror)
        t1 = time.perf_counter()
        lp = lv = 0.0
        for i in range(a.batches):
            p, v = trainer(seed=gen)
            if i >= a.batches - 100:
                lp += float(p) / 100
                lv += float(v) / 100
        torch.cuda.synchronize()
        t_train = time.perf_counter() - t1
        st = store.stats()
        print("gen %d: %d games (%.0f plies avg, %.2f M sims) in %.2f s | buffer %d games / %d examples -> %d unique (merge-positions %s) | "
              "%d batches in %.2f s, loss_p %.4f loss_v %.4f" %
              (gen, a.games, prog["moves"] / a.games, prog["sims"] / 1e6, t_play, st["n_games"], st["n_examples"], n_unique,
               a.merge_positions, a.batches, t_train, lp, lv), flush=True)
        if a.eval_every and gen % a.eval_every == 0:                        # Trainer.test_agent (train.py:238-270)
            net.eval()
            t2 = time.perf_counter()
            out = []
            for agent, opp, sims in (("net", "random", 0), ("net", "uct", 100), ("zero", "uct", 200), ("net", "uct", 200)):
                s1, s2, _ = arena.play_tests(net, a.game, a.tests, agent, opp, opponent_sims=sims, device=dev, seed=gen,
                                             eval_precision=a.precision, c_puct=2.5)
                out.append("%s vs %s%s: %+.3f" % (agent, opp, sims or "", float((s1.sum() + s2.sum()) / (2 * a.tests))))
            print("        test_agent (%d tests each, %.2f s): %s" % (a.tests, time.perf_counter() - t2, " | ".join(out)), flush=True)
        if a.save:
            os.makedirs(a.save, exist_ok=True)
            torch.save(net.state_dict(), os.path.join(a.save, "%d.pth" % gen))
    if generator is not None:
        generator.close()
    if reanalyser is not None:
        reanalyser.close()
    if forker is not None:
        forker.close()


if __name__ == "__main__":
    main()
