"""`ExampleGenerator` with the reference's signature (examplegenerator.py:80-175), on the HIP engine.

Reference: `n_pools` pools, each = one busy-polling `handle_gpu` process + `n_processes` worker
processes playing one game at a time, a pickled batch-1 board per leaf over a Pipe
(examplegenerator.py:39-77,106-138).  Here: one process per GPU, all games of the shard resident on
the device as engine slots, one `net.forward` per tick over every outstanding leaf; across GPUs the
games shard over `torch.distributed` ranks and the examples are all-gathered once at generation end
(RCCL over xGMI; nothing is exchanged during the search).
"""
import copy

import numpy as np
import torch

from .engine import (EngineError, SearchSettings, SelfPlayEngine, SelfPlayStream, check_stream_request, close_all, device_export_layout,
                     examples_from_export, make_evaluator, run_selfplay, run_selfplay_pools, slot_groups, stream_capacity,
                     unpack_device_export, unpack_resign_info)
from .games import Game
from . import distributed as azdist

_ENGINE_KW = ("n_playouts", "c_puct", "temperature", "dirichlet_ratio", "use_dirichlet", "keep_search_tree",
              "backup", "use_puct", "num_probabilistic_actions")


def _sum_progress(progs):
    """The pools' progress dicts as one: counters summed, fault flags OR-ed, the per-pool dicts kept under "pools"."""
    out = {}
    for k in progs[0]:
        vals = [p[k] for p in progs]
        if k == "error_flags":
            v = 0
            for x in vals:
                v |= int(x)
            out[k] = v
        elif all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in vals):
            out[k] = max(vals) if k in ("ticks", "tail_compactions") else sum(vals)
        else:
            out[k] = vals[0]
    out["pools"] = list(progs)
    return out


class ExampleGenerator:
    def __init__(self, net, game_name, device, n_pools=1, n_processes=1, **kwargs):
        self.net2 = copy.deepcopy(kwargs["net2"]) if kwargs.get("net2") is not None else None  # examplegenerator.py:88-90
        self.is_test = bool(kwargs.get("is_test", False))
        self.generate_statistics = bool(kwargs.get("generate_statistics", False))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise EngineError("ExampleGenerator needs a HIP device: self-play runs in HIP kernels, there is no "
                              "CPU fallback (got device=%s)" % (device,))
        self.net = copy.deepcopy(net)  # examplegenerator.py:86: a frozen copy of the current net
        self.game_name = game_name
        self.game = Game(game_name)
        # n_pools = "amount of GPUs to utilize" (train.py:32): with several HIP devices visible to ONE process (no torch.distributed)
        # pool i is an engine of its own on the device the reference would pick (examplegenerator.py:144-150) and plays
        # int(n_games / n_pools) games; on one device the pools collapse into one engine that plays the same COUNT.
        # pool_devices=[...] names the devices explicitly (also: several pools on one device, which is how the path is tested).
        self.n_pools, self.n_processes = int(n_pools), n_processes  # (no worker processes here: module doc)
        self.pool_devices = kwargs.get("pool_devices")
        self.kwargs = kwargs
        # engine extensions (not reference keywords)
        self.n_slots = kwargs.get("n_slots")           # concurrent games per GPU; default min(n_games, 4096)
        self.seed = int(kwargs.get("seed", np.random.randint(0, 2 ** 31 - 1)))
        self.eval_backend = kwargs.get("eval_backend", "fused")   # "fused" (csrc/az_net.hip) | "torch"
        # fused backend: "f32x" = fp32-grade (split-fp16 operands, the reference's Net.forward is fp32: network.py:48-64);
        # "f16" = fp16 operands, ~2.5x the throughput, opt-in (tolerances: tests/test_precision_search_gpu.py)
        self.eval_precision = kwargs.get("eval_precision", "f32x")
        self.eval_dtype = kwargs.get("eval_dtype", torch.float32)   # torch backend only
        self.use_graph = bool(kwargs.get("use_graph", True))
        self.overlap = int(kwargs.get("overlap", 1))  # slot groups ticking on their own HIP streams (engine.run_selfplay)
        self.last_progress = None
        self._generation = 0
        # continuous=True: ONE engine in stream mode (engine.SelfPlayStream) lives across the calls; a call takes its games off
        # the stream while the slots play on, instead of building an engine and playing a closed generation to its last game.
        # stream_capacity: rows of the record ring (default: engine.stream_capacity - a call's games + 2 per slot)
        self.continuous = bool(kwargs.get("continuous", False))
        self.stream_capacity = kwargs.get("stream_capacity")
        self._stream = self._stream_engine = self._stream_evaluator = None
        self._stream_net = None  # the weights and buffers the stream's evaluator was built from
        if self.continuous:
            if self.n_pools > 1 or self.pool_devices is not None:
                raise ValueError("continuous=True drives one engine per process: n_pools > 1 / pool_devices are not supported with it")
            if self.overlap > 1:
                raise ValueError("continuous=True ticks the engine on one stream: overlap > 1 is not supported with it")
            if self.eval_backend != "fused":
                raise ValueError("continuous=True needs eval_backend=\"fused\" (got %r)" % (self.eval_backend,))
        # The search settings (search_settings.SearchSettings; an off k or p is the same as none: these engines are built here).
        # playout_cap=(n_fast, p_full): every move is searched in full (n_playouts) with probability p_full, else with n_fast
        # playouts, and ONLY the full-search moves become examples.  The mask of full-search moves is a side table of one engine: it
        # does not travel with a gather (as game starts do not).
        # forced_playouts=k or (k, prune), eval_mirror=p, solver=True, fpu=r or (r, r_root): forced playouts with policy target
        # pruning, evaluation in a random left-right orientation, the MCTS-Solver and first-play urgency in every search.  They
        # leave the records' layout alone (pruned and adjusted counts sit where the raw ones sat), so they go to EVERY engine this
        # generator builds (pools, ranks, overlap, the stream of continuous=True).
        self.settings = SearchSettings.from_kwargs(kwargs).check(
            self._check_start_positions, is_test=self.is_test, use_puct=bool(kwargs.get("use_puct", True)),
            n_playouts=int(kwargs.get("n_playouts", 100)), overlap=self.overlap)  # (100: SelfPlayEngine's default)
        self.playout_cap, self.forced_playouts = self.settings.playout_cap, self.settings.forced_playouts
        self.eval_mirror, self.solver, self.fpu = self.settings.eval_mirror, bool(self.settings.solver), self.settings.fpu
        # resign=v, (v, playthrough) or (v, playthrough, min_ply): self-play resignation (SelfPlayEngine.set_resign) in every engine
        # this generator builds (pools, ranks, the stream of continuous=True); the returned games are the shortened ones, in the
        # reference's format.  resign_stats accumulates over the calls what THIS process's engines played (see _note_resign).
        self.resign = self.settings.resign
        self.resign_stats = {"games": 0, "resigned": 0, "playthrough_would_resign": 0, "playthrough_wrong": 0,
                             "low": np.zeros((0, 2), dtype=np.float64), "ret0": np.zeros((0,), dtype=np.float64),
                             "weight": np.zeros((0,), dtype=np.float64)}

    def _engine_kwargs(self):
        return {k: self.kwargs[k] for k in _ENGINE_KW if k in self.kwargs}

    def _new_engine(self, n_slots, **kw):
        """A self-play engine with this generator's search settings (forced_playouts and eval_mirror among them; reset() comes
        after)."""
        engine = SelfPlayEngine(self.game, n_slots, **kw, **self._engine_kwargs())
        try:
            self.settings.apply(engine)
        except Exception:
            close_all(engine)
            raise
        return engine

    def _note_resign(self, info, buf, n, dims):
        """One engine's games into resign_stats.  info: SelfPlayEngine.resign_info_device's tensors for the n games packed in
        `buf` (the results are read from its game_ret0 array).  games / resigned: counted; playthrough_would_resign: play-through
        games that have a resign ply; playthrough_wrong: those among them whose resigner - the player to move at that ply - did
        not go on to lose; low / ret0 / weight: per-player lowest criterion, result and sampling weight of every game that was
        PLAYED OUT (a play-through game, or one without a resign ply) - the arguments of resign.false_positive_rate /
        resign.calibrate(..., weights=).  A game with a resign ply is played out with probability playthrough and carries the
        weight 1 / playthrough, a game without one the weight 1 (resign.played_out_weights): the weighted rate is unbiased for
        every threshold.  With playthrough = 0 no game with a resign ply is played out and nothing can be said about them."""
        layout, _ = device_export_layout(n, *dims)
        off = next(o for name, _, _, o in layout if name == "game_ret0")
        ret0 = buf[off:off + 4 * n].cpu().numpy().view(np.float32).astype(np.float64)
        r = unpack_resign_info(*info)
        st = self.resign_stats
        through = r["playthrough"] & (r["ply"] >= 0)
        lost = np.where((r["ply"] & 1) == 0, ret0 < 0.0, ret0 > 0.0)          # did the player to move at the resign ply lose?
        st["games"] += int(n)
        st["resigned"] += int(r["resigned"].sum())
        st["playthrough_would_resign"] += int(through.sum())
        st["playthrough_wrong"] += int((through & ~lost).sum())
        out = ~r["resigned"]
        st["low"] = np.concatenate([st["low"], r["low"][out]])
        st["ret0"] = np.concatenate([st["ret0"], ret0[out]])
        weight = np.where(r["ply"][out] >= 0, 1.0 / self.resign[1] if self.resign[1] > 0.0 else 1.0, 1.0)
        st["weight"] = np.concatenate([st["weight"], weight])

    def _pool_device_list(self):
        """Devices of the reference's pools when this one process drives several GPUs, else None (one engine)."""
        if self.pool_devices is not None:
            return [torch.device(d) for d in self.pool_devices]
        n_dev = torch.cuda.device_count()
        if self.n_pools < 2 or n_dev < 2 or azdist.world_size() > 1:
            return None
        devs, device_no = [], 1  # examplegenerator.py:144-150: the first pool goes to cuda:1, the count wraps to cuda:0
        for _ in range(self.n_pools):
            if device_no >= n_dev:
                device_no = 0
            devs.append(torch.device("cuda", device_no))
            device_no += 1
        return devs

    def _play_pools(self, n_games, devices):
        """One engine + evaluator per pool, each on its device, driven from this thread (engine.run_selfplay_pools); the pools'
        packed records are brought to self.device and laid out like the ranks of an all-gather."""
        n_each = int(n_games / len(devices))
        if n_each < 1:
            raise ValueError("n_games=%d is fewer than the %d pools" % (n_games, len(devices)))
        n_slots = int(self.n_slots or min(n_each, 4096))
        engines, evaluators = [], []
        try:
            for i, dev in enumerate(devices):
                with torch.cuda.device(dev):
                    engines.append(self._new_engine(n_slots, max_games=n_each, device=dev,
                                                    seed=self.seed + 1000003 * self._generation + 7919 * i))
                    net = self.net if self.eval_backend == "fused" else copy.deepcopy(self.net)  # a torch pool gets its own copy
                    evaluators.append(make_evaluator(net, dev, self.eval_backend, self.eval_precision, n_slots, self.eval_dtype))
            progs = run_selfplay_pools(engines, evaluators, n_each, use_graph=self.use_graph)
            self.last_progress = _sum_progress(progs)
            bufs = []
            for e in engines:
                with torch.cuda.device(e.device):
                    b = e.export_device()
                    info = e.resign_info_device() if self.resign is not None else None
                    torch.cuda.current_stream(e.device).synchronize()
                if info is not None:
                    self._note_resign(info, b, n_each, (e.max_plies, e.max_children))
                bufs.append(b.to(self.device))
            dims = (engines[0].max_plies, engines[0].max_children)
        finally:
            close_all(*engines, drain=True)  # a pool that raised leaves the others' enqueued batches behind
            close_all(*evaluators)
        self._generation += 1
        return torch.cat(bufs), bufs[0].numel(), n_each, len(devices), dims

    @staticmethod
    def _net_tensors(net):
        return list(net.parameters()) + list(net.buffers())

    def _take_and_gather(self, n_games):
        """continuous=True: this rank's int(n_games / world) games off its stream (built by the first call), then the same
        exchange as _play_and_gather - one generation's payload.  self.net is read again at every call: broadcast from rank 0
        when distributed, and when its weights or buffers differ from what the stream's evaluator was built from, a new
        evaluator takes over (SelfPlayStream.set_evaluator: games in flight go on under the new net)."""
        world, rank = azdist.world_size(), azdist.rank()
        n_local = int(n_games) if world == 1 else int(n_games / world)
        if n_local < 1:
            raise ValueError("n_games=%d is fewer than the %d ranks" % (n_games, world))
        if world > 1 or not azdist._single():
            self.net = self.net.to(self.device)
            azdist.broadcast_net(self.net, src=0)
        now = self._net_tensors(self.net)
        if self._stream is None:
            n_slots = int(self.n_slots or min(n_local, 4096))
            cap = stream_capacity(n_local, n_slots, self.stream_capacity)
            engine = self._new_engine(n_slots, max_games=cap, device=self.device,
                                      seed=self.seed + 7919 * rank)  # (the seed of a first closed generation: same games, id for id)
            evaluator = None
            try:
                evaluator = make_evaluator(self.net, self.device, self.eval_backend, self.eval_precision, n_slots, self.eval_dtype)
                self._stream = SelfPlayStream(engine, evaluator, use_graph=self.use_graph)  # (the engine carries the settings)
            except Exception:
                close_all(engine, evaluator, drain=True)
                raise
            self._stream_engine, self._stream_evaluator = engine, evaluator
            self._stream_net = [t.detach().clone() for t in now]
        else:
            check_stream_request(n_local, self._stream_engine.sizes.max_games)
            same = len(now) == len(self._stream_net) and all(
                a.shape == b.shape and torch.equal(a.detach().to(b.device), b) for a, b in zip(now, self._stream_net))
            if not same:
                old = self._stream_evaluator
                self._stream_evaluator = make_evaluator(self.net, self.device, self.eval_backend, self.eval_precision,
                                                        self._stream_engine.G, self.eval_dtype)
                self._stream.set_evaluator(self._stream_evaluator)
                close_all(old)
                self._stream_net = [t.detach().clone() for t in now]
        engine = self._stream_engine
        buf, _ = self._stream.take(n_local)
        if self.resign is not None:
            self._note_resign(self._stream.last_resign_info, buf, n_local, (engine.max_plies, engine.max_children))
        prog = engine.progress()
        prog["ticks"] = self._stream.ticks
        self.last_progress = prog
        self._generation += 1
        return azdist.all_gather_device_exports(buf), buf.numel(), n_local, world, (engine.max_plies, engine.max_children)

    def close(self):
        """Release the stream of continuous=True (drained first), its engine and its evaluator."""
        stream, self._stream = self._stream, None
        if stream is not None:
            stream.close()
            close_all(self._stream_engine, self._stream_evaluator)
        self._stream_engine = self._stream_evaluator = self._stream_net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_start_positions(self, what):
        """A start per game is a single-process, closed-generation path: the multi-rank gather and the pools carry one start ply."""
        if azdist.world_size() > 1:
            bad = "torch.distributed with world size %d" % azdist.world_size()
        elif self.n_pools > 1:
            bad = "n_pools=%d" % self.n_pools
        elif self.pool_devices is not None:
            bad = "pool_devices"
        elif self.continuous:
            bad = "continuous=True"
        else:
            return
        raise ValueError("%s is not supported with %s: games with a side table of their own (start positions, a playout cap's mask of "
                         "full-search moves) are played by ONE engine in a closed generation" % (what, bad))

    def _play_from_starts(self, n_games, histories=None, fork=None, into=None):
        """One closed generation on one engine whose game i starts after histories[i], or from the stored position fork[1][i]
        of the DeviceReplay fork[0] (neither: from the initial position - the path of playout_cap).  -> the export dict of host
        arrays (engine.export()) or, with `into`, the number of games appended to that store.  Under playout_cap the dict
        carries "keep", the host copy of the mask of full-search moves, and the store takes only those moves (append_engine)."""
        n = int(n_games)
        n_slots = int(self.n_slots or min(n, 4096))
        engine = self._new_engine(n_slots, max_games=n, device=self.device, seed=self.seed + 1000003 * self._generation)
        evaluator = None
        try:
            if fork is not None:
                engine.set_game_starts_device(*fork[0].gather_forks(fork[1]))
            elif histories is not None:
                engine.set_game_starts(histories)
            if self.playout_cap is not None:
                engine.set_playout_cap(*self.playout_cap)
            evaluator = make_evaluator(self.net, self.device, self.eval_backend, self.eval_precision, n_slots, self.eval_dtype)
            self.last_progress = run_selfplay(engine, evaluator, n, use_graph=self.use_graph)
            if self.resign is not None:
                self._note_resign(engine.resign_info_device(), engine.export_device(), n, (engine.max_plies, engine.max_children))
            if into is not None:
                into.append_engine(engine)
                out = n
            else:
                out = engine.export()
                if self.playout_cap is not None:
                    out["keep"] = engine.full_moves_device().cpu().numpy()
        finally:
            close_all(engine, evaluator, drain=True)
        self._generation += 1
        return out

    def _play_and_gather(self, n_games):
        """This rank's shard of the generation on the HIP engine, then the generation-end exchange on DEVICE buffers.
        -> (gathered uint8 device tensor [world * nbytes], nbytes per rank, games per rank, world, (max_plies, max_children))"""
        if self.continuous:
            return self._take_and_gather(n_games)
        pool_devs = self._pool_device_list()
        if pool_devs is not None:
            return self._play_pools(n_games, pool_devs)
        world, rank = azdist.world_size(), azdist.rank()
        if world == 1:  # the reference plays int(n_games / n_pools) games in each of its n_pools pools (examplegenerator.py:149):
            n_local = int(n_games / self.n_pools) * self.n_pools if self.n_pools > 1 else int(n_games)  # same count here
        else:
            n_local = int(n_games / world)
        if n_local < 1:
            raise ValueError("n_games=%d is fewer than the %d ranks / pools" % (n_games, max(world, self.n_pools)))
        if world > 1 or not azdist._single():
            # every handler gets a copy of THE current net (examplegenerator.py:121): the training rank's weights and
            # BatchNorm statistics, whatever this rank was constructed with
            self.net = self.net.to(self.device)
            azdist.broadcast_net(self.net, src=0)
        n_slots = int(self.n_slots or min(n_local, 4096))
        engine = self._new_engine(n_slots, max_games=n_local, device=self.device,
                                  seed=self.seed + 1000003 * self._generation + 7919 * rank)
        evaluators = []
        try:
            sizes = [n for _, n in slot_groups(n_slots, self.overlap)] if self.overlap > 1 else [n_slots]
            evaluators = [make_evaluator(self.net, self.device, self.eval_backend, self.eval_precision, n, self.eval_dtype)
                          for n in sizes]
            self.last_progress = run_selfplay(engine, evaluators if self.overlap > 1 else evaluators[0], n_local,
                                              use_graph=self.use_graph, overlap=self.overlap)
            buf = engine.export_device()
            dims = (engine.max_plies, engine.max_children)
            if self.resign is not None:
                self._note_resign(engine.resign_info_device(), buf, n_local, dims)
            torch.cuda.current_stream(self.device).synchronize()
        finally:
            close_all(engine, *evaluators)
        self._generation += 1
        return azdist.all_gather_device_exports(buf), buf.numel(), n_local, world, dims

    def generate_examples(self, n_games, start_positions=None):
        """-> list of games; a game is a list of [info_state_str, board (C+1,H,W) f64, pi list[A], z]
        (examplegenerator.py:164-175, game_utils.py:169,200-204).  With torch.distributed initialised the net is broadcast
        from rank 0, each rank plays int(n_games / world_size) games (remainder dropped like int(n_games / n_pools),
        examplegenerator.py:149), the packed records are all-gathered on the device (RCCL) and every rank returns the
        same gathered list.  The reference-format lists are built from ONE device-to-host copy of the gathered buffer.
        start_positions: a list of at least n_games action lists - game i starts after start_positions[i] (an opening set, a
        curriculum, endgames) and its keys are the full histories, prefix included.  One process, one engine, a closed
        generation: ValueError with torch.distributed world > 1, n_pools > 1, pool_devices or continuous=True.
        With playout_cap=(n_fast, p_full) the games hold only their full-search examples (same limits)."""
        if start_positions is not None:
            self._check_start_positions("generate_examples(start_positions=...)")
            histories = self._histories(n_games, start_positions)
            ex = self._play_from_starts(n_games, histories)
            return examples_from_export(self.game, ex, histories, keep=ex.get("keep"))
        if self.playout_cap is not None:  # only the full-search moves become examples; one engine, whose mask says which
            self._check_start_positions("playout_cap")
            ex = self._play_from_starts(n_games)
            return examples_from_export(self.game, ex, keep=ex["keep"])
        gathered, nbytes, n_local, world, (mp, mc) = self._play_and_gather(n_games)
        host = gathered.cpu().numpy()
        games = []
        for r in range(world):
            ex = unpack_device_export(host[r * nbytes:(r + 1) * nbytes], n_local, mp, mc)
            games.extend(examples_from_export(self.game, ex))
        return games

    @staticmethod
    def _histories(n_games, start_positions):
        histories = [[int(a) for a in h] for h in start_positions][:int(n_games)]
        if len(histories) < int(n_games) or int(n_games) < 1:
            raise ValueError("start_positions holds %d histories, %d games were asked for" % (len(histories), int(n_games)))
        return histories

    def generate_into(self, replay, n_games, start_positions=None, fork_from=None):
        """The same generation, delivered straight into a DeviceReplay on this rank's GPU (engine -> all-gather -> replay
        store, records never leave HBM and never become Python lists).  Returns the number of games appended.
        start_positions: as in generate_examples.  fork_from: an int64 tensor / array of n_games indices into the store's
        de-duplicated list (dedupe() first) - game i is forked off that stored position, store -> engine -> store on the device
        (replay.Forker keeps an engine across such calls).  Both are single-process, closed-generation paths."""
        if start_positions is not None and fork_from is not None:
            raise ValueError("give start_positions or fork_from, not both")
        if start_positions is not None:
            self._check_start_positions("generate_into(start_positions=...)")
            return self._play_from_starts(n_games, self._histories(n_games, start_positions), into=replay)
        if fork_from is not None:
            self._check_start_positions("generate_into(fork_from=...)")
            idx = replay._indices(fork_from)
            if int(idx.numel()) != int(n_games):
                raise ValueError("fork_from holds %d indices, %d games were asked for" % (int(idx.numel()), int(n_games)))
            return self._play_from_starts(n_games, fork=(replay, idx), into=replay)
        if self.playout_cap is not None:  # the kept path: the store takes the engine's full-search moves only
            self._check_start_positions("playout_cap")
            return self._play_from_starts(n_games, into=replay)
        gathered, nbytes, n_local, world, _ = self._play_and_gather(n_games)
        for r in range(world):
            replay.append_device(gathered[r * nbytes:(r + 1) * nbytes], n_local)
        return n_local * world

    def generate_tests(self, n_games, game_fn, n_playouts_mcts):
        """n_games calls of `game_fn` (test_zero_vs_mcts / test_net_vs_mcts / test_zero_vs_random / test_net_vs_random:
        two games each, the agent once as first and once as second player) against an MCTSBot with n_playouts_mcts
        simulations -> average reward sum(score1 + score2) / (2 n_games) (examplegenerator.py:177-195).  All 2 n_games
        games are slots of one device arena (alphazero_openspiel_amd.arena); with torch.distributed the tests shard over
        the ranks and the mean is all-reduced."""
        from . import arena
        name = getattr(game_fn, "__name__", str(game_fn))
        pairing = {"test_zero_vs_mcts": ("zero", "uct"), "test_net_vs_mcts": ("net", "uct"),
                   "test_zero_vs_random": ("zero", "random"), "test_net_vs_random": ("net", "random")}.get(name)
        if pairing is None and name != "test_zero_vs_zero":
            raise NotImplementedError("generate_tests supports the pairings of game_utils.py:53-145, got %s" % name)
        world, rank = azdist.world_size(), azdist.rank()
        # the reference plays int(n_games / n_pools) tests in each of its n_pools pools and divides the summed scores by
        # 2 * n_games AS REQUESTED (examplegenerator.py:149,189): same count (same rule as _play_and_gather) and same divisor
        if world == 1:
            n_local = int(n_games / self.n_pools) * self.n_pools if self.n_pools > 1 else int(n_games)
        else:
            n_local = int(n_games / world)
        if n_local < 1:
            raise ValueError("n_games=%d is fewer than the %d ranks / pools" % (n_games, max(world, self.n_pools)))
        if world > 1:
            self.net = self.net.to(self.device)
            azdist.broadcast_net(self.net, src=0)
        kw = {k: self.kwargs[k] for k in arena.ENGINE_KW if k in self.kwargs}
        statistics = [None] * n_local  # the pairings against bots return no statistics (game_utils.py:65,83)
        if name == "test_zero_vs_zero" and self.generate_statistics:
            # both search trees after every move (game_utils.py:29-31): the reference's own per-game loop over façade bots,
            # one device search per step - an inspection mode (tournament.py:39-52 plays one test per pairing with it)
            from .game_utils import test_zero_vs_zero
            net1 = self.net.to(self.device).eval()
            net2 = (self.net2 if self.net2 is not None else self.net).to(self.device).eval()
            out = [test_zero_vs_zero(net1, None, self.game_name, policy_fn2=net2, generate_statistics=True,
                                     settings1=self.kwargs.get("settings1", kw), settings2=self.kwargs.get("settings2", kw))
                   for _ in range(n_local)]
            s1, s2 = np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64)
            statistics = [o[2] for o in out]
        elif name == "test_zero_vs_zero":  # two networks, each with its settings (game_utils.py:120-145; net2 defaults to net)
            if world > 1 and self.net2 is not None:
                self.net2 = self.net2.to(self.device)
                azdist.broadcast_net(self.net2, src=0)
            s1, s2, self.last_progress = arena.play_zero_vs_zero(
                self.net, self.net2 if self.net2 is not None else self.net, self.game_name, n_local,
                settings1=self.kwargs.get("settings1", kw), settings2=self.kwargs.get("settings2", kw), device=self.device,
                seed=self.seed + 1000003 * self._generation + 7919 * rank, eval_backend=self.eval_backend,
                eval_precision=self.eval_precision)
        else:
            s1, s2, self.last_progress = self._play_tests(arena, n_local, pairing, n_playouts_mcts, rank, kw)
        self._generation += 1
        total = torch.tensor([float(s1.sum() + s2.sum()), float(2 * n_local)], dtype=torch.float64)
        total = azdist.all_reduce_sum(total, self.device)
        avg_reward = float(total[0]) / (2 * n_games)  # examplegenerator.py:189: sum(examples) / (2 * n_games)
        if self.generate_statistics:  # examplegenerator.py:192-193 (this rank's tests)
            return avg_reward, statistics
        return avg_reward

    def _play_tests(self, arena, n_local, pairing, n_playouts_mcts, rank, kw):
        return arena.play_tests(
            self.net, self.game_name, n_local, pairing[0], pairing[1], opponent_sims=int(n_playouts_mcts), device=self.device,
            seed=self.seed + 1000003 * self._generation + 7919 * rank, n_slots=self.n_slots, eval_backend=self.eval_backend,
            eval_precision=self.eval_precision, **kw)
