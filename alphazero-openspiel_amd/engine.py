"""Python handle on the HIP self-play engine (C ABI: include/az_engine.h) + the tick loop.

PyTorch is plumbing here: it owns the observation / prior / value device tensors, the stream and the
PV-net; the search, game dynamics and rollout loop are the HIP kernels in csrc/az_engine.hip.
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib
from .games import Game, boards_from_bitboards
from .search_settings import SearchSettings, fpu_pair  # noqa: F401 (fpu_pair: importable from here as before)


class EngineError(RuntimeError):
    pass


def _device_index(device):
    if isinstance(device, int):
        return device
    device = torch.device(device)
    if device.type != "cuda":
        raise EngineError("the self-play engine runs on a HIP device only (got %s); there is no CPU path" % device)
    return device.index if device.index is not None else torch.cuda.current_device()


class SelfPlayEngine:
    """G concurrent games of AlphaZero self-play on one GPU.

    Keyword names follow the reference's kwargs (mcts.py:96-101, alphazerobot.py:26,34-38,
    game_utils.py:155): n_playouts, c_puct, use_dirichlet, dirichlet_ratio, temperature,
    keep_search_tree, backup."""

    def __init__(self, game_name, n_slots, n_playouts=100, c_puct=2.5, temperature=1.0, dirichlet_ratio=0.25,
                 use_dirichlet=True, keep_search_tree=True, backup="on-policy", max_games=None, device=0,
                 rng="philox", seed=0, nodes_per_slot=0, max_sims_per_tick=0, chain_window_us=0, manual_moves=False,
                 dirichlet_alpha=0.3, arena_agent=None, opponent=None, opponent_sims=0, opponent_uct_c=1.0, arena_flip=False,
                 use_puct=True, use_probabilistic_actions=False, num_probabilistic_actions=1000, spare_pools=0):
        self.lib = _lib.load()
        self.game = Game(game_name) if isinstance(game_name, str) else game_name
        self.device_index = _device_index(device)
        self.device = torch.device("cuda", self.device_index)
        if backup not in _lib.BACKUPS:
            raise ValueError("backup must be one of %s" % sorted(_lib.BACKUPS))
        cfg = _lib.AzConfig()
        cfg.struct_size = C.sizeof(_lib.AzConfig)
        cfg.game, cfg.rows, cfg.cols = self.game.game_id, self.game.rows, self.game.cols
        cfg.n_slots = int(n_slots)
        cfg.n_playouts = int(n_playouts)
        cfg.use_dirichlet = int(bool(use_dirichlet))
        cfg.keep_search_tree = int(bool(keep_search_tree))
        cfg.backup = _lib.BACKUPS[backup]
        cfg.rng_mode = {"philox": _lib.RNG_PHILOX, "injected": _lib.RNG_INJECTED}[rng]
        cfg.max_sims_per_tick = int(max_sims_per_tick)
        cfg.chain_window_us = int(chain_window_us)
        cfg.device = self.device_index
        cfg.manual_moves = int(bool(manual_moves))
        cfg.nodes_per_slot = int(nodes_per_slot)
        cfg.spare_pools = int(spare_pools)  # 0 = default (n_slots / 16, at least 16)
        cfg.max_games = int(max_games if max_games is not None else n_slots)
        cfg.c_puct = float(c_puct)
        cfg.dirichlet_ratio = float(dirichlet_ratio)
        cfg.dirichlet_alpha = float(dirichlet_alpha)
        cfg.temperature = float(temperature)
        cfg.seed = int(seed) & (2 ** 64 - 1)
        # evaluation arena (alphazero_openspiel_amd.arena): agent "zero" | "net" against opponent "random" | "uct"
        cfg.arena_agent = _lib.ARENA_AGENTS[arena_agent]
        cfg.arena_opponent = _lib.OPPONENTS[opponent]
        cfg.opponent_sims = int(opponent_sims)
        cfg.opponent_uct_c = float(opponent_uct_c)
        cfg.arena_flip = int(bool(arena_flip))
        # MCTS(use_puct=False) (mcts.py:80,199-200): the rule of trees that update_root starts from a leaf root
        cfg.select_rule = _lib.SELECT_PUCT if use_puct else _lib.SELECT_UCT
        # alphazerobot.py:34-36,81-86: an arena "zero" agent samples its moves (self-play always does), for the first n plies
        cfg.arena_probabilistic = int(bool(use_probabilistic_actions) and arena_agent == "zero")
        cfg.num_probabilistic_actions = int(num_probabilistic_actions) if int(num_probabilistic_actions) > 0 else -1
        self.cfg = cfg
        self.backup = backup
        self._h = C.c_void_p()
        rc = self.lib.az_engine_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise EngineError("az_engine_create failed (%d): %s" % (rc, self.lib.az_last_error(None).decode()))
        z = _lib.AzSizes()
        self._check(self.lib.az_engine_sizes(self._h, C.byref(z)))
        self.sizes = z
        self.G, self.A = z.n_slots, z.num_actions
        self.obs_shape = (z.obs_planes, z.rows, z.cols)
        self.max_plies, self.max_children = z.max_plies, z.max_children
        self._starts()
        self.playout_cap = None      # set_playout_cap: (n_fast, p_full) while a cap is in force
        self.forced_playouts = None  # set_forced_playouts: (k, prune) while the setting is in force
        self.eval_mirror = None      # set_eval_mirror: p_mirror while the setting is in force
        self.solver = False          # set_solver: True while the setting is in force
        self.fpu = None              # set_fpu: (reduction, root reduction) while the setting is in force
        self.arena_search = None     # set_arena_search: dict(fpu=, solver=, eval_mirror=) while an arena agent carries a setting
        self.resign = None           # set_resign: (v, playthrough, min_ply) while the setting is in force
        self.n_games = 0

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc < 0:
            raise EngineError("engine call failed (%d): %s" % (rc, self.lib.az_last_error(self._h).decode()))
        return rc

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _starts(self, history=(), histories=None, game_starts=None):
        """Where the games start, as the Python side keeps it - always the three together: start_history, the one prefix of
        every game (injected draws are indexed from its end unless set_injected_rng(absolute_ply=True)); start_histories, one
        history per game (set_start_positions / set_game_starts; None when the states came as positions); game_starts, the
        int32 array [n] of the games' start plies (set_game_starts / set_game_starts_device)."""
        self.start_history = [int(a) for a in history]
        self.start_histories = None if histories is None else [[int(a) for a in h] for h in histories]
        self.game_starts = game_starts

    def _int_ptr(self, t, dtype, shape):
        """Pointer to a contiguous integer tensor of this dtype and shape on the engine's device (None stays None)."""
        if t is None:
            return None
        if t.dtype != dtype or not t.is_contiguous() or t.device != self.device or tuple(t.shape) != shape:
            raise EngineError("expected a contiguous %s %s tensor on %s, got %s %s on %s"
                              % (dtype, shape, self.device, t.dtype, tuple(t.shape), t.device))
        return C.c_void_p(t.data_ptr())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.az_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc_io(self):
        """(obs[G,C+1,H,W], priors[G,A], values[G]) float32 device tensors of the right shape."""
        obs = torch.zeros((self.G,) + self.obs_shape, dtype=torch.float32, device=self.device)
        pri = torch.full((self.G, self.A), 1.0 / self.A, dtype=torch.float32, device=self.device)
        val = torch.zeros((self.G,), dtype=torch.float32, device=self.device)
        return obs, pri, val

    # ------------------------------------------------------------------ C ABI
    def reset(self, n_games, seed=None):
        if seed is None:
            seed = self.cfg.seed
        self._check(self.lib.az_engine_reset(self._h, int(seed) & (2 ** 64 - 1), int(n_games), self._stream()))
        self.n_games = int(n_games)

    def set_start_prefix(self, actions):
        arr = (C.c_int32 * max(1, len(actions)))(*[int(a) for a in actions])
        self._check(self.lib.az_engine_set_start_prefix(self._h, arr, len(actions)))
        self._starts(history=actions)

    def set_start_positions(self, histories):
        """A start position per game (manual_moves engines): histories[i] is the action list that leads from the initial
        position to game i's; reset(n <= len(histories)) afterwards.  An illegal action or a prefix that ends the game raises
        EngineError naming the game's index.  May be called again (the next chunk); set_start_prefix returns to one prefix."""
        actions, lengths, stride = pack_histories(histories)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.az_engine_set_start_positions(self._h, actions.ctypes.data_as(ip), lengths.ctypes.data_as(ip),
                                                           stride, len(lengths)))
        self._starts(histories=histories)

    def set_start_states_device(self, bb, ply):
        """The device form of set_start_positions: game i starts from the state (bb[i, 0], bb[i, 1], ply[i]) - bb an int64
        device tensor [n, 2] holding the 64-bit boards (torch has no uint64 arithmetic; the bits are what counts), ply int32 [n],
        as DeviceReplay.gather_states returns them.  Every state is checked on the device; a bad one raises EngineError
        naming the lowest offending game and the rule it breaks, and the previous table stays.  reset(n) afterwards."""
        n = int(ply.numel())
        self._check(self.lib.az_engine_set_start_states_device(self._h, self._int_ptr(bb, torch.int64, (n, 2)),
                                                               self._int_ptr(ply, torch.int32, (n,)), n, self._stream()))
        self._starts()

    def set_game_starts(self, histories):
        """A start position per game for SELF-PLAY (az_engine_set_game_starts): game i of the next generation starts after the
        action list histories[i], plays to its end and is recorded like any other game; reset(n <= len(histories)) afterwards.
        Plain self-play engines only.  An illegal action or a prefix that ends the game raises EngineError naming "game <i>" and
        an earlier table stays in force.  The games carry the history keys of their prefixes into a replay store; export()
        then returns "start_ply" as an int32 array and start_histories keeps the prefixes for examples_from_export."""
        actions, lengths, stride = pack_histories(histories)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.az_engine_set_game_starts(self._h, actions.ctypes.data_as(ip), lengths.ctypes.data_as(ip),
                                                       stride, len(lengths)))
        self._starts(histories=histories, game_starts=lengths.copy())

    def set_game_starts_device(self, bb, ply, keys=None):
        """The device form of set_game_starts: game i starts from the state (bb[i, 0], bb[i, 1], ply[i]) - tensors as
        DeviceReplay.gather_forks returns them - and carries the history key pair keys[i] (int64 [n, 2] holding the 64-bit
        words; None: the games are keyed from their start states, as ordinary games that start there).  Every state is
        checked on the device; a bad one raises EngineError naming the lowest offending game, and the previous table stays."""
        n = int(ply.numel())
        self._check(self.lib.az_engine_set_game_starts_device(
            self._h, self._int_ptr(bb, torch.int64, (n, 2)), self._int_ptr(ply, torch.int32, (n,)),
            self._int_ptr(keys, torch.int64, (n, 2)), n, self._stream()))
        self._starts(game_starts=ply.cpu().numpy().astype(np.int32))

    def game_starts_device(self, n_games=None):
        """-> (ply int32 [n], keys int64 [n, 2] or None) device tensors: every game id's start ply and history key pair, what
        DeviceReplay.append_device(buf, n, start_ply=ply, keys=keys) takes beside export_device().  keys is None when the
        games carry no given pairs (no table, or set_game_starts_device(keys=None)).  n_games: default the last reset's."""
        n = int(self.n_games if n_games is None else n_games)
        ply = torch.empty((n,), dtype=torch.int32, device=self.device)
        keys = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        keyed = self._check(self.lib.az_engine_game_starts_device(self._h, C.c_void_p(ply.data_ptr()), C.c_void_p(keys.data_ptr()),
                                                                  n, self._stream()))
        return ply, (keys if keyed else None)

    def set_playout_cap(self, n_fast, p_full=1.0):
        """Playout cap randomisation (az_engine_set_playout_cap): from the next reset() on, every move is searched in full
        (n_playouts) with probability p_full and otherwise fast (n_fast playouts, 1 <= n_fast <= n_playouts); every move is
        still recorded, and full_moves_device() tells the two kinds apart.  Plain self-play engines only, not in stream mode
        (EngineError names the reason otherwise).  n_fast = 0 clears the cap.  reset() afterwards."""
        self._check(self.lib.az_engine_set_playout_cap(self._h, int(n_fast), float(p_full)))
        self.playout_cap = (int(n_fast), float(p_full)) if int(n_fast) else None

    def set_forced_playouts(self, k, prune=True):
        """Forced playouts and policy target pruning (az_engine_set_forced_playouts; KataGo, Wu 2019, section 3.2): from the
        next reset() / stream_begin() on, every full search gives a root child with n > 0 visits and n^2 < k P N a playout
        before any other child, and with prune the recorded child visits are the pruned ones - the raw counts are not kept, so
        export(), export_device(), stream_take() and DeviceReplay.append_* all deliver the pruned target.  Fast moves under a
        playout cap are searched and recorded as without the setting.  Plain PUCT self-play engines only (EngineError names
        the reason otherwise).  k = 0 clears the setting.  reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_forced_playouts(self._h, float(k), int(prune)))
        self.forced_playouts = (float(k), bool(prune)) if float(k) > 0.0 else None

    def set_eval_mirror(self, p):
        """Evaluation in a random left-right orientation (az_engine_set_eval_mirror): from the next reset() / stream_begin() on,
        every network request of a search is shown to the network mirrored with probability p and its priors are mapped back
        (the value is used as it is).  The coin is a Philox draw keyed by (seed, game id, root ply, request), so a game still
        depends on (seed, game id, network) alone; the records do not change shape.  Self-play and manual_moves engines
        (EngineError names the reason for an arena engine).  p = 0 clears the setting.  reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_eval_mirror(self._h, float(p)))
        self.eval_mirror = float(p) if float(p) > 0.0 else None

    def set_solver(self, on=True):
        """MCTS-Solver (az_engine_set_solver): from the next reset() / stream_begin() on, the search proves wins, losses and
        draws inside its tree - it never selects a move proven lost, stops a playout at a proven node, ends a search whose root
        is proven, plays a proven win and records exact targets there.  PUCT self-play and manual_moves engines (EngineError
        names the reason for an arena engine, use_puct=False and an engine with forced playouts).  on=False clears the setting.
        reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_solver(self._h, int(bool(on))))
        self.solver = bool(on)

    def set_fpu(self, reduction, root=0.0):
        """First-play urgency (az_engine_set_fpu): from the next reset() / stream_begin() on, an unvisited child enters the PUCT
        comparison with Q = -parent.Q - f * sqrt(prior mass of the visited children) in place of the reference's 0; f = `root` at
        the root of a search and `reduction` below, both finite and >= 0.  reduction=0 is not the reference ("worth what the parent
        is worth"): clear_fpu() clears.  PUCT self-play and manual_moves engines (EngineError names the reason for an arena engine
        and use_puct=False).  reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_fpu(self._h, 1, float(reduction), float(root)))
        self.fpu = (float(reduction), float(root))

    def clear_fpu(self):
        """Back to the reference's Q = 0 for an unvisited child (az_engine_set_fpu with on = 0).  reset() or stream_begin()
        afterwards."""
        self._check(self.lib.az_engine_set_fpu(self._h, 0, 0.0, 0.0))
        self.fpu = None

    def set_resign(self, v, playthrough=0.1, min_ply=0):
        """Self-play resignation (az_engine_set_resign): from the next reset() / stream_begin() on, a game ends at its first
        RESIGN PLY - a qualifying ply (min_ply plies from the game's own start; a full search under a playout cap) whose criterion
        max(-root.Q, best visited child Q) lies below -v - with a loss for the player who moved there; the records are the plain
        game's up to and including that ply.  A game plays through all the same iff one Philox draw keyed by (seed, game id) is
        below `playthrough`; resign_info() tells per game the first resign ply, whether the game resigned or played through, and
        per player the lowest criterion seen - what resign.calibrate turns into a threshold.  v in (0, 1], playthrough in [0, 1],
        min_ply >= 0.  Plain self-play engines (EngineError names the reason for an arena or manual_moves engine).
        clear_resign() clears.  reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_resign(self._h, 1, float(v), float(playthrough), int(min_ply)))
        self.resign = (float(v), float(playthrough), int(min_ply))

    def clear_resign(self):
        """Every game is played to its end again (az_engine_set_resign with on = 0).  reset() or stream_begin() afterwards."""
        self._check(self.lib.az_engine_set_resign(self._h, 0, 0.0, 0.0, 0))
        self.resign = None

    def resign_info_device(self, first=0, n=None):
        """-> (ply int32 [n], flags uint8 [n], low float64 [n, 2]) device tensors: the resignation side information of games
        [first, first + n) (az_engine_resign_info_device) - the first resign ply (-1: none), bit 0 = resigned there / bit 1 = a
        play-through game, and per player the lowest criterion at a qualifying ply (+inf: none).  One kernel on the current
        stream, no host synchronisation.  n: default the last reset's games from `first` on; in stream mode name it, with ids
        inside the ring's window - and read BEFORE stream_take() hands the games' rows out again."""
        n = int(self.n_games - int(first) if n is None else n)
        ply = torch.empty((max(n, 0),), dtype=torch.int32, device=self.device)
        flags = torch.empty((max(n, 0),), dtype=torch.uint8, device=self.device)
        low = torch.empty((max(n, 0), 2), dtype=torch.float64, device=self.device)
        self._check(self.lib.az_engine_resign_info_device(self._h, int(first), n, C.c_void_p(ply.data_ptr()),
                                                          C.c_void_p(flags.data_ptr()), C.c_void_p(low.data_ptr()), self._stream()))
        return ply, flags, low

    def resign_info(self, first=0, n=None):
        """resign_info_device as numpy arrays: dict(ply int32 [n], resigned bool [n], playthrough bool [n], low float64 [n, 2])."""
        return unpack_resign_info(*self.resign_info_device(first, n))

    def set_arena_search(self, fpu=None, solver=False, eval_mirror=0.0):
        """Search settings of an arena AGENT (az_engine_set_arena_search): from the next reset() on the "zero" agent of an
        evaluation engine searches with first-play urgency (fpu=r or (r, r_root), as set_fpu), the MCTS-Solver (solver=True, as
        set_solver; a won root plays a proven win, a drawn root never a proven loss) and / or the evaluation mirror (eval_mirror=p,
        as set_eval_mirror) - what a match between two settings needs (arena.play_match).  Arena engines with agent "zero" under
        use_puct only (EngineError names the reason otherwise); set_arena_search() with nothing on clears all three.  reset()
        afterwards."""
        s = SearchSettings.from_kwargs(dict(fpu=fpu, solver=solver, eval_mirror=eval_mirror))
        rec = _lib.AzArenaSearch()
        rec.struct_size = C.sizeof(_lib.AzArenaSearch)
        rec.fpu_on = int(s.fpu is not None)
        rec.fpu_reduction, rec.fpu_reduction_root = s.fpu or (0.0, 0.0)
        rec.solver = int(bool(s.solver))
        rec.p_mirror = s.eval_mirror or 0.0
        self._check(self.lib.az_engine_set_arena_search(self._h, C.byref(rec)))
        on = s.fpu is not None or bool(s.solver) or rec.p_mirror > 0.0
        self.arena_search = dict(fpu=s.fpu, solver=bool(s.solver), eval_mirror=rec.p_mirror) if on else None

    def set_arena_openings(self, prefixes):
        """An opening per evaluation game (az_engine_set_arena_openings): game i of the next reset() starts after the action list
        prefixes[i]; the agent still plays player (i & 1) ^ arena_flip, whatever the opening's length.  Arena engines only.  An
        illegal action or a prefix that ends the game raises EngineError naming "game <i>" and an earlier table stays in force;
        reset(n <= len(prefixes)) afterwards; set_start_prefix returns to one start.  Both engines of a duel take the same list.
        export() then returns "start_ply" as an int32 array (game_starts)."""
        actions, lengths, stride = pack_histories(prefixes)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.az_engine_set_arena_openings(self._h, actions.ctypes.data_as(ip), lengths.ctypes.data_as(ip),
                                                          stride, len(lengths)))
        self._starts(histories=prefixes, game_starts=lengths.copy())

    def read_proofs(self, slot):
        """The proof status of every node of a slot's tree in the order of read_tree() (az_engine_read_proofs) -> int8 array:
        0 unknown, 1 win, 2 draw, 3 loss for the player who moved into the node.  All 0 without set_solver."""
        n = self._check(self.lib.az_engine_read_proofs(self._h, int(slot), None, 0))
        out = np.zeros(n, np.int8)
        self._check(self.lib.az_engine_read_proofs(self._h, int(slot), out.ctypes.data_as(C.POINTER(C.c_int8)), n))
        return out

    def export_proofs_device(self, buf=None):
        """Every slot's root status and root child statuses as a uint8 device tensor [n_slots, 1 + max_children] (column 0 the
        root, 0 beyond n_children) on the current stream: one kernel, no host synchronisation, may be captured in a graph."""
        if buf is None:
            buf = torch.empty((self.G, 1 + self.max_children), dtype=torch.uint8, device=self.device)
        elif buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device:
            raise EngineError("expected a contiguous uint8 tensor on %s" % (self.device,))
        self._check(self.lib.az_engine_export_proofs_device(self._h, C.c_void_p(buf.data_ptr()), int(buf.numel()), self._stream()))
        return buf

    def read_request_mirror(self, slot):
        """The orientation bit of the slot's outstanding request (az_engine_read_request_mirror): 1 = the observation in the
        request buffer is the mirrored position's; 0 with no setting in force.  EngineError unless the slot is in phase 3 or 4."""
        return int(self._check(self.lib.az_engine_read_request_mirror(self._h, int(slot))))

    def full_moves_device(self, n_games=None):
        """-> uint8 device tensor [n, max_plies] by absolute ply: 1 where a recorded ply was searched in full, 0 elsewhere (a
        fast move under a playout cap, a ply that was not played); all recorded plies give 1 without a cap.  What
        DeviceReplay.append_device(buf, n, keep=) and examples_from_export(keep=) take beside export_device() / export().
        n_games: default the last reset's."""
        n = int(self.n_games if n_games is None else n_games)
        full = torch.empty((n, self.max_plies), dtype=torch.uint8, device=self.device)
        self._check(self.lib.az_engine_full_moves_device(self._h, C.c_void_p(full.data_ptr()), n, self._stream()))
        return full

    def set_injected_rng(self, etas, us, absolute_ply=False):
        """etas: per game, per ply, the Dirichlet draw (ragged lists ok); us: per game, per ply uniforms.  Lists are
        indexed by plies played since the start position unless absolute_ply (then by the state's ply number)."""
        n = len(us)
        e = np.zeros((n, self.max_plies, self.max_children), dtype=np.float64)
        u = np.zeros((n, self.max_plies), dtype=np.float64)
        off = 0 if absolute_ply else len(self.start_history)
        for g in range(n):
            for i, row in enumerate(etas[g] if etas is not None else []):
                e[g, off + i, :len(row)] = row
            u[g, off:off + len(us[g])] = us[g]
        dp = C.POINTER(C.c_double)
        self._check(self.lib.az_engine_set_injected_rng(self._h, e.ctypes.data_as(dp), u.ctypes.data_as(dp), n))

    def _ptr(self, t, shape):
        if t is None:
            return None
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or tuple(t.shape) != shape:
            raise EngineError("expected a contiguous float32 %s tensor on %s, got %s %s on %s"
                              % (shape, self.device, t.dtype, tuple(t.shape), t.device))
        return C.c_void_p(t.data_ptr())

    def advance(self, priors, values, obs):
        """One tick: consume (priors, values) for last tick's requests, search on, write new requests to obs."""
        self._check(self.lib.az_engine_advance(self._h, self._ptr(priors, (self.G, self.A)),
                                               self._ptr(values, (self.G,)),
                                               self._ptr(obs, (self.G,) + self.obs_shape), self._stream()))

    def advance_slots(self, first_slot, n_slots, priors, values, obs):
        """The tick of slots [first_slot, first_slot + n_slots) only, on the current stream; priors / values / obs are the
        whole-engine tensors.  Disjoint slot groups may run concurrently on different streams (see run_selfplay(overlap=))."""
        self._check(self.lib.az_engine_advance_slots(self._h, int(first_slot), int(n_slots),
                                                     self._ptr(priors, (self.G, self.A)), self._ptr(values, (self.G,)),
                                                     self._ptr(obs, (self.G,) + self.obs_shape), self._stream()))

    def compact_rows(self):
        """Tail of a generation (every game handed out): list the slots that still play and switch the request buffers to
        dense rows -> the number of live slots.  Afterwards tick with advance_rows(n_rows >= that number, ...)."""
        n = C.c_int32(0)
        self._check(self.lib.az_engine_compact_rows(self._h, C.byref(n), self._stream()))
        return int(n.value)

    def advance_rows(self, n_rows, priors, values, obs):
        """One tick over the dense list: priors / values / obs are the whole-engine tensors, only their first n_rows rows
        are used (evaluate just those: evaluator(obs[:n_rows], priors[:n_rows], values[:n_rows]))."""
        self._check(self.lib.az_engine_advance_rows(self._h, int(n_rows), self._ptr(priors, (self.G, self.A)),
                                                    self._ptr(values, (self.G,)),
                                                    self._ptr(obs, (self.G,) + self.obs_shape), self._stream()))

    def opponent_moves(self):
        """Arena engines: let the opponent bot choose its move in every slot where it is to move (applied by the next advance)."""
        self._check(self.lib.az_engine_opponent_moves(self._h, self._stream()))

    def exchange_moves(self, other):
        """Two engines facing each other (opponent="external", arena_flip False / True): pass on the moves just played."""
        self._check(self.lib.az_engine_exchange_moves(self._h, other._h, self._stream()))

    def update_root(self, actions, keep_subtree=True):
        arr = (C.c_int32 * self.G)(*[int(a) for a in actions])
        self._check(self.lib.az_engine_update_root(self._h, arr, int(bool(keep_subtree)), self._stream()))

    def progress(self, check=True):
        p = _lib.AzProgress()
        rc = self.lib.az_engine_progress(self._h, C.byref(p), self._stream())
        if check:
            self._check(rc)
        return {name: getattr(p, name) for name, _ in _lib.AzProgress._fields_ if name != "reserved"}

    def games_done(self):
        """Cheap poll (two words) for the tick loop; raises on device faults like progress()."""
        done, flags = C.c_int64(), C.c_uint32()
        rc = self.lib.az_engine_poll(self._h, C.byref(done), C.byref(flags), self._stream())
        if rc < 0:
            self.progress()  # raises with the decoded fault names
            self._check(rc)
        return done.value

    def read_root(self, slot):
        mc = self.max_children
        rn, rq = C.c_int64(), C.c_double()
        acts, cn = (C.c_int32 * mc)(), (C.c_int64 * mc)()
        cq, cp = (C.c_double * mc)(), (C.c_double * mc)()
        n = self._check(self.lib.az_engine_read_root(self._h, slot, C.byref(rn), C.byref(rq), acts, cn, cq, cp))
        return {"N": rn.value, "Q": rq.value, "actions": list(acts[:n]), "cN": list(cn[:n]),
                "cQ": list(cq[:n]), "cP": list(cp[:n])}

    def read_slot(self, slot):
        s = _lib.AzSlotInfo()
        self._check(self.lib.az_engine_read_slot(self._h, slot, C.byref(s)))
        return {"phase": s.phase, "game_id": s.game_id, "ply": s.ply, "sims_done": s.sims_done, "root": s.root,
                "alloc": s.alloc, "bb": [s.bb[0], s.bb[1]], "leaf_bb": [s.leaf_bb[0], s.leaf_bb[1]],
                "leaf_ply": s.leaf_ply, "depth": s.depth}

    def read_root_noise(self, slot):
        """The Dirichlet vector a Philox engine staged with the slot's root request (az_engine_read_root_noise) -> float64
        array [max_children]; only the first n_legal entries belong to the draw.  EngineError unless the slot is in phase 3."""
        eta = np.zeros(self.max_children, dtype=np.float64)
        self._check(self.lib.az_engine_read_root_noise(self._h, int(slot), eta.ctypes.data_as(C.POINTER(C.c_double))))
        return eta

    def read_tree(self, slot):
        """Whole tree of a slot, breadth-first: dict of numpy arrays parent/action/N/Q/P."""
        n = self._check(self.lib.az_engine_read_tree(self._h, slot, 0, None, None, None, None, None))
        par, act = np.zeros(n, np.int32), np.zeros(n, np.int32)
        N, Q, P = np.zeros(n, np.int64), np.zeros(n, np.float64), np.zeros(n, np.float64)
        ip, lp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        self._check(self.lib.az_engine_read_tree(self._h, slot, n, par.ctypes.data_as(ip), act.ctypes.data_as(ip),
                                                 N.ctypes.data_as(lp), Q.ctypes.data_as(dp), P.ctypes.data_as(dp)))
        return {"parent": par, "action": act, "N": N, "Q": Q, "P": P}

    def export(self):
        """Finished games as numpy arrays (copies)."""
        v = _lib.AzExampleView()
        self._check(self.lib.az_engine_export(self._h, C.byref(v), self._stream()))
        n, mp, mc = v.n_games, v.max_plies, v.max_children

        def arr(ptr, shape, dtype):
            cnt = int(np.prod(shape))
            return np.ctypeslib.as_array(ptr, shape=(cnt,)).view(dtype).reshape(shape).copy()

        return {
            "game_len": arr(v.game_len, (n,), np.int32), "game_ret0": arr(v.game_ret0, (n,), np.float32),
            "states": arr(v.states, (n, mp, 2), np.uint64), "move": arr(v.move, (n, mp), np.uint16),
            "n_children": arr(v.n_children, (n, mp), np.uint8),
            "child_action": arr(v.child_action, (n, mp, mc), np.uint16),
            "child_visits": arr(v.child_visits, (n, mp, mc), np.uint32),
            "value": arr(v.value, (n, mp), np.float64),
            "start_ply": len(self.start_history) if self.game_starts is None else self.game_starts[:n].copy(),
        }


    def export_device(self):
        """Finished games of the generation packed into one uint8 device tensor (layout: include/az_engine.h,
        az_engine_export_device) - the payload of the generation-end all-gather and of DeviceReplay.append_device."""
        nbytes = self._check(self.lib.az_engine_export_device_bytes(self._h))
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        self._check(self.lib.az_engine_export_device(self._h, C.c_void_p(buf.data_ptr()), int(nbytes), self._stream()))
        return buf


    # ------------------------------------------------------------------ stream mode (include/az_engine.h)
    def stream_begin(self, seed=None):
        """Start an open-ended run instead of reset(n_games): game ids 0, 1, 2, ..., records in a ring of max_games rows.
        Plain self-play engines only (EngineError names the reason otherwise); reset() returns to a closed generation."""
        if seed is None:
            seed = self.cfg.seed
        self._check(self.lib.az_engine_stream_begin(self._h, int(seed) & (2 ** 64 - 1), self._stream()))
        self.n_games = 0

    def stream_ready(self):
        """Finished games in id order that have not been taken yet (at most max_games); synchronises the current stream."""
        return int(self._check(self.lib.az_engine_stream_ready(self._h, self._stream())))

    def stream_take_bytes(self, n_games):
        return int(self._check(self.lib.az_engine_stream_take_bytes(self._h, int(n_games))))

    def stream_take(self, n_games, out=None):
        """The next n_games finished games -> (uint8 device tensor in the packed layout of export_device() for a generation of
        n_games games, id of the first one).  One kernel on the current stream; call stream_ready() first.
        out: a uint8 device tensor to pack into (at least stream_take_bytes(n_games) bytes) instead of a fresh one."""
        if out is None:
            out = torch.empty(self.stream_take_bytes(n_games), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise EngineError("expected a contiguous uint8 tensor on %s" % (self.device,))
        first = C.c_int64(-1)
        self._check(self.lib.az_engine_stream_take_device(self._h, int(n_games), C.c_void_p(out.data_ptr()), int(out.numel()),
                                                          C.byref(first), self._stream()))
        return out, int(first.value)

    def roots_device_bytes(self):
        return int(self._check(self.lib.az_engine_roots_device_bytes(self._h)))

    def alloc_roots(self):
        """A uint8 device tensor that holds one root export (layout: roots_export_layout)."""
        return torch.empty(self.roots_device_bytes(), dtype=torch.uint8, device=self.device)

    def export_roots_device(self, buf):
        """Pack every slot's root into `buf` (alloc_roots()) on the current stream: one kernel, no host synchronisation, may
        be captured in a graph.  buf[:16] is the header: int32 {slots in phase 5 or idle, n_slots, max_children, error_flags}."""
        if buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device:
            raise EngineError("expected a contiguous uint8 tensor on %s" % (self.device,))
        self._check(self.lib.az_engine_export_roots_device(self._h, C.c_void_p(buf.data_ptr()), int(buf.numel()), self._stream()))
        return buf

    def read_roots(self, buf=None):
        """The root of EVERY slot from one kernel and one device-to-host copy: dict of numpy arrays game_id / phase / ply /
        sims_done / n_children [G], root_n [G] int64, root_q [G] float64, child_action [G, mc] int32 (-1 beyond n_children),
        child_n [G, mc] int64, child_q / child_p [G, mc] float64, plus n_finished and error_flags from the header.  Row for
        row what read_slot / read_root return for one slot per (synchronising) call."""
        buf = self.export_roots_device(self.alloc_roots() if buf is None else buf)
        return unpack_roots_export(buf.cpu().numpy(), self.G, self.max_children)

    def lines_device_bytes(self, max_depth):
        if not 1 <= int(max_depth) <= self.max_plies:
            raise EngineError("max_depth %d is outside [1, max_plies = %d]" % (int(max_depth), self.max_plies))
        return int(self._check(self.lib.az_engine_lines_device_bytes(self._h, int(max_depth))))

    def export_lines_device(self, max_depth, buf=None):
        """Pack the greedy line of every slot's finished search (the principal variation, and the off-policy value target A0GB
        at its end) into `buf` (default: a fresh uint8 device tensor; layout: lines_export_layout) on the current stream: one
        kernel, no host synchronisation, may be captured in a graph.  max_depth = the steps kept per line, 1..max_plies; depth
        and value are those of the whole line whatever it is."""
        if buf is None:
            buf = torch.empty(self.lines_device_bytes(max_depth), dtype=torch.uint8, device=self.device)
        elif buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device:
            raise EngineError("expected a contiguous uint8 tensor on %s" % (self.device,))
        self._check(self.lib.az_engine_export_lines_device(self._h, int(max_depth), C.c_void_p(buf.data_ptr()), int(buf.numel()),
                                                           self._stream()))
        return buf


def unpack_resign_info(ply, flags, low):
    """The three tensors of SelfPlayEngine.resign_info_device -> the dict of SelfPlayEngine.resign_info (host copies)."""
    flags = flags.cpu().numpy()
    return {"ply": ply.cpu().numpy(), "resigned": (flags & 1) != 0, "playthrough": (flags & 2) != 0, "low": low.cpu().numpy()}


def pack_histories(histories):
    """Action lists -> (actions int32 [n, stride], lengths int32 [n], stride): the arguments of az_engine_set_start_positions."""
    lengths = np.asarray([len(h) for h in histories], dtype=np.int32)
    stride = max(1, int(lengths.max()) if len(lengths) else 1)
    actions = np.zeros((len(lengths), stride), dtype=np.int32)
    for i, h in enumerate(histories):
        actions[i, :len(h)] = [int(a) for a in h]
    return actions, lengths, stride


def _packed_layout(spec):
    """(name, dtype, shape) per array -> ([(name, dtype, shape, byte offset)], total bytes), every array 16-byte aligned."""
    out, off = [], 0
    for name, dt, shape in spec:
        out.append((name, dt, shape, off))
        off += (int(np.prod(shape)) * np.dtype(dt).itemsize + 15) & ~15
    return out, off


def roots_export_layout(n_slots, max_children):
    """(name, dtype, shape, byte offset) of every array in the packed root export (include/az_engine.h,
    az_engine_export_roots_device) + total bytes."""
    G, mc = int(n_slots), int(max_children)
    spec = (("header", np.int32, (4,)), ("game_id", np.int32, (G,)), ("phase", np.int32, (G,)), ("ply", np.int32, (G,)),
            ("sims_done", np.int32, (G,)), ("n_children", np.int32, (G,)), ("root_n", np.uint32, (G,)),
            ("root_q", np.float64, (G,)), ("child_action", np.int32, (G, mc)), ("child_n", np.uint32, (G, mc)),
            ("child_q", np.float64, (G, mc)), ("child_p", np.float64, (G, mc)))
    return _packed_layout(spec)


def unpack_roots_export(host_bytes, n_slots, max_children):
    """A host copy of a packed root export -> the dict SelfPlayEngine.read_roots() returns."""
    host_bytes = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    layout, total = roots_export_layout(n_slots, max_children)
    if host_bytes.size < total:
        raise ValueError("root export buffer holds %d bytes, layout needs %d" % (host_bytes.size, total))
    out = {}
    for name, dt, shape, off in layout:
        cnt = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = host_bytes[off:off + cnt].view(dt).reshape(shape)
    hdr = out.pop("header")
    if int(hdr[1]) != int(n_slots) or int(hdr[2]) != int(max_children):
        raise ValueError("root export header says %d slots x %d children, expected %d x %d"
                         % (hdr[1], hdr[2], n_slots, max_children))
    out["n_finished"], out["error_flags"] = int(hdr[0]), int(hdr[3]) & 0xFFFFFFFF
    out["root_n"] = out["root_n"].astype(np.int64)
    out["child_n"] = out["child_n"].astype(np.int64)
    return out


def lines_export_layout(n_slots, max_depth):
    """(name, dtype, shape, byte offset) of every array in the packed line export (include/az_engine.h,
    az_engine_export_lines_device) + total bytes."""
    G, D = int(n_slots), int(max_depth)
    spec = (("header", np.int32, (4,)), ("game_id", np.int32, (G,)), ("phase", np.int32, (G,)), ("ply", np.int32, (G,)),
            ("depth", np.int32, (G,)), ("leaf_n", np.uint32, (G,)), ("value", np.float64, (G,)),
            ("line_action", np.int32, (G, D)), ("line_n", np.uint32, (G, D)), ("line_q", np.float64, (G, D)))
    return _packed_layout(spec)


def read_lines(buf):
    """A packed line export (SelfPlayEngine.export_lines_device; a uint8 device tensor, or a host copy of one) -> dict of numpy
    arrays game_id / phase / ply / depth [G], leaf_n [G] int64, value [G] float64, line_action [G, D] int32 (-1 beyond the
    line), line_n [G, D] int64, line_q [G, D] float64, plus n_finished, max_depth and error_flags from the header (which also
    gives G and D)."""
    host = buf.cpu().numpy() if torch.is_tensor(buf) else buf
    host = np.ascontiguousarray(host, dtype=np.uint8).reshape(-1)
    if host.size < 16:
        raise ValueError("line export buffer holds %d bytes, not even the header" % host.size)
    hdr = host[:16].view(np.int32)
    G, D = int(hdr[1]), int(hdr[2])
    if G < 1 or D < 1:
        raise ValueError("line export header says %d slots x depth %d" % (G, D))
    layout, total = lines_export_layout(G, D)
    if host.size < total:
        raise ValueError("line export buffer holds %d bytes, its header's layout needs %d" % (host.size, total))
    out = {}
    for name, dt, shape, off in layout:
        cnt = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = host[off:off + cnt].view(dt).reshape(shape)
    out.pop("header")
    out["n_finished"], out["max_depth"], out["error_flags"] = int(hdr[0]), D, int(hdr[3]) & 0xFFFFFFFF
    out["leaf_n"] = out["leaf_n"].astype(np.int64)
    out["line_n"] = out["line_n"].astype(np.int64)
    return out


def device_export_layout(n_games, max_plies, max_children):
    """(name, dtype, shape, byte offset) of every array in the packed device export (csrc/az_records.h) + total bytes."""
    n, mp, mc = int(n_games), int(max_plies), int(max_children)
    spec = (("game_len", np.int32, (n,)), ("game_ret0", np.float32, (n,)), ("states", np.uint64, (n, mp, 2)),
            ("move", np.uint16, (n, mp)), ("n_children", np.uint8, (n, mp)), ("child_action", np.uint16, (n, mp, mc)),
            ("child_visits", np.uint32, (n, mp, mc)), ("value", np.float64, (n, mp)))
    return _packed_layout(spec)


def unpack_device_export(host_bytes, n_games, max_plies, max_children, start_ply=0):
    """A host copy of a packed device export -> the dict engine.export() returns (arrays are views).
    start_ply: one start ply for every game, or an array [n_games] (a generation with a start per game)."""
    host_bytes = np.ascontiguousarray(host_bytes, dtype=np.uint8)
    layout, total = device_export_layout(n_games, max_plies, max_children)
    if host_bytes.size < total:
        raise ValueError("export buffer holds %d bytes, layout needs %d" % (host_bytes.size, total))
    ex = {"start_ply": int(start_ply) if np.ndim(start_ply) == 0 else np.asarray(start_ply, dtype=np.int32).reshape(-1)}
    for name, dt, shape, off in layout:
        cnt = int(np.prod(shape)) * np.dtype(dt).itemsize
        ex[name] = host_bytes[off:off + cnt].view(dt).reshape(shape)
    return ex


# ---------------------------------------------------------------------- host logic on engine records
def pi_from_visits(actions, visits, num_actions):
    """MCTS.get_normalized_visit_counts + remove_illegal_actions (mcts.py:155-162, alphazerobot.py:7-18)
    from the recorded root child visit counts, with numpy's own arithmetic -> list[A] of python floats."""
    total = int(np.sum(visits.astype(np.int64)))
    nv = np.zeros(num_actions, dtype=np.float64)
    nv[actions] = visits.astype(np.float64) / float(total)
    s = np.sum(nv)
    if s > 1e-6:
        nv = nv / s
    else:
        nv = np.zeros(num_actions)
        nv[actions] = 1.0 / len(actions)
    return nv.tolist()


def pis_from_visits(actions, visits, n_children, num_actions):
    """pi_from_visits for many recorded plies at once: actions / visits [n, max_children], n_children [n] -> float64 [n, A].
    Row for row the same IEEE operations in the same order (numpy reduces a C-contiguous last axis with the pairwise sum it
    uses for a 1-D array; tests/test_host_logic.py checks the rows against pi_from_visits bit for bit)."""
    n, mc = visits.shape
    live = np.arange(mc)[None, :] < np.asarray(n_children).reshape(-1, 1)
    v = np.where(live, visits, 0).astype(np.int64)
    total = v.sum(axis=1)
    frac = v.astype(np.float64) / np.where(total > 0, total, 1).astype(np.float64)[:, None]
    rows = np.repeat(np.arange(n), mc).reshape(n, mc)
    nv = np.zeros((n, num_actions), dtype=np.float64)
    nv[rows[live], actions.astype(np.int64)[live]] = frac[live]
    s = np.sum(nv, axis=1)
    ok = s > 1e-6
    out = np.zeros_like(nv)
    out[ok] = nv[ok] / s[ok][:, None]
    if not ok.all():  # no visit mass on any legal action: uniform over the children (alphazerobot.py:15-17)
        bad = ~ok & (np.asarray(n_children).reshape(-1) > 0)
        uni = np.zeros_like(nv)
        cnt = np.asarray(n_children).reshape(-1).astype(np.float64)
        sel = live & bad[:, None]
        uni[rows[sel], actions.astype(np.int64)[sel]] = np.repeat(1.0 / cnt[bad], np.asarray(n_children).reshape(-1)[bad])
        out[bad] = uni[bad]
    return out


def examples_from_export(game, ex, start_history=(), keep=None):
    """Engine records -> the reference's list of games, each a list of `[info_state_str, board (C+1,H,W)
    float64, pi list[A], value]` (game_utils.py:169,200-204; consumed by train.py:109-126,172-198).
    All plies of all games are converted in bulk (one numpy pass for boards, one for pi); what remains per example is
    building its 4-element list.
    keep: an array [G, max_plies] by absolute ply (SelfPlayEngine.full_moves_device, a playout cap's mask) - only plies with a
    non-zero entry become examples; the others are dropped from the lists, while the key strings still run over every move
    and the values stay those of the plies' own (absolute) numbers."""
    A = game.num_distinct_actions()
    lens = np.asarray(ex["game_len"]).astype(np.int64)
    G = len(lens)
    if G == 0:
        return []
    # a start per game (SelfPlayEngine.set_game_starts): "start_ply" is an array [G] and start_history a list of G histories
    p0 = np.asarray(ex["start_ply"]).astype(np.int64).reshape(-1, 1) if np.ndim(ex["start_ply"]) else int(ex["start_ply"])
    per_game = len(start_history) > 0 and isinstance(start_history[0], (list, tuple, np.ndarray))
    if np.ndim(ex["start_ply"]) and not per_game:
        # (after set_game_starts_device the histories are not known - start_histories is None: there are no key strings to build)
        raise ValueError("a start ply per game needs a start history per game: the key strings are prefix + moves")
    if per_game and len(start_history) < G:
        raise ValueError("%d games but %d start histories" % (G, len(start_history)))
    mp = ex["move"].shape[1]
    ply = np.arange(mp)[None, :]
    valid = (ply >= p0) & (ply < p0 + lens[:, None])           # [G, mp], row-major = game by game, ply by ply
    kept = valid if keep is None else valid & (np.asarray(keep).reshape(valid.shape) != 0)
    boards = boards_from_bitboards(game, ex["states"][kept], np.broadcast_to(ply, kept.shape)[kept])
    pis = pis_from_visits(ex["child_action"][kept], ex["child_visits"][kept], ex["n_children"][kept], A).tolist()
    values = ex["value"][kept].tolist()
    moves = ex["move"][valid].tolist()
    is_kept = kept[valid].tolist()
    prefixes = [", ".join(str(int(a)) for a in h) for h in (start_history if per_game else [start_history])]
    games, k, j = [], 0, 0  # k: the ply among the valid ones, j: among the kept ones
    for g, n in enumerate(lens.tolist()):
        key, plies = prefixes[g if per_game else 0], []
        for i in range(k, k + n):
            if is_kept[i]:
                plies.append([key, boards[j], pis[j], values[j]])
                j += 1
            key = (key + ", " if key else "") + str(moves[i])
        games.append(plies)
        k += n
    return games


# ---------------------------------------------------------------------- evaluation of the request batch
class DeviceEvaluator:
    """The engine-side replacement of Evaluator + handle_gpu (examplegenerator.py:39-77): one
    `net.forward` over the whole device-resident request batch, no pipes, no host copies.
    dtype: torch.float32 (reference arithmetic) or torch.float16 / torch.bfloat16 autocast."""

    def __init__(self, net, device, dtype=torch.float32, channels_last=False):
        # a private copy: the caller's module (a Trainer's current_net) keeps its device and its train/eval mode
        self.net = copy.deepcopy(net).to(device).eval()
        self.device = torch.device(device)
        self.dtype = dtype
        self.channels_last = channels_last
        if channels_last:
            self.net = self.net.to(memory_format=torch.channels_last)

    @torch.no_grad()
    def __call__(self, obs, priors_out, values_out):
        x = obs.contiguous(memory_format=torch.channels_last) if self.channels_last else obs
        if self.dtype == torch.float32:
            p, v = self.net(x)
        else:
            with torch.autocast("cuda", dtype=self.dtype):
                p, v = self.net(x)
        priors_out.copy_(p)
        values_out.copy_(v.reshape(-1))


class HostPolicyEvaluator:
    """Routes requests through a reference-style `policy_fn(state) -> (priors, value)` on the host
    (Evaluator.evaluate_nn's contract, examplegenerator.py:44-54).  Slow by construction — it exists for
    parity tests and for AlphaZeroBot(policy_fn=<python callable>)."""

    def __init__(self, engine, board_fn):
        """board_fn(board float64 (C+1,H,W)) -> (priors[A], value)"""
        self.engine = engine
        self.board_fn = board_fn

    def __call__(self, obs, priors_out, values_out):
        e = self.engine
        boards = obs.detach().cpu().numpy().astype(np.float64)
        n = boards.shape[0]  # all slots, or the dense rows of a thinned-out generation
        pri = np.empty((n, e.A), dtype=np.float32)
        val = np.empty((n,), dtype=np.float32)
        for g in range(n):
            p, v = self.board_fn(boards[g])
            pri[g] = np.asarray(p, dtype=np.float32)
            val[g] = np.float32(v)
        priors_out.copy_(torch.from_numpy(pri))
        values_out.copy_(torch.from_numpy(val))


def module_of(policy_fn):
    """The nn.Module behind a policy_fn: the module itself or the owner of a bound `.predict`; None for any other callable."""
    if isinstance(policy_fn, torch.nn.Module):
        return policy_fn
    owner = getattr(policy_fn, "__self__", None)
    if isinstance(owner, torch.nn.Module) and getattr(policy_fn, "__name__", "") == "predict":
        return owner
    return None


def default_device(policy_fn):
    """Where to run when the caller names no device: the network's, if it has a parameter and that is on a GPU, else the
    current HIP device."""
    mod = module_of(policy_fn)
    par = next(mod.parameters(), None) if mod is not None else None
    return par.device if par is not None and par.is_cuda else torch.device("cuda", torch.cuda.current_device())


def make_evaluator(net_or_fn, device, backend, precision, max_boards, dtype=torch.float32):
    """The device evaluator of a network: backend "fused" = FusedNet (csrc/az_net.hip) at `precision` for up to max_boards
    rows, anything else = DeviceEvaluator (torch forward) at `dtype`."""
    mod = module_of(net_or_fn)
    if mod is None:
        raise TypeError("the device arena needs the network itself (an nn.Module or its bound .predict), not an arbitrary "
                        "python policy_fn")
    if backend == "fused":
        from .fusednet import FusedNet
        return FusedNet(mod, device, max_boards=max_boards, precision=precision)
    return DeviceEvaluator(mod, device, dtype=dtype)


def close_all(*things, drain=False):
    """close() whatever has one (engines, FusedNets; a DeviceEvaluator and None have none), in the order given.
    drain: wait for each thing's device first (a pool that raised leaves the others' enqueued batches behind)."""
    for t in things:
        if drain:
            try:
                torch.cuda.synchronize(t.device)
            except Exception:
                pass
        if hasattr(t, "close"):
            t.close()


# ---------------------------------------------------------------------- the tick loop
class TickDriver:
    """Enqueues ticks on the current stream, eagerly or as replays of a captured HIP graph, and counts them.
    tick: zero-argument callable, what one tick launches (e.g. [az_engine_advance, PV-net forward])."""

    def __init__(self, device, tick):
        self.device, self.tick = device, tick
        self.ticks = 0
        self.graph, self.tpg = None, 1  # tpg: ticks per graph

    def _eager(self, n):
        for _ in range(n):
            self.tick()
        self.ticks += n

    def _capture(self):
        torch.cuda.synchronize(self.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for _ in range(self.tpg):
                self.tick()

    def capture(self, ticks_per_graph=1):
        """From now on run() replays a graph of ticks_per_graph ticks.  Two eager ticks first, on a side stream: MIOpen /
        workspace allocation and the kernels' first-use attribute calls must happen outside capture."""
        self.tpg = max(1, int(ticks_per_graph))
        main = torch.cuda.current_stream(self.device)
        torch.cuda.synchronize(self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self._eager(2)
        main.wait_stream(side)
        self._capture()

    def recapture(self):
        """Capture again after what tick() launches has changed (a new row count).  One eager tick first: new kernel
        variants set their attributes on first use, which must not happen inside a capture."""
        self._eager(1)
        self._capture()

    def run(self, n):
        """n ticks' worth: n eager ticks, or max(1, n // ticks_per_graph) replays."""
        if self.graph is None:
            return self._eager(n)
        for _ in range(max(1, n // self.tpg)):
            self.graph.replay()
            self.ticks += self.tpg


def tick_until(driver, check_every, done, max_ticks, what, *engines):
    """driver.run(check_every) until done() says so after a batch; EngineError with the engines' progress once
    driver.ticks >= max_ticks (None: no limit)."""
    while True:
        driver.run(check_every)
        if done():
            return
        if max_ticks is not None and driver.ticks >= max_ticks:
            raise EngineError("%s did not finish within %d ticks: %s"
                              % (what, max_ticks, " / ".join(repr(e.progress()) for e in engines)))


def stream_take_layout(n_games, max_plies, max_children):
    """(name, dtype, shape, byte offset) of every array in a take of n_games games off a stream + total bytes: the packed
    device export of a generation of n_games games (device_export_layout), by construction."""
    return device_export_layout(n_games, max_plies, max_children)


class SelfPlayStream:
    """Continuous self-play: an engine in stream mode (az_engine_stream_begin), its request buffers and ONE tick driver.
    Slots never wait for the end of a generation: a finished slot takes the next game id at once, and take(n) hands the next n
    finished games over, in id order, while the others play on.  With an unchanged net the games are, id for id, those of the
    closed generation run_selfplay plays from the same seed.

    set_evaluator(ev) swaps the network between takes.  Games in flight go on under the new network from the next tick and
    keep their search trees - a game that straddles the swap was searched partly with the old and partly with the new net
    (the usual semantics of asynchronous self-play, and the one place where a streamed game is not what a closed generation
    would have played).

    forced_playouts=k or (k, prune): SelfPlayEngine.set_forced_playouts before the stream begins (an engine that already carries
    the setting streams with it as well: the pruned counts travel in the records themselves).
    eval_mirror=p: SelfPlayEngine.set_eval_mirror before the stream begins (an engine that already carries the setting streams
    with it as well).
    solver=True / False: SelfPlayEngine.set_solver before the stream begins (None leaves the engine's setting as it is).
    fpu=r or (r, r_root): SelfPlayEngine.set_fpu before the stream begins (None leaves the engine's setting as it is).
    resign=v, (v, playthrough) or (v, playthrough, min_ply): SelfPlayEngine.set_resign before the stream begins (None leaves the
    engine's setting as it is).  While the engine carries the setting, take() reads the resignation side information of the
    games it takes BEFORE it takes them (their rows are handed out again afterwards) and keeps it on last_resign_info: the
    device tensors (ply, flags, low) of SelfPlayEngine.resign_info_device, None without the setting."""

    def __init__(self, engine, evaluator, seed=None, use_graph=True, ticks_per_graph=16, check_every=32, forced_playouts=None,
                 eval_mirror=None, solver=None, fpu=None, resign=None):
        self.engine, self.evaluator = engine, evaluator
        self.use_graph, self.check_every = bool(use_graph), max(1, int(check_every))
        self.ticks_per_graph = min(max(1, int(ticks_per_graph)), self.check_every)
        SearchSettings.from_kwargs(dict(forced_playouts=forced_playouts, eval_mirror=eval_mirror, solver=solver, fpu=fpu, resign=resign),
                                   off="clear").apply(engine)  # (None leaves the engine's setting, an off value clears it)
        self.last_resign_info = None
        engine.stream_begin(seed)
        self.obs, self.pri, self.val = engine.alloc_io()
        self.taken = 0          # games handed over so far = the id of the next one
        self.idle_sum = 0       # sum over the checks of the slots found stalled (only counted when count_idle)
        self.checks = 0
        self.count_idle = False  # measurement aid: a full progress() per check
        self.captures = 0
        self.driver = TickDriver(engine.device, self._tick)
        if self.use_graph:
            self.driver.capture(self.ticks_per_graph)
            self.captures += 1

    def _tick(self):
        self.engine.advance(self.pri, self.val, self.obs)
        self.evaluator(self.obs, self.pri, self.val)

    @property
    def ticks(self):
        return self.driver.ticks

    def set_evaluator(self, evaluator):
        """Play on with another network.  Synchronises the device and captures the tick graph again (a graph holds the
        evaluator's kernels and buffers); the caller closes the old evaluator afterwards."""
        torch.cuda.synchronize(self.engine.device)
        self.evaluator = evaluator
        if self.driver.graph is not None:
            self.driver.graph = None
            self.driver.recapture()
            self.captures += 1

    def take(self, n_games, max_ticks=None, out=None):
        """Tick in batches of check_every until n_games games are ready, then -> (packed uint8 device tensor, id of the first
        game): SelfPlayEngine.stream_take.  max_ticks bounds the ticks spent in THIS call (EngineError with the engine's
        progress beyond it)."""
        e, n = self.engine, int(n_games)
        if n < 1 or n > e.sizes.max_games:
            raise ValueError("take(%d): a take holds between 1 and max_games = %d games" % (n, e.sizes.max_games))
        start = self.driver.ticks

        def ready():  # the two-word poll first: the ring is scanned only once enough games have finished
            self.checks += 1
            if self.count_idle:
                self.idle_sum += e.progress()["slots_idle"]
            return e.games_done() - self.taken >= n and e.stream_ready() >= n

        if not ready():  # (games may be waiting already: after a larger capacity filled up, or when taking a few at a time)
            tick_until(self.driver, self.check_every, ready, None if max_ticks is None else start + int(max_ticks),
                       "take(%d) off the self-play stream" % n, e)
        if getattr(e, "resign", None) is not None:  # (first: the take frees the rows, and the next tick may hand them out)
            self.last_resign_info = e.resign_info_device(self.taken, n)
        buf, first = e.stream_take(n, out)
        self.taken = first + n
        return buf, first

    def close(self):
        """Drain the stream (the ticks in flight use the request buffers and the evaluator); the caller closes engine and
        evaluator afterwards."""
        if self.engine is not None:
            torch.cuda.synchronize(self.engine.device)
        self.driver = None
        self.engine = self.evaluator = None
        self.obs = self.pri = self.val = None


def stream_capacity(n_local, n_slots, capacity=None):
    """Rows of the record ring behind ExampleGenerator(continuous=True): by default the n_local games a call takes plus two
    per slot (one in play, one finished and waiting for the take); never fewer than the slots or than one call's games."""
    cap = int(n_local) + 2 * int(n_slots) if capacity is None else int(capacity)
    if cap < max(int(n_local), int(n_slots)):
        raise ValueError("stream capacity %d is smaller than a call's %d games or the %d slots" % (cap, n_local, n_slots))
    return cap


def check_stream_request(n_local, capacity):
    """A later call may ask for another number of games while it fits the ring."""
    if int(n_local) > int(capacity):
        raise ValueError("continuous=True: %d games per call exceed the stream's capacity of %d games (fixed by the first call)"
                         % (n_local, capacity))
    return int(n_local)


def slot_groups(n_slots, k):
    """Split [0, n_slots) into k contiguous groups whose sizes are multiples of 8 (a tower workgroup evaluates 8 boards)."""
    per = -(-n_slots // max(1, int(k)))
    per = -(-per // 8) * 8
    groups, first = [], 0
    while first < n_slots:
        groups.append((first, min(per, n_slots - first)))
        first += per
    return groups


def _tail_levels(n_slots):
    """Row counts worth switching to as a generation thins out.  The fused towers run 256 workgroups per round: the fp32-grade
    one (the default) takes 511 / 276 / 150 us at 4096 / 2048 / 1024 boards with a board per wave, and 120 / 67 us at 512 / 256
    with a board per workgroup (az_tower_x3c_kernel; profiles/r3_tower_vs_boards.txt) - so halve down to 256 rows."""
    return [n for n in (n_slots // 2, n_slots // 4, n_slots // 8, n_slots // 16) if n >= 256]


def run_selfplay(engine, evaluator, n_games, seed=None, check_every=32, max_ticks=None, use_graph=False,
                 on_tick=None, overlap=1, ticks_per_graph=16, compact_tail=True):
    """ExampleGenerator.run_games without processes: tick the engine until n_games are finished.
    Returns the final progress dict.

    overlap = k > 1 (BASELINE.json configs[4]: "overlapped PV-eval / tree-search HIP streams"): the slots are split into k
    groups, each with its own HIP stream (and graph) ticking [az_engine_advance_slots, PV-net forward of the group]; a
    group's tree search and launch gaps then run beside another group's forward.  `evaluator` must then be a list of k
    evaluators, one per group (a FusedNet owns its intermediate buffers).  The games do not depend on the grouping:
    random streams are keyed by game id.

    compact_tail: once every game has been handed to a slot the batch thins out (a generation lasts as long as its longest
    game); when at most half / a quarter of the slots still play, the engine switches to dense request rows
    (az_engine_compact_rows / az_engine_advance_rows) and the network evaluates only those rows.  The games are the same
    (a board's evaluation does not depend on its row)."""
    if overlap > 1:
        return _run_selfplay_overlapped(engine, evaluator, n_games, seed, check_every, max_ticks, use_graph, overlap)
    steps = selfplay_steps(engine, evaluator, n_games, seed, check_every, max_ticks, use_graph, on_tick, ticks_per_graph, compact_tail)
    while True:
        try:
            next(steps)
        except StopIteration as stop:
            return stop.value


def run_selfplay_pools(engines, evaluators, n_games_each, **kw):
    """k engines - one per "pool" of the reference (examplegenerator.py:140-162: n_pools = the amount of GPUs to utilize), each on
    its own device - driven from ONE host thread: every pass enqueues a batch of ticks on each device and only then waits for
    the batch before, so the devices run side by side.  -> list of the final progress dicts."""
    gens = [selfplay_steps(e, ev, n_games_each, **kw) for e, ev in zip(engines, evaluators)]
    out = [None] * len(gens)
    live = list(range(len(gens)))
    while live:
        for i in list(live):
            try:
                with torch.cuda.device(engines[i].device):
                    next(gens[i])
            except StopIteration as stop:
                out[i] = stop.value
                live.remove(i)
    return out


def selfplay_steps(engine, evaluator, n_games, seed=None, check_every=32, max_ticks=None, use_graph=False, on_tick=None,
                   ticks_per_graph=16, compact_tail=True):
    """Generator form of run_selfplay (one stream): yields after every batch of enqueued ticks, BEFORE it waits for them;
    the final progress dict is the generator's return value."""
    engine.reset(n_games, seed)
    obs, pri, val = engine.alloc_io()
    n_first = min(int(n_games), engine.G)  # games handed out by the reset
    levels = _tail_levels(engine.G) if (compact_tail and on_tick is None) else []
    rows = None  # None: one row per slot

    def tick():
        if rows is None:
            engine.advance(pri, val, obs)
            evaluator(obs, pri, val)
        else:
            engine.advance_rows(rows, pri, val, obs)
            evaluator(obs[:rows], pri[:rows], val[:rows])

    drv = TickDriver(engine.device, tick)
    if use_graph:
        # several ticks per captured graph: fewer graph-boundary bubbles on the stream (+2-3 % games/s at 8-16)
        drv.capture(1 if on_tick is not None else min(int(ticks_per_graph), check_every))
    compactions = 0
    while True:
        if on_tick is None:
            drv.run(check_every)
        else:
            for _ in range(check_every):
                drv.run(1)
                on_tick(engine, drv.ticks)
        yield drv.ticks  # (a driver of several engines enqueues the others' batches here)
        done = engine.games_done()
        if done >= n_games:
            break
        if max_ticks is not None and drv.ticks >= max_ticks:
            raise EngineError("self-play did not finish within %d ticks: %r" % (max_ticks, engine.progress()))
        # the tail: every game handed out (a finished slot took the next id until they ran out) and few slots still playing
        if levels and min(n_games, n_first + done) >= n_games and n_games - done <= levels[0]:
            live = engine.compact_rows()
            while levels and live <= levels[0]:
                rows = levels.pop(0)
            compactions += 1
            if drv.graph is not None:
                drv.recapture()  # for the new row count
    prog = engine.progress()
    prog["ticks"] = drv.ticks
    prog["tail_compactions"] = compactions
    return prog


class OverlappedTicker:
    """k slot groups of one engine, each ticking on its own HIP stream (optionally as a captured graph)."""

    def __init__(self, engine, evaluators, overlap, use_graph=True, io=None):
        self.engine = engine
        self.groups = slot_groups(engine.G, overlap)
        if not isinstance(evaluators, (list, tuple)) or len(evaluators) != len(self.groups):
            raise ValueError("overlap=%d needs a list of %d evaluators (one per slot group), got %r"
                             % (overlap, len(self.groups), type(evaluators)))
        self.evaluators = list(evaluators)
        self.obs, self.pri, self.val = io if io is not None else engine.alloc_io()
        dev = engine.device
        self.streams = [torch.cuda.Stream(dev) for _ in self.groups]
        self.graphs = []
        torch.cuda.synchronize(dev)
        main = torch.cuda.current_stream(dev)
        for i, st in enumerate(self.streams):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                for _ in range(2):  # warm-up outside capture
                    self._tick(i)
            st.synchronize()
            if use_graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    self._tick(i)
                self.graphs.append(g)
        self.ticks = 2

    def _tick(self, i):
        first, n = self.groups[i]
        self.engine.advance_slots(first, n, self.pri, self.val, self.obs)
        self.evaluators[i](self.obs[first:first + n], self.pri[first:first + n], self.val[first:first + n])

    def tick(self):
        """One tick of every group (enqueued group after group; the streams run them concurrently)."""
        for i, st in enumerate(self.streams):
            with torch.cuda.stream(st):
                if self.graphs:
                    self.graphs[i].replay()
                else:
                    self._tick(i)
        self.ticks += 1

    def run(self, n):
        for _ in range(n):
            self.tick()

    def synchronize(self):
        for st in self.streams:
            st.synchronize()


def _run_selfplay_overlapped(engine, evaluators, n_games, seed, check_every, max_ticks, use_graph, overlap):
    engine.reset(n_games, seed)
    torch.cuda.current_stream(engine.device).synchronize()
    tk = OverlappedTicker(engine, evaluators, overlap, use_graph=use_graph)

    def done():
        tk.synchronize()
        return engine.games_done() >= n_games

    tick_until(tk, check_every, done, max_ticks, "self-play", engine)
    prog = engine.progress()
    prog["ticks"] = tk.ticks
    return prog
