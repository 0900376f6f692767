"""Device-resident replay store + training step — the consumer side of self-play.

Reference: the Trainer's FIFO buffer of games (train.py:226-236,295-298), `remove_duplicates` (train.py:156-201) and
`net_step`'s batch sampling (train.py:107-120) run in HIP kernels on the engine's records (C ABI: include/az_replay.h),
so a generation goes  engine -> DeviceReplay.append_engine -> dedupe -> sample -> net_step  without the examples ever
becoming Python lists.  The network update (forward, MSE + cross-entropy, Adam: train.py:115-130) is plain PyTorch.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .games import Game


def dedupe_mode(by="history", mirror=False):
    """The arguments of DeviceReplay.dedupe -> None for the history rule (az_replay_dedupe), else the `mirror` argument of
    az_replay_dedupe_positions (0 or 1).  ValueError for an unknown rule, and for mirror=True with by="history": a history has
    no mirror key."""
    if by not in ("history", "position"):
        raise ValueError("dedupe: by must be 'history' or 'position', not %r" % (by,))
    if by == "history":
        if mirror:
            raise ValueError("dedupe: mirror=True needs by='position' - a history has no mirror key")
        return None
    return 1 if mirror else 0


class DeviceReplay:
    def __init__(self, game_name, max_games, device=0, max_examples=None):
        self.lib = _lib.load()
        self.game = Game(game_name) if isinstance(game_name, str) else game_name
        dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if dev.type != "cuda":
            raise RuntimeError("DeviceReplay lives in HBM: a HIP device is required")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        cfg = _lib.AzReplayConfig()
        cfg.struct_size = C.sizeof(_lib.AzReplayConfig)
        cfg.game, cfg.rows, cfg.cols = self.game.game_id, self.game.rows, self.game.cols
        cfg.device = self.device.index
        cfg.max_games = int(max_games)
        cfg.max_examples = int(max_examples if max_examples is not None else max_games * self.game.max_game_length())
        self._h = C.c_void_p()
        rc = self.lib.az_replay_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise RuntimeError("az_replay_create failed (%d): %s" % (rc, self.lib.az_replay_last_error(None).decode()))
        self.A = self.game.num_distinct_actions()
        self.obs_shape = (4, self.game.rows, self.game.cols)

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError("replay call failed (%d): %s" % (rc, self.lib.az_replay_last_error(self._h).decode()))
        return rc

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.az_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_capacity(self, n_games):
        """Trainer.update_buffer_size (train.py:295-298): the FIFO's current size in games."""
        self._check(self.lib.az_replay_set_capacity(self._h, int(n_games)))

    def append_engine(self, engine):
        """All finished games of the engine's generation, device to device (train.py:226-227)."""
        self._check(self.lib.az_replay_append_engine(self._h, engine._h, self._stream()))

    def append_export(self, ex):
        """Games in the export layout (engine.export() / distributed.unpack_export) from host memory.  One start ply for
        every game: the export of a generation with a start per game (SelfPlayEngine.set_game_starts: "start_ply" is an
        array) is refused - such games carry history keys that a host view does not; append them with append_engine, or with
        append_device(buf, n, start_ply=ply, keys=keys)."""
        if np.ndim(ex.get("start_ply", 0)) != 0:
            raise ValueError("append_export takes one start ply for every game; a generation with a start per game goes "
                             "through append_engine or append_device(buf, n, start_ply=, keys=)")
        v = _lib.AzExampleView()
        keep = {k: np.ascontiguousarray(ex[k]) for k in ("game_len", "game_ret0", "states", "move", "n_children",
                                                         "child_action", "child_visits", "value")}
        v.n_games = len(keep["game_len"])
        v.max_plies = keep["move"].shape[1]
        v.max_children = keep["child_action"].shape[2]
        v.game_len = keep["game_len"].ctypes.data_as(C.POINTER(C.c_int32))
        v.game_ret0 = keep["game_ret0"].ctypes.data_as(C.POINTER(C.c_float))
        v.states = keep["states"].ctypes.data_as(C.POINTER(C.c_uint64))
        v.move = keep["move"].ctypes.data_as(C.POINTER(C.c_uint16))
        v.n_children = keep["n_children"].ctypes.data_as(C.POINTER(C.c_uint8))
        v.child_action = keep["child_action"].ctypes.data_as(C.POINTER(C.c_uint16))
        v.child_visits = keep["child_visits"].ctypes.data_as(C.POINTER(C.c_uint32))
        v.value = keep["value"].ctypes.data_as(C.POINTER(C.c_double))
        self._check(self.lib.az_replay_append_host(self._h, C.byref(v), int(ex.get("start_ply", 0)), self._stream()))

    def append_device(self, buf, n_games, start_ply=0, keys=None, keep=None):
        """Games from a packed DEVICE export (engine.export_device(), or one rank's section of the all-gathered buffer):
        engine -> RCCL all-gather -> replay store with no host copy of the records.
        start_ply: one start ply for every game, or - a generation with a start per game - an int32 device tensor [n_games],
        with keys = the games' history key pairs (int64 [n_games, 2]) or None (keyed from their start states): the two tensors
        SelfPlayEngine.game_starts_device() returns.
        keep: a uint8 device tensor [n_games, max_plies] by absolute ply (SelfPlayEngine.full_moves_device(): the full-search
        moves of a generation under a playout cap) - only plies with a non-zero byte become examples; a game's FIFO length is
        its number of kept plies, and the keys are still those of the full histories."""
        if buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device:
            raise RuntimeError("append_device expects a contiguous uint8 tensor on %s" % (self.device,))
        from .engine import device_export_layout
        need = device_export_layout(n_games, self.game.max_game_length(), self.game.max_children())[1]
        if buf.numel() < need:
            raise RuntimeError("export buffer holds %d bytes, %d games need %d" % (buf.numel(), n_games, need))
        n, per_game = int(n_games), torch.is_tensor(start_ply)
        if keys is not None and not per_game:
            raise ValueError("keys go with a start ply per game: give start_ply as an int32 tensor [n_games]")
        for t, dt, shape in ((start_ply if per_game else None, torch.int32, (n,)), (keys, torch.int64, (n, 2)),
                             (keep, torch.uint8, (n, self.game.max_game_length()))):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != self.device or tuple(t.shape) != shape):
                raise RuntimeError("append_device expects a contiguous %s %s tensor on %s" % (dt, shape, self.device))
        head = (self._h, C.c_void_p(buf.data_ptr()), n)
        ply = C.c_void_p(start_ply.data_ptr()) if per_game else None
        key_ptr = C.c_void_p(keys.data_ptr()) if keys is not None else None
        if keep is not None:    # the narrowest of the three entries that takes what was given
            rc = self.lib.az_replay_append_device_kept(*head, 0 if per_game else int(start_ply), ply, key_ptr,
                                                       C.c_void_p(keep.data_ptr()), self._stream())
        elif per_game:
            rc = self.lib.az_replay_append_device_starts(*head, ply, key_ptr, self._stream())
        else:
            rc = self.lib.az_replay_append_device(*head, int(start_ply), self._stream())
        self._check(rc)

    def dedupe(self, by="history", mirror=False):
        """Trainer.remove_duplicates over the flattened buffer; returns the number of unique examples.
        by="history" (the reference's rule): examples merge when their action histories are equal.
        by="position": examples merge when their positions (bb0, bb1, ply & 1) are equal, whatever the move order that led
        there; with mirror=True a position and its left-right mirror image merge too, the mirrored member's policy mapped
        through the action mirror (az_replay_dedupe_positions, include/az_replay.h).  The average goes into the first occurrence
        in its own orientation; sample(), gather_states(), gather_forks() and the refreshes read that record as always."""
        mode = dedupe_mode(by, mirror)
        if mode is None:
            self._check(self.lib.az_replay_dedupe(self._h, self._stream()))
        else:
            self._check(self.lib.az_replay_dedupe_positions(self._h, mode, self._stream()))
        return self.stats()["n_unique"]

    def unique_counts(self):
        """-> int32 device tensor [n_unique]: how many stored examples went into each entry of the de-duplicated list (the last
        dedupe() of either kind).  RuntimeError (AZ_E_STATE) before a dedupe and after an append or a capacity change."""
        # n_unique from a read-back of no rows: stats() would report - and clear - fault flags that are not this call's
        n = int(self._check(self.lib.az_replay_read_unique(self._h, 0, None, None, None, None, None, None)))
        out = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._check(self.lib.az_replay_unique_counts_device(self._h, C.c_void_p(out.data_ptr()) if n else None, n, self._stream()))
        return out

    def stats(self):
        s = _lib.AzReplayStats()
        self._check(self.lib.az_replay_stats_get(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.AzReplayStats._fields_}

    def sample(self, batch, indices=None, seed=0, mirror=None, out=None):
        """-> (x [B,4,H,W], pi [B,A], z [B]) float32 device tensors.  indices: int64 tensor/array of positions in the
        de-duplicated list (the reference's np.random.randint draw); None = drawn on the device.
        mirror: None / False = every row as it was played; True = each row left-right mirrored or not by a coin drawn on the
        device from (seed, call counter, row); a bool / uint8 tensor or array of length batch = row b mirrored where mirror[b]
        (az_replay_sample_sym: the mirrored position, the mirrored policy, the same value).
        out: (x, pi, z) contiguous float32 tensors of those shapes on the store's device, filled and returned instead of
        newly allocated ones; anything else is refused."""
        batch = int(batch)
        shapes = ((batch,) + self.obs_shape, (batch, self.A), (batch,))
        if out is None:
            out = tuple(torch.empty(sh, dtype=torch.float32, device=self.device) for sh in shapes)
        else:
            out = tuple(out)
            if len(out) != 3:
                raise ValueError("out must be the three tensors (x, pi, z)")
            for name, t, sh in zip(("x", "pi", "z"), out, shapes):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != sh or t.device != self.device \
                        or not t.is_contiguous():
                    raise ValueError("out: %s must be a contiguous float32 tensor of shape %s on %s" % (name, sh, self.device))
        x, pi, z = out
        keep = []  # tensors made here that the kernel reads
        idx_ptr = flip_ptr = None
        if indices is not None:
            idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).to(self.device)
            assert idx.numel() == batch
            idx_ptr = C.c_void_p(idx.data_ptr())
            keep.append(idx)
        ptrs = (C.c_void_p(x.data_ptr()), C.c_void_p(pi.data_ptr()), C.c_void_p(z.data_ptr()), self._stream())
        if mirror is None or (isinstance(mirror, (bool, np.bool_)) and not mirror):
            self._check(self.lib.az_replay_sample(self._h, idx_ptr, batch, int(seed) & (2 ** 64 - 1), *ptrs))
        else:
            if not isinstance(mirror, (bool, np.bool_)):
                flips = mirror if torch.is_tensor(mirror) else torch.as_tensor(np.asarray(mirror))
                if flips.dtype not in (torch.bool, torch.uint8) or flips.numel() != batch:
                    raise ValueError("mirror must be None, a bool, or a bool / uint8 tensor or array of length batch")
                flips = flips.reshape(-1).to(device=self.device, dtype=torch.uint8).contiguous()
                flip_ptr = C.c_void_p(flips.data_ptr())
                keep.append(flips)
            self._check(self.lib.az_replay_sample_sym(self._h, idx_ptr, flip_ptr, batch, int(seed) & (2 ** 64 - 1), *ptrs))
        if keep:
            torch.cuda.current_stream(self.device).synchronize()  # they must outlive the kernel
        return x, pi, z

    # ------------------------------------------------------------------ reanalyse (include/az_replay.h)
    def _indices(self, indices):
        idx = indices if torch.is_tensor(indices) else torch.as_tensor(np.asarray(indices, dtype=np.int64))
        return idx.to(device=self.device, dtype=torch.int64).contiguous().reshape(-1)

    def gather_states(self, indices):
        """Positions of the de-duplicated list (indices: int64 tensor / array, the index space of sample()) -> (bb int64 [n, 2],
        ply int32 [n]) device tensors, the arguments of SelfPlayEngine.set_start_states_device.  bb holds the 64-bit boards bit
        for bit (`.cpu().numpy().view(np.uint64)` shows them).  Asynchronous; an index outside the list raises the BAD_INDEX
        fault flag (stats()) and gives a state with ply -1, which no engine accepts."""
        idx = self._indices(indices)
        n = int(idx.numel())
        bb = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        ply = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._check(self.lib.az_replay_gather_states(self._h, C.c_void_p(idx.data_ptr()), n, C.c_void_p(bb.data_ptr()),
                                                     C.c_void_p(ply.data_ptr()), self._stream()))
        return bb, ply

    def gather_forks(self, indices):
        """gather_states plus the stored history key pair of each example -> (bb int64 [n, 2], ply int32 [n], keys int64 [n, 2])
        device tensors, the arguments of SelfPlayEngine.set_game_starts_device: games forked off these positions carry on the
        stored histories, so a fork's first example merges with the example it came from at the next dedupe().  Asynchronous;
        a bad index raises the BAD_INDEX fault flag and gives ply -1.  Nothing is marked for a refresh: a fork appends."""
        idx = self._indices(indices)
        n = int(idx.numel())
        bb = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        ply = torch.empty((n,), dtype=torch.int32, device=self.device)
        keys = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        self._check(self.lib.az_replay_gather_forks(self._h, C.c_void_p(idx.data_ptr()), n, C.c_void_p(bb.data_ptr()),
                                                    C.c_void_p(ply.data_ptr()), C.c_void_p(keys.data_ptr()), self._stream()))
        if idx is not indices:
            torch.cuda.current_stream(self.device).synchronize()  # a copy of the indices made here must outlive the kernel
        return bb, ply, keys

    def refresh_from_roots(self, indices, roots_buf, value_target="soft-Z"):
        """Overwrite the targets of the examples gather_states(indices) named from the finished searches in roots_buf (the packed
        root export of an engine whose game j searched indices[j]; SelfPlayEngine.export_roots_device): pi = the normalised root
        visit counts, z by value_target ("soft-Z", "A0C", None = keep).  -> the number of examples refreshed.  RuntimeError
        (AZ_E_STATE) if the store has changed since gather_states."""
        if value_target not in _lib.REFRESH_MODES:
            raise ValueError("value_target must be one of %s: on-policy needs the game's outcome, off-policy the searches' "
                             "greedy lines as well (refresh_from_search)" % sorted(map(str, _lib.REFRESH_MODES)))
        if roots_buf.dtype != torch.uint8 or not roots_buf.is_contiguous() or roots_buf.device != self.device:
            raise RuntimeError("refresh_from_roots expects a contiguous uint8 tensor on %s" % (self.device,))
        idx = self._indices(indices)
        return int(self._check(self.lib.az_replay_refresh_from_roots(
            self._h, C.c_void_p(idx.data_ptr()), int(idx.numel()), C.c_void_p(roots_buf.data_ptr()), int(roots_buf.numel()),
            _lib.REFRESH_MODES[value_target], self._stream())))

    def refresh_from_search(self, indices, roots_buf, lines_buf, value_target="off-policy"):
        """refresh_from_roots with the searches' greedy lines at hand (lines_buf: SelfPlayEngine.export_lines_device of the same
        engine at the same moment as roots_buf, any max_depth; None for the targets that do not need it): value_target may also
        be "off-policy" - z = the value at the end of the most-visited line (A0GB).  pi comes from the roots as always."""
        if value_target not in _lib.SEARCH_REFRESH_MODES:
            raise ValueError("value_target must be one of %s: on-policy needs the game's outcome"
                             % sorted(map(str, _lib.SEARCH_REFRESH_MODES)))
        if value_target == "off-policy" and lines_buf is None:
            raise ValueError("value_target off-policy needs lines_buf (SelfPlayEngine.export_lines_device)")
        for buf in (roots_buf, lines_buf):
            if buf is not None and (buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.device):
                raise RuntimeError("refresh_from_search expects contiguous uint8 tensors on %s" % (self.device,))
        idx = self._indices(indices)
        return int(self._check(self.lib.az_replay_refresh_from_search(
            self._h, C.c_void_p(idx.data_ptr()), int(idx.numel()), C.c_void_p(roots_buf.data_ptr()), int(roots_buf.numel()),
            C.c_void_p(lines_buf.data_ptr()) if lines_buf is not None else None, int(lines_buf.numel()) if lines_buf is not None else 0,
            _lib.SEARCH_REFRESH_MODES[value_target], self._stream())))

    def read_unique(self):
        n = self.stats()["n_unique"]
        key = np.zeros(n, np.uint64)
        pi = np.zeros((n, self.A), np.float64)
        z = np.zeros(n, np.float64)
        bidx = np.zeros(n, np.int64)
        bb = np.zeros((n, 2), np.uint64)
        ply = np.zeros(n, np.int32)
        self._check(self.lib.az_replay_read_unique(
            self._h, n, key.ctypes.data_as(C.POINTER(C.c_uint64)), pi.ctypes.data_as(C.POINTER(C.c_double)),
            z.ctypes.data_as(C.POINTER(C.c_double)), bidx.ctypes.data_as(C.POINTER(C.c_int64)),
            bb.ctypes.data_as(C.POINTER(C.c_uint64)), ply.ctypes.data_as(C.POINTER(C.c_int32))))
        return {"key": key, "pi": pi, "z": z, "buffer_index": bidx, "bitboards": bb, "ply": ply}

    def read_example(self, index):
        pi = np.zeros(self.A, np.float64)
        z = C.c_double()
        self._check(self.lib.az_replay_read_example(self._h, int(index), pi.ctypes.data_as(C.POINTER(C.c_double)),
                                                    C.byref(z)))
        return pi, z.value


class Reanalyser:
    """Refresh stored targets by searching stored positions again with the current network ("Reanalyse").

        re = Reanalyser(store, net, n_slots=4096, n_playouts=400, value_target="soft-Z")
        store.dedupe(); re.reanalyse(n=8192, seed=gen)      # 8192 distinct positions of the de-duplicated list, in chunks of 4096
        re.set_evaluator(net)                               # after training: the next call searches with the new weights

    One Analyzer (a manual_moves engine and an evaluator) lives across the calls.  A chunk goes gather_states ->
    load_states_device -> search_device -> refresh_from_roots: positions and roots stay in HBM, the host sees the 16-byte
    headers of the exports and the refreshed count.  value_target: "soft-Z", "A0C" or None (pi only) - the targets that
    are functions of a search root - or "off-policy" (A0GB, the value at the end of the most-visited line): the chunk's
    greedy lines are then exported too (Analyzer.lines_device, one kernel, depth 1: the value does not depend on it) and the
    refresh goes through refresh_from_search.  Further keywords go to the Analyzer (c_puct, use_dirichlet, eval_precision,
    eval_mirror=p for searches whose requests are evaluated left-right mirrored with probability p, solver=True for MCTS-Solver
    searches, fpu=r or (r, r_root) for first-play urgency (SelfPlayEngine.set_fpu) in the searches, ...).  With solver=True a search ends as soon as its root is proven and the refresh reads that root as it stands: the
    raw visit counts and Q of what may be a handful of playouts, not the adjusted counts and exact value self-play records there.
    The store must not change between the calls made here (it is the caller's between reanalyse() calls); the next dedupe()
    averages a refreshed first occurrence with its stale duplicates, as the reference's aliasing does."""

    def __init__(self, store, policy_fn, n_slots, n_playouts, value_target="soft-Z", **kwargs):
        from .analysis import Analyzer
        if value_target not in _lib.SEARCH_REFRESH_MODES:
            raise ValueError("value_target must be one of %s: on-policy needs the game's outcome"
                             % sorted(map(str, _lib.SEARCH_REFRESH_MODES)))
        self.store, self.value_target = store, value_target
        kwargs.setdefault("device", store.device)
        kwargs.setdefault("seed", 0)  # (keys the root noise only, and that is off unless use_dirichlet is asked for)
        self.analyzer = Analyzer(policy_fn, store.game, int(n_slots), n_playouts=int(n_playouts), **kwargs)
        self.n_slots = self.analyzer.engine.G

    def set_evaluator(self, policy_fn):
        self.analyzer.set_evaluator(policy_fn)

    def close(self):
        self.analyzer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def draw(self, n=None, seed=0):
        """n distinct indices of the de-duplicated list, drawn on the device (None, or more than there are: all of them)."""
        n_unique = self.store.stats()["n_unique"]
        if n_unique < 1:
            raise RuntimeError("Reanalyser: the store has no de-duplicated list (dedupe() first)")
        if n is None or int(n) >= n_unique:
            return torch.arange(n_unique, dtype=torch.int64, device=self.store.device)
        gen = torch.Generator(device=self.store.device)
        gen.manual_seed(int(seed))
        return torch.randperm(n_unique, generator=gen, device=self.store.device)[:int(n)].contiguous()

    def reanalyse(self, n=None, indices=None, seed=0):
        """Search the positions `indices` (default: draw(n, seed)) and overwrite their targets -> the number refreshed."""
        idx = self.draw(n, seed) if indices is None else self.store._indices(indices)
        an, done = self.analyzer, 0
        for first in range(0, int(idx.numel()), self.n_slots):
            chunk = idx[first:first + self.n_slots]
            bb, ply = self.store.gather_states(chunk)
            an.load_states_device(bb, ply, seed=an.seed + first)
            roots = an.search_device()
            if self.value_target == "off-policy":
                done += self.store.refresh_from_search(chunk, roots, an.lines_device(1), self.value_target)
            else:
                done += self.store.refresh_from_roots(chunk, roots, self.value_target)
        return done


class Forker:
    """Fork new self-play games out of stored positions and append them: the on-policy counterpart of Reanalyser.

        fk = Forker(store, net, n_slots=1024, n_playouts=100)
        store.dedupe(); fk.fork(n=256, seed=gen)         # 256 games from uniformly drawn stored positions, played to the end
        fk.set_net(net)                                   # after training: the next call plays with the new weights

    A call goes gather_forks -> set_game_starts_device -> self-play -> append_engine: positions, key pairs and records stay in
    HBM.  A fork's first example carries the key of the example it came from (include/az_replay.h, the key rule), so the next
    dedupe() averages the fresh search and outcome with the stored targets; the rest of the game is new data under the stored
    history.  The stored keys must be history keys (the key rule): games from the initial position, from set_game_starts or from
    earlier forks are; the games of an engine with ONE shared set_start_prefix of length > 0 are keyed from that prefix's
    position instead - a fork off such a game still merges with its parent, but when it repeats the parent's next move the next
    dedupe() meets one `key` with two `key2` and raises the KEY_COLLISION fault.  Do not fork out of such a store.  One engine lives across the calls; further keywords go to it (c_puct, temperature, backup, ...).  Positions are
    drawn WITH replacement: two forks of one position are two different games (the random stream is keyed by game id).
    fpu=r or (r, r_root): the forked games are searched with first-play urgency (SelfPlayEngine.set_fpu)."""

    def __init__(self, store, net, n_slots, n_playouts, eval_backend="fused", eval_precision="f32x", use_graph=False, seed=0,
                 max_games=None, fpu=None, **kwargs):
        from .engine import SearchSettings, SelfPlayEngine, make_evaluator
        settings = SearchSettings.from_kwargs(dict(fpu=fpu))
        self.store, self.seed, self.use_graph, self.calls = store, int(seed), bool(use_graph), 0
        self.eval_backend, self.eval_precision = eval_backend, eval_precision
        self.engine = SelfPlayEngine(store.game, int(n_slots), n_playouts=int(n_playouts), device=store.device, seed=self.seed,
                                     max_games=int(max_games if max_games is not None else n_slots), **kwargs)
        self.evaluator = None
        try:
            settings.apply(self.engine)
            self.evaluator = make_evaluator(net, store.device, eval_backend, eval_precision, self.engine.G)
        except Exception:
            self.engine.close()
            raise
        self.last_progress = None

    def set_net(self, net):
        from .engine import close_all, make_evaluator
        torch.cuda.synchronize(self.store.device)
        old, self.evaluator = self.evaluator, make_evaluator(net, self.store.device, self.eval_backend, self.eval_precision,
                                                             self.engine.G)
        close_all(old)

    def close(self):
        from .engine import close_all
        close_all(self.engine, self.evaluator, drain=True)
        self.engine = self.evaluator = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def draw(self, n, seed=0):
        """n indices of the de-duplicated list, uniform with replacement, drawn on the device."""
        n_unique = self.store.stats()["n_unique"]
        if n_unique < 1:
            raise RuntimeError("Forker: the store has no de-duplicated list (dedupe() first)")
        gen = torch.Generator(device=self.store.device)
        gen.manual_seed(int(seed))
        return torch.randint(n_unique, (int(n),), generator=gen, device=self.store.device, dtype=torch.int64)

    def fork(self, n=None, indices=None, seed=None):
        """Play one game from each position `indices` (default: draw(n, seed)) to its end and append the games -> their number.
        At most the engine's max_games per call."""
        from .engine import run_selfplay
        seed = self.seed + 1000003 * self.calls if seed is None else int(seed)
        idx = self.draw(n, seed) if indices is None else self.store._indices(indices)
        n = int(idx.numel())
        if n < 1 or n > self.engine.sizes.max_games:
            raise ValueError("fork: %d games asked for, the engine holds 1..%d per call" % (n, self.engine.sizes.max_games))
        bb, ply, keys = self.store.gather_forks(idx)
        self.engine.set_game_starts_device(bb, ply, keys)
        self.last_progress = run_selfplay(self.engine, self.evaluator, n, seed=seed, use_graph=self.use_graph)
        self.store.append_engine(self.engine)
        self.calls += 1
        return n


def net_step(net, optimizer, x, pi_target, z_target):
    """One parameter update as Trainer.net_step does it (train.py:103,115-130): loss = MSE(v, z) +
    (-sum(pi * log p) / batch); returns (loss_p, loss_v)."""
    net.zero_grad()
    p, v = net(x)
    loss_v = torch.nn.functional.mse_loss(v, z_target.unsqueeze(1))
    loss_p = -torch.sum(pi_target * torch.log(p)) / pi_target.size(0)
    (loss_v + loss_p).backward()
    optimizer.step()
    return loss_p, loss_v


def make_optimizer(net, lr=0.001):
    """The Trainer's optimiser (train.py:86): Adam, weight decay 1e-4."""
    return torch.optim.Adam(net.parameters(), lr=lr, weight_decay=0.0001)


class GraphedNetStep:
    """net_step captured once as a HIP graph (forward, loss, backward, Adam with capturable state) and replayed per batch:
    the update is the same sequence of kernels as `net_step`, minus ~100 kernel launches' worth of host latency per step.
    Usage: step = GraphedNetStep(net, batch, replay); loss_p, loss_v = step(seed)  (samples on the device, straight into the
    graph's input tensors, then replays).  mirror=True: every batch is sampled with device-drawn left-right flips
    (DeviceReplay.sample(mirror=True)), which doubles the distinct positions the net sees at no cost in search or memory."""

    def __init__(self, net, batch, store, lr=0.001, mirror=False):
        self.net, self.store, self.batch, self.mirror = net, store, batch, bool(mirror)
        dev = store.device
        self.opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=0.0001, capturable=True)
        self.x = torch.zeros((batch,) + store.obs_shape, dtype=torch.float32, device=dev)
        self.pi = torch.full((batch, store.A), 1.0 / store.A, dtype=torch.float32, device=dev)
        self.z = torch.zeros((batch,), dtype=torch.float32, device=dev)
        self.loss_p = torch.zeros((), device=dev)
        self.loss_v = torch.zeros((), device=dev)
        # Warm-up outside capture (MIOpen kernel selection, allocator, Adam state creation), then put EVERYTHING it
        # touched back: weights, BatchNorm running statistics and Adam moments / step counters — the captured step
        # must be the first real update.
        import copy
        saved = copy.deepcopy(net.state_dict())
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        net.load_state_dict(saved)
        for st in self.opt.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        self.opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph):
            self._step()

    def _step(self):
        self.opt.zero_grad(set_to_none=True)
        p, v = self.net(self.x)
        lv = torch.nn.functional.mse_loss(v, self.z.unsqueeze(1))
        lp = -torch.sum(self.pi * torch.log(p)) / self.pi.size(0)
        (lv + lp).backward()
        self.opt.step()
        self.loss_p.copy_(lp.detach())
        self.loss_v.copy_(lv.detach())

    def __call__(self, seed=0, indices=None):
        self.store.sample(self.batch, indices=indices, seed=seed, mirror=self.mirror, out=(self.x, self.pi, self.z))
        self.graph.replay()
        return self.loss_p, self.loss_v
