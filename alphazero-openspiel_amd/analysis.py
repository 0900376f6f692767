"""Batched position analysis: what search + net think of MANY given positions, one engine slot per position.

The reference answers this one state at a time (`MCTS.search(state)`, mcts.py:164-180; `AlphaZeroBot.step`,
alphazerobot.py:42-93), and so does this package's `mcts.MCTS` facade (a 1-slot engine: one board per net forward).
Here every position is a game id of ONE `manual_moves` engine: `az_engine_set_start_positions` gives each game its own
start position, one tick advances every search by a playout and asks the network for all their leaves in one forward,
and `az_engine_export_roots_device` packs all the roots into one buffer (one kernel, one device-to-host copy) - no
per-slot `read_slot` / `read_root` round trips anywhere in the loop.

    res = analyze_positions(net, "connect_four", histories, n_playouts=400)
    res["visits"][i], res["q"][i], res["priors"][i], res["best_action"][i]      # position i, in the order given

A search here is the same arithmetic as a 1-slot search of the same position (tests/test_analysis_gpu.py compares every
field of every root with `==`), and with the fused network at f32x the result does not depend on the slot count either.
"""
import numpy as np
import torch

from .engine import (DeviceEvaluator, EngineError, HostPolicyEvaluator, SearchSettings, SelfPlayEngine, TickDriver, close_all, default_device,
                     make_evaluator, read_lines)
from .games import Game, State

PHASE_IDLE, PHASE_SEARCH_DONE = 0, 5
_PROGRESS_SUMS = ("moves", "sims", "evals", "terminal_hits", "sum_depth", "sum_children", "nodes_allocated", "compactions")


def position_prefixes(game, histories):
    """histories (a list of action lists and / or `games.State`s) -> list of int action lists from the initial position.
    Pure host logic.  A State of another game, a terminal State and an empty list raise ValueError (with the index)."""
    game = Game(game) if isinstance(game, str) else game
    histories = list(histories)
    if not histories:
        raise ValueError("analyze_positions needs at least one position")
    out = []
    for i, h in enumerate(histories):
        if isinstance(h, State):
            if h.get_game().name != game.name:
                raise ValueError("position %d is a state of %s, the analysis runs %s" % (i, h.get_game().name, game.name))
            if h.is_terminal():
                raise ValueError("position %d is terminal: there is nothing to search" % i)
            h = h.history()
        out.append([int(a) for a in h])
    return out


def _make_evaluator(policy_fn, device, backend, precision, n_slots):
    """-> (evaluator, owned): a network becomes the package's device evaluator (engine.make_evaluator); an evaluator object
    is taken as it is (and stays the caller's)."""
    from .fusednet import FusedNet
    if isinstance(policy_fn, (FusedNet, DeviceEvaluator, HostPolicyEvaluator)):
        return policy_fn, False
    return make_evaluator(policy_fn, device, backend, precision, n_slots), True


class Analyzer:
    """n_slots searches side by side on one `manual_moves` engine, and what is needed to go on from them.

        an = Analyzer(net, "connect_four", n_slots=4096, n_playouts=400)
        an.load(histories)                       # at most n_slots positions; position i is slot i and game id i
        roots = an.search()                      # engine.read_roots(): every slot's root, one copy
        res = an.results()                       # visits / q / priors [n, A], root_q, root_n, best_action [n]

    With pv_depth = D > 0 every root export is followed by a line export (engine.export_lines_device, one more kernel), and
    results() also holds the principal variation of every search: pv_actions [n, D] (-1 padded), pv_n, pv_q [n, D], pv_len
    (the whole line's length, which may exceed D) and greedy_value (the off-policy value target A0GB at the line's end).

    Play the best move in 4096 games at once, to the end (a slot whose game is over goes idle and is left alone):

        an.load(histories); an.search()
        while True:
            res = an.results()
            live = res["phase"] == 5             # search done; 0 = idle, the game is over
            if not live.any():
                break
            an.update_root(np.where(live, res["best_action"], -1), keep_subtree=True)
            an.search()

    policy_fn: the network (an nn.Module or its bound .predict), or an evaluator object (FusedNet, DeviceEvaluator,
    HostPolicyEvaluator); None = set `.evaluator` (any callable(obs, priors_out, values_out)) before the first search.
    eval_mirror=p: every request of every search is evaluated left-right mirrored with probability p and mapped back
    (SelfPlayEngine.set_eval_mirror; the coin is keyed by seed, position index, ply and request).
    solver=True: MCTS-Solver (SelfPlayEngine.set_solver) - a search ends as soon as its root is proven, and results() gains
    solved [n] (object array: +1 / 0 / -1 for the side to move, None while unknown) and solved_children [n, A] int8 (the same
    for the side to move after each move; -128 where unknown or no child).
    fpu=r or (r, r_root): first-play urgency in every search (SelfPlayEngine.set_fpu): an unvisited child is valued at its parent's
    value minus r * sqrt(explored prior mass) (r_root at the root, default 0) in place of the reference's 0."""

    def __init__(self, policy_fn, game_name, n_slots, n_playouts=100, c_puct=2.5, use_dirichlet=False, device=None,
                 eval_backend="fused", eval_precision="f32x", seed=None, check_every=16, pv_depth=0, eval_mirror=None, solver=False,
                 fpu=None, **kwargs):
        # (solver=False is this signature's "not named"; eval_mirror=0 is named and clears)
        settings = SearchSettings.from_kwargs(dict(eval_mirror=eval_mirror, solver=solver or None, fpu=fpu), off="clear")
        if int(n_slots) < 1:
            raise ValueError("n_slots must be positive")
        if int(check_every) < 1:
            raise ValueError("check_every must be positive")
        if int(pv_depth) < 0:
            raise ValueError("pv_depth must not be negative")
        self.device = torch.device(device if device is not None else default_device(policy_fn))
        self.n_playouts, self.check_every = int(n_playouts), int(check_every)
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        kwargs.setdefault("keep_search_tree", True)
        self.engine = SelfPlayEngine(game_name, int(n_slots), n_playouts=self.n_playouts, c_puct=c_puct,
                                     use_dirichlet=use_dirichlet, manual_moves=True, max_games=int(n_slots),
                                     device=self.device, seed=self.seed, **kwargs)
        self.evaluator, self._owns_evaluator = None, False
        self._eval_backend, self._eval_precision = eval_backend, eval_precision
        try:
            self.solver = bool(settings.solver)
            settings.apply(self.engine)
            if policy_fn is not None:
                self.evaluator, self._owns_evaluator = _make_evaluator(policy_fn, self.engine.device, eval_backend,
                                                                       eval_precision, int(n_slots))
        except Exception:
            self.engine.close()
            raise
        self.obs, self.pri, self.val = self.engine.alloc_io()
        self.roots_buf = self.engine.alloc_roots()
        self.pv_depth = int(pv_depth)
        if self.pv_depth > self.engine.max_plies:
            self.engine.close()
            raise ValueError("pv_depth %d: a game of %s has at most %d plies" % (self.pv_depth, self.engine.game.name, self.engine.max_plies))
        self.lines_buf = None
        if self.pv_depth:
            self.lines_buf = torch.empty(self.engine.lines_device_bytes(self.pv_depth), dtype=torch.uint8, device=self.engine.device)
        self._value_lines_buf = None
        self.lines = None
        self._header = torch.empty(4, dtype=torch.int32).pin_memory()
        self.n = 0
        self.ticks = 0
        self.roots = None

    def close(self):
        close_all(self.evaluator if self._owns_evaluator else None, self.engine)
        self.evaluator = None

    def set_evaluator(self, policy_fn):
        """Search on with another network (or evaluator object): the engine stays, an evaluator this Analyzer made is closed."""
        new, owned = _make_evaluator(policy_fn, self.engine.device, self._eval_backend, self._eval_precision, self.engine.G)
        torch.cuda.synchronize(self.engine.device)
        if self._owns_evaluator:
            close_all(self.evaluator)
        self.evaluator, self._owns_evaluator = new, owned

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ one batch of positions
    def load(self, histories, seed=None):
        """Start a search from each of len(histories) <= n_slots positions (action lists from the initial position)."""
        if not 1 <= len(histories) <= self.engine.G:
            raise ValueError("%d positions for an engine of %d slots" % (len(histories), self.engine.G))
        self.engine.set_start_positions(histories)
        self.engine.reset(len(histories), self.seed if seed is None else seed)
        self.n = len(histories)
        self.roots = self.lines = None

    def load_states_device(self, bb, ply, seed=None):
        """The device twin of load: start a search from each of the n <= n_slots states (bb int64 [n, 2], ply int32 [n] device
        tensors, e.g. DeviceReplay.gather_states); nothing goes through the host."""
        n = int(ply.numel())
        if not 1 <= n <= self.engine.G:
            raise ValueError("%d positions for an engine of %d slots" % (n, self.engine.G))
        self.engine.set_start_states_device(bb, ply)
        self.engine.reset(n, self.seed if seed is None else seed)
        self.n = n
        self.roots = self.lines = None

    def update_root(self, actions, keep_subtree=True):
        """MCTS.update_root for every loaded position (actions [n]; -1 leaves a slot alone) and arm the next search."""
        acts = np.full(self.engine.G, -1, dtype=np.int64)
        acts[:self.n] = np.asarray(actions, dtype=np.int64).reshape(-1)[:self.n]
        self.engine.update_root(acts.tolist(), keep_subtree=keep_subtree)
        self.roots = self.lines = None

    def search_again(self):
        """Another n_playouts on the same roots (MCTS.search called twice, mcts.py:164-180)."""
        from . import _lib
        self.update_root([_lib.ACTION_SEARCH_AGAIN] * self.n)

    def _finished(self):
        """Root export + its 16-byte header: (slots finished or idle, error flags).  One kernel, one small copy."""
        self.engine.export_roots_device(self.roots_buf)
        if self.pv_depth:
            self.engine.export_lines_device(self.pv_depth, self.lines_buf)
        self._header.copy_(self.roots_buf[:16].view(torch.int32), non_blocking=True)
        torch.cuda.current_stream(self.engine.device).synchronize()
        return int(self._header[0]), int(self._header[3]) & 0xFFFFFFFF

    def search(self, max_ticks=None):
        """Tick (advance + forward) until every slot has finished its search; -> engine.read_roots() of that moment."""
        with torch.cuda.device(self.engine.device):
            self.search_device(max_ticks)
            self.roots = self.engine.read_roots(self.roots_buf)
            self.lines = read_lines(self.lines_buf) if self.pv_depth else None
        return self.roots

    def search_device(self, max_ticks=None):
        """search() without the read-back: -> roots_buf, the packed root export of the finished searches (device).  The host
        sees only the 16-byte header the loop polls."""
        if self.evaluator is None:
            raise EngineError("Analyzer has no evaluator: pass the network, or set .evaluator")
        e = self.engine
        limit = int(max_ticks) if max_ticks is not None else 4 * self.n_playouts + 64

        def tick():
            e.advance(self.pri, self.val, self.obs)
            self.evaluator(self.obs, self.pri, self.val)

        drv = TickDriver(e.device, tick)  # eager ticks: this loop captures no graph
        with torch.cuda.device(e.device):
            while True:
                done, flags = self._finished()
                if flags:
                    e.progress()  # raises with the decoded fault names
                if done >= e.G:
                    break
                if drv.ticks >= limit:
                    raise EngineError("analysis did not finish within %d ticks: %r" % (limit, e.progress()))
                drv.run(self.check_every)
            self.ticks += drv.ticks
        self.roots = self.lines = None
        return self.roots_buf

    def lines_device(self, max_depth=1):
        """The packed line export (engine.export_lines_device) of the finished searches -> a device buffer this Analyzer owns
        and rewrites per call.  The value target and the line's length do not depend on max_depth; Reanalyser takes 1."""
        D = int(max_depth)
        if self.pv_depth and D == self.pv_depth:
            return self.engine.export_lines_device(D, self.lines_buf)
        need = self.engine.lines_device_bytes(D)
        if self._value_lines_buf is None or self._value_lines_buf.numel() != need:
            self._value_lines_buf = torch.empty(need, dtype=torch.uint8, device=self.engine.device)
        return self.engine.export_lines_device(D, self._value_lines_buf)

    def results(self):
        """The loaded positions' roots as dense arrays: visits [n, A] int64, q / priors [n, A] float64 (zero where there is
        no child), root_q, root_n, best_action [n] (first maximum of the visits: the engine's rule), phase [n]."""
        if self.roots is None:
            self.roots = self.engine.read_roots(self.roots_buf)
        res = dense_roots(self.roots, self.n, self.engine.A)
        if self.pv_depth:
            if self.lines is None:
                self.lines = read_lines(self.engine.export_lines_device(self.pv_depth, self.lines_buf))
            res.update(dense_lines(self.lines, self.n))
        if self.solver:
            res.update(dense_proofs(self.engine.export_proofs_device().cpu().numpy(), self.roots, self.n, self.engine.A))
        return res


SOLVED_UNKNOWN = -128  # solved_children: no child, or nothing proven


def dense_proofs(proofs, roots, n, num_actions):
    """export_proofs_device() rows [G, 1 + mc] + read_roots() dict -> solved [n] (object: +1 / 0 / -1 for the side to move at the
    root, None = unknown) and solved_children [n, A] int8 (the value, for the root's side to move, of playing the action;
    SOLVED_UNKNOWN where unknown).  A status is seen by the player who moved INTO a node: the root's changes sign."""
    value = np.array([SOLVED_UNKNOWN, 1, 0, -1], dtype=np.int8)  # by status, for the player who moved into the node
    solved = np.empty(n, dtype=object)
    for i in range(n):
        st = int(proofs[i, 0])
        solved[i] = None if st == 0 else -int(value[st])
    act = roots["child_action"][:n]
    live = act >= 0
    rows = np.broadcast_to(np.arange(n)[:, None], act.shape)[live]
    ch = np.full((n, num_actions), SOLVED_UNKNOWN, dtype=np.int8)
    ch[rows, act[live]] = value[proofs[:n, 1:][live]]
    return {"solved": solved, "solved_children": ch}


def dense_lines(lines, n):
    """read_lines() dict -> the principal-variation arrays of the first n slots (see Analyzer)."""
    return {"pv_actions": lines["line_action"][:n].astype(np.int64), "pv_n": lines["line_n"][:n].copy(),
            "pv_q": lines["line_q"][:n].copy(), "pv_len": lines["depth"][:n].astype(np.int64),
            "greedy_value": lines["value"][:n].copy()}


def dense_roots(roots, n, num_actions):
    """read_roots() dict -> per-action arrays of the first n slots (see Analyzer.results)."""
    act = roots["child_action"][:n]
    live = act >= 0
    rows = np.broadcast_to(np.arange(n)[:, None], act.shape)[live]
    cols = act[live]
    visits = np.zeros((n, num_actions), dtype=np.int64)
    q = np.zeros((n, num_actions), dtype=np.float64)
    pri = np.zeros((n, num_actions), dtype=np.float64)
    visits[rows, cols] = roots["child_n"][:n][live]
    q[rows, cols] = roots["child_q"][:n][live]
    pri[rows, cols] = roots["child_p"][:n][live]
    # children are in ascending-action order, so the first maximum over the dense row is the first maximum over the children
    best = np.where(visits.sum(axis=1) > 0, np.argmax(visits, axis=1), np.where(live.any(axis=1), act[:, 0], -1))
    return {"visits": visits, "q": q, "priors": pri, "root_q": roots["root_q"][:n].copy(),
            "root_n": roots["root_n"][:n].copy(), "best_action": best.astype(np.int64), "phase": roots["phase"][:n].copy()}


def analyze_positions(policy_fn, game_name, histories, n_playouts=100, c_puct=2.5, use_dirichlet=False, n_slots=None,
                      device=None, eval_backend="fused", eval_precision="f32x", seed=None, check_every=16, pv_depth=0,
                      eval_mirror=None, solver=False, fpu=None, **kwargs):
    """Search every given position with n_playouts of PUCT search, all of them side by side on the device.

    policy_fn   the network (nn.Module or its bound .predict) or an evaluator object, as elsewhere in the package
    histories   a list of action lists (from the initial position) or of `games.State`
    n_slots     positions searched at once (default min(n, 4096)); more positions run in chunks on ONE engine and ONE
                evaluator.  With the fused network at f32x the results do not depend on it.
    pv_depth    D > 0: also return every position's principal variation - pv_actions [n, D] (-1 padded), pv_n, pv_q [n, D],
                pv_len [n] (the whole greedy line's length) and greedy_value [n] (the off-policy target A0GB at its end)
    eval_mirror p: every request is evaluated left-right mirrored with probability p (SelfPlayEngine.set_eval_mirror)
    solver      True: MCTS-Solver (SelfPlayEngine.set_solver); the result gains solved [n] and solved_children [n, A] (Analyzer)
    fpu         r or (r, r_root): first-play urgency in every search (SelfPlayEngine.set_fpu)
    kwargs      further SelfPlayEngine keywords (dirichlet_ratio, use_puct, nodes_per_slot, max_sims_per_tick, ...)

    Returns a dict, rows in the order given: visits [n, A] int64, q [n, A], priors [n, A] float64 (zero where there is no
    child), root_q [n], root_n [n], best_action [n] (first maximum of the visits) and progress (the engine's counters summed
    over the chunks, plus ticks / chunks / n_slots).  With use_dirichlet the root noise of a position is keyed by
    (seed + index of its chunk's first position, index within the chunk, ply)."""
    game = Game(game_name) if isinstance(game_name, str) else game_name
    prefixes = position_prefixes(game, histories)
    n = len(prefixes)
    n_slots = int(n_slots) if n_slots else min(n, 4096)
    if n_slots < 1:
        raise ValueError("n_slots must be positive")
    an = Analyzer(policy_fn, game, n_slots, n_playouts=n_playouts, c_puct=c_puct, use_dirichlet=use_dirichlet, device=device,
                  eval_backend=eval_backend, eval_precision=eval_precision, seed=seed, check_every=check_every, pv_depth=pv_depth,
                  eval_mirror=eval_mirror, solver=solver, fpu=fpu, **kwargs)
    try:
        parts = []
        prog = {k: 0 for k in _PROGRESS_SUMS}
        prog["error_flags"] = 0
        for first in range(0, n, n_slots):
            chunk = prefixes[first:first + n_slots]
            try:
                an.load(chunk, seed=an.seed + first)
            except EngineError as err:
                raise EngineError("positions %d..%d: %s" % (first, first + len(chunk) - 1, err)) from None
            an.search()
            parts.append(an.results())
            p = an.engine.progress()
            for k in _PROGRESS_SUMS:
                prog[k] += p[k]
            prog["error_flags"] |= p["error_flags"]
        prog.update(ticks=an.ticks, chunks=len(parts), n_slots=n_slots, positions=n)
    finally:
        an.close()
    out = {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0] if k != "phase"}
    out["progress"] = prog
    return out
