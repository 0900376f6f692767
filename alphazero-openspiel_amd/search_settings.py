"""The search settings of the package as one value: parsed once, checked once, applied in one order.

Every facade that takes playout_cap=, forced_playouts=, eval_mirror=, solver= and fpu= (ExampleGenerator, SelfPlayStream, Analyzer
and with it the Reanalyser, Forker, the arena and SelfPlayEngine.set_arena_search, the tools and the example) builds a SearchSettings
from its keywords and lets it call the engine's setters.  Which engine kinds may carry which setting is the engine's table
("Search settings"); here are the keywords' forms and the rules the facades state before an engine exists."""
import numpy as np

KEYS = ("playout_cap", "forced_playouts", "eval_mirror", "solver", "fpu", "resign")
ARENA_KEYS = ("fpu", "solver", "eval_mirror")  # SelfPlayEngine.set_arena_search: the settings an arena agent may carry (resign is
#                                                refused: an evaluation game is played to its end)


def fpu_pair(fpu):
    """fpu=r or (r, r_root) -> (reduction, root reduction) as floats: both finite and >= 0, the root's 0 when left out (ValueError
    otherwise).  The one validation of every fpu= keyword of the package."""
    pair = tuple(fpu) if isinstance(fpu, (tuple, list)) else (fpu, 0.0)
    if len(pair) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) for x in pair):
        raise ValueError("fpu must be a reduction r or a pair (r, r_root) of numbers, got %r" % (fpu,))
    r, r_root = float(pair[0]), float(pair[1])
    if not (0.0 <= r < float("inf") and 0.0 <= r_root < float("inf")):
        raise ValueError("fpu reductions must be finite and >= 0, got %r" % (fpu,))
    return r, r_root


def _playout_cap(cap):
    try:
        n_fast, p_full = cap
        return int(n_fast), float(p_full)
    except (TypeError, ValueError):
        raise ValueError("playout_cap must be a pair (n_fast, p_full), got %r" % (cap,))


def _forced_playouts(fp):
    try:
        k, prune = fp if isinstance(fp, (tuple, list)) else (fp, True)
        k = float(k)
    except (TypeError, ValueError):
        raise ValueError("forced_playouts must be k or a pair (k, prune), got %r" % (fp,))
    if not (0.0 <= k < float("inf")) or prune not in (0, 1, False, True):
        raise ValueError("forced_playouts needs a finite k >= 0 and prune False / True, got %r" % (fp,))
    return k, bool(prune)


def _eval_mirror(p_given):
    try:
        p = float(p_given)
    except (TypeError, ValueError):
        p = float("nan")
    if not 0.0 <= p <= 1.0:  # (NaN fails both comparisons)
        raise ValueError("eval_mirror must be a probability in [0, 1], got %r" % (p_given,))
    return p


def _resign(given):
    """resign=v, (v, playthrough) or (v, playthrough, min_ply) -> (v, playthrough, min_ply): v in (0, 1], playthrough in [0, 1]
    (0.1 when left out), min_ply an int >= 0 (0 when left out)."""
    tup = tuple(given) if isinstance(given, (tuple, list)) else (given,)
    try:
        if not 1 <= len(tup) <= 3 or any(isinstance(x, bool) for x in tup):
            raise TypeError
        v, p = float(tup[0]), float(tup[1]) if len(tup) > 1 else 0.1
        min_ply = tup[2] if len(tup) > 2 else 0
        if int(min_ply) != min_ply:
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("resign must be v, (v, playthrough) or (v, playthrough, min_ply), got %r" % (given,))
    if not (0.0 < v <= 1.0 and 0.0 <= p <= 1.0 and int(min_ply) >= 0):  # (NaN fails the comparisons)
        raise ValueError("resign needs v in (0, 1], playthrough in [0, 1] and min_ply >= 0, got %r" % (given,))
    return v, p, int(min_ply)


_PARSE = {"playout_cap": _playout_cap, "forced_playouts": _forced_playouts, "eval_mirror": _eval_mirror, "solver": bool, "fpu": fpu_pair,
          "resign": _resign}
_OFF = {"forced_playouts": lambda v: v[0] == 0.0, "eval_mirror": lambda v: v == 0.0, "solver": lambda v: not v}


class SearchSettings:
    """playout_cap (n_fast, p_full), forced_playouts (k, prune), eval_mirror p, solver bool, fpu (r, r_root) and resign (v,
    playthrough, min_ply), normalised; None where the keyword was not named or was None.

    A field that is None LEAVES the engine's setting alone: apply() does not call its setter.  A named setting may be in its OFF
    form (k = 0, p = 0, solver=False; a cap and fpu have none as keywords), and what that means is the one difference between the
    facades - stated here, by `off` of from_kwargs:
      "clear"   the off form stays in the record and apply() calls the setter with it, which clears what the engine carries
                (SelfPlayStream, which is handed an engine that may carry settings; the Analyzer's eval_mirror=0);
      "absent"  the off form is the same as not naming the keyword: None (ExampleGenerator, the arena, the tools - they build
                their engines, so there is nothing to clear)."""

    def __init__(self, given=None, **fields):
        self.given = dict(given or {})  # the keywords as they came, for the messages
        for key in KEYS:
            setattr(self, key, fields.get(key))

    @classmethod
    def from_kwargs(cls, kwargs, off="absent"):
        if off not in ("clear", "absent"):
            raise ValueError("off must be \"clear\" or \"absent\"")
        given = {k: kwargs[k] for k in KEYS if kwargs.get(k) is not None}
        fields = {k: _PARSE[k](v) for k, v in given.items()}
        if off == "absent":
            fields = {k: v for k, v in fields.items() if not (k in _OFF and _OFF[k](v))}
        return cls(given, **fields)

    def __eq__(self, other):
        return isinstance(other, SearchSettings) and all(getattr(self, k) == getattr(other, k) for k in KEYS)

    def __repr__(self):
        return "SearchSettings(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in KEYS if getattr(self, k) is not None)

    def check(self, context=None, is_test=False, use_puct=True, n_playouts=100, overlap=1):
        """The rules a self-play facade states before it has an engine (ValueError).  context(what): the facade's own refusal of a
        setting that is a side table of ONE engine (ExampleGenerator._check_start_positions), asked for a playout cap."""
        if self.playout_cap is not None:
            n_fast, p_full = self.playout_cap
            if not 1 <= n_fast <= n_playouts or not 0.0 <= p_full <= 1.0:
                raise ValueError("playout_cap=(n_fast, p_full) needs 1 <= n_fast <= n_playouts = %d and 0 <= p_full <= 1, got %r"
                                 % (n_playouts, self.given["playout_cap"]))
            if context is not None:
                context("playout_cap")
            if overlap > 1:
                raise ValueError("playout_cap is not supported with overlap > 1: the capped generation is ticked on one stream")
        if self.resign is not None and is_test:
            raise ValueError("resign is a self-play setting: it is not supported with is_test=True (evaluation games are played to "
                             "their end)")
        why_not_test = {"forced_playouts": "record no policy target", "eval_mirror": "show the network every position as it is",
                        "solver": "measure the reference's search", "fpu": "measure the reference's search"}
        why_puct = {"forced_playouts": "the rules are stated for the PUCT value", "solver": "its select rule is stated for the PUCT value",
                    "fpu": "that rule already values an unvisited child at +infinity"}
        for key in ("forced_playouts", "eval_mirror", "solver", "fpu"):
            if key not in self.given or (key == "solver" and not self.solver):  # (an off k or p that was named is still asked)
                continue
            if is_test:
                raise ValueError("%s is a self-play setting: it is not supported with is_test=True (evaluation games %s)"
                                 % (key, why_not_test[key]))
            if not use_puct and key in why_puct:
                raise ValueError("%s is not supported with use_puct=False: %s" % (key, why_puct[key]))
            if key == "solver" and self.forced_playouts is not None and self.forced_playouts[0] > 0.0:
                raise ValueError("solver is not supported together with forced_playouts")
        return self

    def apply(self, engine):
        """The setters of the settings every engine of a facade carries, in the one order (which setter refuses first shows):
        forced playouts, mirror, solver, fpu, resignation.  The cap is a side table of one engine: the path that reads its mask sets it."""
        if self.forced_playouts is not None:
            engine.set_forced_playouts(*self.forced_playouts)
        if self.eval_mirror is not None:
            engine.set_eval_mirror(self.eval_mirror)
        if self.solver is not None:
            engine.set_solver(self.solver)
        if self.fpu is not None:
            engine.set_fpu(*self.fpu)
        if self.resign is not None:
            engine.set_resign(*self.resign)

    def apply_arena(self, engine):
        """The arena counterpart (SelfPlayEngine.set_arena_search): nothing on, nothing called."""
        if self.resign is not None:
            raise ValueError("resign is a self-play setting: an arena engine plays every evaluation game to its end")
        if self.fpu is not None or self.solver or self.eval_mirror:
            engine.set_arena_search(fpu=self.fpu, solver=bool(self.solver), eval_mirror=self.eval_mirror or 0.0)
