"""Evaluation arena on the device: the network-driven agent against a bot, thousands of games at a time.

Reference: `game_utils.play_game` and the `test_*_vs_*` pairings (game_utils.py:16-145), driven in bulk by
`ExampleGenerator(is_test=True).generate_tests` (examplegenerator.py:25-37,177-195) from `Trainer.test_agent`
(train.py:238-270).  There every test is a worker process playing two games (agent first, agent second) with a pipe
round trip per leaf; here all games of an evaluation are slots of one engine:

  agent "zero"    AlphaZeroBot outside self-play (alphazerobot.py:42-93): n_playouts of PUCT search per move, no root
                  noise, the most visited move, tree kept across both players' moves      - az_advance_kernel
  agent "net"     NeuralNetBot (alphazerobot.py:96-120): argmax of the masked, renormalised priors
  opponent "uct"  open_spiel MCTSBot(uct_c, max_search_nodes, RandomRolloutEvaluator(1))   - az_opponent_kernel
  opponent "random"  pyspiel.make_uniform_random_bot

One arena tick = [az_engine_advance, az_engine_opponent_moves, PV-net forward].  Game id i gives the agent side i & 1:
the pair (2k, 2k+1) is one reference `test_*` call and scores  ret0(2k) - ret0(2k+1)  (score1 + score2).

Beyond the reference: a "zero" agent may search with first-play urgency, the MCTS-Solver or the evaluation mirror
(SelfPlayEngine.set_arena_search) and every game may start from its own opening (set_arena_openings); play_match puts two
settings head to head over paired openings - each opening played twice with the colours swapped, scored per pair.
"""
import math

import numpy as np
import torch

from .engine import EngineError, SearchSettings, SelfPlayEngine, TickDriver, close_all, default_device, make_evaluator, tick_until
from .games import load_game
from .search_settings import ARENA_KEYS

ENGINE_KW = ("n_playouts", "c_puct", "temperature", "keep_search_tree", "use_puct", "use_probabilistic_actions",
              "num_probabilistic_actions")
SEARCH_KW = ARENA_KEYS  # SelfPlayEngine.set_arena_search: the settings an arena agent may carry


def _apply_search(engine, settings, openings):
    """set_arena_search / set_arena_openings for what `settings` (a dict) and `openings` name; nothing named, nothing called."""
    SearchSettings.from_kwargs({k: settings.get(k) for k in SEARCH_KW + ("resign",)}).apply_arena(engine)  # (resign: refused there)
    if openings is not None:
        engine.set_arena_openings(openings)


def arena_engine(game, n_slots, n_games, agent, opponent, opponent_sims=0, device=0, seed=0, openings=None, **kwargs):
    """An engine configured for evaluation games.  kwargs: the AlphaZeroBot keywords the reference passes through
    (n_playouts default 100: mcts.py:98; c_puct, temperature; dirichlet_ratio is accepted and unused: the test pairings
    construct the bot with use_dirichlet=False, game_utils.py:72), and the agent's search settings fpu=, solver=, eval_mirror=
    (SelfPlayEngine.set_arena_search).  openings: one action list per game (set_arena_openings)."""
    kw = {k: kwargs[k] for k in ENGINE_KW if k in kwargs}
    if agent == "net":
        kw.update(n_playouts=1, keep_search_tree=False)
    else:
        kw.setdefault("n_playouts", 100)
    eng = SelfPlayEngine(game, n_slots, max_games=n_games, device=device, seed=seed, use_dirichlet=False,
                         arena_agent=agent, opponent=opponent, opponent_sims=opponent_sims,
                         opponent_uct_c=float(kwargs.get("opponent_uct_c", 1.0)), **kw)
    try:
        _apply_search(eng, kwargs, openings)
    except Exception:
        eng.close()
        raise
    return eng


def random_openings(game_name, n, plies, seed):
    """n DISTINCT openings of `plies` uniformly random legal moves each from the initial position, none of which ends the game
    -> list of n action lists.  Host code (games.py); a function of (game_name, n, plies, seed) alone.  ValueError when the game
    does not have n distinct openings of that length (found out by running dry: 64 * n + 1024 draws without n distinct ones)."""
    game = load_game(game_name) if isinstance(game_name, str) else game_name
    n, plies = int(n), int(plies)
    if n < 0 or plies < 0:
        raise ValueError("random_openings: n and plies must be >= 0")
    rng = np.random.RandomState(int(seed) & 0xFFFFFFFF)
    seen, out = set(), []
    for _ in range(64 * n + 1024):
        if len(out) == n:
            break
        s, hist = game.new_initial_state(), []
        while len(hist) < plies and not s.is_terminal():
            legal = s.legal_actions()
            a = int(legal[int(rng.randint(len(legal)))])
            s.apply_action(a)
            hist.append(a)
        if len(hist) == plies and not s.is_terminal() and tuple(hist) not in seen:
            seen.add(tuple(hist))
            out.append(hist)
    if len(out) < n:
        raise ValueError("random_openings: found only %d distinct %d-ply openings of %s, %d asked for" % (len(out), plies, game, n))
    return out


def elo_of(p):
    """-400 log10(1 / p - 1): the Elo difference at which the expected score (a win 1, a draw 1/2) is p; -inf / +inf at the ends."""
    if p <= 0.0:
        return -math.inf
    if p >= 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / p - 1.0) + 0.0  # (+ 0.0: p = 1/2 gives 0.0, not -0.0)


def match_stats(ret0, flip=False):
    """The statistics of a paired match from ret0 [2 * n_pairs] = returns()[0] of every game, seen from the agent that plays
    player i & 1 in game i (flip: from the other side): games (2k, 2k+1) are ONE opening played from both sides, so the sample
    is the n_pairs pair scores (score1 + score2) / 2 in [-1, 1] - the two games of a pair are not independent.
    -> dict(wins, draws, losses, pair_scores float64 [n_pairs], score = their mean, stderr = their sample standard deviation
    / sqrt(n_pairs) (0 with one pair), elo / elo_lo / elo_hi = elo_of at p = (score + 1) / 2 and at p -/+ 1.96 * stderr / 2)."""
    r = np.asarray(ret0, dtype=np.float64).reshape(-1)
    if r.size == 0 or r.size % 2:
        raise ValueError("a paired match has 2 * n_pairs games, got %d" % r.size)
    s1, s2 = pair_scores(r)
    mine = np.empty_like(r)
    mine[0::2], mine[1::2] = s1, s2
    if flip:
        mine = -mine
    ps = (mine[0::2] + mine[1::2]) / 2.0
    n = ps.size
    score = float(ps.mean())
    stderr = float(ps.std(ddof=1) / math.sqrt(n)) if n > 1 else 0.0
    p = (score + 1.0) / 2.0
    half = 1.96 * stderr / 2.0
    return {"wins": int((mine > 0).sum()), "draws": int((mine == 0).sum()), "losses": int((mine < 0).sum()),
            "pair_scores": ps, "score": score, "stderr": stderr,
            "elo": elo_of(p), "elo_lo": elo_of(p - half), "elo_hi": elo_of(p + half)}


def run_arena(engine, evaluator, n_games, seed=None, check_every=16, use_graph=True, max_ticks=None):
    """Play n_games evaluation games (ids 0..n_games-1; the agent has side id & 1).  Returns (ret0 [n_games] float32 =
    returns()[0] of every game, progress dict)."""
    engine.reset(n_games, seed)
    obs, pri, val = engine.alloc_io()

    def tick():
        engine.advance(pri, val, obs)
        engine.opponent_moves()
        evaluator(obs, pri, val)

    drv = TickDriver(engine.device, tick)
    if use_graph:
        drv.capture()
    tick_until(drv, check_every, lambda: engine.games_done() >= n_games, max_ticks, "arena", engine)
    prog = engine.progress()
    prog["ticks"] = drv.ticks
    ex = engine.export()
    return ex["game_ret0"].copy(), prog, ex


def pair_scores(ret0):
    """ret0 of games (2k, 2k+1) -> (score1, score2) per pair as the reference's test functions return them: score1 = the
    agent's result as first player, score2 = minus the first player's result when the agent is second (game_utils.py:76-82)."""
    r = np.asarray(ret0, dtype=np.float64)
    return r[0::2], -r[1::2]


def run_duel(eng_a, eng_b, ev_a, ev_b, n_games, seed=None, check_every=16, use_graph=True, max_ticks=None):
    """Two arena engines facing each other (opponent="external", arena_flip False / True), each with its own evaluator:
    test_zero_vs_zero (game_utils.py:120-145).  Games = slots (no refill).  Returns (ret0 [n_games], progress of a)."""
    if n_games > eng_a.G or eng_a.G != eng_b.G:
        raise EngineError("a duel plays one game per slot: n_games <= n_slots, equal on both engines")
    eng_a.reset(n_games, seed)
    eng_b.reset(n_games, None if seed is None else seed + 1)
    io_a, io_b = eng_a.alloc_io(), eng_b.alloc_io()

    def tick():
        eng_a.advance(io_a[1], io_a[2], io_a[0])
        eng_b.advance(io_b[1], io_b[2], io_b[0])
        eng_a.exchange_moves(eng_b)
        ev_a(*io_a)
        ev_b(*io_b)

    drv = TickDriver(eng_a.device, tick)
    if use_graph:
        drv.capture()
    tick_until(drv, check_every, lambda: eng_a.games_done() >= n_games and eng_b.games_done() >= n_games, max_ticks,
               "duel", eng_a, eng_b)
    prog = eng_a.progress()
    prog["ticks"] = drv.ticks
    ex_a, ex_b = eng_a.export(), eng_b.export()
    if not ((ex_a["game_len"] == ex_b["game_len"]).all() and (ex_a["game_ret0"] == ex_b["game_ret0"]).all()):
        raise EngineError("the two engines of a duel disagree about the games they played")
    return ex_a["game_ret0"].copy(), prog, ex_a


def play_zero_vs_zero(policy_fn, policy_fn2, game_name, n_tests, settings1=None, settings2=None, device=None, seed=None,
                      eval_backend="fused", eval_precision="f32x", use_dirichlet=True):
    """n_tests `test_zero_vs_zero` calls (2 games each: network 1 first, network 1 second) in one batch: two AlphaZero agents
    with their own networks and settings (n_playouts, c_puct, ...), both with root noise as in the reference
    (game_utils.py:131-132).  -> (score1 [n_tests], score2 [n_tests], progress), scores from network 1's point of view."""
    device = torch.device(device if device is not None else default_device(policy_fn))
    n_games = 2 * int(n_tests)
    if n_games > 4096:
        raise ValueError("at most 2048 tests per call (one game per slot)")
    seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
    engines, evals = [], []
    try:
        for flip, (fn, settings) in enumerate(((policy_fn, settings1), (policy_fn2 if policy_fn2 is not None else policy_fn, settings2))):
            kw = {k: v for k, v in dict(settings or {}).items() if k in ENGINE_KW + ("dirichlet_ratio",)}
            kw.setdefault("n_playouts", 100)
            engines.append(SelfPlayEngine(game_name, n_games, max_games=n_games, device=device, seed=seed + 17 * flip,
                                          use_dirichlet=use_dirichlet, arena_agent="zero", opponent="external", arena_flip=bool(flip), **kw))
            evals.append(make_evaluator(fn, device, eval_backend, eval_precision, n_games))
        ret0, prog, _ = run_duel(engines[0], engines[1], evals[0], evals[1], n_games, seed=seed)
    finally:
        close_all(*engines, *evals)
    s1, s2 = pair_scores(ret0)
    return s1, s2, prog


def play_match(policy_a, policy_b, game_name, n_pairs, settings_a=None, settings_b=None, openings=None, device=None, seed=None,
               eval_backend="fused", eval_precision="f32x", use_dirichlet=False, use_graph=True, check_every=16, max_ticks=None):
    """A match between two search settings (and / or two networks) over paired openings: a duel of 2 * n_pairs games in which
    games 2k and 2k + 1 both start from openings[k] - A moves as player 0 in the one and as player 1 in the other - so an
    opening that favours one colour favours both sides once.  settings_*: the ENGINE_KW keys plus fpu, solver and eval_mirror
    (SelfPlayEngine.set_arena_search).  openings: n_pairs action lists (random_openings), None = every game from the initial
    position.  policy_b None = policy_a.  Root noise is off unless use_dirichlet: with greedy agents the openings are what
    makes the games differ.  It runs through run_duel (one captured graph when use_graph).
    -> match_stats(ret0) seen from A (wins, draws, losses, pair_scores, score, stderr, elo, elo_lo, elo_hi) plus progress."""
    device = torch.device(device if device is not None else default_device(policy_a))
    n_pairs = int(n_pairs)
    n_games = 2 * n_pairs
    if n_pairs < 1 or n_games > 4096:
        raise ValueError("between 1 and 2048 pairs per call (one game per slot)")
    if openings is not None and len(openings) != n_pairs:
        raise ValueError("%d openings for %d pairs" % (len(openings), n_pairs))
    seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
    table = None if openings is None else [list(openings[k // 2]) for k in range(n_games)]
    engines, evals = [], []
    try:
        for flip, (fn, settings) in enumerate(((policy_a, settings_a), (policy_b if policy_b is not None else policy_a, settings_b))):
            settings = dict(settings or {})
            unknown = sorted(set(settings) - set(ENGINE_KW) - set(SEARCH_KW))
            if unknown:
                raise ValueError("unknown match settings %s (known: %s)" % (unknown, ", ".join(ENGINE_KW + SEARCH_KW)))
            kw = {k: v for k, v in settings.items() if k in ENGINE_KW}
            kw.setdefault("n_playouts", 100)
            engines.append(SelfPlayEngine(game_name, n_games, max_games=n_games, device=device, seed=seed + 17 * flip,
                                          use_dirichlet=use_dirichlet, arena_agent="zero", opponent="external", arena_flip=bool(flip), **kw))
            _apply_search(engines[-1], settings, table)
            evals.append(make_evaluator(fn, device, eval_backend, eval_precision, n_games))
        ret0, prog, _ = run_duel(engines[0], engines[1], evals[0], evals[1], n_games, seed=seed, check_every=check_every,
                                 use_graph=use_graph, max_ticks=max_ticks)
    finally:
        close_all(*engines, *evals)
    out = match_stats(ret0)
    out["progress"] = prog
    return out


def play_tests(policy_fn, game_name, n_tests, agent, opponent, opponent_sims=0, device=None, seed=None, n_slots=None,
               eval_backend="fused", eval_precision="f32x", openings=None, **kwargs):
    """n_tests reference `test_*` calls (2 * n_tests games) in one batch -> (score1 [n_tests], score2 [n_tests], progress).
    kwargs may carry the agent's search settings fpu=, solver=, eval_mirror= (arena_engine); openings: one action list per
    GAME (2 * n_tests; give games 2k and 2k + 1 the same one for a paired test)."""
    device = torch.device(device if device is not None else default_device(policy_fn))
    n_games = 2 * int(n_tests)
    n_slots = int(n_slots or min(n_games, 4096))
    seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
    eng = arena_engine(game_name, n_slots, n_games, agent, opponent, opponent_sims, device=device, seed=seed, openings=openings,
                       **kwargs)
    ev = make_evaluator(policy_fn, device, eval_backend, eval_precision, n_slots)
    try:
        ret0, prog, _ = run_arena(eng, ev, n_games)
    finally:
        close_all(eng, ev)
    s1, s2 = pair_scores(ret0)
    return s1, s2, prog
