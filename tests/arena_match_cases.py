"""The cases of tests/test_arena_match_host.py and tests/test_arena_match_gpu.py: evaluation games in plain Python between an
AlphaZeroBot outside self-play and a bot, or between two such agents, with the settings of az_engine_set_arena_search
(include/az_engine.h) and an opening per game (az_engine_set_arena_openings).  The search and the move step are those of
tests/search_model.py - playout, proven_counts and choose_move, which carry first-play urgency, the MCTS-Solver and the evaluation
mirror.  The agent loop restates orc_play_arena_game / orc_play_duel_game and orc_bot_step of oracle/az_oracle.c: the agent of
game i plays player (i & 1) ^ flip, its tree is kept across both players' moves, update_root runs only with >= 2 moves played
(alphazerobot.py:60-64), the move is the first maximum of the tempered visit fractions or - use_probabilistic_actions - a sample
of them with the uniform of the Philox move stream (seed, game id, ply, purpose 1).  The bot's moves come from
orc.opponent_action.  With every setting off and an empty opening the games are the C oracle's, which
tests/test_arena_match_host.py pins.  No test lives here."""
import numpy as np

import eval_mirror_cases as EM
import search_model as SM
import solver_cases as SC
from alphazero_openspiel_amd import games
from mirror_cases import action_mirror_table
from oracle import binding as orc
from oracle import fakepolicy
from philox_cases import cap_uniform
from search_model import DRAW, LOSS, UNKNOWN, WIN   # (the tests read them here)

C4, B66 = "connect_four", "breakthrough(rows=6,columns=6)"
FPU = (0.3, 0.1)
# the single settings and all three together, as the parity tests run every game
SETTINGS = {
    "fpu": dict(fpu=FPU),
    "solver": dict(solver=True),
    "mirror": dict(eval_mirror=0.5),
    "all": dict(fpu=FPU, solver=True, eval_mirror=0.5),
}


class Agent:
    """AlphaZeroBot(self_play=False) with its MCTS (orc_bot_step), root noise off.  salt: the fake network's; seed: the engine's
    (the mirror's coins and the move stream are keyed by it); fpu, solver, eval_mirror: az_engine_set_arena_search."""

    def __init__(self, game, salt, seed, game_id, n_playouts, c_puct=2.5, temperature=1.0, keep_search_tree=True, use_puct=True,
                 use_probabilistic_actions=False, num_probabilistic_actions=1000, fpu=None, solver=False, eval_mirror=0.0):
        self.salt, self.seed, self.gid = salt, seed, game_id
        self.S, self.temperature, self.keep, self.use_puct = n_playouts, temperature, keep_search_tree, use_puct
        self.n_prob = (int(num_probabilistic_actions) if int(num_probabilistic_actions) > 0 else 0) if use_probabilistic_actions else 0
        self.settings = SM.Settings(c_puct, 0.0, bool(solver), fpu)
        self.p_mirror = float(eval_mirror or 0.0)
        self.table = action_mirror_table(games.load_game(game)) if self.p_mirror > 0.0 else None
        self.root = SM.Node(None, 0.0, True)                            # MCTS.__init__ builds a PUCT root (mcts.py:122)
        self.steps = []                                                 # one dict per move of the agent
        self.mirrored = [0, 0]                                          # requests evaluated as they are / mirrored
        self.fpu_differs = 0                                            # selections the FPU rule made differently
        self.counters = dict.fromkeys(SM.COUNTERS, 0)

    def step(self, state, hist):
        """AlphaZeroBot.step (alphazerobot.py:42-93) in `state`, reached by the moves `hist` from the initial position."""
        A, solver = int(state.num_actions), self.settings.solver
        if self.keep:
            if len(hist) >= 2:                                          # alphazerobot.py:60-64
                self.root = SM.update_root(SM.update_root(self.root, hist[-2], self.use_puct), hist[-1], self.use_puct)
        else:
            self.root = SM.Node(None, 0.0, True)
        root = self.root
        kept_status = root.status
        ran = 0

        def evaluate(s):
            flip = self.p_mirror > 0.0 and bool(EM.coin(self.seed, self.gid, len(hist), EM.PH_WAIT_LEAF, ran, self.p_mirror))
            self.mirrored[int(flip)] += 1
            return SM.evaluate(lambda b: fakepolicy.fake_eval(b, A, self.salt), s, flip, self.table)

        for _ in range(self.S):
            if solver and root.status != UNKNOWN:                       # rule 5: also a kept subtree that is already proven
                break
            self.fpu_differs += len(SM.playout(root, state.clone(), self.settings, evaluate, self.counters).fpu_differs)
            ran += 1
        raw = [c.N for c in root.children]
        counts = SM.proven_counts(root, raw) if solver else list(raw)   # rule 6, before the move is drawn
        u = cap_uniform(self.seed, self.gid, len(hist), purpose=1, idx=0) if len(hist) < self.n_prob else None   # the move stream
        move, _ = SM.choose_move(root, counts, state.legal_actions(), A, self.temperature, u)
        rec = dict(ply=len(hist), status=root.status, kept_status=kept_status, raw=raw, counts=counts, actions=list(root.actions),
                   child_status=[c.status for c in root.children], ran=ran, move=move)
        if root.status != UNKNOWN:
            rec["statuses"] = SM.tree_statuses(root)[0]                 # the order of SelfPlayEngine.read_proofs
        self.steps.append(rec)
        return move


def agent_side(game_id, flip=0):
    return (game_id & 1) ^ flip


def play_arena_game(game, game_id, salt, seed, opening=(), opponent="uct", opponent_sims=0, opponent_uct_c=1.0, **agent_kw):
    """orc_play_arena_game from the position after `opening`: the agent plays player game_id & 1, the bot the other side with the
    moves of orc.opponent_action (Philox stream (seed, game id, ply, purpose 2)).  -> dict(actions: the moves PLAYED (without the
    opening), ret0, game_len, agent)."""
    state, hist = orc.State(game), []
    for a in opening:
        state.apply_action(a)
        hist.append(int(a))
    agent = Agent(game, salt, seed, game_id, **agent_kw)
    while not state.is_terminal():
        if (len(hist) & 1) == agent_side(game_id):
            move = agent.step(state, hist)
        else:
            move = orc.opponent_action(state, opponent, opponent_sims, opponent_uct_c, seed, game_id)
        state.apply_action(move)
        hist.append(int(move))
    played = hist[len(opening):]
    return {"actions": played, "ret0": state.player_return(0), "game_len": len(played), "agent": agent}


def play_duel_game(game, game_id, kw_a, kw_b, opening=()):
    """orc_play_duel_game from the position after `opening`: agent A (kw_a: salt, seed, n_playouts, ... of Agent) plays player
    game_id & 1, agent B the other side.  -> dict(actions, ret0, game_len, a, b)."""
    state, hist = orc.State(game), []
    for a in opening:
        state.apply_action(a)
        hist.append(int(a))
    bots = (Agent(game, game_id=game_id, **kw_a), Agent(game, game_id=game_id, **kw_b))
    while not state.is_terminal():
        bot = bots[0] if (len(hist) & 1) == agent_side(game_id) else bots[1]
        move = bot.step(state, hist)
        state.apply_action(move)
        hist.append(int(move))
    played = hist[len(opening):]
    return {"actions": played, "ret0": state.player_return(0), "game_len": len(played), "a": bots[0], "b": bots[1]}


# ------------------------------------------------------------------------------------------------ the shared cases
def legal_random_prefix(game, seed, plies):
    """`plies` random legal moves from the initial position that do not end the game (a seeded generator, retried)."""
    r = np.random.RandomState(7000 + seed)
    while True:
        s, hist = orc.State(game), []
        while len(hist) < plies and not s.is_terminal():
            a = int(r.choice(s.legal_actions()))
            s.apply_action(a)
            hist.append(a)
        if len(hist) == plies and not s.is_terminal():
            return hist


# arena parity: 5 slots, 12 games (slots refill from the table mid-run), openings of mixed length - odd and even, so the first
# phase is the agent's in some games and the opponent's in others, for both parities of the game id
ARENA_SEED, ARENA_SALT, ARENA_SLOTS, ARENA_GAMES = 2024, 6, 5, 12
ARENA = {
    "c4_uct": dict(game=C4, S=24, opponent="uct", sims=40, lengths=[0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 4]),
    "c4_random": dict(game=C4, S=24, opponent="random", sims=0, lengths=[0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 4]),
    "bt6_uct": dict(game=B66, S=12, opponent="uct", sims=20, lengths=[0, 1, 2, 3, 3, 2, 1, 0, 2, 3, 0, 1]),
}


def arena_openings(key):
    c = ARENA[key]
    return [legal_random_prefix(c["game"], 31 * i + n, n) for i, n in enumerate(c["lengths"])]


# the solver case: connect_four from late positions (solver_cases.c4_late_prefix(seed, empties)) with 12-14 empty cells, one game
# per slot; picked on the CPU so that the agent moves at roots proven won, drawn and lost, at subtrees that were already proven
# when the opponent's move re-rooted onto them, and with counts that rule 6 changes (tests/test_arena_match_host.py asserts it)
SOLVER_CASE = dict(game=C4, S=24, opponent="uct", sims=40, seed=77, salt=13,
                   starts=[(24, 14), (22, 12), (25, 13), (3, 13), (22, 12), (15, 14), (3, 13), (22, 13)])


def solver_openings():
    return [SC.c4_late_prefix(s, e) for s, e in SOLVER_CASE["starts"]]


# duel parity: 10 games, paired openings (games 2k and 2k + 1 share one), A with FPU and the solver, B with the mirror
DUEL_SEED = 5
DUEL = {
    "c4": dict(game=C4, S=24, lengths=[0, 1, 2, 3, 4]),
    "bt6": dict(game=B66, S=12, lengths=[0, 1, 2, 3, 2]),
}
DUEL_A = dict(salt=3, c_puct=2.5, fpu=FPU, solver=True)
DUEL_B = dict(salt=8, c_puct=1.5, eval_mirror=0.5)


def duel_openings(key):
    c = DUEL[key]
    pairs = [legal_random_prefix(c["game"], 100 + 17 * k, n) for k, n in enumerate(c["lengths"])]
    return [pairs[i // 2] for i in range(2 * len(pairs))]


_MODEL = {}


def arena_models(key, setting):
    """The model's ARENA_GAMES games of ARENA[key] under SETTINGS[setting] (None: nothing set); computed once."""
    if ("arena", key, setting) not in _MODEL:
        c = ARENA[key]
        ops = arena_openings(key)
        kw = dict(SETTINGS[setting]) if setting else {}
        _MODEL["arena", key, setting] = [
            play_arena_game(c["game"], i, ARENA_SALT, ARENA_SEED, opening=ops[i], opponent=c["opponent"], opponent_sims=c["sims"],
                            n_playouts=c["S"], **kw) for i in range(ARENA_GAMES)]
    return _MODEL["arena", key, setting]


def solver_models():
    if "solver" not in _MODEL:
        c = SOLVER_CASE
        _MODEL["solver"] = [play_arena_game(c["game"], i, c["salt"], c["seed"], opening=op, opponent=c["opponent"],
                                            opponent_sims=c["sims"], n_playouts=c["S"], solver=True)
                            for i, op in enumerate(solver_openings())]
    return _MODEL["solver"]


def duel_models(key):
    """The model's duel games of DUEL[key]: engine A is reset with DUEL_SEED, engine B with DUEL_SEED + 1 (arena.run_duel)."""
    if ("duel", key) not in _MODEL:
        c = DUEL[key]
        ops = duel_openings(key)
        _MODEL["duel", key] = [play_duel_game(c["game"], i, dict(DUEL_A, seed=DUEL_SEED, n_playouts=c["S"]),
                                              dict(DUEL_B, seed=DUEL_SEED + 1, n_playouts=c["S"]), opening=ops[i])
                               for i in range(len(ops))]
    return _MODEL["duel", key]
