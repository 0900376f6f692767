/*
 * az_engine.h — C ABI of the MI355X-native AlphaZero self-play engine.
 *
 * This is the drop-in boundary for ONE path of danielwillemsen/alphazero-openspiel:
 * PUCT tree search (mcts.py) + self-play rollout loop (game_utils.py:148-206) +
 * agent step (alphazerobot.py:42-93) + game dynamics / state encoding
 * (pyspiel calls, network.py:9-18), run for G concurrent games on one GPU.
 * Leaf evaluation (network.py:48-64) is the caller's: the engine hands out a
 * device batch of observations and takes back device priors/values, so the
 * reference's multiprocess pipe protocol (examplegenerator.py:39-77) has no
 * equivalent here — its two messages are the two pointer arguments of
 * az_engine_advance().
 *
 * Conventions: every entry returns 0 on success, a negative AZ_E_* otherwise;
 * no C++ exception crosses this boundary; az_last_error() gives the text.
 * "dev" pointers are HIP device pointers owned by the caller; `stream` is a
 * hipStream_t passed as void* (NULL = the default stream).  All device work is
 * asynchronous on that stream unless a function says it synchronises.
 * The engine is not re-entrant: one host thread per engine, one engine (or
 * more) per GPU, one process per GPU.
 */
#ifndef AZ_ENGINE_H
#define AZ_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_GAME_CONNECT_FOUR 0 /* "connect_four"                      (train.py:24) */
#define AZ_GAME_BREAKTHROUGH 1 /* "breakthrough(rows=R,columns=C)"    (train.py:24, tournament.py) */

/* value-target modes of play_game_self (game_utils.py:166-194) */
#define AZ_BACKUP_ON_POLICY 0
#define AZ_BACKUP_SOFT_Z 1
#define AZ_BACKUP_A0C 2
#define AZ_BACKUP_OFF_POLICY 3

#define AZ_RNG_PHILOX 0   /* on-device Philox4x32-10 streams keyed by (seed, game id, ply) */
#define AZ_RNG_INJECTED 1 /* Dirichlet vectors and choice-uniforms supplied by the caller (parity mode) */

#define AZ_OK 0
#define AZ_E_INVALID (-1)   /* bad argument / config */
#define AZ_E_HIP (-2)       /* a HIP runtime call failed */
#define AZ_E_STATE (-3)     /* call order violated (e.g. advance before reset) */
#define AZ_E_DEVICE (-4)    /* a device-side fault flag is set (see az_progress.error_flags) */
#define AZ_E_NOMEM (-5)

/* device-side fault bits, OR-ed into az_progress.error_flags */
#define AZ_FAULT_POOL_EXHAUSTED 1u /* a slot's node pool is full even after compaction */
#define AZ_FAULT_PLY_OVERFLOW 2u   /* a game exceeded max_plies */
#define AZ_FAULT_NO_VISITS 4u      /* root has no visited child at move time (S too small) */
#define AZ_FAULT_BAD_PRIOR 8u      /* NaN prior/value fed to advance */
#define AZ_FAULT_ILLEGAL_ACTION 16u /* az_engine_update_root was given an action that is illegal in the slot's root state */
#define AZ_FAULT_VISIT_RANGE 32u    /* AZ_SELECT_UCT: a node's visit count left the log(N) table (N > n_playouts * (max_plies + 2)) */

#define AZ_ACTION_NONE (-1)         /* az_engine_update_root: leave the slot alone */
#define AZ_ACTION_SEARCH_AGAIN (-2) /* az_engine_update_root: search the same root again (MCTS.search called twice, mcts.py:164-180) */

/*
 * Search/agent configuration.  Field ↔ reference keyword (all reach the
 * reference's search as **kwargs: SURVEY.md §5 "Config / flag system"):
 *   n_playouts, c_puct, use_dirichlet, dirichlet_ratio   mcts.py:96-101
 *   temperature                                          alphazerobot.py:38
 *   keep_search_tree                                     alphazerobot.py:26,54-68
 *   backup                                               game_utils.py:155
 * dirichlet_alpha is the literal 0.3 of mcts.py:187; the noise weight is the
 * literal 0.25 of mcts.py:189 (NOT dirichlet_ratio) — reproduced as such.
 */
typedef struct az_config {
    int32_t struct_size; /* = sizeof(az_config); ABI guard */
    int32_t game;        /* AZ_GAME_* */
    int32_t rows, cols;  /* breakthrough board (connect_four: 6,7 enforced) */
    int32_t n_slots;     /* G: concurrent games resident on the device */
    int32_t n_playouts;  /* S */
    int32_t use_dirichlet;
    int32_t keep_search_tree;
    int32_t backup;            /* AZ_BACKUP_* */
    int32_t rng_mode;          /* AZ_RNG_* */
    int32_t max_sims_per_tick; /* bound on NN-free playouts (terminal hits) one slot chains per advance; 0 = default (10) */
    int32_t device;            /* HIP device ordinal */
    int32_t manual_moves;      /* 1: stop after each search (MCTS.search semantics); the caller reads the root and
                                  moves with az_engine_update_root — AlphaZeroBot.step outside self-play */
    int32_t chain_window_us;   /* a slot starts another NN-free playout only this early in a launch; 0 = default (10), <0 = off */
    int64_t nodes_per_slot;    /* node-pool capacity per slot; 0 = default from game and S */
    int64_t max_games;         /* capacity of the example store (games per reset) */
    double c_puct;
    double dirichlet_ratio;
    double dirichlet_alpha;
    double temperature;
    uint64_t seed;
    /* Evaluation arena (game_utils.py:16-145, examplegenerator.py:177-195, train.py:238-270): every game is played
     * between an AGENT driven by the network and an OPPONENT bot; game id i gives the agent the side i & 1, so the pair
     * (2k, 2k+1) is one `test_*_vs_*` call of the reference (agent first, then agent second).  0 / 0 = self-play. */
    int32_t arena_agent;    /* AZ_ARENA_* */
    int32_t arena_opponent; /* AZ_OPPONENT_* */
    int32_t opponent_sims;  /* AZ_OPPONENT_UCT: max_search_nodes of mcts.MCTSBot (game_utils.py:74-75) */
    int32_t arena_flip;     /* 1: the agent takes the OTHER side, (i & 1) ^ 1 - the second network of a two-engine pairing */
    double opponent_uct_c;  /* AZ_OPPONENT_UCT: uct_c (1 in the reference's calls) */
    /* MCTS(use_puct=...) (mcts.py:101,120): the rule of the trees that update_root STARTS when it finds a leaf root
     * (mcts.py:199-200).  The reference keeps the rule per Node, children inherit their parent's (mcts.py:64), and
     * MCTS.__init__ always builds a PUCT root (mcts.py:122): so a tree is PUCT unless it grew from a root created by
     * update_root on a leaf - reproduced here as one rule bit per slot tree.  0 (AZ_SELECT_PUCT) = use_puct=True. */
    int32_t select_rule; /* AZ_SELECT_* */
    /* AlphaZeroBot(use_probabilistic_actions=True) outside self-play (alphazerobot.py:34,83-84; tournament.py:35-36):
     * the AZ_ARENA_ZERO agent samples its move from the tempered visit distribution instead of taking the argmax. */
    int32_t arena_probabilistic;
    /* num_probabilistic_actions (alphazerobot.py:36,81-85): a sampling agent (self-play, or arena_probabilistic) samples
     * only while fewer than this many moves have been played, then plays the argmax.  0 = the reference's default, 1000; < 0 = never sample. */
    int32_t num_probabilistic_actions;
    /* node pools shared as compaction targets (a slot owns one pool of nodes_per_slot nodes; re-rooting copies the kept
     * subtree into a spare pool when the pool cannot hold another search): 0 = default (n_slots / 16, at least 16) */
    int32_t spare_pools;
} az_config;

#define AZ_SELECT_PUCT 0 /* Q + c_puct * P * sqrt(N_parent) / (N + 1)                         mcts.py:78 */
#define AZ_SELECT_UCT 1  /* inf if N == 0 else Q + c_puct * P * sqrt(log(N_parent) / N)       mcts.py:80 */

#define AZ_ARENA_SELF_PLAY 0
#define AZ_ARENA_ZERO 1 /* AlphaZeroBot outside self-play: search, then the most visited move (alphazerobot.py:86-91), tree kept
                           across both players' moves (alphazerobot.py:60-64) */
#define AZ_ARENA_NET 2  /* NeuralNetBot (alphazerobot.py:96-120): one evaluation, argmax of the masked, renormalised priors;
                           configure n_playouts = 1, use_dirichlet = 0, keep_search_tree = 0 */
#define AZ_OPPONENT_NONE 0
#define AZ_OPPONENT_RANDOM 1 /* pyspiel.make_uniform_random_bot: a uniformly random legal action */
#define AZ_OPPONENT_UCT 2    /* open_spiel.python.algorithms.mcts.MCTSBot(game, player, uct_c, max_search_nodes,
                                RandomRolloutEvaluator(1)) - third party, absent from the reference tree, version unpinned:
                                restated from its published algorithm (DESIGN_HISTORY.md section 6) */
#define AZ_OPPONENT_EXTERNAL 3 /* the opponent's moves come from ANOTHER engine (az_engine_exchange_moves): two AlphaZero agents with
                                  their own networks and settings - test_zero_vs_zero (game_utils.py:120-145) */

typedef struct az_sizes {
    int32_t num_actions;  /* A   = game.num_distinct_actions() */
    int32_t obs_planes;   /* C+1 = state_shape[0] + 1 (network.py:15) */
    int32_t rows, cols;   /* H, W */
    int32_t max_children; /* upper bound on legal actions of any state */
    int32_t max_plies;    /* upper bound on game length */
    int32_t n_slots;
    int32_t spare_pools;  /* pools beyond the slots' own: (n_slots + spare_pools) * nodes_per_slot nodes are allocated */
    int64_t nodes_per_slot;
    int64_t max_games;
    int64_t device_bytes; /* HBM held by the engine */
} az_sizes;

typedef struct az_progress {
    int64_t games_started, games_done;
    int64_t moves;         /* AlphaZeroBot.step calls completed */
    int64_t sims;          /* MCTS.playout calls completed */
    int64_t evals;         /* policy_fn requests issued (leaf + root-Dirichlet) */
    int64_t terminal_hits; /* playouts that ended on a terminal state (no evaluation) */
    int64_t sum_depth;     /* Σ select depth over playouts */
    int64_t sum_children;  /* Σ children scanned by select */
    int64_t nodes_allocated;
    int64_t compactions;
    int64_t slots_waiting; /* slots with an evaluation request outstanding after the last advance */
    int64_t slots_idle;
    int64_t slots_search_done; /* manual_moves: slots whose S playouts are complete */
    uint32_t error_flags; /* AZ_FAULT_* */
    uint32_t reserved;
} az_progress;

/* Host view of finished games, valid until the next reset/export/destroy.
 * Replaces the pickled list-of-games a pool returns (examplegenerator.py:151-152,172-173);
 * the Python façade turns each ply into the reference's [key, board, pi, z] record
 * (game_utils.py:169). */
typedef struct az_example_view {
    int64_t n_games;            /* finished games, ids 0..n_games-1 */
    int32_t max_plies;          /* row stride of the per-ply arrays */
    int32_t max_children;       /* row stride of counts/actions */
    const int32_t *game_len;    /* [n_games] plies */
    const float *game_ret0;     /* [n_games] returns()[0] */
    const uint64_t *states;     /* [n_games][max_plies][2] bitboards (layout: az_games.h) */
    const uint16_t *move;       /* [n_games][max_plies] action played */
    const uint8_t *n_children;  /* [n_games][max_plies] number of root children (= legal actions) */
    const uint16_t *child_action; /* [n_games][max_plies][max_children] ascending legal actions */
    const uint32_t *child_visits; /* [n_games][max_plies][max_children] root child N before the move */
    const double *value;        /* [n_games][max_plies] value target (soft-Z / A0C / off-policy; on-policy: filled from ret0) */
} az_example_view;

typedef struct az_engine az_engine;

/* lifecycle ------------------------------------------------------------- */
int az_engine_create(const az_config *cfg, az_engine **out);
int az_engine_destroy(az_engine *e);
const char *az_last_error(const az_engine *e); /* e may be NULL: error of the last failed create */
int az_engine_sizes(const az_engine *e, az_sizes *out);

/* Start a generation of n_games self-play games (ExampleGenerator.generate_examples(n_games),
 * examplegenerator.py:164-175).  Game ids are 0..n_games-1; id i uses RNG stream (seed, i).
 * Slots pick up ids in order and refill from a device-side counter as games finish. */
int az_engine_reset(az_engine *e, uint64_t seed, int64_t n_games, void *stream);

/* Parity mode (rng_mode = AZ_RNG_INJECTED): host arrays, copied.
 * etas [n_games][max_plies][max_children]: the np.random.dirichlet draw of each move (mcts.py:187)
 * us   [n_games][max_plies]: the uniform behind np.random.choice of each move (alphazerobot.py:84) */
int az_engine_set_injected_rng(az_engine *e, const double *etas, const double *us, int64_t n_games);

/* Start every slot from a given position instead of the initial one (test hook for mid-game search
 * traces).  actions: host [n] action prefix applied to the initial state. Call after reset. */
int az_engine_set_start_prefix(az_engine *e, const int32_t *actions, int32_t n);

/* A start position per GAME: game id i (0 <= i < n_games) starts from the position that the action prefix
 * actions[i * stride .. i * stride + lengths[i]) reaches from the initial one (host arrays, copied; 0 <= lengths[i] <= stride).
 * manual_moves engines only - the batched form of MCTS.search(state) for many given states: reset with at most n_games games,
 * tick until every slot has finished its search, read all roots with az_engine_export_roots_device.  Self-play and arena
 * engines return AZ_E_INVALID here: a self-play engine takes its per-game starts, with the record offset, the value targets and
 * the replay keys that go with them, through az_engine_set_game_starts; an arena engine keeps ONE start ply (side assignment).  Every prefix is replayed on the host with the game's legality checks: an illegal action, or a
 * prefix that ends the game, is refused with AZ_E_INVALID and az_last_error names the index of the offending game; nothing is
 * changed then.  As with az_engine_set_start_prefix the caller resets afterwards.  May be called again on the same engine
 * (the next chunk of positions); it supersedes a single prefix, and az_engine_set_start_prefix clears the table.
 * Injected Dirichlet draws are indexed by the state's ply number, as everywhere.  Synchronises the device. */
int az_engine_set_start_positions(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride, int64_t n_games);

/* The device form of az_engine_set_start_positions: game id i starts from the state (bb[i][0], bb[i][1], ply[i]), bit
 * layouts of az_games.h - what az_replay_gather_states writes.  bb_dev: device u64 [n_games][2], ply_dev: device i32 [n_games].
 * manual_moves engines only, 1 <= n_games <= max_games; it fills the same table, supersedes a prefix or an earlier table, and
 * the caller resets afterwards (as the host form).  A search depends on a state only through these three words (player to
 * move = ply & 1, no history), so a position given this way searches exactly as the same position reached by a prefix.
 * Every state is checked ON THE DEVICE before the table changes (az_check_state of az_games.h, one thread per state):
 *   both games     0 <= ply < max_plies; no cell held by both sides; no bit outside the board; the position is not
 *                  terminal; the side to move has a legal move
 *   connect_four   the sentinel bit 6 of every column is clear; every column is filled from the bottom without holes;
 *                  popc(bb0) == (ply + 1) / 2 and popc(bb1) == ply / 2
 *   breakthrough   both sides have a piece; no black piece on the last row, no white piece on the first
 * A bad state -> AZ_E_INVALID, az_last_error names the lowest offending index ("game <i>") and the first rule it breaks;
 * nothing is changed then.  Synchronises the device.  There is no host-state form: host callers give prefixes. */
int az_engine_set_start_states_device(az_engine *e, const uint64_t *bb_dev, const int32_t *ply_dev, int64_t n_games, void *stream);

/*
 * A start position per game for SELF-PLAY: a closed generation in which game id i starts from its own position, plays to the
 * end and is recorded like any other game.  It is what forking games out of the replay store, playing a generation over a list of
 * openings and the on-policy answer to reanalyse (play a stored position out with today's network) need.
 *
 * Plain self-play engines only (arena_agent == AZ_ARENA_SELF_PLAY, manual_moves == 0, not in stream mode): an arena engine, a
 * manual_moves engine and a streaming engine return AZ_E_INVALID and az_last_error names the reason; az_engine_stream_begin on an
 * engine with such a table stays refused.  1 <= n_games <= max_games; the caller resets afterwards (az_engine_reset with more
 * games than the table holds is refused); the table supersedes a single prefix and az_engine_set_start_prefix clears it.
 *
 * az_engine_set_game_starts: the arguments of az_engine_set_start_positions.  Every prefix is replayed on the host with the
 *   legality checks; an illegal action or a prefix that ends the game is refused with AZ_E_INVALID, az_last_error names
 *   "game <i>", and nothing changes (an earlier table stays in force).
 * az_engine_set_game_starts_device: the arguments of az_engine_set_start_states_device plus keys_dev (device u64 [n_games][2], or
 *   NULL).  Every state goes through az_check_state on the device first, as there.  Synchronises the device.
 *
 * What differs per game: the row offset of its records (rows stay indexed by ABSOLUTE ply within a game's row, game_len counts the
 * plies played from the game's own start), the on-policy value fill, and the rule of the game's first tree - a kept tree whose
 * game starts at ply >= 1 begins under select_rule, one at ply 0 under PUCT (see select_rule above), decided per game and for
 * every slot that takes a later id mid-run.  Root noise, injected draws and the random streams stay keyed by (seed, game id,
 * absolute ply): game i of a table engine is, bit for bit, game i of a plain engine with az_engine_set_start_prefix(prefix i)
 * and the same seed.  The tick kernel reads a game's start from the table at reset, at take-next and at game end only.
 *
 * History keys.  Next to each start state the table keeps the game's history key pair (key, key2), the replay store's two chains
 * (include/az_replay.h, "the key rule"; csrc/az_keychain.h).  The prefix form computes it on the host: the chains of an ordinary
 * game from the initial position, run over the prefix.  The device form takes keys_dev[i] (what az_replay_gather_forks hands
 * out); with keys_dev == NULL the table is UNKEYED: a game's pair is the seed the store forms for an ordinary game starting at
 * that state and ply, and az_replay_append_engine keys the games as it keys such games.
 *
 * az_engine_game_starts_device: writes every game id's start ply to ply_out_dev (i32 [n_games]) and, when keys_out_dev is not
 * NULL, its key pair (u64 [n_games][2]); with no table, the uniform values of the engine's one start.  Asynchronous on `stream`.
 * The companion of az_engine_export_device (whose layout does not change) for az_replay_append_device_starts.  Returns 1 when
 * the table carries GIVEN pairs (pass them on as keys_dev there), 0 when it does not (pass NULL), < 0 on error.
 *
 * Limits: no table in stream mode, and the multi-rank gather carries one start ply.  Arena engines take their openings per game
 * through az_engine_set_arena_openings (below).
 */
int az_engine_set_game_starts(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride, int64_t n_games);
int az_engine_set_game_starts_device(az_engine *e, const uint64_t *bb_dev, const int32_t *ply_dev, const uint64_t *keys_dev,
                                     int64_t n_games, void *stream);
int az_engine_game_starts_device(az_engine *e, int32_t *ply_out_dev, uint64_t *keys_out_dev, int64_t n_games, void *stream);

/*
 * Playout cap randomisation (KataGo: Wu 2019, section 3.1) for SELF-PLAY: every move is searched in full (n_playouts) with
 * probability p_full and otherwise fast (n_fast playouts); only full-search moves are meant to become training examples, the fast
 * ones carry the game to its outcome.  The reference has no counterpart (play_game_self searches every move alike,
 * game_utils.py:156-197); with no cap set nothing changes, bit for bit.
 *
 * az_engine_set_playout_cap: plain self-play engines only (arena_agent == AZ_ARENA_SELF_PLAY, manual_moves == 0, not in stream
 *   mode): the others return AZ_E_INVALID and az_last_error names the reason; az_engine_stream_begin refuses an engine with a cap.
 *   1 <= n_fast <= n_playouts (n_fast >= 2 without root Dirichlet expansion, the rule az_engine_create applies to n_playouts),
 *   0 <= p_full <= 1; n_fast == 0 clears the cap.  Call it before az_engine_reset (the next call the engine accepts): it holds for
 *   every later generation, and composes with a start prefix and with a game-start table.
 * The draw: the search a slot arms - at reset, when it takes the next game, after every move - has the kind of one uniform u, the
 *   first philox_u01 of the stream (seed, game id, ply, purpose 3, index 0), ply = the absolute ply of the position to be
 *   searched; the move is full iff u < p_full.  (az_engine_reset draws the generation's whole schedule, one byte per game id and
 *   ply, with one small kernel on `stream`; the tick kernel reads a byte where a slot arms a search.)  It comes from Philox whatever rng_mode is, so the schedule is a function of (seed, game id, ply)
 *   alone and AZ_RNG_INJECTED engines take a cap too.  (Purposes 0, 1, 2: root noise, move choice, arena opponent.)
 * The search: a full move adds n_playouts playouts to its tree, a fast one n_fast (a kept tree works as without a cap).  Root
 *   noise, temperature and move sampling are the same for both kinds.  az_slot_info.sims_done and the root export's sims_done count
 *   the current search from 0; az_progress.sims counts the playouts actually run.  Node pools stay sized by n_playouts.
 * Records: every move is recorded exactly as without a cap (packed export, az_example_view and the on-policy value fill do not
 *   change); beside them the engine keeps one byte per (game, ply): 1 = full search, 0 = fast.
 *
 * az_engine_full_moves_device: writes that mask to full_out_dev, a device u8 [n_games][max_plies] indexed by absolute ply like the
 *   other per-ply arrays: 1 for a recorded full-search ply, 0 elsewhere; with no cap every recorded ply gives 1.  One small kernel,
 *   asynchronous on `stream`.  The companion of az_engine_export_device for az_replay_append_device_kept.  Returns 1 when a cap is
 *   in force, 0 when none is, < 0 on error (AZ_E_STATE in stream mode).
 */
int az_engine_set_playout_cap(az_engine *e, int32_t n_fast, double p_full);
int az_engine_full_moves_device(az_engine *e, uint8_t *full_out_dev, int64_t n_games, void *stream);

/*
 * Forced playouts and policy target pruning (KataGo: Wu 2019, section 3.2) for SELF-PLAY: with root noise on, a root child that
 * has been tried gets a minimum number of visits in proportion to its (noised) prior, so the search finds out whether a move the
 * noise promoted is good; the visits it did not earn are then taken out of the recorded policy target again.  The reference has
 * no counterpart; with nothing set every kernel computes what it computed before, bit for bit.
 *
 * az_engine_set_forced_playouts: plain PUCT self-play engines only (arena_agent == AZ_ARENA_SELF_PLAY, manual_moves == 0,
 *   select_rule == AZ_SELECT_PUCT; closed generations and stream mode alike): the others return AZ_E_INVALID and az_last_error
 *   names the reason.  k finite and >= 0 (k == 0 clears the setting), prune 0 or 1.  Call it before az_engine_reset or
 *   az_engine_stream_begin (the next call the engine accepts): it holds for every later generation, and composes with a start
 *   prefix, a game-start table, a playout cap, both rng_modes and keep_search_tree.
 * Which searches: full ones.  Under a playout cap a fast move is searched and recorded exactly as without forcing; with no cap
 *   every search is full.
 * Forcing: at depth 0 of every playout, a root child with n > 0 visits, prior P (the node's own, after noise) and root count N
 *   (the parent count of the PUCT term, mcts.py:78) is forced iff (double)n * (double)n < (k * P) * (double)N in f64, i.e.
 *   n < sqrt(k P N) without a sqrt rounding.  A forced child's selection value is +infinity, so the first-maximum rule picks the
 *   lowest forced child.  A NaN prior makes the comparison false (AZ_FAULT_BAD_PRIOR is raised as before).
 * Pruning (prune == 1): once per full move, after the move has been chosen from the RAW counts (temperature, sampling, argmax
 *   and the value targets do not change) and before the record is written.  N = the root's count, b = the first child with the
 *   largest raw n, U(i) = (c_puct * P_i) * sqrt((double)N), V = Q_b + U(b) / (double)(n_b + 1).  For every child i != b with
 *   n_i > 0: F_i = the largest integer f >= 0 with (double)f * (double)f <= (k * P_i) * (double)N; lo_i = max(n_i - F_i, 0);
 *   m_i = the smallest integer in [lo_i, n_i] such that Q_i + U(i) / (double)(n + 1) < V for every n with m_i <= n < n_i; if
 *   m_i < n_i and m_i == 1 then m_i = 0.  Child b keeps n_b, an unvisited child stays 0.
 * Records: the child_visits row of a full move holds m WHERE THE RAW COUNTS WERE WRITTEN before; the raw counts are not kept.
 *   The packed export, az_example_view, az_engine_stream_take_device and every az_replay_append_* entry therefore carry the
 *   pruned target with no change.  With prune == 0 the records hold raw counts.  az_progress counts the playouts that were run.
 */
int az_engine_set_forced_playouts(az_engine *e, double k, int32_t prune);

/*
 * Evaluation in a random left-right orientation (AlphaGo Zero: Silver et al. 2017, "Methods"; KataGo): both games are symmetric
 * under the mirror column c <-> cols-1-c, so every network request may be shown to the network mirrored and its answer mapped back.
 * A left/right bias of the net then averages out over a search instead of being written into every visit count.  It costs no
 * extra evaluation, launch or memory.  The reference has no counterpart; with nothing set every kernel computes what it computed
 * before, bit for bit.
 *
 * az_engine_set_eval_mirror: self-play engines (closed generations and stream mode) and manual_moves engines (analysis, reanalyse);
 *   an arena engine (arena_agent != AZ_ARENA_SELF_PLAY) returns AZ_E_INVALID and az_last_error names the reason.  p_mirror finite
 *   and in [0, 1]; p_mirror == 0 clears the setting.  Call it before az_engine_reset or az_engine_stream_begin (the next call the
 *   engine accepts): it holds for every later generation, and composes with a start prefix, both start tables, a playout cap,
 *   forced playouts, both rng_modes, keep_search_tree, az_engine_advance_slots on several streams and the dense rows of
 *   az_engine_advance_rows.  Nothing travels beside the packed export: records, pools, ranks and the replay store do not change.
 * The coin: every request a slot issues is mirrored iff u < p_mirror, u the first philox_u01 of a Philox stream - from Philox
 *   whatever rng_mode is, as the cap schedule, so a game still depends on (seed, game id, network) alone, whichever slot, slot
 *   group, stream, pool or rank plays it:
 *     leaf request (az_slot_info.phase == 4)            (seed, game id, absolute ply of the slot's ROOT, purpose 4, index = the
 *                                                        sims_done az_slot_info reports for the waiting slot)
 *     root-expansion request (az_slot_info.phase == 3)  (seed, game id, root ply, purpose 5, index 0)
 *   (Purposes 0, 1, 2, 3: root noise, move choice, arena opponent, playout cap.)  A search re-armed with AZ_ACTION_SEARCH_AGAIN
 *   counts from 0 at the same root, so it draws the same coins again.
 * A mirrored request: the observation written to obs_out is that of az_mirror_state(state) (csrc/az_games.h: the W-flip of the
 *   plain observation); when the answer is consumed, action a takes priors[row][az_mirror_action(a)]; the value is used as it is.
 *   az_slot_info.leaf_bb keeps the unmirrored state; the NaN check and AZ_FAULT_BAD_PRIOR behave as before.
 *
 * az_engine_read_request_mirror: the parity read-back - the bit (0 or 1) of the slot's outstanding request; 0 with no setting in
 *   force.  AZ_E_STATE when the slot is not in phase 3 or 4 (or before az_engine_reset), AZ_E_INVALID for a bad slot.  Host code
 *   only: no kernel runs.  Synchronises the device as az_engine_read_slot.
 *
 * Limits: one orientation per request, not the average of both (two evaluations per request: another feature).  An arena agent takes
 *   the setting through az_engine_set_arena_search (below), which is how its effect on playing strength is measured.
 */
int az_engine_set_eval_mirror(az_engine *e, double p_mirror);
int az_engine_read_request_mirror(az_engine *e, int32_t slot);

/*
 * Self-play resignation (AlphaGo Zero: Silver et al. 2017, "Methods"; KataGo) for SELF-PLAY: a game whose side to move has been
 * lost for a while is ended early instead of being searched to its last ply, and a fraction of the games plays through all the
 * same, so the rate of false positives of any threshold can be measured.  The reference has no counterpart (play_game_self plays
 * every game out, game_utils.py:156-197); with nothing set every kernel computes what it computed before, bit for bit.
 *
 * az_engine_set_resign: plain self-play engines (arena_agent == AZ_ARENA_SELF_PLAY, manual_moves == 0; closed generations and stream
 *   mode): an arena or a manual_moves engine returns AZ_E_INVALID and az_last_error names the reason.  on != 0: v in (0, 1],
 *   p_playthrough in [0, 1], min_ply >= 0; on == 0 clears the setting (the other arguments are not read).  Call it before
 *   az_engine_reset or az_engine_stream_begin (the next call the engine accepts, as after every setter: a generation or a stream
 *   that was running is over, az_engine_advance refuses until one of the two is called); it may be called between generations with
 *   another v, holds for every later generation, and composes with a start prefix, a game-start table, a playout cap, forced
 *   playouts, the mirror, the solver, first-play urgency, both rng_modes, keep_search_tree, az_engine_advance_slots on several
 *   streams and the dense rows of az_engine_advance_rows.
 * The criterion: once the search at absolute ply t has ended, the move is chosen and the ply is recorded exactly as without the
 *   setting (state, move, child actions, child visits, value target), and the move is applied.  A game that this move ends keeps
 *   its result.  Otherwise crit = max(r, b) in f64, r = -root.Q (the AZ_BACKUP_SOFT_Z target's expression), b = the largest Q of
 *   a root child with a visit, -99.0 for a child without one (the AZ_BACKUP_A0C target's expression; the counts are those the move
 *   was drawn from).  Ply t QUALIFIES when t - start_ply >= min_ply, start_ply the game's own start (a start prefix's or its entry
 *   of the game-start table), and - under a playout cap - its search was a full one.  It is a RESIGN PLY when it qualifies and
 *   crit < -v.
 * Play-through: game id g plays through iff u < p_playthrough, u the first philox_u01 of the Philox stream (seed, game id, ply 0,
 *   purpose 6, index 0) - from Philox whatever rng_mode is, so a game's fate depends on (seed, game id, network) alone, whichever
 *   slot, slot group, stream, pool or rank plays it.  (Purposes 0..5: root noise, move choice, arena opponent, playout cap, the two
 *   orientation coins.)  A play-through game is the game without the setting, bit for bit.
 * Resigning: at the first resign ply of a game that does not play through, the game ends: game_len = t - start_ply + 1 (the resign
 *   ply is the last recorded one), game_ret0 = -1 when the player to move at t was player 0 and +1 otherwise, and the slot takes
 *   the next game as after a terminal move.  The records of a resigned game are the first game_len plies of the game without the
 *   setting; only game_ret0 (and with AZ_BACKUP_ON_POLICY the value fill that follows from it) differs.  The packed export,
 *   az_example_view, az_engine_stream_take_device and every az_replay_append_* entry read game_len and game_ret0 and do not change.
 * Side information, per game, beside the records (not in the packed export): resign_ply (int32: the first resign ply, resigned or
 *   not; -1 = none), flags (u8: bit 0 = the game resigned there, bit 1 = it is a play-through game - written at the first resign
 *   ply, so a game without one shows 0), low[2] (f64, per player: the lowest crit that player saw at a qualifying ply, +infinity =
 *   none; from it and game_ret0 the host computes the false-positive rate of ANY threshold from one batch of play-through games).
 *   A game's information is cleared when a slot takes its id.  In stream mode it therefore stays valid until the id one ring
 *   length later is handed out: read it BEFORE az_engine_stream_take_device frees the row.
 *
 * az_engine_resign_info_device: writes the side information of games [first_game, first_game + n_games) to ply_out_dev (int32
 *   [n_games]), flags_out_dev (u8 [n_games]) and low_out_dev (f64 [n_games][2]), device memory.  One small kernel, a thread per
 *   game, asynchronous on `stream`, no host synchronisation: it may be captured in a graph.  Closed generation: ids within
 *   [0, n_games of the last az_engine_reset).  Stream mode: ids within the ring's window [first game not yet taken, + max_games).
 *   AZ_E_INVALID outside the window or with a null output, AZ_E_STATE with nothing set or before az_engine_reset /
 *   az_engine_stream_begin.  A game still in play shows what it has seen so far.  An id of the window that no slot has taken yet
 *   (az_progress.games_started counts the ids handed out) shows what its row last held: in a closed generation the cleared
 *   state az_engine_reset left, in a stream after a wrap the information of the game one ring length earlier - the entry runs
 *   no host synchronisation, so it does not read the hand-out counter: bound first_game + n_games by games_started.
 *
 * Limits: one ply below the threshold resigns (a rule of several consecutive plies is another feature); arena and duel engines
 *   play every game out.
 */
int az_engine_set_resign(az_engine *e, int32_t on, double v, double p_playthrough, int32_t min_ply);
int az_engine_resign_info_device(az_engine *e, int64_t first_game, int64_t n_games, int32_t *ply_out_dev, uint8_t *flags_out_dev,
                                 double *low_out_dev, void *stream);

/*
 * MCTS-Solver (Winands, Bjornsson, Saito 2008; "certainty propagation"): the search proves wins, losses and draws inside its tree
 * and acts on them.  The reference scores a terminal node again on every visit (mcts.py:148-152) and knows no proof; with nothing
 * set every kernel computes what it computed before, bit for bit.
 *
 * Status: every node carries a proof status in the word that was padding, seen by the player who moved INTO the node (as its Q):
 *   AZ_PROOF_UNKNOWN 0, AZ_PROOF_WIN 1 (+1), AZ_PROOF_DRAW 2 (0), AZ_PROOF_LOSS 3 (-1).  A fresh node is 0.
 * 1. Terminal: a playout whose move ends the game marks that node with player_return(mover) - the value it backs up.
 * 2. Propagation: right after that backup, from the node that has just become proven upward.  A WIN node makes its parent LOSS;
 *    otherwise, if every child of the parent is proven, the parent takes minus the best child value (best DRAW -> DRAW, all LOSS
 *    -> WIN); otherwise the walk stops.  A newly proven parent repeats the step, as far as the root.  An expanded unproven node
 *    therefore always has an unproven child.
 * 3. Select, at every depth: a LOSS child's selection value is -infinity (after the PUCT value, before the first-maximum rule).
 * 4. A playout that selects a proven child stops there: it backs up the proven value as a terminal would, asks for no evaluation,
 *    counts in terminal_hits and sum_depth, and chains inside a tick under max_sims_per_tick / chain_window_us like a terminal
 *    hit.  The N and Q arithmetic (mcts.py:82-89) does not change.
 * 5. A search whose root is proven ends at once (phase 2, or 5 on a manual_moves engine) - also a kept subtree or a root searched
 *    again that is proven when the search is armed.  az_progress.sims and az_slot_info.sims_done count the playouts that ran.  The
 *    root request for Dirichlet noise that the start of a search makes is still made.
 * 6. The move at a proven root (self-play): at a root WON for the player to move (status LOSS: some child is WIN) the counts of
 *    the children that are not WIN become 0; at a DRAW root those of the LOSS children become 0; at a lost root (every child LOSS)
 *    the counts stay.  The adjusted counts are written where the raw counts were, and - unlike pruning - the move is drawn from
 *    them with the same temperature / sampling / argmax arithmetic.  The soft-Z, A0C and off-policy value targets of such a ply are
 *    the proven value for the player to move, exactly (+1.0, 0.0, -1.0); on-policy targets stay the game's outcome.
 * 7. Re-rooting, both compaction paths and az_engine_update_root copy whole node records, status included; a re-expansion that
 *    only rewrites P leaves it alone.
 *
 * az_engine_set_solver: on != 0 sets, 0 clears.  Plain PUCT self-play engines (closed generations, stream mode, dense rows) and
 *   manual_moves engines; both rng_modes (AZ_RNG_INJECTED is allowed: the solver draws nothing).  AZ_E_INVALID, with the reason
 *   in az_last_error, for an arena engine, select_rule == AZ_SELECT_UCT, and an engine with forced playouts in force - and
 *   az_engine_set_forced_playouts refuses an engine with the solver set: the combination is not built.  Composes with a playout
 *   cap, the evaluation mirror, start prefixes and tables, keep_search_tree.  The caller starts a generation next
 *   (az_engine_reset / az_engine_stream_begin).
 * az_engine_read_proofs: the status of every node of a slot's tree in the order of az_engine_read_tree (node 0 = the root) ->
 *   the number of nodes; at most n are written.  Host code only; synchronises the device.  Works with the solver off (all 0).
 * az_engine_export_proofs_device: per slot 1 + max_children bytes - the root's status, then its children's in child order (0
 *   beyond n_children) - az_engine_proofs_device_bytes() in all.  One kernel, a wave per slot, asynchronous on `stream` and
 *   graph-capturable; it sits beside az_engine_export_roots_device, whose layout does not change.
 *
 * Limits: win / draw / loss only (no score bounds), no preference for the shortest win or the longest loss, no forced playouts, no
 *   UCT rule.  An arena agent takes the setting through az_engine_set_arena_search (below), which is how its effect on playing
 *   strength is measured.
 */
#define AZ_PROOF_UNKNOWN 0
#define AZ_PROOF_WIN 1
#define AZ_PROOF_DRAW 2
#define AZ_PROOF_LOSS 3
int az_engine_set_solver(az_engine *e, int32_t on);
int64_t az_engine_read_proofs(az_engine *e, int32_t slot, int8_t *out, int64_t n);
int64_t az_engine_proofs_device_bytes(const az_engine *e);
int az_engine_export_proofs_device(az_engine *e, void *dev_buf, int64_t bytes, void *stream);

/*
 * First-play urgency (FPU) reduction, as Lc0 and KataGo select: what an unvisited child is worth in the PUCT comparison.  The
 * reference scores it with Q = 0 (Node.Q starts at 0, mcts.py:78) - the value of a draw, whatever the position is worth: in a won
 * position every untried move looks worse than it should, in a lost one every untried move looks like salvation and the search
 * sprays its playouts over all of them.  With the setting an unvisited child is valued at its parent's own value, minus a penalty
 * that grows with the prior mass already explored.  It costs no evaluation, no launch and no memory; with nothing set every
 * kernel computes what it computed before, bit for bit.
 *
 * The rule.  All arithmetic is IEEE double, one rounding per operation.  Consider a node X whose children are compared by the PUCT
 *   rule (mcts.py:38-52,78).
 *   v = -X.Q: X's value for the player who chooses there.  X.Q is the node record's own Q as it stands before this playout's
 *     backup; for the root it is root.Q, the root_q of az_engine_read_root.
 *   m = the sum of P_i over the children with N_i > 0.  P is the node's own prior (after the noise at the root, after the mirror
 *     mapping).  The sum is a butterfly over 64 values: child i in position i, +0.0 for unvisited children and for positions
 *     beyond the children; for off = 32, 16, 8, 4, 2, 1 every position l takes x[l] + x[l ^ off]; m is position 0.  The order is
 *     part of the definition.
 *   f = reduction_root at depth 0 (X is the search's root), reduction below.
 *   A child with N == 0 enters the comparison with Q_eff = v - f * sqrt(m): two roundings, no fused multiply-add, no clamp.  Its
 *     value is Q_eff + ((c_puct * P) * sqrt((double)N_X)) / (double)(0 + 1), the association of the existing line.
 *   A child with N > 0 is valued as before.
 *   Everything after the value is unchanged: forcing (n > 0 only, so the two never meet on one child), the solver's -infinity, the
 *   first-maximum rule, AZ_FAULT_BAD_PRIOR (a NaN prior makes m NaN and ends there through the empty ballot), the backup, N and Q.
 *   The rule acts in every search of the engine: fast and full under a cap, kept trees, roots searched again.
 *
 * az_engine_set_fpu: on == 0 clears the setting and the other two arguments are ignored (reduction == 0 is NOT the reference: it
 *   means "an unvisited child is worth what its parent is worth", so clearing has its own flag).  With on != 0 both reductions
 *   must be finite and >= 0, else AZ_E_INVALID.  Plain PUCT self-play engines (closed generations, az_engine_advance_slots on
 *   several streams, the dense rows of az_engine_advance_rows, stream mode) and manual_moves engines (analysis, reanalyse); both
 *   rng_modes (it draws nothing).  AZ_E_INVALID, with the reason in az_last_error, for an arena engine and for select_rule ==
 *   AZ_SELECT_UCT (that rule already gives an unvisited child +infinity).  Call it before az_engine_reset or
 *   az_engine_stream_begin (the next call the engine accepts): it holds for every later generation, and composes with a start
 *   prefix, both start tables, a playout cap, forced playouts, the evaluation mirror, the solver and keep_search_tree.  Records,
 *   exports, pools, ranks and the replay store do not change.
 *
 * Limits: no UCT rule, no separate treatment of the fast moves of a playout cap.  An arena agent takes the setting through
 *   az_engine_set_arena_search (below), which is how its effect on playing strength is measured (Lc0 and KataGo use values around
 *   0.2 to 0.4 below the root and 0 at a noised root; the matches played here are in DESIGN_HISTORY.md).
 */
int az_engine_set_fpu(az_engine *e, int32_t on, double reduction, double reduction_root);

/*
 * Arena matches between search settings: an evaluation game whose AGENT searches with first-play urgency, the MCTS-Solver or the
 * evaluation mirror, and evaluation games that start from a position per game.  Engine A plays setting X, engine B setting Y
 * (az_engine_exchange_moves), over N openings each played twice with the colours swapped: what measures whether a setting plays
 * better.  az_engine_set_fpu / _set_solver / _set_eval_mirror / _set_game_starts keep refusing arena engines (an arena engine with
 * none of the calls below measures the reference's search); these two entries accept arena engines ONLY.
 *
 * az_engine_set_arena_search: AZ_ARENA_ZERO agents, every opponent kind (AZ_OPPONENT_EXTERNAL included).  AZ_E_INVALID, with the
 *   reason in az_last_error, for a self-play engine or a manual_moves engine (they have their own setters), for AZ_ARENA_NET (it
 *   searches nothing) and for select_rule == AZ_SELECT_UCT.  s == NULL, or a record with fpu_on == 0, solver == 0 and
 *   p_mirror == 0, clears all three.  struct_size must be sizeof(az_arena_search); `reserved` is not looked at.  The value checks
 *   are those of the three setters and apply to a setting that is on: fpu_reduction and fpu_reduction_root finite and >= 0 with
 *   fpu_on != 0; p_mirror in [0, 1], NaN refused.  On a refusal nothing changes.  Synchronises the device; the caller resets next.
 *   The rules are the ones stated above, word for word: FPU acts at every select level of the agent's tree; the mirror's coins are
 *   purposes 4 and 5 keyed by (seed, game id, root ply, ...) - the two engines of a duel have their own seeds and so their own
 *   coins; solver rules 1-5 and 7 apply unchanged, and a kept subtree that is already proven when the opponent's move re-roots
 *   onto it ends its search at once.  Rule 6 applies to the AGENT's move: the counts are adjusted before the move is drawn, and
 *   the argmax (or, under arena_probabilistic, the sample) runs on the adjusted counts - a won root plays a proven win, the first
 *   of the most visited among them; a drawn root never plays a proven loss; a lost root plays as before.  (The argmax is the first
 *   maximum of the tempered fractions of the ADJUSTED counts: when every remaining count is tied it is the lowest such action; a
 *   child whose count became 0 has fraction 0 and cannot be the maximum while another count is positive - and one is: a WIN child
 *   was visited when it was proven, and a drawn root has a child that is not LOSS, visited likewise.)  az_engine_read_proofs and
 *   az_engine_export_proofs_device work on arena engines.  Playout cap and forced playouts stay refused there.  With the entry
 *   never called, or cleared, every arena launch is the kernel instantiation it was before, bit for bit.
 *
 * az_engine_set_arena_openings: the arguments, the host replay and the legality checks of az_engine_set_game_starts (an illegal
 *   action or a prefix that ends the game -> AZ_E_INVALID naming "game <i>", the earlier table stays in force; az_engine_reset with
 *   more games than the table holds is refused), for arena engines of both agent kinds and every opponent kind; self-play and
 *   manual_moves engines are refused.  It supersedes a prefix, and az_engine_set_start_prefix clears it.  The agent of game i plays
 *   player (i & 1) ^ arena_flip whatever the opening's length is (the rule (ply ^ i ^ arena_flip) & 1 on the ABSOLUTE ply): who
 *   moves first in game i follows from its own start ply, at reset and when a slot takes a later id.  A kept tree's first rule is
 *   decided from the game's own ply (an arena bot calls update_root with >= 2 moves played).  Records stay indexed by absolute
 *   ply, game_len counts from the game's own start, and az_engine_game_starts_device answers for arena engines too.  Both engines
 *   of a duel take the same table: az_engine_exchange_moves refuses (AZ_E_STATE) a pair whose tables differ in length or in any
 *   start ply.
 */
typedef struct az_arena_search {
    int32_t struct_size;            /* = sizeof(az_arena_search); ABI guard, as az_config */
    int32_t fpu_on;                 /* the arguments of az_engine_set_fpu */
    double  fpu_reduction, fpu_reduction_root;
    int32_t solver;                 /* az_engine_set_solver */
    int32_t reserved;
    double  p_mirror;               /* az_engine_set_eval_mirror; 0 = off */
} az_arena_search;
int az_engine_set_arena_search(az_engine *e, const az_arena_search *s);
int az_engine_set_arena_openings(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride, int64_t n_games);

/*
 * One tick = MCTS.playout's select + expand + backup (mcts.py:126-153) for all slots, fused with the
 * agent's move step when a slot has finished its S playouts (alphazerobot.py:71-93,
 * game_utils.py:156-197, mcts.py:155-162,192-203) and the root Dirichlet expansion (mcts.py:182-190):
 *   1. consume priors[g]/values[g] for the request slot g issued on the PREVIOUS tick
 *      (expand + backup, or root expansion); ignored for slots without a request;
 *   2. run playouts/moves until the slot needs the network again, and write that state's
 *      observation (state_to_board, network.py:9-18, float32) to obs_out[g].
 * priors: dev float32 [G][A] (softmax output), values: dev float32 [G], obs_out: dev float32 [G][C+1][H][W].
 * priors/values may be NULL on the first tick after reset.
 */
int az_engine_advance(az_engine *e, const float *priors, const float *values, float *obs_out, void *stream);

/* The same tick for the slots [first_slot, first_slot + n_slots) only.  priors / values / obs_out are still the
 * WHOLE-engine arrays ([G][A], [G], [G][C+1][H][W]); the launch reads and writes the rows of its slots.  Slot groups
 * are independent (they share only the game-id counter, by device atomics), so disjoint groups may be advanced
 * concurrently on DIFFERENT streams: while one group's PV-net forward runs, another group's tree search runs beside it
 * (BASELINE.json configs[4]: "overlapped PV-eval / tree-search HIP streams"; the reference's analogue is its pool of
 * worker processes running beside the inference server, examplegenerator.py:106-138).  Which group plays which game
 * does not change a game: random streams are keyed by game id.  az_engine_progress / poll / export synchronise only the
 * stream they are given: synchronise the other group streams first.  priors/values must not be NULL here (give
 * initialised buffers on the first tick: slots without an outstanding request ignore them). */
int az_engine_advance_slots(az_engine *e, int32_t first_slot, int32_t n_slots, const float *priors, const float *values,
                            float *obs_out, void *stream);

/* Arena engines only: compute the opponent bot's move for every slot whose opponent is to move (one thread per slot:
 * a uniformly random legal action, or a UCT search with random rollouts).  The next az_engine_advance applies the moves.
 * One arena tick = az_engine_advance, az_engine_opponent_moves, PV-net forward.  Asynchronous on `stream`. */
int az_engine_opponent_moves(az_engine *e, void *stream);

/* The tail of a generation.  Once every game has been handed to a slot, finished slots stay idle and the batch thins out while a
 * tick still spans all n_slots rows of the request buffers (a generation lasts as long as its longest game).
 * az_engine_compact_rows (synchronises `stream`) lists the slots that still play, densely and in slot order, and returns their
 * number; from then on the engine is ticked with az_engine_advance_rows over n_rows >= that number rows: list entry i writes its
 * request to row i of obs_out and finds the answer to its previous request in the row it was written to, so the network only has to
 * evaluate the first n_rows rows (`az_net_forward(..., n_rows, ...)`).  May be called again as the list thins further; refused
 * while games are still being handed out, and on arena / manual_moves engines.  az_engine_reset returns to one row per slot.
 * Replaces nothing in the reference (its worker processes simply exit, examplegenerator.py:134-138). */
int az_engine_compact_rows(az_engine *e, int32_t *n_live_out, void *stream);
int az_engine_advance_rows(az_engine *e, int32_t n_rows, const float *priors, const float *values, float *obs_out, void *stream);

/* Two arena engines facing each other (both AZ_OPPONENT_EXTERNAL, same game, same n_slots, arena_flip 0 and 1, games = slots:
 * no refill): for every slot, hand a's agent move to b and b's to a as soon as it has been played.  One tick of such a
 * pairing = advance(a), advance(b), az_engine_exchange_moves(a, b), forward(net of a), forward(net of b). */
int az_engine_exchange_moves(az_engine *a, az_engine *b, void *stream);

/* MCTS.update_root(action) (mcts.py:192-203) for every slot, manual_moves engines only: applies
 * actions[g] (host array [G]; AZ_ACTION_NONE = leave the slot alone) to the slot's root state, keeps the chosen
 * child's subtree (or starts a fresh tree when keep_subtree == 0 or the root is a leaf) and arms the
 * next search.  A slot whose game ends goes idle.  An action that is illegal in the root state raises
 * AZ_FAULT_ILLEGAL_ACTION and idles the slot (the state is left untouched).  AZ_ACTION_SEARCH_AGAIN re-arms a finished
 * search on the SAME root: the tree is kept, another n_playouts run, the root is re-expanded with a fresh Dirichlet
 * draw - what calling MCTS.search(state) twice does in the reference (mcts.py:164-190). */
int az_engine_update_root(az_engine *e, const int32_t *actions, int32_t keep_subtree, void *stream);

/* Counters; synchronises `stream`. */
int az_engine_progress(az_engine *e, az_progress *out, void *stream);

/* Cheap completion poll for the tick loop: number of finished games and the device fault flags (two words, one
 * small copy); synchronises `stream`.  Returns AZ_E_DEVICE if a fault flag is set. */
int az_engine_poll(az_engine *e, int64_t *games_done, uint32_t *error_flags, void *stream);

/* Copy finished games to host memory owned by the engine; synchronises `stream`. */
int az_engine_export(az_engine *e, az_example_view *out, void *stream);

/* The same records, device to device: the finished games of the generation packed into ONE caller-owned device buffer
 * (asynchronous on `stream`), ready for the generation-end collective (RCCL all-gather over xGMI) and for
 * az_replay_append_device on the receiving side - the replacement of the pickled `pool.map_async(...).get()` gather of
 * examplegenerator.py:151-152 without a host round trip.  Layout, n = games of the generation (the n_games given to
 * az_engine_reset), mp = max_plies, mc = max_children, every array 16-byte aligned, in this order:
 *   game_len i32[n] | game_ret0 f32[n] | states u64[n][mp][2] | move u16[n][mp] | n_children u8[n][mp] |
 *   child_action u16[n][mp][mc] | child_visits u32[n][mp][mc] | value f64[n][mp]
 * (the arrays of az_example_view; on-policy value targets are filled in on the device). */
int64_t az_engine_export_device_bytes(const az_engine *e);
int az_engine_export_device(az_engine *e, void *dev_buf, int64_t bytes, void *stream);

/*
 * Stream mode: continuous self-play over a record store of FIXED size.  az_engine_reset starts a closed generation: once its
 * last id is handed out the slots go idle one by one, and the records are indexed by game id into max_games rows.  A stream
 * never ends: game ids are 0, 1, 2, ... (below 2^31: a slot keeps its id in an int32), id i uses RNG stream (seed, i) exactly
 * as in a closed generation - a game depends on (seed, id, network) alone, so the games a stream delivers, in id order, ARE the
 * closed generation of the same seed cut into pieces - and id i records into row i % max_games of the store, a ring.
 *
 * az_engine_stream_begin replaces az_engine_reset (slots 0..G-1 start ids 0..G-1).  Plain self-play engines only: an arena
 * engine, manual_moves, AZ_RNG_INJECTED, a start prefix, a start-position table or max_games < n_slots return AZ_E_INVALID and
 * az_last_error names the reason.  A later az_engine_reset returns the engine to a closed generation.
 *
 * An id is handed out only while id < read_pos + max_games, read_pos = the first id not yet taken: a row is never overwritten
 * before its game has been taken.  A slot that finishes a game while no id may be handed out goes idle (az_progress.slots_idle
 * counts them) and asks again at the start of each of its ticks, so it comes back by itself once a take has raised the limit;
 * no id is skipped or handed out twice.  The engine is ticked with az_engine_advance on ONE stream, and the stream_* calls are
 * given the same stream; az_engine_advance_slots, az_engine_compact_rows, az_engine_advance_rows, az_engine_export,
 * az_engine_export_device and az_replay_append_engine return AZ_E_STATE in stream mode.  az_progress.games_done and
 * az_engine_poll count every game finished since az_engine_stream_begin; fault flags work as in a closed generation.
 *
 * az_engine_stream_ready (synchronises `stream`): the number of consecutive finished games starting at read_pos, at most max_games.
 * az_engine_stream_take_bytes(n): the size of a take of n games = az_engine_export_device_bytes of a generation of n games.
 * az_engine_stream_take_device: packs games [read_pos, read_pos + n) into dev_buf (16-byte aligned) in exactly the layout of
 *   az_engine_export_device for a generation of n games - az_replay_append_device and the generation-end all-gather consume it
 *   unchanged; on-policy value targets are filled in on the device.  One kernel, asynchronous on `stream`: it gathers the rows
 *   from the ring (wraparound included), frees them and raises the hand-out limit for the ticks that follow on the stream.
 *   *first_game_out (may be NULL) receives read_pos, which then advances by n.  AZ_E_STATE if more games are asked for than
 *   the last az_engine_stream_ready found (ask it first); AZ_E_INVALID if n < 1, n > max_games or the buffer is too small.
 */
int az_engine_stream_begin(az_engine *e, uint64_t seed, void *stream);
int64_t az_engine_stream_ready(az_engine *e, void *stream);
int64_t az_engine_stream_take_bytes(const az_engine *e, int64_t n_games);
int az_engine_stream_take_device(az_engine *e, int64_t n_games, void *dev_buf, int64_t bytes, int64_t *first_game_out, void *stream);

/* Every slot's root, packed into ONE caller-owned device buffer by one kernel: asynchronous on `stream`, no host
 * synchronisation, usable inside a captured graph - what az_engine_read_root / az_engine_read_slot give for one slot per
 * synchronising call.  The values are the node records' own (no arithmetic), so they equal az_engine_read_root's.
 * Layout, G = n_slots, mc = max_children, every array 16-byte aligned (and so must dev_buf be), in this order:
 *   header i32[4] | game_id i32[G] | phase i32[G] | ply i32[G] | sims_done i32[G] | n_children i32[G] | root_n u32[G] |
 *   root_q f64[G] | child_action i32[G][mc] | child_n u32[G][mc] | child_q f64[G][mc] | child_p f64[G][mc]
 * header = { number of slots whose phase is 5 (search done) or 0 (idle), G, mc, az_progress.error_flags }: a tick loop learns
 * from one 16-byte copy when every search has finished.  phase / game_id / ply / sims_done are az_slot_info's; children are in
 * ascending-action order; rows of the child arrays beyond n_children hold action -1 and zeros. */
int64_t az_engine_roots_device_bytes(const az_engine *e);
int az_engine_export_roots_device(az_engine *e, void *dev_buf, int64_t bytes, void *stream);

/* Every slot's GREEDY LINE - the principal variation of its finished search, and the reference's off-policy value target
 * A0GB at its end (game_utils.py:181-194) - packed into ONE caller-owned device buffer by one kernel, a wave per slot:
 * asynchronous on `stream`, no host synchronisation, usable inside a captured graph, for every engine the root export accepts.
 * The walk: at a node with children value = node.Q and the next node is the child with the largest N + P (-99.0 for a child
 * with N = 0; the first maximum = the lowest action wins), the sign flips at every step; a final leaf with N > 0 gives
 * value = leaf.Q and one more flip; the target is value * sign.  It is the function self-play's off-policy backup runs.
 * Layout, G = n_slots, D = max_depth (1 <= D <= max_plies), every array 16-byte aligned (and so must dev_buf be), in order:
 *   header i32[4] | game_id i32[G] | phase i32[G] | ply i32[G] | depth i32[G] | leaf_n u32[G] | value f64[G] |
 *   line_action i32[G][D] | line_n u32[G][D] | line_q f64[G][D]
 * header = { number of slots whose phase is 5 or 0, G, D, az_progress.error_flags }, as in the root export.  depth = the full
 * length of the line in moves (it may exceed D: the arrays then hold the first D steps), leaf_n = N of the node it ends at,
 * value = the target over the FULL line whatever D is.  line_*[d] = action, N and Q of the node reached after d + 1 moves: the
 * node records' own values, no arithmetic.  Rows beyond min(depth, D) hold action -1 and zeros.  A slot whose phase is not 5
 * (a search still running, an idle slot) gets depth = -1, value = 0 and empty rows.  A line cannot be longer than
 * max_plies - ply + 1 moves: a walk that reaches that bound, or leaves the slot's pool, ends there with depth = -2 (a corrupt
 * tree; the rows hold the steps taken).
 * AZ_E_INVALID, and nothing is written: max_depth outside [1, max_plies], bytes < az_engine_lines_device_bytes, dev_buf not
 * 16-byte aligned. */
int64_t az_engine_lines_device_bytes(const az_engine *e, int32_t max_depth);
int az_engine_export_lines_device(az_engine *e, int32_t max_depth, void *dev_buf, int64_t bytes, void *stream);

/* debug / parity read-back of one slot's root (mcts.root.{N,Q,children[a].{N,Q,P}}, read by
 * game_utils.py:30-31,174,178,183-193).  Arrays sized max_children.  Returns n_children or <0.
 * Synchronises the device. */
int az_engine_read_root(az_engine *e, int32_t slot, int64_t *root_n, double *root_q, int32_t *actions,
                        int64_t *child_n, double *child_q, double *child_p);

/* The whole search tree of one slot in breadth-first order (node 0 = root; children of a node are
 * consecutive and in ascending-action order): parent index, action leading to the node, N, Q, P.
 * What deep-copying `mcts.root` gives the reference's statistics code (game_utils.py:30-31,183-193).
 * Arrays sized max_nodes (any may be NULL).  Returns the node count, or <0; if the tree has more than max_nodes
 * nodes the first max_nodes are written and the full count is returned.  Synchronises the device. */
int64_t az_engine_read_tree(az_engine *e, int32_t slot, int64_t max_nodes, int32_t *parent, int32_t *action,
                            int64_t *n, double *q, double *p);

typedef struct az_slot_info {
    int32_t phase; /* 0 idle, 1 run, 2 move pending, 3 waiting root eval, 4 waiting leaf eval, 5 search done (manual_moves) */
    int32_t game_id, ply, sims_done;
    uint32_t root, alloc;
    uint64_t bb[2];      /* root state */
    uint64_t leaf_bb[2]; /* state of the outstanding request */
    int32_t leaf_ply, depth;
} az_slot_info;
int az_engine_read_slot(az_engine *e, int32_t slot, az_slot_info *out);

/* test / parity read-back of the root noise a slot has STAGED: the Dirichlet vector that the tick which issued the slot's root
 * request drew on the device (AZ_RNG_PHILOX with use_dirichlet; np.random.dirichlet, mcts.py:187) and that the next tick mixes into
 * the root priors.  eta_out: host array of max_children doubles, entry k = the draw of the k-th legal action in ascending order.
 * Entries at and beyond the position's number of legal actions are NOT part of the draw: they hold whatever an earlier ply of the
 * slot left there (on a fresh engine: unset device memory) and nothing reads them.  The row is the vector the next tick
 * consumes only while the slot waits for its root evaluation (az_slot_info.phase == 3): in any other phase the call returns
 * AZ_E_STATE, as it does before az_engine_reset.  AZ_E_INVALID: a bad slot, a NULL pointer, an AZ_RNG_INJECTED engine or one
 * without use_dirichlet (their draws are the caller's own tables, or none).  Host code only: no kernel runs.  Synchronises the
 * device as az_engine_read_slot. */
int az_engine_read_root_noise(az_engine *e, int32_t slot, double *eta_out);

#ifdef __cplusplus
}
#endif
#endif /* AZ_ENGINE_H */
