/*
 * az_replay.h — C ABI of the device-resident replay store.
 *
 * Replaces, next to the self-play engine, the consumer side of its output in the reference's Trainer:
 *   - the FIFO buffer of games                       train.py:226-236,295-298
 *   - Trainer.remove_duplicates                      train.py:156-201
 *   - the batch sampling of Trainer.net_step         train.py:107-113,119-120
 * so that finished games go engine -> replay -> training batch without leaving HBM and without being turned into
 * Python lists.  The network update itself (forward, loss, Adam: train.py:115-130) stays PyTorch.
 *
 * Semantics kept from the reference:
 *   - the buffer is a FIFO of GAMES: appending beyond `max_games` drops the oldest games (train.py:233-236);
 *   - an example's key is its action history (`state.information_state()`, game_utils.py:169), here a 64-bit
 *     hash of (length, actions) — duplicates are examples with equal history;
 *   - remove_duplicates walks the flattened buffer in order; for every key the pi vectors and the z values of
 *     its occurrences are summed IN THAT ORDER (float64, one rounding per addition) and divided by the count,
 *     the unique list is in first-occurrence order, AND the averaged pi / z are written back into the first
 *     occurrence stored in the buffer (the reference keeps a reference to that list object, train.py:191-197 —
 *     so the next generation's dedupe sees the averaged record).  All of it reproduced, bit for bit.
 *
 * Conventions as in az_engine.h (int status, az_replay_last_error, stream = hipStream_t as void*).
 */
#ifndef AZ_REPLAY_H
#define AZ_REPLAY_H

#include <stdint.h>

#include "az_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct az_replay az_replay;

typedef struct az_replay_config {
    int32_t struct_size;
    int32_t game, rows, cols; /* as az_config */
    int32_t device;
    int32_t reserved;
    int64_t max_games;        /* FIFO capacity in games (Trainer.n_games_buffer_max, train.py:38) */
    int64_t max_examples;     /* capacity in examples (plies) */
} az_replay_config;

typedef struct az_replay_stats {
    int64_t n_games, n_examples; /* currently stored */
    int64_t n_unique;            /* after the last az_replay_dedupe / az_replay_dedupe_positions (0 before) */
    int64_t games_dropped;       /* total FIFO evictions */
    int64_t fault_flags;         /* AZ_REPLAY_FAULT_* raised on the device since the last az_replay_stats_get (reading clears them) */
} az_replay_stats;

#define AZ_REPLAY_FAULT_KEY_COLLISION 1u /* remove_duplicates met two different histories with one 64-bit key */
#define AZ_REPLAY_FAULT_BAD_INDEX 2u     /* az_replay_sample / az_replay_gather_states / az_replay_refresh_from_roots /
                                            az_replay_refresh_from_search were given an index outside [0, n_unique) */
#define AZ_REPLAY_FAULT_ROOT_MISMATCH 4u /* a refresh skipped a root (or a root and line pair) that does not belong to its example */

/* value_mode of the refresh entries.  0-2 are functions of a search root alone (az_replay_refresh_from_roots takes these);
 * 3 needs the greedy line as well (az_replay_refresh_from_search with a line export). */
#define AZ_REFRESH_KEEP_Z 0 /* pi only */
#define AZ_REFRESH_SOFT_Z 1 /* z = -root.Q                                         game_utils.py:172-174 */
#define AZ_REFRESH_A0C 2    /* z = max(child.Q if child.N > 0 else -99.0)          game_utils.py:177-179 */
#define AZ_REFRESH_OFF_POLICY 3 /* z = the value at the end of the most-visited line (A0GB)  game_utils.py:181-194 */

int az_replay_create(const az_replay_config *cfg, az_replay **out);
int az_replay_destroy(az_replay *r);
const char *az_replay_last_error(const az_replay *r);

/* Trainer.update_buffer_size / the FIFO trim (train.py:230-236,295-298): set the current capacity in games
 * (<= max_games); older games beyond it are dropped at the next append. */
int az_replay_set_capacity(az_replay *r, int64_t n_games);

/* Append every finished game of the engine's current generation, device to device, in game-id order
 * (`for examples in games: self.buffer.append(examples)`, train.py:226-227).  pi of an example is formed from the
 * recorded root visit counts with the reference's arithmetic (mcts.py:161-162, alphazerobot.py:13-14).
 * Synchronises `stream`. */
int az_replay_append_engine(az_replay *r, az_engine *e, void *stream);

/* Append games given as host arrays in the layout of az_example_view (used by tests and by the multi-rank gather).
 * The view is validated before anything is copied or launched: max_children must be the game's, every game_len must lie
 * in [0, max_plies - start_ply], every n_children of a recorded ply must be <= max_children and every child action an
 * action of the game; otherwise AZ_E_INVALID and the store is unchanged. */
int az_replay_append_host(az_replay *r, const az_example_view *v, int32_t start_ply, void *stream);

/* Append n_games games from a DEVICE buffer in the packed layout of az_engine_export_device (this rank's own export,
 * or one rank's section of the all-gathered buffer): engine -> RCCL all-gather -> replay store without touching the
 * host.  The board geometry (max_plies, max_children) is the store's.  The game lengths are read back and checked as in
 * az_replay_append_host before any kernel runs (AZ_E_INVALID, store unchanged); child counts are clamped to max_children
 * on the device.  Synchronises `stream`. */
int az_replay_append_device(az_replay *r, const void *dev_buf, int64_t n_games, int32_t start_ply, void *stream);

/*
 * Games that start from their own positions (az_engine_set_game_starts / az_engine_set_game_starts_device).
 *
 * THE KEY RULE.  An example is keyed by the history that leads to it, as the reference keys it by the information-state string
 * (train.py:177).  A game that was given the prefix P and then plays m_1..m_k carries, at its example after m_1..m_j, exactly the
 * (key, key2) of an ordinary game from the initial position whose history is P + m_1..m_j: its chains start from P's pair and
 * the second chain's step index is the ABSOLUTE ply (csrc/az_keychain.h).  Hence
 *   - a fork's first example has the key of the stored example it was forked from, and az_replay_dedupe averages the two in
 *     buffer order, as the reference averages any two examples with one information-state string;
 *   - two prefixes that transpose into one position stay apart, as their strings differ;
 *   - games appended without a table - no prefix, or the one shared az_engine_set_start_prefix - keep the keys they always had,
 *     bit for bit: seeded from their start state, stepping with the index 1, 2, ... from there.  A shared prefix of length > 0
 *     is therefore NOT the history P + ... of the rule, and a store that holds such games must not be forked: a fork still merges
 *     with its parent, but `key` carries no step index, so a fork that repeats the parent's next move produces the parent
 *     continuation's `key` with another `key2`, and the next az_replay_dedupe raises AZ_REPLAY_FAULT_KEY_COLLISION (AZ_E_DEVICE).
 *     Games from the initial position, games of a table with given pairs and their forks are all keyed by the rule.
 *
 * az_replay_append_engine on an engine with a game-start table uses each game's own start ply, its key pair when the table
 * carries given pairs, and forms the on-policy z with the sign of the absolute ply.
 *
 * az_replay_append_device_starts: az_replay_append_device for such a generation: dev_buf = the packed export, start_ply_dev
 * (device i32 [n_games]) and keys_dev (device u64 [n_games][2]) = what az_engine_game_starts_device wrote.  Lengths and start
 * plies are read back and 0 <= start_ply[g] <= max_plies and 0 <= game_len[g] <= max_plies - start_ply[g] are checked before any
 * kernel runs (AZ_E_INVALID, store unchanged).  keys_dev == NULL: every game is keyed from its start state, as an ordinary
 * game that starts there.  Synchronises `stream`.
 *
 * az_replay_gather_forks: az_replay_gather_states plus keys_out (device u64 [n][2]) = the stored (key, key2) of each example:
 * the three inputs of az_engine_set_game_starts_device.  Same index space, same AZ_REPLAY_FAULT_BAD_INDEX behaviour (ply -1,
 * zero keys), asynchronous.  It records no epoch: a fork appends, it overwrites nothing.
 */
int az_replay_gather_forks(az_replay *r, const int64_t *indices, int64_t n, uint64_t *bb_out, int32_t *ply_out, uint64_t *keys_out,
                           void *stream);
int az_replay_append_device_starts(az_replay *r, const void *dev_buf, int64_t n_games, const int32_t *start_ply_dev,
                                   const uint64_t *keys_dev, void *stream);

/*
 * Appending only SOME plies of a generation: the examples of an engine under a playout cap (az_engine_set_playout_cap), whose
 * fast-search moves carry a game to its outcome but are not trained on.
 *
 * az_replay_append_device_kept: az_replay_append_device_starts with start_ply_dev == NULL allowed (every game then starts at
 * start_ply, which is ignored otherwise) plus keep_dev, a device u8 [n_games][max_plies] indexed by ABSOLUTE ply (what
 * az_engine_full_moves_device writes).  Only plies with a non-zero byte become stored examples, in ply order; a game's FIFO length
 * is its number of kept plies, and a game with none is skipped, as a game of length 0 is.  The key chains still step over every
 * move of the game, so a kept example carries the key of its full history (the key rule); on-policy z keeps the sign of the
 * absolute ply; pi is formed by the one routine every append uses.  Lengths, start plies and the mask are read back and checked
 * before any kernel runs (AZ_E_INVALID, store unchanged): the checks of az_replay_append_device_starts, and a non-zero keep byte
 * outside a game's plies [start, start + len) is refused.  keep_dev == NULL keeps every ply.  Synchronises `stream`.
 *
 * az_replay_append_engine on an engine with a cap in force applies the engine's own mask in this way; on an engine without one it
 * does what it always did.
 */
int az_replay_append_device_kept(az_replay *r, const void *dev_buf, int64_t n_games, int32_t start_ply, const int32_t *start_ply_dev,
                                 const uint64_t *keys_dev, const uint8_t *keep_dev, void *stream);

/* Trainer.remove_duplicates over the whole (flattened) buffer.  Synchronises `stream`.  Records are grouped by the
 * 64-bit history hash; every member of a group is then checked against the group's first record (a second, independent
 * 64-bit hash of the history, the ply and the position): a mismatch - two different histories under one key, which the
 * reference, keying on the exact information-state string (train.py:177), would keep apart - returns AZ_E_DEVICE. */
int az_replay_dedupe(az_replay *r, void *stream);

/*
 * Merging transpositions and mirror images (replaces nothing in the reference: Trainer.remove_duplicates keys on the history
 * alone).  The net sees (bb0, bb1, ply & 1) only, both games transpose and both are left-right symmetric, so examples of one
 * position reached along different histories - or of a position and its mirror image - are labels of one input.
 *
 * az_replay_dedupe_positions is az_replay_dedupe with another equivalence:
 *
 * GROUP.  Two stored examples are the same iff their canonical triples (c0, c1, ply & 1) are equal.
 *   - With mirror == 0, (c0, c1) = (bb0, bb1) as stored.
 *   - With mirror != 0, let m = az_mirror_state(s).  flip = 1 iff (m.bb0, m.bb1) < (s.bb0, s.bb1), compared as unsigned pairs
 *     with bb0 the major word.  (c0, c1) is the smaller pair.
 *   - A position that is its own mirror image has flip = 0.
 *   - mirror is 0 or 1.  Anything else returns AZ_E_INVALID (and the store, its epoch included, is as it was).
 *
 * GROUPING IS EXACT, NOT HASHED.  The records are sorted on the full triple with three stable LSD passes - parity, then c1,
 * then c0 - and a segment starts where any of the three words differs from the previous record's.  This pass has no collision
 * case: it neither raises nor clears AZ_REPLAY_FAULT_KEY_COLLISION.
 *
 * ORDER.  Members of a group are in buffer order (the sort is stable).  The unique list is in first-occurrence order, as
 * az_replay_dedupe's.
 *
 * AVERAGE.  All arithmetic is float64, one rounding per operation, in the reference's order:
 *   - acc = pi_first[a];
 *   - for every later member j in buffer order: acc = acc + pi_j[a'];
 *   - a' = a when flip_j == flip_first, else a' = az_mirror_action(a);
 *   - then pi_first[a] = acc / (double)cnt.  z is treated likewise, with no mapping.
 *   - A group of one is not written.
 *   - The average is written into the FIRST OCCURRENCE IN ITS OWN STORED ORIENTATION, as the history pass writes back
 *     (train.py:191-197).  Later members are left alone.
 *   - Deliberately not done: a self-symmetric position is not averaged with its own mirrored policy.
 *
 * BOOKKEEPING is exactly az_replay_dedupe's: the epoch advances, n_unique is set, unique[] points at first occurrences, the
 * call synchronises `stream`, and an empty store returns AZ_OK with n_unique = 0.
 *
 * EVERY READER OF THE UNIQUE LIST STAYS UNCHANGED: az_replay_sample, _sample_sym, _gather_states, _gather_forks, the two
 * refresh entries and az_replay_read_unique read the first occurrence's own state, ply and history key pair.  A fork from a
 * merged entry carries the first occurrence's history.
 *
 * MIXING THE TWO RULES.  A later az_replay_dedupe regroups by history over whatever the buffer then holds, as it always did.
 *
 * Limits: ply & 1, not ply, is part of the key; self-symmetric positions are not symmetrised; a second position dedupe
 * averages the written-back first occurrence with its members again, as a second az_replay_dedupe does (the reference's
 * aliasing).
 *
 * az_replay_unique_counts_device writes the member count of every unique entry of the last dedupe, of either kind, to a device
 * i32 [n] in the order of the unique list.  n must equal n_unique, else AZ_E_INVALID.  AZ_E_STATE before any dedupe, and once
 * an append or a capacity change has moved the epoch (the state is looked at first).  Asynchronous on `stream`.  Both dedupe
 * entries fill the counts, in a store-owned array sized like the unique list.
 */
int az_replay_dedupe_positions(az_replay *r, int32_t mirror, void *stream);
int az_replay_unique_counts_device(az_replay *r, int32_t *counts_out_dev, int64_t n, void *stream);

/* The sampling of net_step (train.py:108-120): gather `batch` examples of the de-duplicated list into
 * x [batch][4][H][W] float32, pi [batch][A] float32, z [batch] float32 (all device).  `indices` (device int64
 * [batch], values in [0, n_unique)) are the `np.random.randint(len(flattened_buffer), size=batch_size)` draw;
 * pass NULL to draw them on the device (one splitmix64 draw per row over (seed, call counter, row), scaled to
 * [0, n_unique) by the high half of a 64x64-bit product).  An index outside [0, n_unique) fills its
 * row with NaN and raises AZ_REPLAY_FAULT_BAD_INDEX (asynchronous: reported by az_replay_stats_get). */
int az_replay_sample(az_replay *r, const int64_t *indices, int32_t batch, uint64_t seed, float *x, float *pi,
                     float *z, void *stream);

/* az_replay_sample with a left-right mirror bit per row (no counterpart in the reference).  Both games are symmetric under
 * column c -> cols-1-c: the mirror image of a position has the mirrored policy and the same value (az_mirror_state /
 * az_mirror_action in csrc/az_games.h), so a row may be handed to the net in either orientation.  `flips` (device uint8
 * [batch], 0 = as stored, non-zero = mirrored) chooses per row; pass NULL to draw the bits on the device, one fair coin per
 * row over (seed, call counter, row) that goes through a splitmix64 step of its own after the word that picks the example, so
 * the orientation says nothing about the index.  A mirrored row holds the observation of the mirrored position, pi with
 * pi_out[mirror(a)] = pi[a], and z as stored; a row that is not mirrored holds exactly what az_replay_sample writes.  indices,
 * the device draw for indices == NULL (with equal seed and call counter both entries pick the same examples), the NaN row and
 * AZ_REPLAY_FAULT_BAD_INDEX for an index outside [0, n_unique), and AZ_E_STATE before a dedupe are az_replay_sample's; the two
 * entries count their calls in one counter.  Asynchronous on `stream`; nothing is read back, so with device `indices` and
 * `flips` a call can be captured into a graph (a replay then repeats the call number it was captured with). */
int az_replay_sample_sym(az_replay *r, const int64_t *indices, const uint8_t *flips, int32_t batch, uint64_t seed, float *x,
                         float *pi, float *z, void *stream);

/*
 * Reanalyse: search stored positions again with the current network and overwrite their targets, device to device:
 *   az_replay_gather_states -> az_engine_set_start_states_device -> reset, tick -> az_engine_export_roots_device
 *   (+ az_engine_export_lines_device) -> az_replay_refresh_from_roots (az_replay_refresh_from_search)
 * The store counts its appends, dedupes and capacity changes (an epoch); az_replay_gather_states records the epoch and a
 * refresh under another one returns AZ_E_STATE: after a FIFO eviction or a new dedupe the indices may name other records.
 *
 * az_replay_gather_states: indices = device int64 [n], the index space of az_replay_sample (the de-duplicated list,
 * [0, n_unique)).  Writes bb_out u64[n][2], ply_out i32[n]: the inputs of az_engine_set_start_states_device.  Asynchronous.
 * An index outside the list raises AZ_REPLAY_FAULT_BAD_INDEX and gives the state ply = -1, which the engine's check refuses.
 *
 * az_replay_refresh_from_roots: roots = a device buffer (16-byte aligned) in the layout of az_engine_export_roots_device, of an
 * engine whose game id j searched indices[j].  For every slot with phase 5 and 0 <= game_id < n: pi of the stored example (the
 * FIRST occurrence the unique entry points at; its duplicates are left alone) becomes the normalised root visit counts - the
 * arithmetic of the append path, 1/n_children each when no child has a visit - and z follows value_mode.  A slot whose ply
 * differs from the stored example's, or with a child action outside [0, A), is skipped and raises
 * AZ_REPLAY_FAULT_ROOT_MISMATCH; a bad index is skipped and raises AZ_REPLAY_FAULT_BAD_INDEX.  The 16-byte header is read
 * first: AZ_E_INVALID when its slot / child counts do not fit roots_bytes or the store's game, AZ_E_DEVICE when it carries
 * engine fault flags; nothing is written then.  Synchronises `stream`; returns the number of examples refreshed, or < 0.
 *
 * Duplicate indices in one call: the result of the lowest slot is stored (without root noise all of them are the same bits).
 * The next az_replay_dedupe averages a refreshed first occurrence with its stale duplicates, exactly as the reference's
 * aliasing treats any first occurrence (train.py:191-197).  The off-policy target (A0GB) is no function of a root: given
 * AZ_REFRESH_OFF_POLICY this entry returns AZ_E_INVALID and leaves the store untouched - use az_replay_refresh_from_search.
 * On-policy targets (the game's outcome) cannot be refreshed by a search at all.
 *
 * az_replay_refresh_from_search: the same refresh (the same claim, write and release kernels) with the greedy lines of the
 * searches at hand: lines = a device buffer (16-byte aligned) in the layout of az_engine_export_lines_device, exported from the
 * same engine at the same moment as roots; any max_depth will do, the value does not depend on it.  With lines == NULL and
 * value_mode 0, 1 or 2 it is az_replay_refresh_from_roots (lines is read in AZ_REFRESH_OFF_POLICY only).
 * AZ_REFRESH_OFF_POLICY requires lines: its header is validated against lines_bytes and against the roots' slot count before
 * anything is written (AZ_E_INVALID; AZ_E_DEVICE when either header carries engine fault flags); pi comes from the roots as in
 * the other modes and z = value[slot].  A slot whose game_id, ply or phase in lines differs from the roots', or whose
 * depth < 0, is skipped and raises AZ_REPLAY_FAULT_ROOT_MISMATCH.  The epoch refusal (AZ_E_STATE) is that of the other entry.
 */
int az_replay_gather_states(az_replay *r, const int64_t *indices, int64_t n, uint64_t *bb_out, int32_t *ply_out, void *stream);
int64_t az_replay_refresh_from_roots(az_replay *r, const int64_t *indices, int64_t n, const void *roots, int64_t roots_bytes,
                                     int32_t value_mode, void *stream);
int64_t az_replay_refresh_from_search(az_replay *r, const int64_t *indices, int64_t n, const void *roots, int64_t roots_bytes,
                                      const void *lines, int64_t lines_bytes, int32_t value_mode, void *stream);

/* Counters and device fault flags; synchronises the device.  Returns AZ_E_DEVICE when a fault flag is set; the flags are
 * reported ONCE (cleared by this call).  az_replay_dedupe clears AZ_REPLAY_FAULT_KEY_COLLISION when it starts, leaves a group
 * whose members differ untouched (nothing is averaged across different histories) and returns AZ_E_DEVICE for that pass. */
int az_replay_stats_get(az_replay *r, az_replay_stats *out);

/* Debug/parity read-back of the de-duplicated list (host arrays; any may be NULL): key hash, pi [n][A] float64,
 * z float64, index of the record in the flattened buffer, its bitboards and ply.  Returns n_unique or <0. */
int64_t az_replay_read_unique(az_replay *r, int64_t max_n, uint64_t *key, double *pi, double *z, int64_t *buffer_index,
                              uint64_t *bitboards, int32_t *ply);
/* Test hook for the collision guard of az_replay_dedupe: overwrite the 64-bit grouping key of stored example `index`
 * (its second hash, ply and position stay), so two different histories can be made to share a key. */
int az_replay_debug_set_key(az_replay *r, int64_t index, uint64_t key);
/* Read back one stored example of the flattened buffer (after write-back): pi [A], z. */
int az_replay_read_example(az_replay *r, int64_t index, double *pi, double *z);

#ifdef __cplusplus
}
#endif
#endif /* AZ_REPLAY_H */
