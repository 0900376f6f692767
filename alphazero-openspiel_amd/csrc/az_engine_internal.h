// az_engine_internal.h — definitions shared by az_engine.hip, az_starts.hip and az_replay.hip (NOT part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/az_engine.h"
#include "az_games.h"
#include "az_keychain.h"
#include "az_records.h"
#include "az_starts.h"

#define NONE32 0xFFFFFFFFu

enum { PH_IDLE = 0, PH_RUN = 1, PH_MOVE = 2, PH_WAIT_ROOT = 3, PH_WAIT_LEAF = 4, PH_SEARCH_DONE = 5, PH_NEED_ROOT = 6,
       PH_OPPONENT = 7 /* arena: the opponent bot is to move */, PH_OPP_DONE = 8 /* ... and has chosen (opp_action) */ };
enum { ST_MOVES = 0, ST_SIMS, ST_EVALS, ST_TERM, ST_DEPTH, ST_CHILDREN, ST_NODES, ST_COMPACT, ST_N };

// One search-tree node (mcts.py:10-20 Node: N, Q, P, children).  32 bytes, so a block of sibling nodes is one
// contiguous run and a lane fetches its child with two 16-byte loads.
struct __attribute__((aligned(32))) AzNode {
    uint32_t N;    // visit count
    uint32_t C0;   // index of the first child in the slot's pool half (NONE32 = leaf)
    uint32_t META; // action leading here | n_children << 16
    uint32_t status; // MCTS-Solver proof (AZ_PROOF_*), seen by the player who moved INTO the node like Q; 0 = unknown, and all a
                     // kernel without the solver ever writes
    double Q, P;
};

struct PwPlan { // numpy pairwise-sum recursion for a length-A vector, flattened (see np_sum_sparse)
    int n_blocks;
    int lo[16], len[16];
    int n_ops;
    int ops[32]; // >=0: push block i, -1: add top two
};
static inline void pw_build(PwPlan &pw, int lo, int n) { // numpy pairwise_sum recursion (PW_BLOCKSIZE 128)
    if (n <= 128) {
        pw.lo[pw.n_blocks] = lo;
        pw.len[pw.n_blocks] = n;
        pw.ops[pw.n_ops++] = pw.n_blocks++;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    pw_build(pw, lo, n2);
    pw_build(pw, lo + n2, n - n2);
    pw.ops[pw.n_ops++] = -1;
}

// Playout cap randomisation, device side (one record per engine, written by az_engine_set_playout_cap).  az_engine_reset draws the
// generation's schedule into `sched` (one byte per game id and absolute ply, 1 = full search: az_cap_schedule_kernel); a slot that
// arms a search reads its byte and starts a fast search's counter at S - n_fast, so the tick kernel's `sims >= S` ends both kinds.
// sims_base [G]: that start value, subtracted by the read-back paths only; rec_full: one byte per (game row, ply) beside
// rec_nchild, written by move_step with the record: 1 = the recorded move was searched in full.
struct CapDev {
    int n_fast, pad;
    double p_full;
    int *sims_base;
    uint8_t *sched, *rec_full;
};

// Self-play resignation, device side (one record per engine, written by az_engine_set_resign; include/az_engine.h states the
// rule).  The three arrays are indexed by the row of the rec_* arrays that holds the game (rec_row), beside the records:
// resign_ply [max_games] the game's first resign ply (-1: none), flags [max_games] bit 0 = the game ended there, bit 1 = it is a
// play-through game, low [max_games][2] per player the lowest criterion at a qualifying ply (+inf: none).  A row is cleared when a
// slot takes the game id that maps to it (az_reset_kernel, take_next_game); move_step alone writes it after that.
struct ResDev {
    double v, p_playthrough;
    int min_ply, pad;
    int *resign_ply;
    uint8_t *flags;
    double *low;
};

struct Params {
    // geometry / config
    AzGeom geom;
    int game, A, maxc, max_plies, obs_elems, pstride;
    int G, S, use_dirichlet, keep_tree, backup, rng_mode, max_sims_per_tick, manual_moves, chain_clocks;
    uint32_t cap, need_per_move;
    int forced_prune; // az_engine_set_forced_playouts (with forced_k at the end of the record; here it fills a hole of the layout)
    double c_puct, one_minus_ratio, alpha, inv_temp;
    uint64_t seed;
    long long n_games, max_games;
    AzState start;
    PwPlan pw;
    // node pools (array of structures: a child block is one contiguous run of 32-byte nodes): G + n_spare pools of `cap` nodes.
    // A slot OWNS one pool (which[g] & POOL_MASK); a compaction copies the kept subtree into a spare pool taken from
    // spare[] (entry = pool id, -1 = taken) and hands the old pool back through the same entry.
    AzNode *nodes;
    int n_spare;
    int *spare;
    // handed-over compaction: a slot that must compact while re-rooting takes a spare pool, becomes its owner (root 0) and
    // publishes a job once its own state is stored; the extra workgroups of the SAME launch copy the subtree, a workgroup per
    // job, and leave only when every slot wave of the launch has finished and the list is drained.  Nothing about a job outlives
    // its launch (no host-side parity or epoch: a captured graph replays any number of launches).
    int defer_compact;              // this launch carries the extra workgroups (set per launch by the host)
    int *cj_job, *cj_seen;          // [G] by ROW of the launch: slot + 1 whose copy the row's wave handed over (0: none); the epoch in
                                    // which the row's wave last finished
    int *cjob_count;                // [0] = the epoch of the running launch (advanced by the last extra workgroup out), [2] = extra
                                    // workgroups finished
    int *cj_from, *cj_entry;        // [G] the pool the subtree is copied out of; the spare[] entry that takes it back
    uint32_t *cj_root;              // [G] index of the new root in that pool
    // per slot
    int *phase, *gid, *ply, *sims, *which, *depth, *leaf_ply;
    uint32_t *root, *alloc, *leaf_node, *path;
    uint64_t *bb0, *bb1, *leaf_bb0, *leaf_bb1;
    unsigned long long *stats; // [G][ST_N]
    // dense rows (tail of a generation): row_slot[i] = the i-th slot that still plays, req_row[g] = the row of the request /
    // answer buffers that holds slot g's outstanding request; n_rows_live (device) = length of the list
    int *row_slot, *req_row, *n_rows_live;
    // global counters
    unsigned long long *next_game, *games_done;
    // stream mode (az_engine_stream_begin): game ids are open-ended, id i records into row i % max_games of the rec_* arrays, and
    // an id may be handed out only while it is below *hand_limit (device memory: a captured tick graph bakes Params, and
    // az_engine_stream_take_device raises the limit between replays)
    int stream_mode;
    unsigned long long *hand_limit;
    unsigned int *faults;
    // injected randomness
    const double *etas, *us;
    double *eta_buf; // [G][maxc] Dirichlet draw staged with the root request (Philox mode)
    // arena (evaluation games against a bot)
    int arena_agent, opp_kind, opp_sims, arena_flip;
    double opp_c;
    int *opp_action;           // [G] the opponent bot's chosen move
    uint32_t uct_cap;          // UCT opponent: nodes per slot
    uint32_t *uct_N, *uct_C0, *uct_META; // [G][uct_cap] explore_count, first child, action | n_children << 16
    double *uct_W;             // [G][uct_cap] total_reward, seen by the player who moved into the node
    const double *log_table;   // [log_n] log(n) computed on the host (glibc), so that host and device agree bit for bit
    uint32_t log_n;
    int arena_prob, n_prob_plies; // use_probabilistic_actions outside self-play; num_probabilistic_actions (alphazerobot.py:34-36)
    int select_rule;           // AZ_SELECT_*: rule of the trees update_root starts from a leaf root (mcts.py:199-200)
    // records
    int *rec_len;
    float *rec_ret0;
    uint64_t *rec_states;
    uint16_t *rec_move, *rec_child_action;
    uint8_t *rec_nchild;
    uint32_t *rec_child_visits;
    double *rec_value;
    // start position per GAME ID: null = every game starts from `start`.  Set for manual_moves engines by
    // az_engine_set_start_positions / az_engine_set_start_states_device, for plain self-play engines by az_engine_set_game_starts /
    // az_engine_set_game_starts_device, for arena engines by az_engine_set_arena_openings.  Read by game id at reset, at take-next
    // and at game end only - never per tick.
    const AzState *starts;
    // playout cap randomisation (az_engine_set_playout_cap): null = none.  One pointer (Params grows by 8 bytes); only the cold
    // paths (reset, move_step, the read-backs) follow it.  Register figures of the tick kernel: DESIGN.md section 4.
    const CapDev *capdev;
    // forced playouts and policy target pruning (az_engine_set_forced_playouts): k = 0 = none.  Read by the FORCED instantiations
    // of az_advance_kernel only, which the host launches while forced_k > 0; the others never touch the two fields.
    double forced_k;
    // evaluation in a random left-right orientation (az_engine_set_eval_mirror): 0 = none.  Read by the MIRROR instantiations of
    // az_advance_kernel only, which the host launches while p_mirror > 0; appended, so no other field moves.
    double p_mirror;
    // MCTS-Solver (az_engine_set_solver): 0 = off.  Read by the host's launch alone, which picks the SOLVER instantiations of
    // az_advance_kernel while it is set; appended, so no other field moves.
    int solver;
    // first-play urgency (az_engine_set_fpu): fpu_on = 0 = the reference's Q = 0 for an unvisited child.  fpu_on is read by the host's
    // launch alone, which picks the FPU instantiations of az_advance_kernel while it is set (the word was padding); these read the
    // two reductions, appended, so no other field moves.
    int fpu_on;
    double fpu_reduction, fpu_reduction_root;
    // self-play resignation (az_engine_set_resign): null = none.  One pointer, appended, so no other field moves; only the cold
    // paths (reset, game turnover, move_step after the move is recorded, the read-back) follow it.
    const ResDev *resdev;
};
static_assert(sizeof(Params) == 992, "Params is passed by value to every kernel and baked into captured graphs: its layout does not move");

// The engine's own record arrays as a view (az_records.h); the tick kernel keeps reading p.rec_* itself.
static inline AzRecords records_of(const Params &p) {
    return AzRecords{p.rec_len, p.rec_ret0, p.rec_states, p.rec_move, p.rec_nchild, p.rec_child_action, p.rec_child_visits, p.rec_value};
}

// Where games start.  The table lives in device memory by game id and is read at reset, at take-next and at game end only.
enum StartKind {
    START_UNIFORM = 0,  // every game starts from Params::start (Params::starts is null); prefixed: a non-empty prefix gave it
    START_PER_POSITION, // manual_moves engines (az_engine_set_start_positions / _start_states_device): Params::starts = states
    START_PER_GAME,     // plain self-play engines (az_engine_set_game_starts / _device) and arena engines
                        // (az_engine_set_arena_openings): the same, and plies, keys, h_plies count
};
struct StartTable {
    StartKind kind = START_UNIFORM;
    bool prefixed = false;
    // START_PER_GAME: the key pairs were GIVEN (a prefix's chain, or the caller's keys_dev) and the games' key chains step by
    // absolute ply; otherwise they are the start states' own seeds and the games are keyed as ordinary ones (az_keychain.h)
    bool keyed = false;
    int64_t n = 0, cap = 0;    // entries in force (0 = no table), entries allocated (kept across setter calls)
    AzState *states = nullptr; // [cap]
    int32_t *plies = nullptr;  // [cap] the states' plies as plain int32 (what the replay append indexes with)
    uint64_t *keys = nullptr;  // [cap][2] history key pairs
    unsigned long long *check = nullptr; // result word of the device forms' validity pass
    std::vector<int32_t> h_plies;        // START_PER_GAME: host copy of plies[0..n)
};

struct az_engine {
    az_config cfg;
    Params p;
    az_sizes sizes;
    std::string err;
    std::vector<void *> dev_allocs;
    bool reset_done = false;
    int64_t n_games = 0;
    double *d_etas = nullptr, *d_us = nullptr;
    int *d_actions = nullptr;
    int64_t ticks = 0;
    int64_t inj_games = 0;
    StartTable start; // where games start: read through the accessors below, written by csrc/az_starts.hip alone
    CapDev cap = {0, 0, 0.0, nullptr, nullptr, nullptr}; // host copy of the playout cap's record; d_cap: the device record (p.capdev when a cap is in force)
    CapDev *d_cap = nullptr;
    ResDev res = {0.0, 0.0, 0, 0, nullptr, nullptr, nullptr}; // host copy of the resignation record; d_res: the device record (p.resdev while set)
    ResDev *d_res = nullptr;
    bool rows_mapped = false; // az_engine_compact_rows has been called since the last reset
    int rows_live = 0;
    bool streaming = false;   // az_engine_stream_begin since the last az_engine_reset
    int64_t read_pos = 0;     // stream mode: the first game id not yet taken
    int64_t ready_known = 0;  // ... and how many consecutive finished games the last az_engine_stream_ready found from there
    std::vector<int32_t> h_ring; // ... host copy of the rec_len ring for that scan
    bool may_compact = false; // a pool cannot hold a whole game: re-rooting may have to compact (launches carry extra workgroups)
    // az_engine_export's host copy of the records, in the packed layout (az_records.h); 16-byte elements keep it aligned
    struct alignas(16) HostBlock { unsigned char b[16]; };
    std::vector<HostBlock> h_records;
};

// What the rest of the library asks about the start of games (nobody outside csrc/az_starts.hip reads StartTable's kind or keyed).
// Entries of the table in force by game id; 0 = none, every game starts from Params::start.
static inline int64_t start_table_n(const az_engine *e) { return e->start.kind == START_UNIFORM ? 0 : e->start.n; }
// No table, and a non-empty prefix gave Params::start.
static inline bool start_prefixed(const az_engine *e) { return e->start.kind == START_UNIFORM && e->start.prefixed; }
// Device array of the games' own start plies [start_table_n]; null = Params::start.ply for every game.
static inline const int32_t *start_plies_dev(const az_engine *e) { return e->start.kind == START_PER_GAME ? e->start.plies : nullptr; }
// Device array of the games' GIVEN key pairs [start_table_n][2]; null = every game is keyed from its start state.
static inline const uint64_t *start_keys_dev(const az_engine *e) {
    return e->start.kind == START_PER_GAME && e->start.keyed ? e->start.keys : nullptr;
}
// Start ply of game g, on the host.
static inline int start_ply_of(const az_engine *e, int64_t g) {
    return e->start.kind == START_PER_GAME ? e->start.h_plies[(size_t)g] : e->p.start.ply;
}
// Releases the table's arrays (the caller has taken it out of force).
static inline void start_table_free(StartTable &t) {
    if (t.states) (void)hipFree(t.states);
    if (t.plies) (void)hipFree(t.plies);
    if (t.keys) (void)hipFree(t.keys);
    t.states = nullptr;
    t.plies = nullptr;
    t.keys = nullptr;
    t.cap = 0;
}

#define HIPCHK(e, call)                                                                      \
    do {                                                                                     \
        hipError_t _s = (call);                                                              \
        if (_s != hipSuccess) {                                                              \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_s);                    \
            return AZ_E_HIP;                                                                 \
        }                                                                                    \
    } while (0)

// The packed root export (layout: include/az_engine.h, az_engine_export_roots_device): written by az_engine.hip, read by the
// replay store's az_replay_refresh_from_roots.
#define AZ_ROOTS_ARRAYS 12
static inline void roots_offsets(size_t G, size_t mc, size_t off[AZ_ROOTS_ARRAYS + 1]) {
    const size_t sizes[AZ_ROOTS_ARRAYS] = {16, G * 4, G * 4, G * 4, G * 4, G * 4, G * 4, G * 8, G * mc * 4, G * mc * 4, G * mc * 8, G * mc * 8};
    off[0] = 0;
    for (int i = 0; i < AZ_ROOTS_ARRAYS; i++) off[i + 1] = off[i] + ((sizes[i] + 15) & ~(size_t)15);
}
struct RootsOut {
    int *header, *game_id, *phase, *ply, *sims_done, *n_children;
    uint32_t *root_n;
    double *root_q;
    int *child_action;
    uint32_t *child_n;
    double *child_q, *child_p;
};
static inline RootsOut roots_arrays(void *dev_buf, size_t G, size_t mc) {
    size_t off[AZ_ROOTS_ARRAYS + 1];
    roots_offsets(G, mc, off);
    char *b = (char *)dev_buf;
    RootsOut o;
    o.header = (int *)(b + off[0]);
    o.game_id = (int *)(b + off[1]);
    o.phase = (int *)(b + off[2]);
    o.ply = (int *)(b + off[3]);
    o.sims_done = (int *)(b + off[4]);
    o.n_children = (int *)(b + off[5]);
    o.root_n = (uint32_t *)(b + off[6]);
    o.root_q = (double *)(b + off[7]);
    o.child_action = (int *)(b + off[8]);
    o.child_n = (uint32_t *)(b + off[9]);
    o.child_q = (double *)(b + off[10]);
    o.child_p = (double *)(b + off[11]);
    return o;
}

// The packed line export (layout: include/az_engine.h, az_engine_export_lines_device): written by az_engine.hip, read by the
// replay store's az_replay_refresh_from_search.
#define AZ_LINES_ARRAYS 10
static inline void lines_offsets(size_t G, size_t D, size_t off[AZ_LINES_ARRAYS + 1]) {
    const size_t sizes[AZ_LINES_ARRAYS] = {16, G * 4, G * 4, G * 4, G * 4, G * 4, G * 8, G * D * 4, G * D * 4, G * D * 8};
    off[0] = 0;
    for (int i = 0; i < AZ_LINES_ARRAYS; i++) off[i + 1] = off[i] + ((sizes[i] + 15) & ~(size_t)15);
}
struct LinesOut {
    int *header, *game_id, *phase, *ply, *depth;
    uint32_t *leaf_n;
    double *value;
    int *line_action;
    uint32_t *line_n;
    double *line_q;
};
static inline LinesOut lines_arrays(void *dev_buf, size_t G, size_t D) {
    size_t off[AZ_LINES_ARRAYS + 1];
    lines_offsets(G, D, off);
    char *b = (char *)dev_buf;
    LinesOut o;
    o.header = (int *)(b + off[0]);
    o.game_id = (int *)(b + off[1]);
    o.phase = (int *)(b + off[2]);
    o.ply = (int *)(b + off[3]);
    o.depth = (int *)(b + off[4]);
    o.leaf_n = (uint32_t *)(b + off[5]);
    o.value = (double *)(b + off[6]);
    o.line_action = (int *)(b + off[7]);
    o.line_n = (uint32_t *)(b + off[8]);
    o.line_q = (double *)(b + off[9]);
    return o;
}
