// az_starts.hip — where games start: the setters that install az_engine::start (StartTable, az_engine_internal.h) and
// az_engine_game_starts_device, which reads it back.  The C ABI: include/az_engine.h.
//
// One prefix for every game (az_engine_set_start_prefix), or a table by game id in device memory: for manual_moves engines
// (az_engine_set_start_positions / az_engine_set_start_states_device) and, with each game's start ply and history key pair beside
// its state, for plain self-play engines (az_engine_set_game_starts / az_engine_set_game_starts_device) and for arena engines
// (az_engine_set_arena_openings).  A table comes in a host
// form (an action prefix per game, replayed by az_starts.h) or a device form (states, checked on the device); each form has one
// install routine, and starts_in_force is the one place that says which kind of start holds.  A refused call changes nothing.
#include "az_engine_internal.h"

// The table holds at least n_games entries (a table that has to grow is dropped first: it is out of force until it is filled).
static int starts_reserve(az_engine *e, int64_t n_games) {
    StartTable &t = e->start;
    if (n_games <= t.cap) return AZ_OK;
    start_table_free(t);
    t.kind = START_UNIFORM;
    t.keyed = false;
    t.n = 0;
    e->p.starts = nullptr;
    HIPCHK(e, hipMalloc((void **)&t.states, (size_t)n_games * sizeof(AzState)));
    HIPCHK(e, hipMalloc((void **)&t.plies, (size_t)n_games * sizeof(int32_t)));
    HIPCHK(e, hipMalloc((void **)&t.keys, (size_t)n_games * 2 * sizeof(uint64_t)));
    t.cap = n_games;
    return AZ_OK;
}

// Everything that says where games start, set at once.  START_UNIFORM: every game starts from `uniform` (a table keeps its memory
// and is out of force).  Otherwise: the first n entries of the table, and `uniform` is the initial position (a table supersedes a
// single prefix).  The caller must reset again so that the slots pick the new start up.
static void starts_in_force(az_engine *e, StartKind kind, bool keyed, int64_t n, const AzState &uniform, std::vector<int32_t> h_plies) {
    StartTable &t = e->start;
    t.kind = kind;
    t.prefixed = kind == START_UNIFORM && uniform.ply > 0;
    t.keyed = kind == START_PER_GAME && keyed;
    t.n = kind == START_UNIFORM ? 0 : n;
    t.h_plies = std::move(h_plies);
    e->p.start = uniform;
    e->p.starts = kind == START_UNIFORM ? nullptr : t.states;
    e->reset_done = false;
}

extern "C" int az_engine_set_start_prefix(az_engine *e, const int32_t *actions, int32_t n) {
    if (!e || (n > 0 && !actions)) return AZ_E_INVALID;
    AzState s;
    AzKeyPair k;
    int bad = az_replay_prefix(e->cfg.game, e->p.geom, e->p.A, actions, n, s, k);
    if (bad) {
        e->err = bad == AZ_PREFIX_ILLEGAL ? "illegal prefix action" : "prefix ends the game";
        return AZ_E_INVALID;
    }
    starts_in_force(e, START_UNIFORM, false, 0, s, {}); // one prefix for every game again
    return AZ_OK;
}

// ---- the host form: an action prefix per game ------------------------------------------------------------------------------------
static int install_starts_host(az_engine *e, const char *what, StartKind kind, const int32_t *actions, const int32_t *lengths,
                               int64_t stride, int64_t n_games) {
    const std::string name(what);
    if (!lengths || n_games < 1 || n_games > e->cfg.max_games || stride < 0) {
        e->err = name + ": n_games must be in [1, max_games], lengths non-null, stride >= 0";
        return AZ_E_INVALID;
    }
    std::vector<AzState> tab((size_t)n_games);
    std::vector<int32_t> plies((size_t)n_games);
    std::vector<uint64_t> keys((size_t)n_games * 2);
    for (int64_t i = 0; i < n_games; i++) {
        const int32_t n = lengths[i];
        if (n < 0 || n > stride || (n > 0 && !actions)) {
            e->err = name + ": game " + std::to_string(i) + ": prefix length " + std::to_string(n) + " outside [0, stride]";
            return AZ_E_INVALID;
        }
        AzKeyPair k;
        int bad = az_replay_prefix(e->cfg.game, e->p.geom, e->p.A, n > 0 ? actions + i * stride : nullptr, n, tab[(size_t)i], k);
        if (bad) {
            e->err = name + ": game " + std::to_string(i) + (bad == AZ_PREFIX_ILLEGAL ? ": illegal prefix action" : ": prefix ends the game");
            return AZ_E_INVALID;
        }
        plies[(size_t)i] = tab[(size_t)i].ply;
        keys[(size_t)i * 2] = k.key;
        keys[(size_t)i * 2 + 1] = k.key2;
    }
    HIPCHK(e, hipSetDevice(e->cfg.device));
    HIPCHK(e, hipDeviceSynchronize()); // a reset of the previous chunk, a generation that still plays, or an append may be reading the table
    int rc = starts_reserve(e, n_games);
    if (rc != AZ_OK) return rc;
    HIPCHK(e, hipMemcpy(e->start.states, tab.data(), (size_t)n_games * sizeof(AzState), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->start.plies, plies.data(), (size_t)n_games * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->start.keys, keys.data(), (size_t)n_games * 2 * sizeof(uint64_t), hipMemcpyHostToDevice));
    starts_in_force(e, kind, true, n_games, az_initial_state(e->cfg.game, e->p.geom), std::move(plies));
    return AZ_OK;
}

// ---- the device form: the states come as bitboards and plies in device memory (az_replay_gather_states writes them) -------------
// One thread per state runs az_check_state; the lowest offending index and its rule reach the host as one word,
// (index << 8) | rule, through a 64-bit atomicMin, and only a clean pass is followed by the kernel that fills the table.
#define START_CHECK_CLEAN ~0ull
template <int GAME>
__global__ void az_check_start_states_kernel(AzGeom geom, int max_plies, const uint64_t *bb, const int32_t *ply, long long n,
                                             unsigned long long *result) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    AzState s;
    s.bb0 = bb[2 * i];
    s.bb1 = bb[2 * i + 1];
    s.ply = ply[i];
    int rule = az_check_state<GAME>(s, geom, max_plies);
    if (rule != AZ_STATE_OK) atomicMin(result, ((unsigned long long)i << 8) | (unsigned long long)rule);
}

// The validity pass: every state through az_check_state on the device, the lowest offending index named in az_last_error as
// "<what>: game <i>: <rule>".  plies_out (may be null) receives a host copy of ply_dev.  Synchronises the device first (the states
// are written, and nothing reads the table any more) and `st` at the end.
static int check_start_states_device(az_engine *e, const char *what, const uint64_t *bb_dev, const int32_t *ply_dev, int64_t n_games,
                                     hipStream_t st, std::vector<int32_t> *plies_out) {
    HIPCHK(e, hipSetDevice(e->cfg.device));
    HIPCHK(e, hipDeviceSynchronize());
    if (!e->start.check) HIPCHK(e, hipMalloc((void **)&e->start.check, sizeof(unsigned long long)));
    unsigned long long res = START_CHECK_CLEAN;
    HIPCHK(e, hipMemcpyAsync(e->start.check, &res, sizeof res, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n_games + 255) / 256)), block(256);
    if (e->cfg.game == AZ_GAME_CONNECT_FOUR)
        hipLaunchKernelGGL(az_check_start_states_kernel<AZG_CONNECT_FOUR>, grid, block, 0, st, e->p.geom, e->p.max_plies, bb_dev, ply_dev,
                           (long long)n_games, e->start.check);
    else
        hipLaunchKernelGGL(az_check_start_states_kernel<AZG_BREAKTHROUGH>, grid, block, 0, st, e->p.geom, e->p.max_plies, bb_dev, ply_dev,
                           (long long)n_games, e->start.check);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(&res, e->start.check, sizeof res, hipMemcpyDeviceToHost, st));
    if (plies_out) {
        plies_out->resize((size_t)n_games);
        HIPCHK(e, hipMemcpyAsync(plies_out->data(), ply_dev, (size_t)n_games * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(e, hipStreamSynchronize(st));
    if (res != START_CHECK_CLEAN) {
        e->err = std::string(what) + ": game " + std::to_string(res >> 8) + ": " + az_state_rule_name((int)(res & 0xFF));
        return AZ_E_INVALID;
    }
    return AZ_OK;
}

// keys == null: every game's pair is its start state's own seed (what an ordinary game starting there carries at its first ply)
__global__ void az_fill_starts_kernel(const uint64_t *bb, const int32_t *ply, const uint64_t *keys, long long n, AzState *tab,
                                      int32_t *ply_tab, uint64_t *key_tab) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    AzState s;
    s.bb0 = bb[2 * i];
    s.bb1 = bb[2 * i + 1];
    s.ply = ply[i];
    tab[i] = s;
    ply_tab[i] = s.ply;
    AzKeyPair k;
    if (keys) k.key = keys[2 * i], k.key2 = keys[2 * i + 1];
    else k = az_key_seed(s.ply, s.bb0, s.bb1);
    key_tab[2 * i] = k.key;
    key_tab[2 * i + 1] = k.key2;
}

static int install_starts_device(az_engine *e, const char *what, StartKind kind, const uint64_t *bb_dev, const int32_t *ply_dev,
                                 const uint64_t *keys_dev, int64_t n_games, void *stream) {
    if (!bb_dev || !ply_dev || n_games < 1 || n_games > e->cfg.max_games) {
        e->err = std::string(what) + ": n_games must be in [1, max_games], bb_dev and ply_dev non-null";
        return AZ_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> plies; // (the host copy that only a per-game table keeps)
    int rc = check_start_states_device(e, what, bb_dev, ply_dev, n_games, st, kind == START_PER_GAME ? &plies : nullptr);
    if (rc != AZ_OK) return rc;
    rc = starts_reserve(e, n_games);
    if (rc != AZ_OK) return rc;
    const dim3 grid((unsigned)((n_games + 255) / 256)), block(256);
    hipLaunchKernelGGL(az_fill_starts_kernel, grid, block, 0, st, bb_dev, ply_dev, keys_dev, (long long)n_games, e->start.states,
                       e->start.plies, e->start.keys);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(st));
    starts_in_force(e, kind, keys_dev != nullptr, n_games, az_initial_state(e->cfg.game, e->p.geom), std::move(plies));
    return AZ_OK;
}

// ---- the four table entries: who may call, under which name, one install ---------------------------------------------------------
static int needs_manual_moves(az_engine *e, const char *what) {
    if (e->cfg.manual_moves) return AZ_OK;
    e->err = std::string(what) + " needs an engine created with manual_moves = 1: self-play and arena engines keep "
             "ONE start ply for the record offset, the value targets, the replay append and the side assignment";
    return AZ_E_INVALID;
}
static int game_starts_refusal(az_engine *e, const char *what) {
    const char *why = nullptr;
    if (e->p.arena_agent != AZ_ARENA_SELF_PLAY) why = "an arena engine (game id i fixes the agent's side from ONE start ply)";
    else if (e->cfg.manual_moves) why = "a manual_moves engine (az_engine_set_start_positions / az_engine_set_start_states_device are its entries)";
    else if (e->streaming) why = "an engine in stream mode (az_engine_stream_begin: game ids are open-ended, a table is not)";
    if (!why) return AZ_OK;
    e->err = std::string(what) + " is for plain self-play engines in a closed generation: refused for " + why;
    return AZ_E_INVALID;
}

extern "C" int az_engine_set_start_positions(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride,
                                             int64_t n_games) {
    if (!e) return AZ_E_INVALID;
    if (needs_manual_moves(e, "az_engine_set_start_positions")) return AZ_E_INVALID;
    return install_starts_host(e, "az_engine_set_start_positions", START_PER_POSITION, actions, lengths, stride, n_games);
}

extern "C" int az_engine_set_start_states_device(az_engine *e, const uint64_t *bb_dev, const int32_t *ply_dev, int64_t n_games,
                                                 void *stream) {
    if (!e) return AZ_E_INVALID;
    if (needs_manual_moves(e, "az_engine_set_start_states_device")) return AZ_E_INVALID;
    return install_starts_device(e, "az_engine_set_start_states_device", START_PER_POSITION, bb_dev, ply_dev, nullptr, n_games, stream);
}

extern "C" int az_engine_set_game_starts(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride, int64_t n_games) {
    if (!e) return AZ_E_INVALID;
    if (game_starts_refusal(e, "az_engine_set_game_starts")) return AZ_E_INVALID;
    return install_starts_host(e, "az_engine_set_game_starts", START_PER_GAME, actions, lengths, stride, n_games);
}

extern "C" int az_engine_set_game_starts_device(az_engine *e, const uint64_t *bb_dev, const int32_t *ply_dev, const uint64_t *keys_dev,
                                                int64_t n_games, void *stream) {
    if (!e) return AZ_E_INVALID;
    if (game_starts_refusal(e, "az_engine_set_game_starts_device")) return AZ_E_INVALID;
    return install_starts_device(e, "az_engine_set_game_starts_device", START_PER_GAME, bb_dev, ply_dev, keys_dev, n_games, stream);
}

// An opening per evaluation game: the same START_PER_GAME table on an arena engine (both agent kinds, every opponent kind).  The
// kernels read a game's start where they read a self-play table's - at reset, at take-next and at game end - and who moves first
// follows from the game's own ply (az_reset_kernel, opponent_to_move).
extern "C" int az_engine_set_arena_openings(az_engine *e, const int32_t *actions, const int32_t *lengths, int64_t stride, int64_t n_games) {
    if (!e) return AZ_E_INVALID;
    const char *why = nullptr;
    if (e->cfg.manual_moves) why = "a manual_moves engine (az_engine_set_start_positions / az_engine_set_start_states_device are its entries)";
    else if (e->p.arena_agent == AZ_ARENA_SELF_PLAY) why = "a self-play engine (az_engine_set_game_starts / az_engine_set_game_starts_device are its entries)";
    if (why) {
        e->err = std::string("az_engine_set_arena_openings is for arena engines: refused for ") + why;
        return AZ_E_INVALID;
    }
    return install_starts_host(e, "az_engine_set_arena_openings", START_PER_GAME, actions, lengths, stride, n_games);
}

// ---- read-back: every game id's start ply and key pair ---------------------------------------------------------------------------
// table == null: the uniform start of every game, and its seed pair
__global__ void az_game_starts_out_kernel(AzState start, const int32_t *ply_tab, const uint64_t *key_tab, long long n, int32_t *ply_out,
                                          uint64_t *keys_out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ply_out[i] = ply_tab ? ply_tab[i] : start.ply;
    if (!keys_out) return;
    if (key_tab) {
        keys_out[2 * i] = key_tab[2 * i];
        keys_out[2 * i + 1] = key_tab[2 * i + 1];
    } else {
        const AzKeyPair k = az_key_seed(start.ply, start.bb0, start.bb1);
        keys_out[2 * i] = k.key;
        keys_out[2 * i + 1] = k.key2;
    }
}

extern "C" int az_engine_game_starts_device(az_engine *e, int32_t *ply_out_dev, uint64_t *keys_out_dev, int64_t n_games, void *stream) {
    if (!e) return AZ_E_INVALID;
    const bool per_game = e->start.kind == START_PER_GAME;
    if (!ply_out_dev || n_games < 1 || n_games > e->cfg.max_games || (per_game && n_games > e->start.n)) {
        e->err = "az_engine_game_starts_device: ply_out_dev non-null, n_games in [1, max_games] and within the table";
        return AZ_E_INVALID;
    }
    HIPCHK(e, hipSetDevice(e->cfg.device));
    // (a per-game table's pairs are written out whether given or seeded; the return value tells the two apart)
    hipLaunchKernelGGL(az_game_starts_out_kernel, dim3((unsigned)((n_games + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->p.start,
                       per_game ? e->start.plies : nullptr, per_game ? e->start.keys : nullptr, (long long)n_games, ply_out_dev, keys_out_dev);
    HIPCHK(e, hipGetLastError());
    return start_keys_dev(e) ? 1 : 0;
}
