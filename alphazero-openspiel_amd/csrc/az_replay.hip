// az_replay.hip — device-resident replay store: FIFO of games, Trainer.remove_duplicates, batch gather.
// (reference: train.py:107-120 sampling, 156-201 remove_duplicates, 226-236 FIFO.)
//
// Storage = one ring of examples (SoA, capacity `cap`), logical index i -> physical (head + i) % cap, in the
// order the reference's flattened buffer has: games oldest -> newest, plies in order:
//   key u64 (hash of the action history) | bb0, bb1 u64 | ply i32 | z f64 | pi f64[A] (dense)
// and a host-side ring of game lengths for FIFO eviction.  HBM-bound integer/byte work; no MFMA anywhere.
//
// remove_duplicates, exactly: stable radix sort of (key, logical index) -> equal keys are adjacent and in buffer
// order -> one wave per segment, lane = action, each lane adds its pi component over the members IN ORDER in
// float64 (one rounding per addition, as `[sum(x) for x in zip(acc, item)]` does), divides by the count and
// writes the average back into the first member (the reference's aliasing side effect, train.py:191-197)
// -> unique list = first members in ascending buffer order (dict insertion order).
//
// az_replay_dedupe_positions (no counterpart in the reference) is the same pass grouped by the position instead of the history:
// canonical (c0, c1, ply & 1) per example -> three stable sorts on the full key (exact: nothing is hashed) -> the same segment
// scan and the same averaging body, which reads a member stored in the other orientation than the first through
// az_mirror_action.  Both passes leave the members' count of every group for az_replay_unique_counts_device.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <deque>
#include <string>
#include <vector>

#include "../../include/az_replay.h"
#include "az_engine_internal.h"

struct az_replay {
    az_replay_config cfg;
    std::string err;
    AzGeom geom;
    int A = 0, maxc = 0, max_plies = 0;
    PwPlan pw;
    int64_t cap = 0, head = 0, n = 0; // example ring
    std::deque<int32_t> game_len;     // FIFO of games (lengths), oldest first
    int64_t capacity_games = 0, dropped = 0, n_unique = 0;
    uint64_t sample_calls = 0;
    int64_t epoch = 0, gather_epoch = -1; // epoch: appends, dedupes and capacity changes so far; ... at the last az_replay_gather_states
    // device
    uint64_t *key = nullptr, *key2 = nullptr, *bb0 = nullptr, *bb1 = nullptr; // key2: an independent second hash of the history
    unsigned int *faults = nullptr;                                             // AZ_REPLAY_FAULT_* bits
    int32_t *ply = nullptr;
    double *z = nullptr, *pi = nullptr;
    int64_t *unique = nullptr; // [n_unique] logical indices of the first occurrences, ascending
    // count[i] = the members of the group whose first occurrence is logical index i, written by the last dedupe of either kind
    // (the other entries are stale); valid while epoch == count_epoch (az_replay_unique_counts_device)
    int32_t *count = nullptr;
    int64_t count_epoch = -1;
    // az_replay_refresh_from_roots: claim[phys] = the lowest slot that refreshes the example in the running call (REFRESH_FREE
    // between calls), sel[slot] = the example a slot refreshes (-1: none), refreshed = the call's count
    unsigned int *claim = nullptr;
    long long *sel = nullptr;
    int64_t sel_cap = 0;
    unsigned long long *refreshed = nullptr;
    // staging for append
    void *stage = nullptr;
    size_t stage_bytes = 0;
};
static std::string g_replay_err;

#define RCHK(r, call)                                                     \
    do {                                                                  \
        hipError_t _s = (call);                                           \
        if (_s != hipSuccess) {                                           \
            (r)->err = std::string(#call) + ": " + hipGetErrorString(_s); \
            return AZ_E_HIP;                                              \
        }                                                                 \
    } while (0)

extern "C" const char *az_replay_last_error(const az_replay *r) { return r ? r->err.c_str() : g_replay_err.c_str(); }

extern "C" int az_replay_destroy(az_replay *r) {
    if (!r) return AZ_OK;
    (void)hipSetDevice(r->cfg.device);
    (void)hipFree(r->key);
    (void)hipFree(r->key2);
    (void)hipFree(r->faults);
    (void)hipFree(r->bb0);
    (void)hipFree(r->bb1);
    (void)hipFree(r->ply);
    (void)hipFree(r->z);
    (void)hipFree(r->pi);
    (void)hipFree(r->unique);
    (void)hipFree(r->count);
    (void)hipFree(r->claim);
    (void)hipFree(r->sel);
    (void)hipFree(r->refreshed);
    (void)hipFree(r->stage);
    delete r;
    return AZ_OK;
}

extern "C" int az_replay_create(const az_replay_config *cfg, az_replay **out) {
    if (!cfg || !out) {
        g_replay_err = "null argument";
        return AZ_E_INVALID;
    }
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(az_replay_config)) {
        g_replay_err = "az_replay_config.struct_size mismatch";
        return AZ_E_INVALID;
    }
    az_replay_config c = *cfg;
    if (c.game == AZ_GAME_CONNECT_FOUR) {
        c.rows = 6;
        c.cols = 7;
    } else if (c.game != AZ_GAME_BREAKTHROUGH || c.rows < 4 || c.cols < 2 || c.rows * c.cols > 64 || 6 * c.cols > 64) {
        g_replay_err = "unsupported game / board";
        return AZ_E_INVALID;
    }
    if (c.max_games < 1 || c.max_examples < 1) {
        g_replay_err = "max_games and max_examples must be >= 1";
        return AZ_E_INVALID;
    }
    az_replay *r = new az_replay();
    r->cfg = c;
    r->geom = az_make_geom(c.game, c.rows, c.cols);
    r->A = az_num_actions(c.game, c.rows, c.cols);
    r->maxc = az_max_children(c.game, c.rows, c.cols);
    r->max_plies = az_max_plies(c.game, c.rows, c.cols);
    memset(&r->pw, 0, sizeof r->pw);
    pw_build(r->pw, 0, r->A);
    r->cap = c.max_examples;
    r->capacity_games = c.max_games;
    if (hipSetDevice(c.device) != hipSuccess) {
        g_replay_err = "hipSetDevice failed";
        delete r;
        return AZ_E_HIP;
    }
    size_t n = (size_t)r->cap;
    bool ok = hipMalloc((void **)&r->key, n * 8) == hipSuccess && hipMalloc((void **)&r->key2, n * 8) == hipSuccess &&
              hipMalloc((void **)&r->faults, 4) == hipSuccess && hipMemset(r->faults, 0, 4) == hipSuccess &&
              hipMalloc((void **)&r->bb0, n * 8) == hipSuccess &&
              hipMalloc((void **)&r->bb1, n * 8) == hipSuccess && hipMalloc((void **)&r->ply, n * 4) == hipSuccess &&
              hipMalloc((void **)&r->z, n * 8) == hipSuccess && hipMalloc((void **)&r->pi, n * 8 * (size_t)r->A) == hipSuccess &&
              hipMalloc((void **)&r->unique, n * 8) == hipSuccess && hipMalloc((void **)&r->count, n * 4) == hipSuccess &&
              hipMalloc((void **)&r->claim, n * 4) == hipSuccess &&
              hipMemset(r->claim, 0xFF, n * 4) == hipSuccess && hipMalloc((void **)&r->refreshed, 8) == hipSuccess;
    if (!ok) {
        g_replay_err = "hipMalloc of the replay store failed";
        az_replay_destroy(r);
        return AZ_E_NOMEM;
    }
    *out = r;
    return AZ_OK;
}

extern "C" int az_replay_set_capacity(az_replay *r, int64_t n_games) {
    if (!r || n_games < 1 || n_games > r->cfg.max_games) return AZ_E_INVALID;
    r->capacity_games = n_games;
    r->epoch++;
    return AZ_OK;
}

extern "C" int az_replay_stats_get(az_replay *r, az_replay_stats *out) {
    if (!r || !out) return AZ_E_INVALID;
    out->n_games = (int64_t)r->game_len.size();
    out->n_examples = r->n;
    out->n_unique = r->n_unique;
    out->games_dropped = r->dropped;
    out->fault_flags = 0;
    unsigned int f = 0;
    RCHK(r, hipSetDevice(r->cfg.device));
    RCHK(r, hipDeviceSynchronize());
    RCHK(r, hipMemcpy(&f, r->faults, 4, hipMemcpyDeviceToHost));
    out->fault_flags = f;
    if (f) RCHK(r, hipMemset(r->faults, 0, 4)); // reported once: the store is usable again after the caller has dealt with it
    if (f) {
        r->err = "device fault flags set:";
        if (f & AZ_REPLAY_FAULT_KEY_COLLISION) r->err += " KEY_COLLISION";
        if (f & AZ_REPLAY_FAULT_BAD_INDEX) r->err += " BAD_INDEX";
        if (f & AZ_REPLAY_FAULT_ROOT_MISMATCH) r->err += " ROOT_MISMATCH";
        return AZ_E_DEVICE;
    }
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t h, uint64_t v) { return az_key_mix64(h, v); } // (the device index draws use it too)

struct AppendArgs {
    AzRecords src; // one generation of games (the engine's record store, or a packed buffer), device pointers; read only
    const long long *dst_first; // [n_src_games] logical index of the game's first example, -1 = skip
    int n_src_games, max_plies, maxc, start_ply, A, on_policy;
    // a start per GAME (az_engine_set_game_starts, az_replay_append_device_starts): start_plies [n_src_games] replaces start_ply
    // when non-null; start_keys u64 [n_src_games][2] non-null = the games carry GIVEN history key pairs and their chains step by
    // absolute ply (az_keychain.h), null = every game is keyed from its start state as an ordinary game
    const int32_t *start_plies;
    const uint64_t *start_keys;
    // keep u8 [n_src_games][max_plies] by absolute ply, non-null = only the plies with a non-zero byte become examples
    // (az_replay_append_device_kept, an engine under a playout cap); a game's examples are then its kept plies, in ply order
    const uint8_t *keep;
    long long cap, head;
    PwPlan pw;
    uint64_t *key, *key2, *bb0, *bb1;
    int32_t *ply;
    double *z, *pi;
};

// np.sum (pairwise) of the dense length-A vector with non-zeros v[k] at act[k] (ascending), one thread.
__device__ double np_sum_sparse_serial(const PwPlan &pw, const double *v, const int *act, int nc) {
    double stack[6];
    int sp = 0, k = 0;
    for (int o = 0; o < pw.n_ops; o++) {
        int op = pw.ops[o];
        if (op < 0) {
            double b = stack[--sp], a = stack[--sp];
            stack[sp++] = a + b;
            continue;
        }
        int lo = pw.lo[op], n = pw.len[op];
        double res = 0.0;
        if (n < 8) {
            while (k < nc && act[k] < lo + n) res += v[k++];
        } else {
            double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int body = n - (n % 8), k0 = k;
            while (k < nc && act[k] < lo + n) {
                int j = act[k] - lo;
                if (j < body) r[j & 7] += v[k];
                k++;
            }
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (int kk = k0; kk < k; kk++)
                if (act[kk] - lo >= body) res += v[kk];
        }
        stack[sp++] = res;
    }
    return stack[0];
}

// The dense pi [A] of one example from its root's child visit counts (children in ascending-action order, nc <= 64 = the
// capacity of nv / act), one thread: float(visit)/sum(visits) -> remove_illegal_actions (np.sum pairwise, divide; 1/nc when no
// child has a visit) (mcts.py:161-162, alphazerobot.py:13-14).  The append kernel and the refresh kernel both store what THIS gives.
template <typename ActT>
__device__ void pi_from_root_visits(const PwPlan &pw, int A, int nc, const uint32_t *visits, const ActT *actions, double *out) {
    double nv[64];
    int act[64];
    long long tot = 0;
    for (int k = 0; k < nc; k++) tot += visits[k];
    for (int k = 0; k < nc; k++) {
        nv[k] = (double)visits[k] / (double)tot;
        act[k] = actions[k];
    }
    double s = np_sum_sparse_serial(pw, nv, act, nc);
    for (int x = 0; x < A; x++) out[x] = 0.0;
    for (int k = 0; k < nc; k++) out[act[k]] = s > 1e-6 ? nv[k] / s : 1.0 / (double)nc;
}

// one thread per (game, ply) example: state, z, dense pi from the recorded root visits
__global__ void replay_append_kernel(AppendArgs a) {
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int g = (int)(t / a.max_plies), i = (int)(t % a.max_plies);
    if (g >= a.n_src_games) return;
    long long first = a.dst_first[g];
    int len = a.src.game_len[g];
    if (first < 0 || i >= len) return;
    const int sp = a.start_plies ? a.start_plies[g] : a.start_ply;
    size_t src = (size_t)g * a.max_plies + sp + i;
    int rank = i; // the example's place within its game: the number of kept plies before it
    if (a.keep) {
        if (!a.keep[src]) return;
        rank = 0;
        for (int j = 0; j < i; j++) rank += a.keep[src - i + j] != 0;
    }
    long long dst = (a.head + first + rank) % a.cap;
    a.bb0[dst] = a.src.states[src * 2];
    a.bb1[dst] = a.src.states[src * 2 + 1];
    a.ply[dst] = sp + i;
    double zz = a.src.value[src];
    if (a.on_policy) { // game_utils.py:200-204: z_i = returns()[0] * (-1)^i, i the ABSOLUTE ply
        zz = (double)a.src.game_ret0[g];
        if ((sp + i) & 1) zz = -zz;
    }
    a.z[dst] = zz;
    int nc = a.src.n_children[src] < a.maxc ? a.src.n_children[src] : a.maxc;
    pi_from_root_visits(a.pw, a.A, nc, a.src.child_visits + src * a.maxc, a.src.child_action + src * a.maxc, a.pi + (size_t)dst * a.A);
}

// one thread per game: key chain over its moves (key of ply i = hash of the first i actions)
__global__ void replay_keys_kernel(AppendArgs a) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_src_games) return;
    long long first = a.dst_first[g];
    if (first < 0) return;
    int len = a.src.game_len[g];
    const int sp = a.start_plies ? a.start_plies[g] : a.start_ply;
    size_t s0 = (size_t)g * a.max_plies + sp;
    // The two chains (az_keychain.h): the reference keys on the EXACT information-state string (train.py:177); (key, key2)
    // together are a 128-bit fingerprint of the history, and the segment pass raises AZ_REPLAY_FAULT_KEY_COLLISION if two members
    // of one `key` segment differ in key2, ply or position.  An ordinary game is seeded from its start position (identical for
    // all games of a run) and steps with index 1, 2, ...; a game with a given pair continues that pair's history, by absolute ply.
    AzKeyPair k = {0, 0};
    int base = 0;
    if (a.start_keys) {
        k.key = a.start_keys[2 * (size_t)g];
        k.key2 = a.start_keys[2 * (size_t)g + 1];
        base = sp;
    } else if (len > 0) { // (a game without a recorded ply has no start state to read)
        k = az_key_seed(sp, a.src.states[s0 * 2], a.src.states[s0 * 2 + 1]);
    }
    for (int i = 0, rank = 0; i < len; i++) { // (the chains step over EVERY move: a kept example carries the key of its full history)
        if (!a.keep || a.keep[s0 + i]) {
            a.key[(a.head + first + rank) % a.cap] = k.key;
            a.key2[(a.head + first + rank) % a.cap] = k.key2;
            rank++;
        }
        k = az_key_step(k, (uint32_t)a.src.move[s0 + i], base + i + 1);
    }
}

static int append_common(az_replay *r, AppendArgs &a, const std::vector<int32_t> &lens, hipStream_t st) {
    // FIFO bookkeeping on the host (game granularity), like `self.buffer.append(game)` + the trim loop
    std::vector<long long> first(lens.size(), -1);
    long long add = 0;
    for (size_t g = 0; g < lens.size(); g++)
        if (lens[g] > 0) {
            first[g] = r->n + add;
            add += lens[g];
        }
    if (add > r->cap) {
        r->err = "one generation holds more examples than max_examples";
        return AZ_E_INVALID;
    }
    r->epoch++; // from here on the indices of an earlier az_replay_gather_states may name other records
    auto drop_oldest = [r]() -> int32_t { // the oldest game leaves the ring; -> its length
        const int32_t len = r->game_len.front();
        r->head = (r->head + len) % r->cap;
        r->n -= len;
        r->game_len.pop_front();
        r->dropped++;
        return len;
    };
    // make room in the example ring first (evict oldest games if the ring would overflow)
    while (r->n + add > r->cap && !r->game_len.empty()) {
        const int32_t len = drop_oldest();
        for (auto &f : first)
            if (f >= 0) f -= len;
    }
    long long *d_first = nullptr;
    RCHK(r, hipMalloc((void **)&d_first, sizeof(long long) * first.size()));
    RCHK(r, hipMemcpyAsync(d_first, first.data(), sizeof(long long) * first.size(), hipMemcpyHostToDevice, st));
    a.dst_first = d_first;
    a.cap = r->cap;
    a.head = r->head;
    a.A = r->A;
    a.pw = r->pw;
    a.key = r->key;
    a.key2 = r->key2;
    a.bb0 = r->bb0;
    a.bb1 = r->bb1;
    a.ply = r->ply;
    a.z = r->z;
    a.pi = r->pi;
    long long threads = (long long)a.n_src_games * a.max_plies;
    hipLaunchKernelGGL(replay_append_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(replay_keys_kernel, dim3((a.n_src_games + 255) / 256), dim3(256), 0, st, a);
    RCHK(r, hipGetLastError());
    RCHK(r, hipStreamSynchronize(st));
    (void)hipFree(d_first);
    for (size_t g = 0; g < lens.size(); g++)
        if (lens[g] > 0) r->game_len.push_back(lens[g]);
    r->n += add;
    // `while len(self.buffer) > self.n_games_buffer: del self.buffer[0]` (train.py:233-236)
    while ((int64_t)r->game_len.size() > r->capacity_games) drop_oldest();
    r->n_unique = 0;
    return AZ_OK;
}

// A keep mask (device u8 [n][max_plies] by absolute ply) against the games' rows [plies[g], plies[g] + lens[g]) (validated by the
// caller): copied to the host, a non-zero byte outside a game's rows is refused, kept[g] = the game's number of kept plies - its
// FIFO length.  Before any kernel runs: the store stays as it was.
static int kept_counts(az_replay *r, const uint8_t *keep_dev, const std::vector<int32_t> &lens, const std::vector<int32_t> &plies,
                       int32_t max_plies, hipStream_t st, std::vector<int32_t> &kept) {
    const size_t ng = lens.size(), mp = (size_t)max_plies;
    std::vector<uint8_t> h(ng * mp);
    RCHK(r, hipMemcpyAsync(h.data(), keep_dev, ng * mp, hipMemcpyDeviceToHost, st));
    RCHK(r, hipStreamSynchronize(st));
    kept.assign(ng, 0);
    for (size_t g = 0; g < ng; g++)
        for (int32_t i = 0; i < max_plies; i++) {
            if (!h[g * mp + (size_t)i]) continue;
            if (i < plies[g] || i >= plies[g] + lens[g]) {
                r->err = "keep byte at game " + std::to_string(g) + ", ply " + std::to_string(i) + " lies outside the game's recorded plies [" +
                         std::to_string(plies[g]) + ", " + std::to_string(plies[g] + lens[g]) + ")";
                return AZ_E_INVALID;
            }
            kept[g]++;
        }
    return AZ_OK;
}

extern "C" int az_replay_append_engine(az_replay *r, az_engine *e, void *stream) {
    if (!r || !e) return AZ_E_INVALID;
    if (e->cfg.game != r->cfg.game || e->cfg.rows != r->cfg.rows || e->cfg.cols != r->cfg.cols || e->cfg.device != r->cfg.device) {
        r->err = "engine and replay store were created for different games / devices";
        return AZ_E_INVALID;
    }
    if (e->streaming) {
        r->err = "az_replay_append_engine is refused for an engine in stream mode (az_engine_stream_begin): it reads the records by game "
                 "id; append what az_engine_stream_take_device packs with az_replay_append_device";
        return AZ_E_STATE;
    }
    hipStream_t st = (hipStream_t)stream;
    RCHK(r, hipSetDevice(r->cfg.device));
    RCHK(r, hipStreamSynchronize(st));
    std::vector<int32_t> lens((size_t)e->n_games);
    RCHK(r, hipMemcpy(lens.data(), e->p.rec_len, lens.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    AppendArgs a;
    memset(&a, 0, sizeof a);
    a.src = records_of(e->p);
    a.n_src_games = (int)e->n_games;
    a.max_plies = e->p.max_plies;
    a.maxc = e->p.maxc;
    a.start_ply = e->p.start.ply;
    a.start_plies = start_plies_dev(e); // a start per game: its own start ply and, when the table carries given pairs, its own key pair
    a.start_keys = start_keys_dev(e);
    a.on_policy = e->cfg.backup == AZ_BACKUP_ON_POLICY;
    if (!e->p.capdev) return append_common(r, a, lens, st);
    // a playout cap is in force: the engine's own mask of full-search moves decides which plies become examples
    const size_t ng = lens.size(), mp = (size_t)e->p.max_plies;
    uint8_t *d_keep = nullptr;
    RCHK(r, hipMalloc((void **)&d_keep, ng * mp));
    int rc = az_engine_full_moves_device(e, d_keep, (int64_t)ng, st);
    if (rc < 0) r->err = std::string("az_engine_full_moves_device: ") + az_last_error(e);
    std::vector<int32_t> plies(ng), kept;
    for (size_t g = 0; rc >= 0 && g < ng; g++) plies[g] = start_ply_of(e, (int64_t)g); // (rc >= 0: ng is within the table)
    if (rc >= 0) rc = kept_counts(r, d_keep, lens, plies, (int32_t)mp, st, kept);
    if (rc >= 0) {
        a.keep = d_keep;
        rc = append_common(r, a, kept, st); // (synchronises: the mask may be freed afterwards)
    }
    (void)hipFree(d_keep);
    return rc;
}

// A game length the kernels may run with: rows [start_ply, start_ply + len) of a record array with max_plies rows per game.
static bool game_len_ok(az_replay *r, const char *what, int64_t g, int32_t len, int32_t max_plies, int32_t start_ply) {
    if (len >= 0 && len <= max_plies - start_ply) return true;
    r->err = std::string(what) + ": game_len[" + std::to_string(g) + "] = " + std::to_string(len) + " is outside [0, max_plies - start_ply = " +
             std::to_string(max_plies - start_ply) + "]";
    return false;
}

extern "C" int az_replay_append_host(az_replay *r, const az_example_view *v, int32_t start_ply, void *stream) {
    if (!r || !v || v->n_games < 1 || v->max_children != r->maxc || v->max_plies < 1 || v->max_plies > r->max_plies ||
        start_ply < 0 || start_ply > v->max_plies) {
        if (r) r->err = "bad example view (max_children / max_plies must match the game, 0 <= start_ply <= max_plies)";
        return AZ_E_INVALID;
    }
    // everything the kernels index with is checked here, before any copy or launch: the store stays as it was
    for (int64_t g = 0; g < v->n_games; g++) {
        int32_t len = v->game_len[g];
        if (!game_len_ok(r, "az_replay_append_host", g, len, v->max_plies, start_ply)) return AZ_E_INVALID;
        for (int32_t i = 0; i < len; i++) {
            size_t src = (size_t)g * v->max_plies + start_ply + i;
            int nc = v->n_children[src];
            if (nc > v->max_children) {
                r->err = "n_children = " + std::to_string(nc) + " at game " + std::to_string(g) + ", ply " + std::to_string(start_ply + i) +
                         " is above max_children = " + std::to_string(v->max_children);
                return AZ_E_INVALID;
            }
            for (int k = 0; k < nc; k++)
                if (v->child_action[src * v->max_children + k] >= r->A) {
                    r->err = "child_action at game " + std::to_string(g) + ", ply " + std::to_string(start_ply + i) +
                             " is not an action of the game";
                    return AZ_E_INVALID;
                }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    RCHK(r, hipSetDevice(r->cfg.device));
    size_t ng = (size_t)v->n_games, mp = (size_t)v->max_plies, mc = (size_t)v->max_children;
    size_t sizes[AZ_RECORD_ARRAYS], off[AZ_RECORD_ARRAYS + 1];
    records_sizes(ng, mp, mc, sizes);
    records_offsets(ng, mp, mc, off);
    if (off[AZ_RECORD_ARRAYS] > r->stage_bytes) {
        (void)hipFree(r->stage);
        r->stage = nullptr;
        r->stage_bytes = 0;
        RCHK(r, hipMalloc(&r->stage, off[AZ_RECORD_ARRAYS]));
        r->stage_bytes = off[AZ_RECORD_ARRAYS];
    }
    AppendArgs a;
    memset(&a, 0, sizeof a);
    a.src = records_in(r->stage, ng, mp, mc);
    const void *srcs[AZ_RECORD_ARRAYS] = {v->game_len, v->game_ret0, v->states, v->move, v->n_children, v->child_action, v->child_visits, v->value};
    void *dsts[AZ_RECORD_ARRAYS];
    records_ptrs(a.src, dsts);
    for (int i = 0; i < AZ_RECORD_ARRAYS; i++) RCHK(r, hipMemcpyAsync(dsts[i], srcs[i], sizes[i], hipMemcpyHostToDevice, st));
    a.n_src_games = (int)ng;
    a.max_plies = (int)mp;
    a.maxc = (int)mc;
    a.start_ply = start_ply;
    a.on_policy = 0; // host views carry their value targets (az_engine_export fills on-policy z)
    std::vector<int32_t> lens(v->game_len, v->game_len + ng);
    return append_common(r, a, lens, st);
}

// One body for the three device append entries.  dev_buf: a packed export of n_games games in the store's board geometry
// (az_records.h; on_policy = 0: the export has filled those targets in).  start_ply_dev non-null = a start ply per game (replaces
// start_ply), with keys_dev = the games' given key pairs or null; keep_dev non-null = a keep mask (kept_counts).  Everything the
// kernels index with is read back and checked here, before any launch: a refused call leaves the store as it was.
static int append_packed(az_replay *r, const char *what, const void *dev_buf, int64_t n_games, int32_t start_ply,
                         const int32_t *start_ply_dev, const uint64_t *keys_dev, const uint8_t *keep_dev, hipStream_t st) {
    if (!r) return AZ_E_INVALID;
    if (!dev_buf || n_games < 1 || (!start_ply_dev && (start_ply < 0 || start_ply > r->max_plies))) {
        r->err = std::string(what) + ": bad device export (null buffer, n_games < 1, or - without a start ply per game - start_ply outside "
                 "[0, max_plies])";
        return AZ_E_INVALID;
    }
    RCHK(r, hipSetDevice(r->cfg.device));
    const size_t ng = (size_t)n_games;
    AppendArgs a;
    memset(&a, 0, sizeof a);
    a.src = records_in(const_cast<void *>(dev_buf), ng, (size_t)r->max_plies, (size_t)r->maxc);
    a.n_src_games = (int)ng;
    a.max_plies = r->max_plies;
    a.maxc = r->maxc;
    a.start_ply = start_ply;
    a.start_plies = start_ply_dev;
    a.start_keys = keys_dev;
    std::vector<int32_t> lens(ng), plies(ng, start_ply);
    RCHK(r, hipMemcpyAsync(lens.data(), a.src.game_len, ng * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (start_ply_dev) RCHK(r, hipMemcpyAsync(plies.data(), start_ply_dev, ng * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    RCHK(r, hipStreamSynchronize(st));
    for (size_t g = 0; g < ng; g++) { // rows [start_ply, start_ply + len) must lie inside the game's record rows
        if (plies[g] < 0 || plies[g] > r->max_plies) {
            r->err = std::string(what) + ": start_ply[" + std::to_string(g) + "] = " + std::to_string(plies[g]) +
                     " is outside [0, max_plies = " + std::to_string(r->max_plies) + "]";
            return AZ_E_INVALID;
        }
        if (!game_len_ok(r, what, (int64_t)g, lens[g], r->max_plies, plies[g])) return AZ_E_INVALID;
    }
    if (!keep_dev) return append_common(r, a, lens, st);
    std::vector<int32_t> kept;
    int rc = kept_counts(r, keep_dev, lens, plies, r->max_plies, st, kept);
    if (rc != AZ_OK) return rc;
    a.keep = keep_dev;
    return append_common(r, a, kept, st);
}

extern "C" int az_replay_append_device(az_replay *r, const void *dev_buf, int64_t n_games, int32_t start_ply, void *stream) {
    return append_packed(r, "az_replay_append_device", dev_buf, n_games, start_ply, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int az_replay_append_device_starts(az_replay *r, const void *dev_buf, int64_t n_games, const int32_t *start_ply_dev,
                                              const uint64_t *keys_dev, void *stream) {
    if (r && !start_ply_dev) {
        r->err = "az_replay_append_device_starts: null start_ply_dev";
        return AZ_E_INVALID;
    }
    return append_packed(r, "az_replay_append_device_starts", dev_buf, n_games, 0, start_ply_dev, keys_dev, nullptr, (hipStream_t)stream);
}

extern "C" int az_replay_append_device_kept(az_replay *r, const void *dev_buf, int64_t n_games, int32_t start_ply,
                                            const int32_t *start_ply_dev, const uint64_t *keys_dev, const uint8_t *keep_dev, void *stream) {
    return append_packed(r, "az_replay_append_device_kept", dev_buf, n_games, start_ply, start_ply_dev, keys_dev, keep_dev,
                         (hipStream_t)stream);
}

// A fork: the positions of az_replay_gather_states with the stored history key pair of each example, the three inputs of
// az_engine_set_game_starts_device.  Nothing is overwritten later on (a fork APPENDS), so no epoch is recorded.
__global__ void replay_gather_forks_kernel(const int64_t *indices, long long n, long long n_unique, const int64_t *unique, long long head,
                                           long long cap, const uint64_t *bb0, const uint64_t *bb1, const int32_t *ply, const uint64_t *key,
                                           const uint64_t *key2, uint64_t *bb_out, int32_t *ply_out, uint64_t *keys_out,
                                           unsigned int *faults) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long u = indices[i];
    if (u < 0 || u >= n_unique) { // as az_replay_gather_states: a fault flag, and a state no engine accepts
        atomicOr(faults, AZ_REPLAY_FAULT_BAD_INDEX);
        bb_out[2 * i] = bb_out[2 * i + 1] = 0;
        keys_out[2 * i] = keys_out[2 * i + 1] = 0;
        ply_out[i] = -1;
        return;
    }
    long long phys = (head + unique[u]) % cap;
    bb_out[2 * i] = bb0[phys];
    bb_out[2 * i + 1] = bb1[phys];
    ply_out[i] = ply[phys];
    keys_out[2 * i] = key[phys];
    keys_out[2 * i + 1] = key2[phys];
}

extern "C" int az_replay_gather_forks(az_replay *r, const int64_t *indices, int64_t n, uint64_t *bb_out, int32_t *ply_out,
                                      uint64_t *keys_out, void *stream) {
    if (!r || !indices || !bb_out || !ply_out || !keys_out || n < 1) return AZ_E_INVALID;
    if (r->n_unique < 1) {
        r->err = "az_replay_gather_forks before az_replay_dedupe (or the buffer is empty)";
        return AZ_E_STATE;
    }
    RCHK(r, hipSetDevice(r->cfg.device));
    hipLaunchKernelGGL(replay_gather_forks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indices,
                       (long long)n, (long long)r->n_unique, r->unique, (long long)r->head, (long long)r->cap, r->bb0, r->bb1, r->ply, r->key,
                       r->key2, bb_out, ply_out, keys_out, r->faults);
    RCHK(r, hipGetLastError());
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------ dedupe
__global__ void gather_keys_kernel(const uint64_t *key, long long head, long long cap, long long n, uint64_t *out, long long *idx) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = key[(head + i) % cap];
    idx[i] = i;
}
__global__ void seg_flags_kernel(const uint64_t *skey, long long n, unsigned char *flag) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) flag[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1 : 0;
}
// The position rule (az_replay_dedupe_positions): one thread per stored example writes its canonical triple and its flip bit,
// by logical index.  mirror: the smaller of (bb0, bb1) and its mirror image as unsigned pairs, bb0 the major word; flip = the
// mirror image is strictly smaller (a position that is its own mirror image keeps flip = 0).  GAME is a template argument as in
// replay_sample_sym_kernel: az_mirror_bits differs per game.
template <int GAME>
__global__ void canon_keys_kernel(const uint64_t *bb0, const uint64_t *bb1, const int32_t *ply, long long head, long long cap, long long n,
                                  AzGeom geom, int mirror, uint64_t *c0, uint64_t *c1, uint64_t *par, unsigned char *flip) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long phys = (head + i) % cap;
    AzState s;
    s.bb0 = bb0[phys];
    s.bb1 = bb1[phys];
    s.ply = ply[phys];
    bool f = false;
    if (mirror) {
        const AzState m = az_mirror_state<GAME>(s, geom);
        f = m.bb0 < s.bb0 || (m.bb0 == s.bb0 && m.bb1 < s.bb1);
        if (f) s = m;
    }
    c0[i] = s.bb0;
    c1[i] = s.bb1;
    par[i] = (uint64_t)(s.ply & 1);
    flip[i] = f ? 1 : 0;
}
// the next LSD pass's keys: word[] (by logical index) in the order the passes so far have given
__global__ void gather_word_kernel(const uint64_t *word, const long long *idx, long long n, uint64_t *out) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = word[idx[j]];
}
// a segment starts where any of the three words differs from the previous record's: exact, there is no collision case
__global__ void seg_flags3_kernel(const uint64_t *c0, const uint64_t *c1, const uint64_t *par, const long long *sidx, long long n,
                                  unsigned char *flag) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    bool start = j == 0;
    if (!start) {
        const long long i = sidx[j], p = sidx[j - 1];
        start = c0[i] != c0[p] || c1[i] != c1[p] || par[i] != par[p];
    }
    flag[j] = start ? 1 : 0;
}

struct SegArgs {
    const long long *seg_start, *sidx;
    long long n_seg, n, head, cap;
    int A;
    double *pi, *z;
    unsigned char *first_flag;
    int32_t *count; // [logical index of a first occurrence] the group's members
    // the history rule: the exact-key guard
    const uint64_t *key2, *bb0, *bb1;
    const int32_t *ply;
    unsigned int *faults;
    // the position rule: flip bit by logical index, and the board for az_mirror_action
    const unsigned char *flip;
    AzGeom geom;
};
#define SEG_RULE_HISTORY -1 // (the position rule's RULE is the game, AZG_*)
// One wave per segment: members sidx[seg_start[s] .. seg_start[s+1]) are in buffer order (stable sort).  One body for both rules:
//   RULE == SEG_RULE_HISTORY : every member is checked against the first (the 64-bit key is a hash), action a adds up component a
//   RULE == the game         : nothing to check (the sort key is the position itself), and a member stored in the other
//                              orientation than the first adds its component az_mirror_action(a)
template <int RULE> __global__ void seg_average_kernel(SegArgs g) {
    constexpr int GAME = RULE == SEG_RULE_HISTORY ? AZG_CONNECT_FOUR : RULE; // (names a function the history rule never calls)
    long long s = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (s >= g.n_seg) return;
    const long long head = g.head, cap = g.cap;
    const long long *sidx = g.sidx;
    const int A = g.A;
    double *pi = g.pi, *z = g.z;
    long long j0 = g.seg_start[s], j1 = s + 1 < g.n_seg ? g.seg_start[s + 1] : g.n;
    long long first = sidx[j0];
    long long cnt = j1 - j0;
    if (lane == 0) {
        g.first_flag[first] = 1;
        g.count[first] = (int32_t)cnt;
    }
    if (cnt == 1) return; // x / 1 == x: nothing to write
    long long pf = (head + first) % cap;
    if (RULE == SEG_RULE_HISTORY) { // exact-key guard: every member must be the same history as the first (same fingerprint, ply and position)
        bool bad = false;
        for (long long j = j0 + 1 + lane; j < j1; j += 64) {
            long long pm = (head + sidx[j]) % cap;
            bad |= g.key2[pm] != g.key2[pf] || g.ply[pm] != g.ply[pf] || g.bb0[pm] != g.bb0[pf] || g.bb1[pm] != g.bb1[pf];
        }
        if (__ballot(bad) != 0) { // (wave-uniform) the segment is left untouched: nothing is averaged across different histories
            if (lane == 0) atomicOr(g.faults, AZ_REPLAY_FAULT_KEY_COLLISION);
            return;
        }
    }
    const unsigned char flip_first = RULE == SEG_RULE_HISTORY ? 0 : g.flip[first];
    for (int a = lane; a < A; a += 64) { // flattened_buffer_dict[key][2] = [sum(x) for x in zip(acc, item[2])]
        const int am = RULE == SEG_RULE_HISTORY ? a : az_mirror_action<GAME>(a, g.geom);
        double acc = pi[(size_t)pf * A + a];
        for (long long j = j0 + 1; j < j1; j++) {
            const long long m = sidx[j];
            const int am_j = RULE == SEG_RULE_HISTORY || g.flip[m] == flip_first ? a : am;
            acc = acc + pi[(size_t)((head + m) % cap) * A + am_j];
        }
        pi[(size_t)pf * A + a] = acc / (double)cnt;
    }
    if (lane == 0) { // flattened_buffer_dict[key][3] += item[3]
        double acc = z[pf];
        for (long long j = j0 + 1; j < j1; j++) acc += z[(head + sidx[j]) % cap];
        z[pf] = acc / (double)cnt;
    }
}
__global__ void clear_fault_kernel(unsigned int *faults, unsigned int mask) { atomicAnd(faults, ~mask); }
__global__ void iota_kernel(long long *p, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

// Both dedupe entries.  by_position == false: the reference's rule, grouping by the 64-bit history key (one sort, the exact-key
// guard).  by_position == true: grouping by the canonical triple (three stable LSD passes, no collision case; the
// AZ_REPLAY_FAULT_KEY_COLLISION flag is neither raised nor cleared).  Everything after the grouping is one code path.
static int dedupe_common(az_replay *r, hipStream_t st, bool by_position, int mirror) {
    RCHK(r, hipSetDevice(r->cfg.device));
    long long n = r->n;
    r->n_unique = 0;
    r->epoch++;
    // the collision flag describes THIS pass (an earlier one may have tripped on examples that have since been evicted)
    if (!by_position) hipLaunchKernelGGL(clear_fault_kernel, dim3(1), dim3(1), 0, st, r->faults, AZ_REPLAY_FAULT_KEY_COLLISION);
    if (n == 0) {
        r->count_epoch = r->epoch; // (an empty unique list has its counts: none)
        return AZ_OK;
    }
    uint64_t *k_in = nullptr, *k_out = nullptr, *canon = nullptr; // canon: c0 | c1 | parity, n words each, by logical index
    long long *i_in = nullptr, *i_out = nullptr, *seg_start = nullptr, *iota = nullptr, *d_count = nullptr;
    unsigned char *flag = nullptr, *first_flag = nullptr, *flip = nullptr;
    void *tmp = nullptr;
    auto cleanup = [&]() {
        (void)hipFree(k_in); (void)hipFree(k_out); (void)hipFree(i_in); (void)hipFree(i_out); (void)hipFree(seg_start);
        (void)hipFree(iota); (void)hipFree(d_count); (void)hipFree(flag); (void)hipFree(first_flag); (void)hipFree(tmp);
        (void)hipFree(canon); (void)hipFree(flip);
    };
#define DCHK(call)                                                         \
    do {                                                                   \
        hipError_t _s = (call);                                            \
        if (_s != hipSuccess) {                                            \
            r->err = std::string(#call) + ": " + hipGetErrorString(_s);    \
            cleanup();                                                     \
            return AZ_E_HIP;                                               \
        }                                                                  \
    } while (0)
    DCHK(hipMalloc((void **)&k_in, n * 8)); DCHK(hipMalloc((void **)&k_out, n * 8));
    DCHK(hipMalloc((void **)&i_in, n * 8)); DCHK(hipMalloc((void **)&i_out, n * 8));
    DCHK(hipMalloc((void **)&seg_start, n * 8)); DCHK(hipMalloc((void **)&iota, n * 8));
    DCHK(hipMalloc((void **)&d_count, 8)); DCHK(hipMalloc((void **)&flag, n)); DCHK(hipMalloc((void **)&first_flag, n));
    unsigned nb = (unsigned)((n + 255) / 256);
    size_t tb = 0;
    // (keys, indices) sorted on the keys' bits [0, end_bit): an LSD radix sort, stable.  The scratch buffer grows as asked for.
    auto sort_pairs = [&](const uint64_t *kin, uint64_t *kout, const long long *iin, long long *iout, int end_bit) -> hipError_t {
        size_t need = 0;
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, kin, kout, iin, iout, (int)n, 0, end_bit, st);
        if (e != hipSuccess) return e;
        if (need > tb) {
            (void)hipFree(tmp);
            tmp = nullptr;
            tb = 0;
            if ((e = hipMalloc(&tmp, need)) != hipSuccess) return e;
            tb = need;
        }
        return hipcub::DeviceRadixSort::SortPairs(tmp, need, kin, kout, iin, iout, (int)n, 0, end_bit, st);
    };
    if (!by_position) {
        hipLaunchKernelGGL(gather_keys_kernel, dim3(nb), dim3(256), 0, st, r->key, (long long)r->head, (long long)r->cap, n, k_in, i_in);
        DCHK(sort_pairs(k_in, k_out, i_in, i_out, 64));
        hipLaunchKernelGGL(seg_flags_kernel, dim3(nb), dim3(256), 0, st, k_out, n, flag);
    } else {
        DCHK(hipMalloc((void **)&canon, n * 24));
        DCHK(hipMalloc((void **)&flip, n));
        uint64_t *c0 = canon, *c1 = canon + n, *par = canon + 2 * n;
        if (r->cfg.game == AZG_CONNECT_FOUR)
            hipLaunchKernelGGL(canon_keys_kernel<AZG_CONNECT_FOUR>, dim3(nb), dim3(256), 0, st, r->bb0, r->bb1, r->ply, (long long)r->head,
                               (long long)r->cap, n, r->geom, mirror, c0, c1, par, flip);
        else
            hipLaunchKernelGGL(canon_keys_kernel<AZG_BREAKTHROUGH>, dim3(nb), dim3(256), 0, st, r->bb0, r->bb1, r->ply, (long long)r->head,
                               (long long)r->cap, n, r->geom, mirror, c0, c1, par, flip);
        // three stable passes, the minor word first: parity, then c1, then c0.  Each pass's keys are gathered in the order the
        // passes before it gave; the indices ping-pong between i_in and i_out and end in i_out.
        hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, st, i_in, n);
        DCHK(sort_pairs(par, k_out, i_in, i_out, 1));
        hipLaunchKernelGGL(gather_word_kernel, dim3(nb), dim3(256), 0, st, c1, i_out, n, k_in);
        DCHK(sort_pairs(k_in, k_out, i_out, i_in, 64));
        hipLaunchKernelGGL(gather_word_kernel, dim3(nb), dim3(256), 0, st, c0, i_in, n, k_in);
        DCHK(sort_pairs(k_in, k_out, i_in, i_out, 64));
        hipLaunchKernelGGL(seg_flags3_kernel, dim3(nb), dim3(256), 0, st, c0, c1, par, i_out, n, flag);
    }
    hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, st, iota, n);
    size_t tb2 = 0;
    DCHK(hipcub::DeviceSelect::Flagged(nullptr, tb2, iota, flag, seg_start, d_count, (int)n, st));
    if (tb2 > tb) {
        (void)hipFree(tmp);
        tmp = nullptr;
        DCHK(hipMalloc(&tmp, tb2));
        tb = tb2;
    }
    DCHK(hipcub::DeviceSelect::Flagged(tmp, tb2, iota, flag, seg_start, d_count, (int)n, st)); // segment start positions
    long long n_seg = 0;
    DCHK(hipMemcpyAsync(&n_seg, d_count, 8, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    DCHK(hipMemsetAsync(first_flag, 0, n, st));
    SegArgs sa;
    sa.seg_start = seg_start;
    sa.sidx = i_out;
    sa.n_seg = n_seg;
    sa.n = n;
    sa.head = r->head;
    sa.cap = r->cap;
    sa.A = r->A;
    sa.pi = r->pi;
    sa.z = r->z;
    sa.first_flag = first_flag;
    sa.count = r->count;
    sa.key2 = r->key2;
    sa.bb0 = r->bb0;
    sa.bb1 = r->bb1;
    sa.ply = r->ply;
    sa.faults = r->faults;
    sa.flip = flip;
    sa.geom = r->geom;
    const dim3 seg_grid((unsigned)((n_seg + 3) / 4)), seg_block(256);
    if (!by_position) hipLaunchKernelGGL(seg_average_kernel<SEG_RULE_HISTORY>, seg_grid, seg_block, 0, st, sa);
    else if (r->cfg.game == AZG_CONNECT_FOUR) hipLaunchKernelGGL(seg_average_kernel<AZG_CONNECT_FOUR>, seg_grid, seg_block, 0, st, sa);
    else hipLaunchKernelGGL(seg_average_kernel<AZG_BREAKTHROUGH>, seg_grid, seg_block, 0, st, sa);
    DCHK(hipcub::DeviceSelect::Flagged(nullptr, tb2, iota, first_flag, (long long *)r->unique, d_count, (int)n, st));
    if (tb2 > tb) {
        (void)hipFree(tmp);
        tmp = nullptr;
        DCHK(hipMalloc(&tmp, tb2));
    }
    DCHK(hipcub::DeviceSelect::Flagged(tmp, tb2, iota, first_flag, (long long *)r->unique, d_count, (int)n, st)); // dict order
    long long n_unique = 0;
    unsigned int faults = 0;
    DCHK(hipMemcpyAsync(&n_unique, d_count, 8, hipMemcpyDeviceToHost, st));
    DCHK(hipMemcpyAsync(&faults, r->faults, 4, hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    DCHK(hipGetLastError());
    cleanup();
#undef DCHK
    if (n_unique != n_seg) {
        r->err = "internal: unique count mismatch";
        return AZ_E_DEVICE;
    }
    if (!by_position && (faults & AZ_REPLAY_FAULT_KEY_COLLISION)) {
        r->err = "remove_duplicates: two different histories share a 64-bit key (they would have been averaged); not deduplicated";
        return AZ_E_DEVICE;
    }
    r->n_unique = n_unique;
    r->count_epoch = r->epoch;
    return AZ_OK;
}

extern "C" int az_replay_dedupe(az_replay *r, void *stream) {
    if (!r) return AZ_E_INVALID;
    return dedupe_common(r, (hipStream_t)stream, false, 0);
}

extern "C" int az_replay_dedupe_positions(az_replay *r, int32_t mirror, void *stream) {
    if (!r) return AZ_E_INVALID;
    if (mirror != 0 && mirror != 1) {
        r->err = "az_replay_dedupe_positions: mirror must be 0 or 1, not " + std::to_string(mirror);
        return AZ_E_INVALID;
    }
    return dedupe_common(r, (hipStream_t)stream, true, mirror);
}

__global__ void unique_counts_kernel(const int64_t *unique, const int32_t *count, long long n, int32_t *out) {
    long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) out[u] = count[unique[u]];
}

extern "C" int az_replay_unique_counts_device(az_replay *r, int32_t *counts_out_dev, int64_t n, void *stream) {
    if (!r) return AZ_E_INVALID;
    if (r->count_epoch != r->epoch) {
        r->err = r->count_epoch < 0 ? "az_replay_unique_counts_device before any dedupe"
                                    : "az_replay_unique_counts_device: the store has changed (append or capacity) since the last dedupe, or "
                                      "that dedupe failed";
        return AZ_E_STATE;
    }
    if (n != r->n_unique || (n > 0 && !counts_out_dev)) {
        r->err = "az_replay_unique_counts_device: n = " + std::to_string(n) + " is not n_unique = " + std::to_string(r->n_unique) +
                 " (or counts_out_dev is null)";
        return AZ_E_INVALID;
    }
    if (n == 0) return AZ_OK;
    RCHK(r, hipSetDevice(r->cfg.device));
    hipLaunchKernelGGL(unique_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r->unique, r->count,
                       (long long)n, counts_out_dev);
    RCHK(r, hipGetLastError());
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------ sampling
struct SampleArgs {
    AzGeom geom;
    int game, A, batch, planes_elems;
    long long head, cap, n_unique;
    const int64_t *unique, *indices;
    uint64_t seed, call;
    const uint64_t *bb0, *bb1;
    const int32_t *ply;
    const double *z, *pi;
    float *x, *pio, *zo;
    unsigned int *faults;
};
__global__ void replay_sample_kernel(SampleArgs a) {
    int b = blockIdx.x;
    long long u;
    if (a.indices) u = a.indices[b];
    else { // np.random.randint(len(flattened_buffer)) stand-in: one splitmix draw per row
        uint64_t h = mix64(mix64(a.seed, a.call), (uint64_t)b);
        u = (long long)__umul64hi(h, (uint64_t)a.n_unique);
    }
    if (u < 0 || u >= a.n_unique) { // an index outside the de-duplicated list: poison the row and raise a fault (reported
                                     // by the next az_replay_stats_get) instead of silently substituting example 0
        if (threadIdx.x == 0) {
            atomicOr(a.faults, AZ_REPLAY_FAULT_BAD_INDEX);
            a.zo[b] = __builtin_nanf("");
        }
        for (int i = threadIdx.x; i < a.planes_elems; i += blockDim.x) a.x[(size_t)b * a.planes_elems + i] = __builtin_nanf("");
        for (int i = threadIdx.x; i < a.A; i += blockDim.x) a.pio[(size_t)b * a.A + i] = __builtin_nanf("");
        return;
    }
    long long phys = (a.head + a.unique[u]) % a.cap;
    AzState s;
    s.bb0 = a.bb0[phys];
    s.bb1 = a.bb1[phys];
    s.ply = a.ply[phys];
    for (int i = threadIdx.x; i < a.planes_elems; i += blockDim.x)
        a.x[(size_t)b * a.planes_elems + i] = a.game == AZG_CONNECT_FOUR ? az_obs_elem<AZG_CONNECT_FOUR>(s, a.geom, i)
                                                                         : az_obs_elem<AZG_BREAKTHROUGH>(s, a.geom, i);
    for (int i = threadIdx.x; i < a.A; i += blockDim.x) a.pio[(size_t)b * a.A + i] = (float)a.pi[(size_t)phys * a.A + i];
    if (threadIdx.x == 0) a.zo[b] = (float)a.z[phys];
}

// What both sampling entries hand their kernel; takes the call's number from the store's one counter.
static SampleArgs sample_args(az_replay *r, const int64_t *indices, int32_t batch, uint64_t seed, float *x, float *pi, float *z) {
    SampleArgs a;
    a.geom = r->geom;
    a.game = r->cfg.game;
    a.A = r->A;
    a.batch = batch;
    a.planes_elems = 4 * r->cfg.rows * r->cfg.cols;
    a.head = r->head;
    a.cap = r->cap;
    a.n_unique = r->n_unique;
    a.unique = r->unique;
    a.indices = indices;
    a.seed = seed;
    a.call = r->sample_calls++;
    a.bb0 = r->bb0;
    a.bb1 = r->bb1;
    a.ply = r->ply;
    a.z = r->z;
    a.pi = r->pi;
    a.x = x;
    a.pio = pi;
    a.zo = z;
    a.faults = r->faults;
    return a;
}

extern "C" int az_replay_sample(az_replay *r, const int64_t *indices, int32_t batch, uint64_t seed, float *x, float *pi,
                                float *z, void *stream) {
    if (!r || !x || !pi || !z || batch < 1) return AZ_E_INVALID;
    if (r->n_unique < 1) {
        r->err = "az_replay_sample before az_replay_dedupe (or the buffer is empty)";
        return AZ_E_STATE;
    }
    SampleArgs a = sample_args(r, indices, batch, seed, x, pi, z);
    RCHK(r, hipSetDevice(r->cfg.device));
    hipLaunchKernelGGL(replay_sample_kernel, dim3(batch), dim3(128), 0, (hipStream_t)stream, a);
    RCHK(r, hipGetLastError());
    return AZ_OK;
}

// The same gather with a left-right mirror bit per row (az_mirror_state / az_mirror_action): one workgroup per row, the row's
// example chosen exactly as replay_sample_kernel chooses it.  GAME is a template argument here: the mirror of the position is
// formed once per thread and the action mirror runs per element.
template <int GAME> __global__ void replay_sample_sym_kernel(SampleArgs a, const uint8_t *flips) {
    int b = blockIdx.x;
    const uint64_t h = mix64(mix64(a.seed, a.call), (uint64_t)b); // the row's index word, as in replay_sample_kernel
    long long u = a.indices ? a.indices[b] : (long long)__umul64hi(h, (uint64_t)a.n_unique);
    if (u < 0 || u >= a.n_unique) { // as replay_sample_kernel, whatever the row's flip
        if (threadIdx.x == 0) {
            atomicOr(a.faults, AZ_REPLAY_FAULT_BAD_INDEX);
            a.zo[b] = __builtin_nanf("");
        }
        for (int i = threadIdx.x; i < a.planes_elems; i += blockDim.x) a.x[(size_t)b * a.planes_elems + i] = __builtin_nanf("");
        for (int i = threadIdx.x; i < a.A; i += blockDim.x) a.pio[(size_t)b * a.A + i] = __builtin_nanf("");
        return;
    }
    // the coin is the top bit of a further splitmix step over the index word: no bit of the word that picks the example decides it
    const bool flip = flips ? flips[b] != 0 : (mix64(h, 0x6A09E667F3BCC908ull) >> 63) != 0; // (block-uniform)
    long long phys = (a.head + a.unique[u]) % a.cap;
    AzState s;
    s.bb0 = a.bb0[phys];
    s.bb1 = a.bb1[phys];
    s.ply = a.ply[phys];
    if (flip) s = az_mirror_state<GAME>(s, a.geom);
    for (int i = threadIdx.x; i < a.planes_elems; i += blockDim.x) a.x[(size_t)b * a.planes_elems + i] = az_obs_elem<GAME>(s, a.geom, i);
    // pi_out[mirror(i)] = pi[i], written as pi_out[i] = pi[mirror(i)] (an involution): the stores stay in order
    for (int i = threadIdx.x; i < a.A; i += blockDim.x)
        a.pio[(size_t)b * a.A + i] = (float)a.pi[(size_t)phys * a.A + (flip ? az_mirror_action<GAME>(i, a.geom) : i)];
    if (threadIdx.x == 0) a.zo[b] = (float)a.z[phys];
}

extern "C" int az_replay_sample_sym(az_replay *r, const int64_t *indices, const uint8_t *flips, int32_t batch, uint64_t seed, float *x,
                                    float *pi, float *z, void *stream) {
    if (!r || !x || !pi || !z || batch < 1) return AZ_E_INVALID;
    if (r->n_unique < 1) {
        r->err = "az_replay_sample_sym before az_replay_dedupe (or the buffer is empty)";
        return AZ_E_STATE;
    }
    SampleArgs a = sample_args(r, indices, batch, seed, x, pi, z);
    RCHK(r, hipSetDevice(r->cfg.device));
    if (a.game == AZG_CONNECT_FOUR)
        hipLaunchKernelGGL(replay_sample_sym_kernel<AZG_CONNECT_FOUR>, dim3(batch), dim3(128), 0, (hipStream_t)stream, a, flips);
    else
        hipLaunchKernelGGL(replay_sample_sym_kernel<AZG_BREAKTHROUGH>, dim3(batch), dim3(128), 0, (hipStream_t)stream, a, flips);
    RCHK(r, hipGetLastError());
    return AZ_OK;
}

// ------------------------------------------------------------------------------------------------ reanalyse
// Stored positions -> a search (az_engine_set_start_states_device) -> refreshed targets, device to device.
__global__ void replay_gather_states_kernel(const int64_t *indices, long long n, long long n_unique, const int64_t *unique, long long head,
                                            long long cap, const uint64_t *bb0, const uint64_t *bb1, const int32_t *ply, uint64_t *bb_out,
                                            int32_t *ply_out, unsigned int *faults) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long u = indices[i];
    if (u < 0 || u >= n_unique) { // as az_replay_sample: a fault flag, and a state no search accepts
        atomicOr(faults, AZ_REPLAY_FAULT_BAD_INDEX);
        bb_out[2 * i] = bb_out[2 * i + 1] = 0;
        ply_out[i] = -1;
        return;
    }
    long long phys = (head + unique[u]) % cap;
    bb_out[2 * i] = bb0[phys];
    bb_out[2 * i + 1] = bb1[phys];
    ply_out[i] = ply[phys];
}

extern "C" int az_replay_gather_states(az_replay *r, const int64_t *indices, int64_t n, uint64_t *bb_out, int32_t *ply_out, void *stream) {
    if (!r || !indices || !bb_out || !ply_out || n < 1) return AZ_E_INVALID;
    if (r->n_unique < 1) {
        r->err = "az_replay_gather_states before az_replay_dedupe (or the buffer is empty)";
        return AZ_E_STATE;
    }
    RCHK(r, hipSetDevice(r->cfg.device));
    hipLaunchKernelGGL(replay_gather_states_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, indices,
                       (long long)n, (long long)r->n_unique, r->unique, (long long)r->head, (long long)r->cap, r->bb0, r->bb1, r->ply, bb_out,
                       ply_out, r->faults);
    RCHK(r, hipGetLastError());
    r->gather_epoch = r->epoch;
    return AZ_OK;
}

#define REFRESH_FREE 0xFFFFFFFFu
struct RefreshArgs {
    RootsOut roots; // (read only here)
    LinesOut lines; // (read only; AZ_REFRESH_OFF_POLICY alone looks at it)
    int G, mc, A, value_mode;
    long long n, n_unique, head, cap;
    const int64_t *indices, *unique;
    PwPlan pw;
    const int32_t *ply;
    double *z, *pi;
    unsigned int *claim, *faults;
    long long *sel;
    unsigned long long *refreshed;
};
// One thread per slot of the root export, three passes on one stream.  claim: which example the slot refreshes (sel[g], -1 =
// none: not a finished search of this call, a bad index, another ply, a child that is no action of the game), and the lowest
// such slot per example wins it, so duplicate indices store ONE of their results whole.
__global__ void replay_refresh_claim_kernel(RefreshArgs a) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    a.sel[g] = -1;
    int gid = a.roots.game_id[g];
    if (a.roots.phase[g] != PH_SEARCH_DONE || gid < 0 || gid >= a.n) return;
    long long u = a.indices[gid];
    if (u < 0 || u >= a.n_unique) {
        atomicOr(a.faults, AZ_REPLAY_FAULT_BAD_INDEX);
        return;
    }
    long long phys = (a.head + a.unique[u]) % a.cap;
    int nc = a.roots.n_children[g];
    bool ok = a.roots.ply[g] == a.ply[phys] && nc >= 0 && nc <= a.mc;
    if (a.value_mode == AZ_REFRESH_OFF_POLICY) // the line must be of the search the root is of, and a whole one
        ok = ok && a.lines.game_id[g] == gid && a.lines.ply[g] == a.roots.ply[g] && a.lines.phase[g] == PH_SEARCH_DONE && a.lines.depth[g] >= 0;
    for (int k = 0; ok && k < nc; k++) {
        int act = a.roots.child_action[(size_t)g * a.mc + k];
        ok = act >= 0 && act < a.A;
    }
    if (!ok) {
        atomicOr(a.faults, AZ_REPLAY_FAULT_ROOT_MISMATCH);
        return;
    }
    a.sel[g] = phys;
    atomicMin(a.claim + phys, (unsigned int)g);
}
__global__ void replay_refresh_write_kernel(RefreshArgs a) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.G) return;
    long long phys = a.sel[g];
    if (phys < 0 || a.claim[phys] != (unsigned int)g) return;
    const size_t row = (size_t)g * a.mc;
    int nc = a.roots.n_children[g];
    pi_from_root_visits(a.pw, a.A, nc, a.roots.child_n + row, a.roots.child_action + row, a.pi + (size_t)phys * a.A);
    if (a.value_mode == AZ_REFRESH_SOFT_Z) { // game_utils.py:172-174
        a.z[phys] = -a.roots.root_q[g];
    } else if (a.value_mode == AZ_REFRESH_A0C) { // game_utils.py:177-179; a root without children keeps its z
        double best = 0.0;
        for (int k = 0; k < nc; k++) {
            double v = a.roots.child_n[row + k] > 0 ? a.roots.child_q[row + k] : -99.0;
            if (k == 0 || v > best) best = v;
        }
        if (nc > 0) a.z[phys] = best;
    } else if (a.value_mode == AZ_REFRESH_OFF_POLICY) { // game_utils.py:182-194, walked by az_engine_export_lines_device
        a.z[phys] = a.lines.value[g];
    }
    atomicAdd(a.refreshed, 1ull);
}
__global__ void replay_refresh_release_kernel(RefreshArgs a) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.G && a.sel[g] >= 0) a.claim[a.sel[g]] = REFRESH_FREE;
}

// Both refresh entries: `what` names the entry in the error texts; lines is read in AZ_REFRESH_OFF_POLICY only.
static int64_t refresh_from_search(az_replay *r, const std::string &what, const int64_t *indices, int64_t n, const void *roots,
                                   int64_t roots_bytes, const void *lines, int64_t lines_bytes, int32_t value_mode, hipStream_t st) {
    const bool off_policy = value_mode == AZ_REFRESH_OFF_POLICY;
    if (roots_bytes < 16) {
        r->err = what + ": roots_bytes does not hold the header";
        return AZ_E_INVALID;
    }
    if (off_policy && lines_bytes < 16) {
        r->err = what + ": lines_bytes does not hold the header";
        return AZ_E_INVALID;
    }
    if (r->n_unique < 1 || r->gather_epoch != r->epoch) {
        r->err = what + ": the store has changed (append, dedupe or capacity) since az_replay_gather_states - the "
                 "indices may name other records";
        return AZ_E_STATE;
    }
    RCHK(r, hipSetDevice(r->cfg.device));
    int32_t hdr[4] = {0, 0, 0, 0}, lhdr[4] = {0, 0, 0, 0};
    RCHK(r, hipMemcpyAsync(hdr, roots, 16, hipMemcpyDeviceToHost, st));
    if (off_policy) RCHK(r, hipMemcpyAsync(lhdr, lines, 16, hipMemcpyDeviceToHost, st));
    RCHK(r, hipStreamSynchronize(st));
    size_t off[AZ_ROOTS_ARRAYS + 1];
    if (hdr[1] >= 1 && hdr[2] == r->maxc) roots_offsets((size_t)hdr[1], (size_t)hdr[2], off);
    if (hdr[1] < 1 || hdr[2] != r->maxc || (int64_t)off[AZ_ROOTS_ARRAYS] > roots_bytes) {
        r->err = what + ": the header says " + std::to_string(hdr[1]) + " slots x " + std::to_string(hdr[2]) +
                 " children: not a root export of this game that fits roots_bytes = " + std::to_string(roots_bytes);
        return AZ_E_INVALID;
    }
    const int G = hdr[1];
    if (off_policy) {
        size_t loff[AZ_LINES_ARRAYS + 1];
        const bool shape = lhdr[1] == G && lhdr[2] >= 1 && lhdr[2] <= r->max_plies;
        if (shape) lines_offsets((size_t)lhdr[1], (size_t)lhdr[2], loff);
        if (!shape || (int64_t)loff[AZ_LINES_ARRAYS] > lines_bytes) {
            r->err = what + ": the lines header says " + std::to_string(lhdr[1]) + " slots x depth " + std::to_string(lhdr[2]) +
                     ": not a line export of the " + std::to_string(G) + " slots of the roots that fits lines_bytes = " +
                     std::to_string(lines_bytes);
            return AZ_E_INVALID;
        }
    }
    if (hdr[3] != 0 || lhdr[3] != 0) {
        r->err = what + ": the export carries engine fault flags " + std::to_string((uint32_t)(hdr[3] | lhdr[3]));
        return AZ_E_DEVICE;
    }
    if (G > r->sel_cap) {
        (void)hipFree(r->sel);
        r->sel = nullptr;
        r->sel_cap = 0;
        RCHK(r, hipMalloc((void **)&r->sel, (size_t)G * sizeof(long long)));
        r->sel_cap = G;
    }
    RefreshArgs a;
    a.roots = roots_arrays(const_cast<void *>(roots), (size_t)G, (size_t)r->maxc);
    a.lines = LinesOut();
    if (off_policy) a.lines = lines_arrays(const_cast<void *>(lines), (size_t)G, (size_t)lhdr[2]);
    a.G = G;
    a.mc = r->maxc;
    a.A = r->A;
    a.value_mode = value_mode;
    a.n = n;
    a.n_unique = r->n_unique;
    a.head = r->head;
    a.cap = r->cap;
    a.indices = indices;
    a.unique = r->unique;
    a.pw = r->pw;
    a.ply = r->ply;
    a.z = r->z;
    a.pi = r->pi;
    a.claim = r->claim;
    a.faults = r->faults;
    a.sel = r->sel;
    a.refreshed = r->refreshed;
    RCHK(r, hipMemsetAsync(r->refreshed, 0, 8, st));
    const dim3 grid((unsigned)((G + 255) / 256)), block(256);
    hipLaunchKernelGGL(replay_refresh_claim_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(replay_refresh_write_kernel, grid, block, 0, st, a);
    hipLaunchKernelGGL(replay_refresh_release_kernel, grid, block, 0, st, a);
    RCHK(r, hipGetLastError());
    unsigned long long count = 0;
    RCHK(r, hipMemcpyAsync(&count, r->refreshed, 8, hipMemcpyDeviceToHost, st));
    RCHK(r, hipStreamSynchronize(st));
    return (int64_t)count;
}

extern "C" int64_t az_replay_refresh_from_roots(az_replay *r, const int64_t *indices, int64_t n, const void *roots, int64_t roots_bytes,
                                                int32_t value_mode, void *stream) {
    if (!r) return AZ_E_INVALID;
    if (!indices || !roots || n < 1 || ((uintptr_t)roots & 15) != 0 ||
        (value_mode != AZ_REFRESH_KEEP_Z && value_mode != AZ_REFRESH_SOFT_Z && value_mode != AZ_REFRESH_A0C)) {
        r->err = "az_replay_refresh_from_roots: null / unaligned argument, n < 1 or a value_mode that is no function of a root";
        return AZ_E_INVALID;
    }
    return refresh_from_search(r, "az_replay_refresh_from_roots", indices, n, roots, roots_bytes, nullptr, 0, value_mode, (hipStream_t)stream);
}

extern "C" int64_t az_replay_refresh_from_search(az_replay *r, const int64_t *indices, int64_t n, const void *roots, int64_t roots_bytes,
                                                 const void *lines, int64_t lines_bytes, int32_t value_mode, void *stream) {
    if (!r) return AZ_E_INVALID;
    if (!indices || !roots || n < 1 || ((uintptr_t)roots & 15) != 0 || ((uintptr_t)lines & 15) != 0 || value_mode < AZ_REFRESH_KEEP_Z ||
        value_mode > AZ_REFRESH_OFF_POLICY) {
        r->err = "az_replay_refresh_from_search: null / unaligned argument, n < 1 or an unknown value_mode";
        return AZ_E_INVALID;
    }
    if (value_mode == AZ_REFRESH_OFF_POLICY && !lines) {
        r->err = "az_replay_refresh_from_search: AZ_REFRESH_OFF_POLICY needs the line export (lines is NULL)";
        return AZ_E_INVALID;
    }
    return refresh_from_search(r, "az_replay_refresh_from_search", indices, n, roots, roots_bytes, lines, lines_bytes, value_mode,
                               (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ read-back
extern "C" int64_t az_replay_read_unique(az_replay *r, int64_t max_n, uint64_t *key, double *pi, double *z, int64_t *buffer_index,
                                         uint64_t *bitboards, int32_t *ply) {
    if (!r || max_n < 0) return AZ_E_INVALID;
    RCHK(r, hipSetDevice(r->cfg.device));
    RCHK(r, hipDeviceSynchronize());
    int64_t n = r->n_unique < max_n ? r->n_unique : max_n;
    std::vector<int64_t> u((size_t)n);
    if (n) RCHK(r, hipMemcpy(u.data(), r->unique, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) {
        int64_t phys = (r->head + u[(size_t)i]) % r->cap;
        if (buffer_index) buffer_index[i] = u[(size_t)i];
        if (key) RCHK(r, hipMemcpy(key + i, r->key + phys, 8, hipMemcpyDeviceToHost));
        if (z) RCHK(r, hipMemcpy(z + i, r->z + phys, 8, hipMemcpyDeviceToHost));
        if (pi) RCHK(r, hipMemcpy(pi + i * r->A, r->pi + (size_t)phys * r->A, 8 * (size_t)r->A, hipMemcpyDeviceToHost));
        if (bitboards) {
            RCHK(r, hipMemcpy(bitboards + 2 * i, r->bb0 + phys, 8, hipMemcpyDeviceToHost));
            RCHK(r, hipMemcpy(bitboards + 2 * i + 1, r->bb1 + phys, 8, hipMemcpyDeviceToHost));
        }
        if (ply) RCHK(r, hipMemcpy(ply + i, r->ply + phys, 4, hipMemcpyDeviceToHost));
    }
    return r->n_unique;
}

extern "C" int az_replay_debug_set_key(az_replay *r, int64_t index, uint64_t key) {
    if (!r || index < 0 || index >= r->n) return AZ_E_INVALID;
    RCHK(r, hipSetDevice(r->cfg.device));
    RCHK(r, hipDeviceSynchronize());
    RCHK(r, hipMemcpy(r->key + (r->head + index) % r->cap, &key, 8, hipMemcpyHostToDevice));
    return AZ_OK;
}

extern "C" int az_replay_read_example(az_replay *r, int64_t index, double *pi, double *z) {
    if (!r || index < 0 || index >= r->n) return AZ_E_INVALID;
    RCHK(r, hipSetDevice(r->cfg.device));
    RCHK(r, hipDeviceSynchronize());
    int64_t phys = (r->head + index) % r->cap;
    if (pi) RCHK(r, hipMemcpy(pi, r->pi + (size_t)phys * r->A, 8 * (size_t)r->A, hipMemcpyDeviceToHost));
    if (z) RCHK(r, hipMemcpy(z, r->z + phys, 8, hipMemcpyDeviceToHost));
    return AZ_OK;
}
