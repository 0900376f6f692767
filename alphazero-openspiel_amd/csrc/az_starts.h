// az_starts.h — the host replay of an action prefix: the position a game starts from and the history key pair it carries.
//
// Plain C++ (no HIP): csrc/az_starts.hip calls it for az_engine_set_start_prefix, az_engine_set_start_positions and
// az_engine_set_game_starts, and tests/test_game_starts_host.py compiles it with g++ against the Python rules (games.py).
#pragma once
#include <stdint.h>

#include "az_games.h"
#include "az_keychain.h"

enum { AZ_PREFIX_OK = 0, AZ_PREFIX_ILLEGAL = 1 /* an illegal action */, AZ_PREFIX_ENDS_GAME = 2 /* a move of the prefix ends the game */ };

template <int GAME> static inline AzState az_initial_state(const AzGeom &g) {
    AzState s;
    az_init_state<GAME>(s, g);
    return s;
}
static inline AzState az_initial_state(int game, const AzGeom &g) {
    return game == AZG_CONNECT_FOUR ? az_initial_state<AZG_CONNECT_FOUR>(g) : az_initial_state<AZG_BREAKTHROUGH>(g);
}

// Plays actions[0..n) from the initial position with the legality check of the game.  On AZ_PREFIX_OK, s is the position and k
// the pair of an ordinary game from the initial position after these moves (az_keychain.h: the j-th move steps with index j).
template <int GAME> static inline int az_replay_prefix(const AzGeom &g, int A, const int32_t *actions, int32_t n, AzState &s, AzKeyPair &k) {
    s = az_initial_state<GAME>(g);
    k = az_key_seed(s.ply, s.bb0, s.bb1);
    float ret0 = 0.f;
    for (int32_t j = 0; j < n; j++) {
        if (!az_action_legal<GAME>(s, g, A, actions[j])) return AZ_PREFIX_ILLEGAL;
        if (az_apply<GAME>(s, g, actions[j], &ret0)) return AZ_PREFIX_ENDS_GAME;
        k = az_key_step(k, (uint32_t)actions[j], j + 1);
    }
    return AZ_PREFIX_OK;
}
static inline int az_replay_prefix(int game, const AzGeom &g, int A, const int32_t *actions, int32_t n, AzState &s, AzKeyPair &k) {
    return game == AZG_CONNECT_FOUR ? az_replay_prefix<AZG_CONNECT_FOUR>(g, A, actions, n, s, k)
                                    : az_replay_prefix<AZG_BREAKTHROUGH>(g, A, actions, n, s, k);
}
