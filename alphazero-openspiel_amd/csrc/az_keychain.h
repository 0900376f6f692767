// az_keychain.h — the replay store's two history-key chains, ONE copy for host and device.
//
// The reference keys an example on its exact information-state string (train.py:177).  The store keys it on a pair of 64-bit
// chains over the same history: `key` groups the examples (az_replay_dedupe sorts on it), `key2` is an independent second
// hash that the segment pass compares (AZ_REPLAY_FAULT_KEY_COLLISION).  A chain is seeded from a start state and stepped once
// per move; the second chain's step also takes a step index.
//   an ordinary game (no table)      seed(start ply, start state), step index of the game's j-th move = j        (j = 1, 2, ...)
//   a game with a GIVEN pair         the pair, step index of the j-th move = start ply + j = the absolute ply after the move
// so a game that was given the pair of the history P and then plays m_1..m_k carries, at m_1..m_j, exactly the pair of an
// ordinary game from the initial position whose history is P + m_1..m_j (include/az_replay.h, "the key rule").
// Used by replay_keys_kernel (csrc/az_replay.hip) and by the host replay of az_engine_set_game_starts (csrc/az_starts.h).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AZ_KEY_HD __host__ __device__ __forceinline__
#else
#define AZ_KEY_HD inline
#endif

struct AzKeyPair {
    uint64_t key, key2;
};

AZ_KEY_HD uint64_t az_key_mix64(uint64_t h, uint64_t v) { // splitmix64 step over (h, v)
    uint64_t z = h + 0x9E3779B97F4A7C15ull * (v + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The pair of a game's first example: a game that starts at `ply` in the position (bb0, bb1).
AZ_KEY_HD AzKeyPair az_key_seed(int ply, uint64_t bb0, uint64_t bb1) {
    AzKeyPair k;
    k.key = az_key_mix64(0x243F6A8885A308D3ull, (uint64_t)ply);
    k.key = az_key_mix64(k.key, bb0);
    k.key = az_key_mix64(k.key, bb1);
    k.key2 = az_key_mix64(0x13198A2E03707344ull ^ (uint64_t)ply, bb0 + 0x9E3779B97F4A7C15ull * bb1); // other seed, other per-step tweak
    return k;
}

// The pair after one more move; step_index: see the head of this file.
AZ_KEY_HD AzKeyPair az_key_step(AzKeyPair k, uint32_t move, int step_index) {
    k.key = az_key_mix64(k.key, (uint64_t)move);
    k.key2 = az_key_mix64(k.key2 ^ 0xA4093822299F31D0ull, ((uint64_t)move << 20) | (uint64_t)step_index);
    return k;
}
