"""The one Python Philox of the suite: Philox4x32-10 and the draws the engine makes with it (include/az_engine.h) - the uniform of
the stream (seed, game id, ply, purpose, index) and the playout cap's schedule (az_engine_set_playout_cap: purpose 3, index 0; the
move is a full search iff u < p_full).  tests/test_playout_cap_host.py checks it against the published vectors.  No test lives
here."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011): counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def cap_uniform(seed, game_id, ply, purpose=3, idx=0):
    """philox_init(seed, game id, ply, purpose, idx) followed by the first philox_u01: key = the seed's two halves, counter =
    (0, idx, ply << 8 | purpose, game id); the first uniform is made of output words 2 (high) and 3 (low), 53 bits."""
    out = philox4x32_10((0, idx & M32, ((ply << 8) | purpose) & M32, game_id & M32), (seed & M32, (seed >> 32) & M32))
    return float(((out[2] << 32) | out[3]) >> 11) * (1.0 / 9007199254740992.0)


def is_full(seed, game_id, ply, p_full):
    return cap_uniform(seed, game_id, ply) < p_full


def schedule(seed, n_games, max_plies, p_full):
    """uint8 [n_games, max_plies]: 1 where the search of game i at absolute ply t is a full one."""
    return np.array([[is_full(seed, i, t, p_full) for t in range(max_plies)] for i in range(n_games)], dtype=np.uint8)
