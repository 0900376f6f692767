// az_games.h — bitboard game dynamics for connect_four and breakthrough(R×C), host+device.
//
// Replaces, for the engine, the OpenSpiel (pyspiel) state API the reference's hot path calls
// (mcts.py:138-149,178,184; alphazerobot.py:55,72; game_utils.py:150-153,156,169,197,201;
// network.py:15-17): apply_action / legal_actions / is_terminal / returns / current_player and
// the observation tensor.  OpenSpiel is absent from the reference tree (third-party, unpinned);
// rules follow the public game definitions, plane order and action codec follow the pins the
// shipped checkpoints give.
//
// Bit layouts
//   connect_four : bit = col*7 + row, row 0 = bottom, bit 6 of every column is a zero sentinel.
//                  bb[0] = player-0 ('x') stones, bb[1] = player-1 ('o') stones.
//   breakthrough : bit = row*C + col, bb[0] = black (player 0, home rows 0..1, moves to higher
//                  rows), bb[1] = white (player 1).  R*C <= 64.
// Player to move = ply & 1 in both games (strict alternation, no passes).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AZ_HD __host__ __device__ __forceinline__
#else
#define AZ_HD inline
#endif

#define AZG_CONNECT_FOUR 0
#define AZG_BREAKTHROUGH 1

struct AzState {
    uint64_t bb0, bb1;
    int ply;
};

struct AzGeom { // wave-uniform constants of the board
    int rows, cols, cells;
    uint64_t board_mask; // breakthrough: all cells
    uint64_t not_col0, not_col_last;
    uint64_t row_last, row_first; // breakthrough goal rows for black / white
};

AZ_HD int az_popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

static inline AzGeom az_make_geom(int game, int rows, int cols) {
    AzGeom g;
    g.rows = rows;
    g.cols = cols;
    g.cells = rows * cols;
    g.board_mask = g.cells >= 64 ? ~0ull : ((1ull << g.cells) - 1);
    g.not_col0 = g.not_col_last = g.row_last = g.row_first = 0;
    if (game == AZG_BREAKTHROUGH)
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++) {
                uint64_t b = 1ull << (r * cols + c);
                if (c > 0) g.not_col0 |= b;
                if (c < cols - 1) g.not_col_last |= b;
                if (r == rows - 1) g.row_last |= b;
                if (r == 0) g.row_first |= b;
            }
    return g;
}

template <int GAME> AZ_HD void az_init_state(AzState &s, const AzGeom &g) {
    s.ply = 0;
    if (GAME == AZG_CONNECT_FOUR) {
        s.bb0 = s.bb1 = 0;
    } else {
        uint64_t two_rows = (g.cols * 2 >= 64) ? ~0ull : ((1ull << (2 * g.cols)) - 1);
        s.bb0 = two_rows;
        s.bb1 = two_rows << ((g.rows - 2) * g.cols);
    }
}

// ---------------------------------------------------------------- connect_four
AZ_HD bool az_c4_has_four(uint64_t b) {
    uint64_t m = b & (b >> 7);
    if (m & (m >> 14)) return true; // horizontal
    m = b & (b >> 6);
    if (m & (m >> 12)) return true; // diagonal
    m = b & (b >> 8);
    if (m & (m >> 16)) return true; // anti-diagonal
    m = b & (b >> 1);
    return (m & (m >> 2)) != 0; // vertical
}

// 7-bit mask of playable columns (ascending column = ascending action)
AZ_HD uint32_t az_c4_legal_mask(const AzState &s) {
    uint64_t occ = s.bb0 | s.bb1;
    uint32_t m = 0;
#if defined(__clang__) // (hipcc; the host tests' g++ -Wall -Werror builds know no such pragma)
#pragma unroll
#endif
    for (int c = 0; c < 7; c++) m |= (uint32_t)(((occ >> (c * 7 + 5)) & 1ull) ^ 1ull) << c;
    return m;
}

// ---------------------------------------------------------------- breakthrough
// action = ((cell*6) + dir)*2 + capture; dir 0..2 black (+1 row; dc=-1,0,+1), 3..5 white (-1 row)
// Per-cell legality of the 3 forward moves of the side to move; bit d of the result = dir (d0+d) legal,
// bit (4+d) = that move is a capture.
AZ_HD uint32_t az_bt_cell_moves(const AzState &s, const AzGeom &g, int cell) {
    int me = s.ply & 1;
    uint64_t own = me ? s.bb1 : s.bb0, opp = me ? s.bb0 : s.bb1;
    uint64_t bit = 1ull << cell;
    if (!(own & bit)) return 0;
    uint32_t out = 0;
    int fwd = me ? -g.cols : g.cols;
    bool row_ok = me ? (cell >= g.cols) : (cell + g.cols < g.cells);
    if (!row_ok) return 0;
    // dc = -1
    if (g.not_col0 & bit) {
        uint64_t t = 1ull << (cell + fwd - 1);
        if (!(own & t)) out |= 1u | ((opp & t) ? 16u : 0u);
    }
    { // dc = 0: only onto an empty cell
        uint64_t t = 1ull << (cell + fwd);
        if (!((own | opp) & t)) out |= 2u;
    }
    if (g.not_col_last & bit) {
        uint64_t t = 1ull << (cell + fwd + 1);
        if (!(own & t)) out |= 4u | ((opp & t) ? 64u : 0u);
    }
    return out;
}

AZ_HD int az_bt_encode(int cell, int me, int d, int capture) { return ((cell * 6 + (me ? 3 : 0) + d) << 1) | capture; }

// ---------------------------------------------------------------- common
// Is `action` - any int, A = az_num_actions - a legal move of the side to move?  az_apply assumes it is.
//   connect_four : a column that is not full
//   breakthrough : the cell holds a piece of the side to move, the direction is one of that side's three, the move is on the
//                  board and not blocked, and the capture bit says what the move does
template <int GAME> AZ_HD bool az_action_legal(const AzState &s, const AzGeom &g, int A, int action) {
    if (action < 0 || action >= A) return false;
    if (GAME == AZG_CONNECT_FOUR) return ((az_c4_legal_mask(s) >> action) & 1u) != 0;
    const int cell = (action >> 1) / 6, d = (action >> 1) % 6 - ((s.ply & 1) ? 3 : 0);
    if (d < 0 || d > 2) return false;
    const uint32_t mv = az_bt_cell_moves(s, g, cell);
    return (mv & (1u << d)) && (int)((mv >> (4 + d)) & 1u) == (action & 1);
}


// Applies `action` for the side to move.  Returns 0 = game continues, 1 = terminal; *ret0 = returns()[0].
template <int GAME> AZ_HD int az_apply(AzState &s, const AzGeom &g, int action, float *ret0) {
    int me = s.ply & 1;
    if (GAME == AZG_CONNECT_FOUR) {
        uint64_t occ = s.bb0 | s.bb1;
        uint64_t nb = (occ | (occ + (1ull << (action * 7)))) ^ occ;
        uint64_t mine = (me ? s.bb1 : s.bb0) | nb;
        if (me) s.bb1 = mine; else s.bb0 = mine;
        s.ply++;
        if (az_c4_has_four(mine)) {
            *ret0 = me ? -1.f : 1.f;
            return 1;
        }
        if (s.ply == 42) {
            *ret0 = 0.f;
            return 1;
        }
        return 0;
    } else {
        int d = (action >> 1) % 6, cell = (action >> 1) / 6;
        int dc = (d % 3) - 1;
        int t = cell + (me ? -g.cols : g.cols) + dc;
        uint64_t from = 1ull << cell, to = 1ull << t;
        uint64_t own = me ? s.bb1 : s.bb0, opp = me ? s.bb0 : s.bb1;
        own = (own ^ from) | to;
        opp &= ~to;
        if (me) { s.bb1 = own; s.bb0 = opp; } else { s.bb0 = own; s.bb1 = opp; }
        s.ply++;
        if ((to & (me ? g.row_first : g.row_last)) || opp == 0) {
            *ret0 = me ? -1.f : 1.f;
            return 1;
        }
        return 0;
    }
}

// Scalar (one thread = one state) legal-action helpers, ascending action order = OpenSpiel's legal_actions() order.
// Used by the arena's opponent bots (random rollouts), where a thread owns a whole game.
template <int GAME> AZ_HD int az_count_legal(const AzState &s, const AzGeom &g) {
    if (GAME == AZG_CONNECT_FOUR) return az_popc64((uint64_t)az_c4_legal_mask(s));
    int me = s.ply & 1, n = 0;
    uint64_t own = me ? s.bb1 : s.bb0;
    while (own) {
        int cell = az_popc64((own & (0 - own)) - 1);
        own &= own - 1;
        n += az_popc64((uint64_t)(az_bt_cell_moves(s, g, cell) & 7u));
    }
    return n;
}
// the n-th (0-based) legal action in ascending order; n must be < az_count_legal
template <int GAME> AZ_HD int az_nth_legal(const AzState &s, const AzGeom &g, int n) {
    if (GAME == AZG_CONNECT_FOUR) {
        uint32_t m = az_c4_legal_mask(s);
        for (int c = 0; c < 7; c++)
            if ((m >> c) & 1u) {
                if (n == 0) return c;
                n--;
            }
        return -1;
    }
    int me = s.ply & 1;
    uint64_t own = me ? s.bb1 : s.bb0;
    while (own) {
        int cell = az_popc64((own & (0 - own)) - 1);
        own &= own - 1;
        uint32_t mv = az_bt_cell_moves(s, g, cell);
        for (int d = 0; d < 3; d++)
            if (mv & (1u << d)) {
                if (n == 0) return az_bt_encode(cell, me, d, (mv >> (4 + d)) & 1u);
                n--;
            }
    }
    return -1;
}

// Can a search start from (bb0, bb1, ply)?  0 = yes; otherwise the first rule, in this order, that the state breaks.  The
// dynamics above assume every one of them (the sentinel bits of az_c4_has_four, shifts that stay on the board, a side to move
// that can move), so a state that did not come from az_apply is checked with this before it reaches a search.
enum {
    AZ_STATE_OK = 0,
    AZ_STATE_BAD_PLY,    // ply outside [0, max_plies)
    AZ_STATE_OVERLAP,    // a cell held by both sides
    AZ_STATE_OFF_BOARD,  // a bit that is no cell
    AZ_STATE_SENTINEL,   // connect_four: bit 6 of a column
    AZ_STATE_FLOATING,   // connect_four: a stone above an empty cell
    AZ_STATE_COUNT,      // connect_four: stone counts that do not follow from ply
    AZ_STATE_EMPTY_SIDE, // breakthrough: a side without a piece
    AZ_STATE_GOAL_ROW,   // breakthrough: a piece on the row that wins the game for its side
    AZ_STATE_TERMINAL,   // the game is over
    AZ_STATE_NO_MOVE,    // the side to move has no legal move
    AZ_STATE_N_RULES
};
static inline const char *az_state_rule_name(int rule) {
    static const char *const names[AZ_STATE_N_RULES] = {
        "ok", "ply outside [0, max_plies)", "a cell held by both sides", "a bit outside the board", "a sentinel bit (bit 6 of a column) is set",
        "a stone above an empty cell", "stone counts do not match ply", "a side has no piece", "a piece on its goal row",
        "the position is terminal", "the side to move has no legal move"};
    return rule >= 0 && rule < AZ_STATE_N_RULES ? names[rule] : "?";
}
template <int GAME> AZ_HD int az_check_state(const AzState &s, const AzGeom &g, int max_plies) {
    if (s.ply < 0 || s.ply >= max_plies) return AZ_STATE_BAD_PLY;
    if (s.bb0 & s.bb1) return AZ_STATE_OVERLAP;
    const uint64_t occ = s.bb0 | s.bb1;
    if (GAME == AZG_CONNECT_FOUR) {
        const uint64_t bottom = 0x0000040810204081ull; // row 0 of the 7 columns (bits 0, 7, ..., 42)
        if (occ >> 49) return AZ_STATE_OFF_BOARD;
        if (occ & (bottom << 6)) return AZ_STATE_SENTINEL;
        if (occ & ~bottom & ~(occ << 1)) return AZ_STATE_FLOATING;
        if (az_popc64(s.bb0) != (s.ply + 1) / 2 || az_popc64(s.bb1) != s.ply / 2) return AZ_STATE_COUNT;
        if (az_c4_has_four(s.bb0) || az_c4_has_four(s.bb1)) return AZ_STATE_TERMINAL;
    } else {
        if (occ & ~g.board_mask) return AZ_STATE_OFF_BOARD;
        if (!s.bb0 || !s.bb1) return AZ_STATE_EMPTY_SIDE;
        if ((s.bb0 & g.row_last) || (s.bb1 & g.row_first)) return AZ_STATE_GOAL_ROW;
    }
    return az_count_legal<GAME>(s, g) > 0 ? AZ_STATE_OK : AZ_STATE_NO_MOVE;
}

// Left-right mirror of the board: column c <-> cols-1-c.  Both games are symmetric under it (az_apply, the legality helpers
// and az_check_state commute with the two functions below), so the mirror image of a training example is the mirrored
// position with the mirrored policy and the same value.  Both are involutions; bits that are no cell stay where they are,
// so az_check_state gives a mirrored state the rule it gives the original.
//   connect_four : the 7-bit column groups swap (a column's sentinel bit travels with it: clear stays clear)
//   breakthrough : every row of C bits is reversed
template <int GAME> AZ_HD uint64_t az_mirror_bits(uint64_t b, const AzGeom &g) {
    if (GAME == AZG_CONNECT_FOUR) {
        const uint64_t c = 0x7Full;
        return (b & ~((1ull << 49) - 1)) | ((b & c) << 42) | ((b & (c << 7)) << 28) | ((b & (c << 14)) << 14) | (b & (c << 21)) |
               ((b >> 14) & (c << 14)) | ((b >> 28) & (c << 7)) | ((b >> 42) & c);
    } else {
        const uint64_t col0 = g.board_mask & ~g.not_col0; // column 0 of every row
        uint64_t out = b & ~g.board_mask;
        for (int c = 0; c < g.cols; c++) { // column c moves by cols-1-2c bits
            uint64_t v = b & (col0 << c);
            int sh = g.cols - 1 - 2 * c;
            out |= sh >= 0 ? v << sh : v >> -sh;
        }
        return out;
    }
}
template <int GAME> AZ_HD AzState az_mirror_state(const AzState &s, const AzGeom &g) {
    AzState m;
    m.bb0 = az_mirror_bits<GAME>(s.bb0, g);
    m.bb1 = az_mirror_bits<GAME>(s.bb1, g);
    m.ply = s.ply;
    return m;
}
// The action that does to az_mirror_state(s) what `action` does to s; action in [0, A).
//   connect_four : a -> 6 - a
//   breakthrough : the cell is mirrored, dc is negated inside the side's own three directions (az_apply: dc = dir % 3 - 1),
//                  the capture bit is kept
// (no run-time division: the replay store's mirrored gather calls this per element.  / 6 and % 6 are multiplies; the row of a
// cell is counted from the row starts at or below it.)
template <int GAME> AZ_HD int az_mirror_action(int action, const AzGeom &g) {
    if (GAME == AZG_CONNECT_FOUR) return 6 - action;
    const int h = action >> 1, cell = h / 6, d = h % 6;
    const uint64_t col0 = g.board_mask & ~g.not_col0;
    const int row = az_popc64(col0 & ((2ull << cell) - 1)) - 1, col = cell - row * g.cols;
    const int mcell = cell + g.cols - 1 - 2 * col, md = d >= 3 ? 8 - d : 2 - d;
    return ((mcell * 6 + md) << 1) | (action & 1);
}

// Observation element idx of state_to_board's (C+1,H,W) tensor (network.py:9-18), C = 3.
//   connect_four planes: 0 empty, 1 player-1 stones, 2 player-0 stones, 3 current player
//   breakthrough planes: 0 black,  1 white,          2 empty,           3 current player
template <int GAME> AZ_HD float az_obs_elem(const AzState &s, const AzGeom &g, int idx) {
    // (no run-time division: this sits at the end of every playout, on the tick kernel's critical path)
    const int cells = GAME == AZG_CONNECT_FOUR ? 42 : g.cells;
    int plane = (idx >= cells) + (idx >= 2 * cells) + (idx >= 3 * cells), cell = idx - plane * cells;
    if (plane == 3) return (float)(s.ply & 1);
    uint64_t bit;
    if (GAME == AZG_CONNECT_FOUR) {
        int row = cell / 7, col = cell - row * 7;
        bit = 1ull << (col * 7 + row);
        uint64_t sel = plane == 0 ? ~(s.bb0 | s.bb1) : (plane == 1 ? s.bb1 : s.bb0);
        return (sel & bit) ? 1.f : 0.f;
    } else {
        bit = 1ull << cell;
        uint64_t sel = plane == 0 ? s.bb0 : (plane == 1 ? s.bb1 : ~(s.bb0 | s.bb1));
        return (sel & bit) ? 1.f : 0.f;
    }
}

static inline int az_num_actions(int game, int rows, int cols) { return game == AZG_CONNECT_FOUR ? 7 : rows * cols * 12; }
static inline int az_max_children(int game, int rows, int cols) {
    if (game == AZG_CONNECT_FOUR) return 7;
    int m = 6 * cols; // 2*cols pieces x 3 directions
    return m > 64 ? 64 : m;
}
static inline int az_max_plies(int game, int rows, int cols) {
    return game == AZG_CONNECT_FOUR ? 42 : 2 * cols * (2 * rows - 5) + 1;
}
