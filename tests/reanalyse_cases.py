"""Shared by test_reanalyse_host.py and test_reanalyse_gpu.py: states that az_check_state (csrc/az_games.h) must refuse, made
by hand from the bit layouts of that header, with the rule each one breaks FIRST in the order the function checks them."""
import numpy as np

from alphazero_openspiel_amd import games

# the enum of az_games.h
(OK, BAD_PLY, OVERLAP, OFF_BOARD, SENTINEL, FLOATING, COUNT, EMPTY_SIDE, GOAL_ROW, TERMINAL, NO_MOVE) = range(11)


def c4_bit(col, row):
    return 1 << (col * 7 + row)


def _c4_full_board():
    b = [0, 0]
    for c in range(7):
        for r in range(6):
            b[(c + r) & 1] |= c4_bit(c, r)
    assert bin(b[0]).count("1") == bin(b[1]).count("1") == 21
    return b


def bad_states(game):
    """[(name, bb0, bb1, ply, rule)] for a `games.Game`."""
    if game.name == "connect_four":
        full = _c4_full_board()
        row0 = c4_bit(0, 0) | c4_bit(1, 0) | c4_bit(2, 0) | c4_bit(3, 0)
        return [("floating stone", c4_bit(0, 1), 0, 1, FLOATING),
                ("stone count that does not match ply", c4_bit(0, 0) | c4_bit(1, 0), 0, 1, COUNT),
                ("four in a row", row0, c4_bit(0, 1) | c4_bit(1, 1) | c4_bit(2, 1), 7, TERMINAL),
                ("full board", full[0], full[1], 42, BAD_PLY),
                ("overlap", c4_bit(3, 0), c4_bit(3, 0), 2, OVERLAP),
                ("sentinel bit set", c4_bit(0, 0) | (1 << 6), c4_bit(1, 0), 3, SENTINEL)]
    s = game.new_initial_state()
    b0, b1 = int(s.bb[0]), int(s.bb[1])
    goal = 1 << ((game.rows - 1) * game.cols)  # first cell of the last row: black's goal, white's at the start
    assert b1 & goal and game.rows * game.cols < 60
    return [("piece on the goal row", b0 | goal, b1 & ~goal, 0, GOAL_ROW),
            ("empty side", b0, 0, 0, EMPTY_SIDE),
            ("bit off the board", b0 | (1 << (game.rows * game.cols + 3)), b1, 0, OFF_BOARD)]


def states_of(game, histories):
    """Action histories -> (bb uint64 [n, 2], ply int32 [n]) by playing them with the Python rules."""
    bb = np.zeros((len(histories), 2), np.uint64)
    for i, h in enumerate(histories):
        bb[i] = games.state_from_history(game, h).bb
    return bb, np.array([len(h) for h in histories], np.int32)
