"""Shared by test_analysis.py and test_analysis_gpu.py: the positions the analysis tests search."""
import numpy as np

from alphazero_openspiel_amd import games


def random_positions(game_name, n, seed, min_ply, max_ply):
    """n action histories: uniformly random legal moves from the initial position to a random target ply in
    [min_ply, max_ply]; if a move would end the game the history stops before it.  Every generated position is returned."""
    rng = np.random.RandomState(seed)
    game = games.load_game(game_name)
    out = []
    for _ in range(n):
        target = int(rng.randint(min_ply, max_ply + 1))
        st = game.new_initial_state()
        while len(st.history()) < target:
            legal = st.legal_actions()
            a = int(legal[rng.randint(len(legal))])
            nxt = st.clone()
            nxt.apply_action(a)
            if nxt.is_terminal():
                break
            st = nxt
        out.append(st.history())
    return out
