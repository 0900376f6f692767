"""What keeps test_deep_lines_gpu.py from passing vacuously, asserted with the C oracle alone (no GPU): the line policy of
deep_line_cases.py drives every case's search across the depths its name promises, a playout ends on a terminal node down
there (so +-1 is backed up the whole line), one case branches at the root - and oracle/fakepolicy.fake_eval, the policy of
every other bit-exact test, stays above depth 16 on the same boards at the same playout counts."""
import numpy as np
import pytest

import deep_line_cases as DL
from oracle import binding as orc
from oracle import fakepolicy, pygames

MIN_DEPTH = {"bt26x2": 130, "bt12x5": 100, "bt8x8": 66, "c4": 42}
_SEARCHED = {}


def _searched(key):
    """(root statistics, playout depths, terminal depths, descent) of the case's search: computed once."""
    if key not in _SEARCHED:
        m, _, depths, terminal = DL.oracle_search(key)
        _SEARCHED[key] = (m.root_stats(), depths, terminal, DL.oracle_descent(m))
    return _SEARCHED[key]


@pytest.mark.parametrize("key", sorted(DL.CASES))
def test_the_search_crosses_the_depths_the_case_is_for(key):
    root, depths, terminal, descent = _searched(key)
    S = DL.CASES[key]["n_playouts"]
    print(key, "deepest playout", max(depths), "terminal hits", len(terminal), "deepest terminal", max(terminal),
          "principal line", len(descent))
    assert root["N"] == S and len(depths) == S
    if key == "c4":
        assert max(depths) == 42 and max(terminal) == 42               # the ply-42 draw, 42 plies under the root
    else:
        assert max(depths) >= MIN_DEPTH[key]
        assert max(terminal) >= 64
    assert len(terminal) > 0
    assert DL.CASES[key]["eta"] or depths[:40] == list(range(40))    # one ply deeper per playout: the chain of a*
    # the descent the GPU test compares node by node reaches those depths too, and ends in a visited leaf
    assert len(descent) >= MIN_DEPTH[key] - 4 and descent[-1][1]["N"] > 0 and not descent[-1][1]["actions"]


def test_boards_are_the_ones_the_issue_is_about():
    """Register boundaries of the select path: connect_four keeps 64 depths, breakthrough 192; 12x5 is the largest game."""
    assert [orc.max_plies(*orc.parse_game(DL.CASES[k]["game"])) for k in ("bt26x2", "bt12x5", "bt8x8", "c4")] == [189, 191, 177, 42]
    assert {c["vs"] > 0 for c in DL.CASES.values()} == {True, False}


def test_one_case_branches_at_the_root():
    visited = {k: [n for n in _searched(k)[0]["cN"] if n > 0] for k in DL.CASES}
    print(visited)
    assert any(len(v) > 1 and max(v) > sum(v) - max(v) for v in visited.values())
    assert len(visited["c4"]) > 1


@pytest.mark.parametrize("key", sorted(DL.CASES))
def test_fake_eval_stays_shallow_on_the_same_boards(key):
    """Why the line policy exists: under hashed logits in [-2, 2] the deepest playout stays below 16 (5-9 on the three boards
    other tests play).  Salts 0 and 2; on the two-column 26x2 board (3-6 legal moves a position) the figure depends on the
    salt - 12 to 21 over salts 0..11 - which is still a third of the way to lane 63 of the path's first register."""
    c = DL.CASES[key]
    A = pygames.load_game(c["game"]).num_distinct_actions()
    for salt in (0, 2):
        m = orc.MCTS(lambda b: fakepolicy.fake_eval(b, A, salt), c["game"], n_playouts=c["n_playouts"], use_dirichlet=False)
        s, deepest, prev = orc.State(c["game"]), 0, 0
        for _ in range(c["n_playouts"]):
            m.playout(s)
            cur = m.counters()["sum_depth"]
            deepest, prev = max(deepest, cur - prev), cur
        print(key, salt, "deepest playout under fake_eval", deepest)
        assert deepest < 16


@pytest.mark.parametrize("key", sorted(DL.CASES))
def test_line_policy_properties(key):
    """Priors sum to 1 within float32, every legal prior is a positive normal float32, a* is legal and keeps almost all the
    mass - on every position of the principal line; and the planes alone give back the position's legal moves."""
    c = DL.CASES[key]
    game = pygames.load_game(c["game"])
    A = game.num_distinct_actions()
    assert A <= 768
    pol = DL.case_policy(key)
    line = DL.principal_line(c["game"], c["salt"])                     # (asserts a* legal and the rebuilt legal list, ply by ply)
    assert len(line) >= MIN_DEPTH[key]
    st = orc.State(c["game"])
    tiny = np.finfo(np.float32).tiny
    values = []
    for a in line:
        legal = st.legal_actions()
        pri, val = pol(st.board())
        assert pri.dtype == np.float32 and pri.shape == (A,) and np.isfinite(pri).all()
        # (a float32 sum of A terms is off by at most (A - 1) roundings of half an ulp of 1.0, and so is the quotient's sum)
        assert abs(float(pri.astype(np.float64).sum()) - 1.0) <= A * np.finfo(np.float32).eps / 2
        assert (pri[legal] >= tiny).all() and (pri >= tiny).all()
        assert a in legal and int(np.argmax(pri)) == a and pri[a] > 0.995
        assert abs(float(val)) <= c["vs"]
        values.append(float(val))
        st.apply_action(a)
    assert st.is_terminal()
    assert (len(set(values)) > len(line) // 2) == (c["vs"] > 0)        # vs > 0: a different value at (almost) every node
    # planes that show no position (a request buffer before its first request): uniform, not an exception
    pri, val = pol(np.zeros((4, game.ROWS, game.COLS)))
    assert float(val) == 0.0 and (pri == np.float32(1.0 / A)).all()
