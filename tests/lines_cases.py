"""Shared by test_lines_gpu.py and test_reanalyse_off_policy_gpu.py: the greedy line of a search tree, walked in numpy on what
az_engine_read_tree returns, by the reference's rule (game_utils.py:183-194) written out here."""
import numpy as np


def walk_tree(tree):
    """tree: SelfPlayEngine.read_tree(slot) (breadth-first; the children of a node are consecutive and in ascending-action
    order, the order of the reference's `children` dict).  -> (line, leaf_n, value): line = [(action, N, Q)] of the node
    reached after each move, leaf_n = N of the last node, value = the reference's `value * value_mult`.

        while not node.is_leaf():
            value = node.Q
            value_list = {a: (child.N + child.P if child.N > 0 else -99.0) for a, child in node.children.items()}
            node = node.children[max(value_list, key=value_list.get)]     # the first maximum
            value_mult *= -1.0
        if node.N > 0:
            value = node.Q
            value_mult *= -1.0
    """
    par, act, N, Q, P = (tree[k] for k in ("parent", "action", "N", "Q", "P"))
    n = len(par)
    first, cnt = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for i in range(1, n):
        if first[par[i]] < 0:
            first[par[i]] = i
        assert first[par[i]] + cnt[par[i]] == i                        # consecutive
        cnt[par[i]] += 1
    node, value, mult, line = 0, 0.0, 1.0, []
    while cnt[node] > 0:
        value = float(Q[node])
        kids = range(int(first[node]), int(first[node] + cnt[node]))
        scores = [float(N[k]) + float(P[k]) if N[k] > 0 else -99.0 for k in kids]
        node = kids[scores.index(max(scores))]                         # list.index: the first maximum, as max() over a dict
        mult *= -1.0
        line.append((int(act[node]), int(N[node]), float(Q[node])))
    if N[node] > 0:
        value = float(Q[node])
        mult *= -1.0
    return line, int(N[node]), value * mult


def bits(x):
    """float64 array / scalar -> its bit patterns (so -0.0 != 0.0 and a NaN equals itself)."""
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_slot_equals_walk(lines, g, tree, D):
    """Slot g of engine.read_lines() against walk_tree(tree): every field with ==, the value bit for bit."""
    line, leaf_n, value = walk_tree(tree)
    k = min(len(line), D)
    assert int(lines["depth"][g]) == len(line), (g, int(lines["depth"][g]), len(line))
    assert int(lines["leaf_n"][g]) == leaf_n, g
    assert bits(lines["value"][g]) == bits(value), (g, float(lines["value"][g]), value)
    assert lines["line_action"][g, :k].tolist() == [s[0] for s in line[:k]], g
    assert lines["line_n"][g, :k].tolist() == [s[1] for s in line[:k]], g
    assert bits(lines["line_q"][g, :k]).tolist() == bits([s[2] for s in line[:k]]).tolist(), g
    assert (lines["line_action"][g, k:] == -1).all() and (lines["line_n"][g, k:] == 0).all(), g
    assert (bits(lines["line_q"][g, k:]) == 0).all(), g
    return line, leaf_n, value
