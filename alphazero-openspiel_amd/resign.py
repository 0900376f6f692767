"""Calibrating self-play resignation from play-through games (host only, numpy).

An engine under SelfPlayEngine.set_resign(v, playthrough) lets a fraction of its games play through, and records per game and
player `low`: the lowest value of the resignation criterion that player saw at a qualifying ply (+inf: none).  A player WOULD have
resigned under a threshold v iff low < -v, so one batch of play-through games tells the false-positive rate of every threshold:
the share of such players who did not go on to lose.  AlphaGo Zero keeps that rate below 5 %.

low: array [n, 2] (column p: player p), ret0: array [n], the games' results seen by player 0 (+1 win, 0 draw, -1 loss) - of
PLAY-THROUGH games only (SelfPlayEngine.resign_info()["playthrough"], or any game of a run with playthrough=1); a game that was
cut at its resign ply says nothing about what would have happened.

weights: array [n] or None.  Under a threshold v0 with playthrough p < 1 the games that were played out are a biased sample: a
game WITH a resign ply is among them with probability p (its coin is independent of the game), a game without one always.
played_out_weights gives the first kind the weight 1 / p and the second 1, and the weighted rate is an unbiased estimate for every
threshold, more eager than v0 or not."""
import numpy as np


def played_out_weights(has_resign_ply, playthrough):
    """Weights of the played-out games of a run under SelfPlayEngine.set_resign(v0, playthrough): 1 / playthrough for a game
    with a resign ply (SelfPlayEngine.resign_info()["ply"] >= 0), 1 for a game without one.  playthrough in (0, 1]."""
    if not 0.0 < float(playthrough) <= 1.0:
        raise ValueError("played-out games can be weighted only under a playthrough share in (0, 1], got %r" % (playthrough,))
    return np.where(np.asarray(has_resign_ply, dtype=bool), 1.0 / float(playthrough), 1.0)


def _would_resign(low, ret0, v):
    low = np.asarray(low, dtype=np.float64).reshape(-1, 2)
    ret0 = np.asarray(ret0, dtype=np.float64).reshape(-1)
    if len(low) != len(ret0):
        raise ValueError("low holds %d games, ret0 %d" % (len(low), len(ret0)))
    if not 0.0 < float(v) <= 1.0:
        raise ValueError("a resignation threshold lies in (0, 1], got %r" % (v,))
    resigns = low < -float(v)                                    # [n, 2]
    lost = np.stack([ret0 < 0.0, ret0 > 0.0], axis=1)            # player 0 loses at ret0 = -1, player 1 at +1
    return resigns, lost


def false_positive_rate(low, ret0, v, weights=None):
    """Among the players of play-through games with low < -v, the share who did not lose (a draw counts: the resignation gave away
    half a point).  -> (rate, players with low < -v); the rate is 0.0 when nobody would have resigned.  weights: per game (module
    doc); the count returned stays the plain number of players seen."""
    resigns, lost = _would_resign(low, ret0, v)
    n = int(resigns.sum())
    if weights is None:
        wrong = int((resigns & ~lost).sum())
        return (wrong / n if n else 0.0), n
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 1)
    if len(w) != len(resigns) or not (w > 0.0).all():
        raise ValueError("weights must hold one positive number per game")
    total = float((resigns * w).sum())
    return (float(((resigns & ~lost) * w).sum()) / total if n else 0.0), n


def calibrate(low, ret0, target=0.05, floor=0.05, min_games=20, weights=None):
    """The smallest v >= floor - the most eager threshold - whose false-positive rate is at or below `target` and stays there for
    every larger v.  Only the criterion values seen can change a rate, so the candidates are `floor` and the thresholds just above
    each seen -low (the rate is a step function of v, and not monotone in general: the answer is the point from which every more
    cautious threshold passes too).  v = 1.0 never resigns (crit >= -1) and always passes.
    ValueError with fewer than min_games play-through games: too few to say.  weights: as false_positive_rate."""
    low = np.asarray(low, dtype=np.float64).reshape(-1, 2)
    if len(low) < int(min_games):
        raise ValueError("calibrate needs at least %d play-through games to say anything, got %d" % (int(min_games), len(low)))
    if not 0.0 < float(floor) <= 1.0 or not 0.0 <= float(target) <= 1.0:
        raise ValueError("floor must lie in (0, 1] and target in [0, 1], got floor=%r target=%r" % (floor, target))
    seen = -low[np.isfinite(low)]
    cands = sorted({float(floor), 1.0} | {float(x) for x in seen if float(floor) < x < 1.0})
    best = 1.0
    for v in reversed(cands):                                    # from the most cautious down, while the rate holds
        if false_positive_rate(low, ret0, v, weights)[0] > float(target):
            break
        best = v
    return best
