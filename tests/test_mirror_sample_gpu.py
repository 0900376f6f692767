"""az_replay_sample_sym (include/az_replay.h) on the device, through the C ABI: the mirrored batch gather against
az_replay_sample, which stays the reference.  Every comparison is on bytes; no tolerance is involved.

Stores hold about 40 unique positions (tests/mirror_cases.py); the batch of 64 is no multiple of the workgroup size (128) and
has more than one row per example."""
import ctypes as C

import numpy as np
import pytest
import torch

import mirror_cases as MC
from alphazero_openspiel_amd import games

pytestmark = pytest.mark.gpu
BATCH = 64


@pytest.fixture(scope="module", params=MC.BOARDS)
def board(request):
    """(game, a store for calls with explicit indices, n_unique); the store's call counter is nobody's business here."""
    rep, n = MC.make_store(request.param)
    assert 36 <= n <= 42
    yield games.load_game(request.param), rep, n
    rep.close()


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _indices(n, batch=BATCH, seed=0):
    """every example at least once, then random ones"""
    rng = np.random.RandomState(seed)
    return _dev(np.concatenate([rng.permutation(n), rng.randint(n, size=batch - n)]), torch.int64)


def test_flips_zero_one_and_mixed_against_the_plain_gather(board):
    game, rep, n = board
    idx = _indices(n)
    plain = MC.call_plain(rep, BATCH, idx)
    want = MC.mirrored(game, plain)
    # the examples are uneven: a mirrored row differs from the stored one in x or in pi (else the checks below show nothing)
    assert not bool((MC.rows_equal((plain[1],), (want[1],))).any())
    assert int((~MC.rows_equal((plain[0],), (want[0],))).sum()) > BATCH // 2
    zeros = MC.call_sym(rep, BATCH, idx, torch.zeros(BATCH, dtype=torch.uint8, device="cuda"))
    assert bool(MC.rows_equal(zeros, plain).all())
    ones = MC.call_sym(rep, BATCH, idx, torch.ones(BATCH, dtype=torch.uint8, device="cuda"))
    assert torch.equal(ones[0], torch.flip(plain[0], dims=[3]))
    m = MC.action_mirror_table(game)
    assert torch.equal(ones[1][:, m], plain[1])  # pi_out[mirror(a)] = pi[a]
    assert torch.equal(MC.bits(ones[2]), MC.bits(plain[2]))
    assert bool(MC.rows_equal(ones, want).all())
    pattern = np.random.RandomState(1).randint(0, 2, BATCH).astype(np.uint8)
    pattern[pattern > 0] = np.random.RandomState(2).randint(1, 256, int(pattern.sum()))  # any non-zero byte mirrors
    assert 0 < (pattern > 0).sum() < BATCH
    mixed = MC.call_sym(rep, BATCH, idx, _dev(pattern, torch.uint8))
    assert (MC.recover_flips(game, plain, mixed) == (pattern > 0)).all()


def test_device_draw_picks_the_rows_of_the_plain_entry_and_shares_its_counter(board):
    game, rep, n = board
    name = game.name
    a, _ = MC.make_store(name)  # plain, plain, plain
    b, _ = MC.make_store(name)  # sym, plain, sym: the same call numbers
    c, _ = MC.make_store(name)  # sym with another seed
    patterns = []
    for call, use_sym in enumerate((True, False, True)):
        plain = MC.call_plain(a, BATCH, seed=11)
        # (the restatement of the index draw, used by the tests below, agrees with the entry)
        explicit = MC.call_plain(rep, BATCH, _dev(MC.drawn_indices(11, call, BATCH, n), torch.int64))
        assert bool(MC.rows_equal(plain, explicit).all())
        got = MC.call_sym(b, BATCH, seed=11) if use_sym else MC.call_plain(b, BATCH, seed=11)
        flips = MC.recover_flips(game, plain, got)  # un-mirroring each row gives the plain entry's row
        if use_sym:
            patterns.append(flips)
            assert 0 < flips.sum() < BATCH
        else:
            assert not flips.any()
    assert (patterns[0] != patterns[1]).any()  # another call number, another pattern
    other = MC.call_sym(c, BATCH, seed=12)
    plain12 = MC.call_plain(rep, BATCH, _dev(MC.drawn_indices(12, 0, BATCH, n), torch.int64))
    assert (MC.recover_flips(game, plain12, other) != patterns[0]).any()  # another seed, another pattern
    for s in (a, b, c):
        s.close()


def test_drawn_flips_are_a_fair_coin_that_does_not_follow_the_index(board):
    game, rep, n = board
    big = 4096
    fresh, _ = MC.make_store(game.name)
    got = MC.call_sym(fresh, big, seed=5)
    fresh.close()
    idx = MC.drawn_indices(5, 0, big, n)
    flips = MC.recover_flips(game, MC.call_plain(rep, big, _dev(idx, torch.int64)), got)
    count = int(flips.sum())
    print("flips: %d of %d" % (count, big))
    assert 1856 <= count <= 2240  # 2048 +- 6 sigma, sigma = 32 for a fair coin
    low = idx < np.median(idx)
    share = float(flips[low].mean())
    print("rows below the median index: %d, of them flipped: %.4f" % (int(low.sum()), share))
    assert 1500 < low.sum() < 2600
    for rows in (flips, ~flips):  # flipped and unflipped rows each use low and high indices
        assert idx[rows].min() < n // 4 and idx[rows].max() >= n - n // 4
    assert 0.43 <= share <= 0.57  # 6 sigma for about 2048 fair draws, sigma ~ 0.011


def test_bad_index_poisons_its_row_whatever_its_flip(board):
    game, rep, n = board
    idx = _indices(n).cpu().numpy()
    idx[[3, 4, 70 % BATCH, 9]] = [-1, n, n + 5, -(2 ** 40)]
    bad = np.zeros(BATCH, bool)
    bad[[3, 4, 70 % BATCH, 9]] = True
    flips = np.zeros(BATCH, np.uint8)
    flips[[3, 9, 20, 21]] = 1
    good_idx = np.where(bad, 0, idx)
    ref = MC.call_sym(rep, BATCH, _dev(good_idx, torch.int64), _dev(flips, torch.uint8))
    assert rep.stats()["fault_flags"] == 0
    got = MC.call_sym(rep, BATCH, _dev(idx, torch.int64), _dev(flips, torch.uint8))
    badt = torch.as_tensor(bad).cuda()
    for t in got:
        assert bool(torch.isnan(t[badt]).all())
    assert bool(MC.rows_equal(got, ref)[~badt].all())
    with pytest.raises(RuntimeError, match="BAD_INDEX"):
        rep.stats()
    assert rep.stats()["fault_flags"] == 0  # reported once
    # and with drawn flips
    got = MC.call_sym(rep, BATCH, _dev(idx, torch.int64), None, seed=3)
    assert all(bool(torch.isnan(t[badt]).all()) for t in got) and not any(bool(torch.isnan(t[~badt]).any()) for t in got)
    with pytest.raises(RuntimeError, match="BAD_INDEX"):
        rep.stats()


def test_refusals(board):
    game, rep, n = board
    x, pi, z = MC.outputs(rep, BATCH)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sym = rep.lib.az_replay_sample_sym
    assert sym(rep._h, None, None, BATCH, 0, None, vp(pi), vp(z), None) == MC.E_INVALID
    assert sym(rep._h, None, None, BATCH, 0, vp(x), None, vp(z), None) == MC.E_INVALID
    assert sym(rep._h, None, None, BATCH, 0, vp(x), vp(pi), None, None) == MC.E_INVALID
    assert sym(rep._h, None, None, 0, 0, vp(x), vp(pi), vp(z), None) == MC.E_INVALID
    assert sym(rep._h, None, None, -3, 0, vp(x), vp(pi), vp(z), None) == MC.E_INVALID
    assert sym(None, None, None, BATCH, 0, vp(x), vp(pi), vp(z), None) == MC.E_INVALID
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (x, pi, z))  # nothing was launched
    undeduped, _ = MC.make_store(game.name, dedupe=False)
    assert sym(undeduped._h, None, None, BATCH, 0, vp(x), vp(pi), vp(z), undeduped._stream()) == MC.E_STATE
    assert b"az_replay_dedupe" in rep.lib.az_replay_last_error(undeduped._h)
    undeduped.close()


def test_a_captured_call_replays_to_the_bytes_of_the_eager_call(board):
    game, rep, n = board
    idx = _indices(n, seed=4)
    flips = _dev(np.random.RandomState(5).randint(0, 2, BATCH), torch.uint8)
    eager = MC.call_sym(rep, BATCH, idx, flips)
    x, pi, z = MC.outputs(rep, BATCH)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = rep.lib.az_replay_sample_sym(rep._h, C.c_void_p(idx.data_ptr()), C.c_void_p(flips.data_ptr()), BATCH, 0,
                                          C.c_void_p(x.data_ptr()), C.c_void_p(pi.data_ptr()), C.c_void_p(z.data_ptr()), rep._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())  # captured, not run
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert bool(MC.rows_equal((x, pi, z), eager).all())
        x.fill_(-7.0)
    # new contents of the device buffers are what the next replay reads
    flips.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert bool(MC.rows_equal((x, pi, z), MC.mirrored(game, MC.call_plain(rep, BATCH, idx))).all())
