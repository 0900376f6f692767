"""Host side of stream mode: the layout of a take, and the capacity rule of ExampleGenerator(continuous=True)."""
import numpy as np
import pytest

from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.engine import (check_stream_request, device_export_layout, stream_capacity, stream_take_layout,
                                            unpack_device_export)
from test_host_logic import _fake_export


@pytest.mark.parametrize("n,mp,mc", [(1, 42, 7), (48, 42, 7), (5, 31, 12), (4096, 42, 7)])
def test_a_take_has_the_layout_of_a_generation_of_as_many_games(n, mp, mc):
    layout, total = stream_take_layout(n, mp, mc)
    assert (layout, total) == device_export_layout(n, mp, mc)
    assert all(off % 16 == 0 for _, _, _, off in layout) and total % 16 == 0
    sizes = [int(np.prod(shape)) * np.dtype(dt).itemsize for _, dt, shape, _ in layout]
    assert all(layout[i][3] + sizes[i] <= layout[i + 1][3] for i in range(len(layout) - 1)) and layout[-1][3] + sizes[-1] <= total


def test_unpack_round_trips_a_packed_take():
    game = games.load_game("connect_four")
    ex = _fake_export(game, n_games=5, seed=3)
    mp, mc = ex["move"].shape[1], ex["child_action"].shape[2]
    layout, total = stream_take_layout(5, mp, mc)
    buf = np.full(total, 0xEE, dtype=np.uint8)  # padding between the arrays is never read
    for name, dt, shape, off in layout:
        raw = np.ascontiguousarray(ex[name], dtype=dt).reshape(-1).view(np.uint8)
        buf[off:off + raw.size] = raw
    got = unpack_device_export(buf, 5, mp, mc)
    for name, dt, shape, _ in layout:
        assert got[name].dtype == dt and got[name].shape == shape and (got[name] == ex[name]).all(), name
    with pytest.raises(ValueError):
        unpack_device_export(buf[:-16], 5, mp, mc)


def test_capacity_rule_of_the_continuous_generator():
    assert stream_capacity(4096, 4096) == 4096 + 2 * 4096
    assert stream_capacity(48, 64) == 48 + 128
    assert stream_capacity(6, 8) == 22
    assert stream_capacity(48, 64, capacity=64) == 64          # an explicit capacity: at least the slots and one call's games
    for n_local, n_slots, cap in ((48, 64, 63), (100, 64, 99)):
        with pytest.raises(ValueError):
            stream_capacity(n_local, n_slots, capacity=cap)
    cap = stream_capacity(48, 64)
    assert check_stream_request(48, cap) == 48 and check_stream_request(cap, cap) == cap and check_stream_request(1, cap) == 1
    with pytest.raises(ValueError, match="capacity"):
        check_stream_request(cap + 1, cap)
