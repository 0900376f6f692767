"""CPU-only checks of the greedy-line route: the C ABI surface of az_engine_export_lines_device / az_replay_refresh_from_search,
the one host description of the export's layout (engine.lines_export_layout, engine.read_lines), and the value targets the
Python refresh entries accept."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from alphazero_openspiel_amd import _lib, engine, replay

ENTRIES = ("az_engine_lines_device_bytes", "az_engine_export_lines_device", "az_replay_refresh_from_search")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declarations():
    """{entry: (return type, [parameter declarations])} from the headers, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _header("az_engine.h") + _header("az_replay.h"), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int|int64_t)\s+(az_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = (ret, [p.strip() for p in params.split(",")])
    return out


def test_headers_declare_the_entries_and_the_constant():
    decl = _declarations()
    for name in ENTRIES:
        assert name in decl, name
    assert decl["az_engine_lines_device_bytes"] == ("int64_t", ["const az_engine *e", "int32_t max_depth"])
    assert decl["az_engine_export_lines_device"] == ("int", ["az_engine *e", "int32_t max_depth", "void *dev_buf", "int64_t bytes",
                                                            "void *stream"])
    assert decl["az_replay_refresh_from_search"][0] == "int64_t"
    assert decl["az_replay_refresh_from_search"][1][3:7] == ["const void *roots", "int64_t roots_bytes", "const void *lines",
                                                             "int64_t lines_bytes"]
    defines = dict(re.findall(r"#define\s+(AZ_[A-Z_0-9]+)\s+(\d+)u?\b", _header("az_replay.h")))
    assert defines["AZ_REFRESH_OFF_POLICY"] == "3"
    assert (defines["AZ_REFRESH_KEEP_Z"], defines["AZ_REFRESH_SOFT_Z"], defines["AZ_REFRESH_A0C"]) == ("0", "1", "2")
    assert _lib.REFRESH_OFF_POLICY == 3


def test_refresh_mode_tables():
    assert _lib.REFRESH_MODES == {None: 0, "soft-Z": 1, "A0C": 2}          # unchanged: what a root alone gives
    assert _lib.SEARCH_REFRESH_MODES == {None: 0, "soft-Z": 1, "A0C": 2, "off-policy": 3}


def test_lib_binds_the_entries_with_matching_arguments():
    decl = _declarations()
    proto = {n: (res, args) for n, res, args in _lib.PROTOTYPES}
    lib = _lib.load()
    for name in ENTRIES:
        res, args = proto[name]
        assert len(args) == len(decl[name][1]), name
        assert res is {"int": C.c_int, "int64_t": C.c_int64}[decl[name][0]], name
        for a, d in zip(args, decl[name][1]):  # pointers are void*, the byte counts are 64-bit, max_depth / value_mode 32-bit
            want = C.c_void_p if "*" in d else {"int64_t": C.c_int64, "int32_t": C.c_int32}[d.split()[0]]
            assert a is want, (name, d)
        assert hasattr(lib, name)


@pytest.mark.parametrize("G,D", [(1, 1), (3, 2), (16, 8), (17, 5), (4096, 42), (5, 1)])
def test_layout_offsets_are_aligned_and_in_order(G, D):
    layout, total = engine.lines_export_layout(G, D)
    assert [name for name, _, _, _ in layout] == ["header", "game_id", "phase", "ply", "depth", "leaf_n", "value", "line_action",
                                                  "line_n", "line_q"]
    assert [np.dtype(dt).name for _, dt, _, _ in layout] == ["int32"] * 5 + ["uint32", "float64", "int32", "uint32", "float64"]
    assert [shape for _, _, shape, _ in layout] == [(4,)] + [(G,)] * 6 + [(G, D)] * 3
    end = 0
    for name, dt, shape, off in layout:
        assert off % 16 == 0 and off >= end and off - end < 16, name   # aligned, after its predecessor, no more than padding
        end = off + int(np.prod(shape)) * np.dtype(dt).itemsize
    assert total % 16 == 0 and 0 <= total - end < 16


def _synthetic(G, D, seed=0):
    rng = np.random.RandomState(seed)
    layout, total = engine.lines_export_layout(G, D)
    buf = np.zeros(total + 5, np.uint8)                                # (a buffer may be longer than the layout)
    want = {}
    for name, dt, shape, off in layout:
        if name == "header":
            arr = np.array([G - 1, G, D, 6], np.int32)
        elif np.dtype(dt).kind == "f":
            arr = rng.standard_normal(shape)
        elif np.dtype(dt).kind == "u":
            arr = rng.randint(0, 2 ** 32, size=shape, dtype=np.int64).astype(np.uint32)  # beyond int32: no sign mishap
        else:
            arr = rng.randint(-2, 50, size=shape).astype(np.int32)
        buf[off:off + arr.nbytes] = np.ascontiguousarray(arr, dtype=dt).view(np.uint8).reshape(-1)
        want[name] = arr
    return buf, want


@pytest.mark.parametrize("G,D", [(1, 1), (5, 3), (16, 8)])
def test_read_lines_round_trips_a_synthetic_buffer(G, D):
    buf, want = _synthetic(G, D)
    got = engine.read_lines(buf)
    assert (got["n_finished"], got["max_depth"], got["error_flags"]) == (G - 1, D, 6)
    assert set(got) == {"game_id", "phase", "ply", "depth", "leaf_n", "value", "line_action", "line_n", "line_q", "n_finished",
                        "max_depth", "error_flags"}
    for k in ("game_id", "phase", "ply", "depth", "value", "line_action", "line_q"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in ("leaf_n", "line_n"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k].astype(np.int64)), k
    assert got["line_n"].min() >= 0
    with pytest.raises(ValueError):
        engine.read_lines(buf[:engine.lines_export_layout(G, D)[1] - 1])
    with pytest.raises(ValueError):
        engine.read_lines(buf[:8])


class _NoStore:
    """What the value-target check of the Python entries may touch before it refuses."""
    device = "cpu"
    game = "connect_four"


def test_on_policy_is_still_refused_and_the_texts_do_not_call_off_policy_impossible():
    with pytest.raises(ValueError) as err:
        replay.Reanalyser(_NoStore(), None, 8, 8, value_target="on-policy")
    assert "on-policy" in str(err.value) and "off-policy" in str(err.value) and "descent" not in str(err.value)
    with pytest.raises(ValueError) as err:
        replay.DeviceReplay.refresh_from_search(_NoStore(), [0], None, None, "on-policy")
    assert "on-policy" in str(err.value) and "off-policy" in str(err.value)
    with pytest.raises(ValueError):                                     # the line export is what makes off-policy possible
        replay.DeviceReplay.refresh_from_search(_NoStore(), [0], None, None, "off-policy")
    with pytest.raises(ValueError) as err:                              # a root alone still does not give it
        replay.DeviceReplay.refresh_from_roots(_NoStore(), [0], None, "off-policy")
    assert "refresh_from_search" in str(err.value) and "descent" not in str(err.value)
    with pytest.raises(ValueError):
        replay.DeviceReplay.refresh_from_roots(_NoStore(), [0], None, "on-policy")
