"""CPU-only checks of the record layout: the HOST build of csrc/az_records.h (records_offsets, records_in, records_ptrs and
records_sizes, through a small stand-alone C++ program compiled at test time with g++) against engine.device_export_layout, and
the three Python layout functions against their offsets written out as literals."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from alphazero_openspiel_amd import games
from alphazero_openspiel_amd.engine import device_export_layout, lines_export_layout, roots_export_layout

_BT8 = games.load_game("breakthrough(rows=8,columns=8)")
SHAPES = [(1, 42, 7), (3, 43, 7), (5, 21, 18), (7, 1, 1), (4, _BT8.max_game_length(), _BT8.max_children())]

_PROGRAM = r"""
#include <cstdio>
#include "az_records.h"
int main() { // per line: n mp mc  ->  the nine offsets | the byte offset of every records_in pointer | the eight sizes
    unsigned long long n, mp, mc;
    alignas(16) static char base[16];
    while (scanf("%llu %llu %llu", &n, &mp, &mc) == 3) {
        size_t off[AZ_RECORD_ARRAYS + 1], sizes[AZ_RECORD_ARRAYS];
        records_offsets(n, mp, mc, off);
        records_sizes(n, mp, mc, sizes);
        const AzRecords v = records_in(base, n, mp, mc); // (pointers are formed, never followed)
        void *p[AZ_RECORD_ARRAYS];
        records_ptrs(v, p);
        const void *typed[AZ_RECORD_ARRAYS] = {v.game_len, v.game_ret0, v.states, v.move, v.n_children, v.child_action, v.child_visits, v.value};
        for (int i = 0; i <= AZ_RECORD_ARRAYS; i++) printf("%zu ", off[i]);
        for (int i = 0; i < AZ_RECORD_ARRAYS; i++) {
            if (p[i] != typed[i]) return 2;
            printf("%zu ", (size_t)((char *)p[i] - base));
        }
        for (int i = 0; i < AZ_RECORD_ARRAYS; i++) printf("%zu ", sizes[i]);
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("records")
    src, exe = d / "records.cpp", d / "records"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])
    text = "".join("%d %d %d\n" % s for s in SHAPES)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(SHAPES)
    rows = [[int(w) for w in line.split()] for line in out]
    return {s: (r[:9], r[9:17], r[17:]) for s, r in zip(SHAPES, rows)}


def test_breakthrough_shape_is_the_games_own():
    assert SHAPES[-1] == (4, 177, 48)


@pytest.mark.parametrize("shape", SHAPES)
def test_header_layout_is_device_export_layout(shape, header_layout):
    off, ptr_off, sizes = header_layout[shape]
    layout, total = device_export_layout(*shape)
    assert [name for name, *_ in layout] == ["game_len", "game_ret0", "states", "move", "n_children", "child_action",
                                             "child_visits", "value"]
    assert off[:8] == [o for *_, o in layout] and off[8] == total
    assert ptr_off == off[:8]
    assert sizes == [int(np.prod(sh)) * np.dtype(dt).itemsize for _, dt, sh, _ in layout]
    assert all(o % 16 == 0 for o in off)


def test_every_array_is_padded_in_some_shape(header_layout):
    """... every array that can be: a states row is 16 bytes, so that array never needs padding."""
    padded = [False] * 8
    for off, _, sizes in header_layout.values():
        for i in range(8):
            padded[i] |= off[i + 1] - off[i] > sizes[i]
    assert padded == [True, True, False, True, True, True, True, True]


# offsets and totals of the three layout functions, written out (computed before they shared one helper)
PINNED = [
    (roots_export_layout, (3, 7), [0, 16, 32, 48, 64, 80, 96, 112, 144, 240, 336, 512], 688),
    (roots_export_layout, (5, 18), [0, 16, 48, 80, 112, 144, 176, 208, 256, 624, 992, 1712], 2432),
    (lines_export_layout, (3, 5), [0, 16, 32, 48, 64, 80, 96, 128, 192, 256], 384),
    (lines_export_layout, (7, 12), [0, 16, 48, 80, 112, 144, 176, 240, 576, 912], 1584),
    (device_export_layout, (3, 43, 7), [0, 16, 32, 2096, 2368, 2512, 4320, 7936], 8976),
    (device_export_layout, (5, 21, 18), [0, 32, 64, 1744, 1968, 2080, 5872, 13440], 14288),
]


@pytest.mark.parametrize("fn,args,offsets,total", PINNED, ids=["%s%s" % (f.__name__, a) for f, a, _, _ in PINNED])
def test_python_layouts_are_pinned(fn, args, offsets, total):
    layout, got_total = fn(*args)
    assert [o for *_, o in layout] == offsets and got_total == total
    assert all(len(entry) == 4 for entry in layout)
