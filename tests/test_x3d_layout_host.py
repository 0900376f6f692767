"""CPU-only checks of the packed-tile tower's column layout (csrc/az_x3d_layout.h), through a small stand-alone C++ program
compiled at test time with g++: the header is plain C++, and the library builds a net's tables with the same code.

For the 6x7, 6x6 and 8x8 boards: every (board, cell) is exactly one column, every residue mod 16 of the cell address
b R + (y + 1) rs + x + 1 is hit once per tile by the lane of that residue (the bank property), every tile the layout declares
top or bottom holds only cells of board row 0 or row H - 1 (what lets the kernel leave out the k-steps of the dy = -1 / dy = +1
taps for it), and the tile-X destination table agrees with the position table."""
import os
import subprocess

import pytest

from conftest import ROOT

BOARDS = [(6, 7), (6, 6), (8, 8)]
# what the kernel variants count on (az_x3d_variant): variant, boards per workgroup, tiles, pure tiles per edge row a 16-residue
# layout can give at best = cells of a row over the workgroup's boards // 16
EXPECT = {(6, 7): (2, 8, 21, 3), (6, 6): (0, 8, 18, 3), (8, 8): (1, 4, 16, 2)}
TAP_OF_PLANE = [0, 1, 2, 3, 5, 6, 7, 8]

_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "az_x3d_layout.h"
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const X3DLayout L = x3d_layout(atoi(argv[1]), atoi(argv[2]));
    const int tiles = L.variant < 0 ? 0 : az_x3d_variant(L.variant).tiles;
    printf("%d %d %d %d %d %d %d\n", L.variant, L.nb, L.R, L.rs, L.n_top, L.n_bot, tiles);
    if (L.variant < 0) return 0;
    printf("%d %d\n", az_x3d_variant(L.variant).skip_top, az_x3d_variant(L.variant).skip_bot);
    for (int i = 0; i < L.n_top; i++) printf("%d ", L.top_tile(i));
    printf("\n");
    for (int i = 0; i < L.n_bot; i++) printf("%d ", L.bot_tile(i));
    printf("\n");
    for (size_t i = 0; i < L.pos.size(); i++) printf("%d ", (int)L.pos[i]);
    printf("\n");
    for (size_t i = 0; i < L.sdst.size(); i++) printf("%d ", (int)L.sdst[i]);
    printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout_of(tmp_path_factory):
    d = tmp_path_factory.mktemp("x3d_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero-openspiel_amd", "csrc"),
                           str(src), "-o", str(exe)])
    cache = {}

    def run(H, W):
        if (H, W) not in cache:
            lines = subprocess.run([str(exe), str(H), str(W)], capture_output=True, text=True, check=True).stdout.splitlines()
            variant, nb, R, rs, n_top, n_bot, tiles = map(int, lines[0].split())
            out = dict(variant=variant, nb=nb, R=R, rs=rs, n_top=n_top, n_bot=n_bot, tiles=tiles)
            if variant >= 0:
                out["skip_top"], out["skip_bot"] = map(int, lines[1].split())
                out["top"] = list(map(int, lines[2].split()))
                out["bot"] = list(map(int, lines[3].split()))
                out["pos"] = list(map(int, lines[4].split()))
                out["sdst"] = list(map(int, lines[5].split()))
            cache[(H, W)] = out
        return cache[(H, W)]

    return run


@pytest.mark.parametrize("H,W", BOARDS)
def test_variant_and_pure_tile_counts(layout_of, H, W):
    L = layout_of(H, W)
    variant, nb, tiles, n_pure = EXPECT[(H, W)]
    assert (L["variant"], L["nb"], L["tiles"]) == (variant, nb, tiles)
    assert nb * H * W == 16 * tiles and len(L["pos"]) == 16 * tiles and len(L["sdst"]) == 16 * tiles * 8
    assert L["n_top"] == n_pure and L["n_bot"] == n_pure
    assert L["top"] == list(range(n_pure)) and L["bot"] == list(range(tiles - n_pure, tiles))
    assert not set(L["top"]) & set(L["bot"])
    # the tiles the kernel variant leaves k-steps out for are among the declared ones
    assert L["skip_top"] <= L["n_top"] and L["skip_bot"] <= L["n_bot"]


@pytest.mark.parametrize("H,W", BOARDS)
def test_every_cell_once_and_residues_flat(layout_of, H, W):
    L = layout_of(H, W)
    cells = [(e >> 8, e & 255) for e in L["pos"]]
    assert sorted(cells) == [(b, p) for b in range(L["nb"]) for p in range(H * W)]
    hist = [0] * 16
    for col, (b, p) in enumerate(cells):
        r = (b * L["R"] + (p // W + 1) * L["rs"] + p % W + 1) % 16
        assert r == col % 16, "lane l15 of every tile holds the position of residue l15"
        hist[r] += 1
    assert hist == [L["tiles"]] * 16
    # the layout's geometry keeps every tap of every position inside the board's region or on a halo cell
    assert L["rs"] >= W + 1 and L["R"] >= H * L["rs"] + W + 1


@pytest.mark.parametrize("H,W", BOARDS)
def test_declared_tiles_are_pure(layout_of, H, W):
    L = layout_of(H, W)
    rows = [[(e & 255) // W for e in L["pos"][16 * t:16 * t + 16]] for t in range(L["tiles"])]
    for t in L["top"]:
        assert rows[t] == [0] * 16, t
    for t in L["bot"]:
        assert rows[t] == [H - 1] * 16, t
    # within a residue: row-0 cells first, row-(H - 1) cells last
    for r in range(16):
        cls = [0 if rows[t][r] == 0 else 2 if rows[t][r] == H - 1 else 1 for t in range(L["tiles"])]
        assert cls == sorted(cls), r


@pytest.mark.parametrize("H,W", BOARDS)
def test_sdst_is_consistent_with_pos(layout_of, H, W):
    L = layout_of(H, W)
    col_of = {(e >> 8, e & 255): col for col, e in enumerate(L["pos"])}
    for col, e in enumerate(L["pos"]):
        b, p = e >> 8, e & 255
        y, x = divmod(p, W)
        for t in range(8):
            dy, dx = TAP_OF_PLANE[t] // 3 - 1, TAP_OF_PLANE[t] % 3 - 1
            yd, xd = y - dy, x - dx
            want = col_of[(b, yd * W + xd)] if 0 <= yd < H and 0 <= xd < W else 0xFFFF
            assert L["sdst"][col * 8 + t] == want, (col, t)


def test_a_board_no_variant_packs_reports_none(layout_of):
    assert layout_of(5, 5)["variant"] == -1
