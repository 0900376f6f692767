// az_x3d_layout.h — column layout of az_tower_x3d_kernel (az_tower_x3d.h) for an H x W board: boards per workgroup, row stride,
// cells per board region, and the tables - which (board, position) is column 16 k + l15 of tile k, and for every column and tap
// plane the column that takes its tile-X term.
//
// Plain C++ (no HIP): az_net.hip builds the tables of a net with it, and tests/test_x3d_layout_host.py compiles it with g++.
//
// Board b's cells: b R + (y + 1) rs + x + 1.  R > H rs + W keeps every tap of every position inside the board or on a halo cell;
// (R, rs) - constants of the kernel variant - make the nb H W cells fall into the 16 residues mod 16 equally often; tile k takes
// the k-th position of every residue, lane l15 the one of residue l15.  WITHIN a residue the order is free, and it is chosen for the
// halo: the cells of board row 0 come first and those of row H - 1 last (in between, and within each class, board, position order).
// Every residue then starts with at least n_top row-0 cells and ends with at least n_bot row-(H - 1) cells, so tiles
// 0 .. n_top - 1 lie wholly on row 0 and tiles tiles - n_bot .. tiles - 1 wholly on row H - 1: the taps with dy = -1 (dy = +1) of
// such a tile read nothing but the zero halo row, and the kernel leaves those k-steps out (X3DS::tile_on).
#pragma once
#include <stdint.h>

#include <vector>

#ifndef AZ_X3D_DEAL
#define AZ_X3D_DEAL 1 // how the connect_four variant deals its pure tiles to the waves (az_tower_x3d.h: X3DV<2>); 0: it skips nothing
#endif
// cells per plane, column tiles per workgroup, row stride, cells per board region; skip_top / skip_bot: how many pure row-0 /
// row-(H - 1) tiles the kernel variant counts on (tiles 0 .. skip_top - 1, tiles - skip_bot .. tiles - 1): a board whose layout
// offers fewer does not take the variant
struct X3DVariant { int pc, tiles, rs, R, skip_top, skip_bot; };
constexpr int AZ_X3D_VARIANTS = 3;
constexpr X3DVariant az_x3d_variant(int v) {
    return v == 0 ? X3DVariant{480, 18, 8, 58, 0, 0} : v == 1 ? X3DVariant{416, 16, 9, 84, 0, 0} : X3DVariant{480, 21, 8, 57, AZ_X3D_DEAL ? 3 : 0, AZ_X3D_DEAL ? 3 : 0};
}
constexpr int az_x3d_tap_of_plane(int t) { return t < 4 ? t : t + 1; } // planes 0..7 = taps 0,1,2,3,5,6,7,8 (plane 8 = tap 4)

struct X3DLayout {
    int variant = -1, nb = 0, R = 0, rs = 0;
    int n_top = 0, n_bot = 0; // tiles 0 .. n_top - 1 hold only row-0 cells, tiles tiles - n_bot .. tiles - 1 only row-(H - 1) cells
    std::vector<uint16_t> pos, sdst; // [16 x tiles] board << 8 | position; [16 x tiles][8] destination column (0xFFFF: off the board)
    int top_tile(int i) const { return i; }
    int bot_tile(int i) const { return (int)pos.size() / 16 - n_bot + i; }
};

static inline int az_x3d_residue(int b, int pp, int W, int R, int rs) { return (b * R + (pp / W + 1) * rs + pp % W + 1) & 15; }

// the layout of variant v for an H x W board (variant = -1: the variant does not suit the board)
static inline X3DLayout x3d_layout_variant(int v, int H, int W) {
    X3DLayout out;
    const X3DVariant V = az_x3d_variant(v);
    const int HW = H * W, ncol = 16 * V.tiles;
    if (HW < 1 || HW > 255 || ncol % HW) return out;
    const int nb = ncol / HW;
    // (rs, R) are compile-time constants of the kernel variant: check that they suit THIS board - every tap of every position
    // inside the board or on a halo cell, the planes large enough, the residues flat
    const int rs = V.rs, R = V.R;
    if (rs < W + 1 || R < H * rs + W + 1 || (nb - 1) * R + (H + 1) * rs + W + 2 > V.pc) return out;
    // per residue: row-0 cells, the rest, row-(H - 1) cells - each in board, position order
    std::vector<uint16_t> cls[16][3];
    for (int b = 0; b < nb; b++)
        for (int pp = 0; pp < HW; pp++) {
            const int y = pp / W, c = H < 2 ? 1 : y == 0 ? 0 : y == H - 1 ? 2 : 1;
            cls[az_x3d_residue(b, pp, W, R, rs)][c].push_back((uint16_t)(b << 8 | pp));
        }
    int n_top = V.tiles, n_bot = V.tiles;
    for (int r = 0; r < 16; r++) {
        if ((int)(cls[r][0].size() + cls[r][1].size() + cls[r][2].size()) != V.tiles) return out;
        n_top = (int)cls[r][0].size() < n_top ? (int)cls[r][0].size() : n_top;
        n_bot = (int)cls[r][2].size() < n_bot ? (int)cls[r][2].size() : n_bot;
    }
    if (n_top < V.skip_top || n_bot < V.skip_bot) return out;
    out.variant = v, out.nb = nb, out.R = R, out.rs = rs, out.n_top = n_top, out.n_bot = n_bot;
    out.pos.assign(ncol, 0);
    std::vector<int> col_of((size_t)nb * HW, -1);
    for (int r = 0; r < 16; r++) {
        int k = 0;
        for (int c = 0; c < 3; c++)
            for (uint16_t e : cls[r][c]) {
                out.pos[k * 16 + r] = e;
                col_of[(size_t)(e >> 8) * HW + (e & 255)] = k * 16 + r;
                k++;
            }
    }
    out.sdst.assign((size_t)ncol * 8, 0xFFFF);
    for (int col = 0; col < ncol; col++) {
        const int b = out.pos[col] >> 8, pp = out.pos[col] & 255, y = pp / W, x = pp % W;
        for (int t = 0; t < 8; t++) { // plane t = tap tap_of_plane(t) with d = (dy, dx): this column's value is a term of out[position - d]
            const int tap = az_x3d_tap_of_plane(t), dy = tap / 3 - 1, dx = tap % 3 - 1, yd = y - dy, xd = x - dx;
            if (yd >= 0 && yd < H && xd >= 0 && xd < W) out.sdst[(size_t)col * 8 + t] = (uint16_t)col_of[(size_t)b * HW + yd * W + xd];
        }
    }
    return out;
}

// the first variant that suits the board
static inline X3DLayout x3d_layout(int H, int W) {
    for (int v = 0; v < AZ_X3D_VARIANTS; v++) {
        X3DLayout out = x3d_layout_variant(v, H, W);
        if (out.variant >= 0) return out;
    }
    return X3DLayout();
}
