// az_tower_x3b_parts.h — the ONE copy of the x3b scheme's arithmetic (az_tower_x3b.h: tiles T and X for channels 48, 49, one
// accumulator per tile holding 2048 x the conv), shared by az_tower_x3b_kernel, az_tower_x3c_kernel and az_tower_x3d_kernel.
// A board gets the same BITS from all three because every accumulator sees the MFMAs of x3b_mfma_main / _t / _x in pass order
// and every epilogue is x3b_epilogue_value: the kernels keep only their own SCHEDULE (which slot issues which pass, where the
// reads, DMA pieces and waits go) and their own stores.  Everything here is force-inlined straight-line code on registers.
#pragma once
#include "az_net_common.h"

constexpr float X3_INV_SPLIT = 1.0f / X3_WSCALE;

// ---- prologue of a column tile ---------------------------------------------------------------------------------------------
// the observation of global row grow (= board * HW + position, >= 0): channels past cin stay 0
__device__ __forceinline__ f32x4 x3b_load_obs(const TowerParams &p, int grow) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    int gb = grow / p.HW, pos = grow - gb * p.HW;
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (c < p.cin) v[c] = p.obs[((size_t)gb * p.cin + c) * p.HW + pos];
    return v;
}
// a = lrelu(bn1(x0)): octet 0 of the planes (the caller splits it with split4_planes and stores hi and lo)
__device__ __forceinline__ f32x4 x3b_input_planes(const TowerParams &p, const f32x4 &v) {
    f32x4 a;
#pragma unroll
    for (int c = 0; c < 4; c++) a[c] = c < p.cin ? lrelu(p.in_scale[c] * v[c] + p.in_shift[c]) : 0.f;
    return a;
}
// block 1's skip conv3(x0) in fp32, the four rows of one output-channel tile this lane holds: the start of the residual stream
__device__ __forceinline__ f32x4 x3b_skip(const f32x4 (&w)[4], const f32x4 &v) {
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; r++) x[r] = w[r][0] * v[0] + w[r][1] * v[1] + w[r][2] * v[2] + w[r][3] * v[3];
    return x;
}
// the initial accumulator: 2048 x conv 0's bias.  Tile T (TT, mt = 3): only channels 48, 49 (lanes q == 0, rows 0, 1) carry a
// bias; its other rows are lo / centre-tap rows
template <bool TT> __device__ __forceinline__ f32x4 x3b_bias0(const TowerParams &p, int mt, int q) {
    if constexpr (!TT) return *(const f32x4 *)(p.epi + 16 * mt + 4 * q) * X3_WSCALE;
    else {
        f32x4 b = q == 0 ? *(const f32x4 *)(p.epi + 48) * X3_WSCALE : (f32x4){0.f, 0.f, 0.f, 0.f};
        b[2] = b[3] = 0.f;
        return b;
    }
}

// ---- scratch destinations of tile X on a row-pair board (x3b, x3c; x3d reads them from the host's table) ---------------------
// Lane (q, l15) of tile X holds rows 4q..4q+3 = (plane 2q, c0), (2q, c1), (2q+1, c0), (2q+1, c1) at position (y, x) =
// (2 nt + (l15 >> 3), l15 & 7); plane t belongs to tap tap_of_plane(t) with d = (dy, dx): the value is a term of
// out[c, (y - dy, x - dx)].  Off-board destinations and padding lanes store to the trash slot.  Plane 8 = the centre tap (rows
// 4..7 of tile T, lanes q == 1).
template <int NT>
__device__ __forceinline__ void x3b_scratch_dst(const TowerParams &p, const int (&grow)[NT], int q, int l15, int s_wave, int trash, int (&sdst)[NT][2], int (&scen)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int y = 2 * nt + (l15 >> 3), x = l15 & 7;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int t = 2 * q + k, tap = X3B::tap_of_plane(t);
            const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
            const int yd = y - dy, xd = x - dx;
            const bool ok = grow[nt] >= 0 && yd >= 0 && yd < p.H && xd >= 0 && xd < p.W;
            sdst[nt][k] = ok ? s_wave + t * X3B::S_PLANE + (yd * 8 + xd) * 8 : trash;
        }
        scen[nt] = (q == 1 && grow[nt] >= 0) ? s_wave + 8 * X3B::S_PLANE + (nt * 16 + l15) * 8 : trash;
    }
}

// ---- the MFMAs of one accumulator in one k-step, by pass ----------------------------------------------------------------------
// The weights carry 2048 in both halves and the activations' lo half is unscaled, so hi'*hi, hi'*lo0 and lo*hi are all 2048 x
// their share of the product (az_net_common.h: split_pair_planes) and add into ONE accumulator.  A call is ONE MFMA; the order
// of the passes per accumulator and k-step is what "same bits" rests on, the slot a pass is issued in is the kernel's.
// the gather k-step's B operand, read dword by dword
__device__ __forceinline__ half8 x3b_gather_b(const unsigned (&sp)[4]) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(half8, (u32x4){sp[0], sp[1], sp[2], sp[3]});
}
// tiles 0..2: hi'*hi, hi'*lo0, lo*hi
template <int PASS> __device__ __forceinline__ void x3b_mfma_main(f32x4 &acc, const half8 &a_hi, const half8 &a_lo, const half8 &b_hi, const half8 &b_lo) {
    static_assert(PASS >= 0 && PASS < 3, "three passes");
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(PASS == 2 ? a_lo : a_hi, PASS == 1 ? b_lo : b_hi, acc, 0, 0, 0);
}
// tile T (hi rows and lo rows in one fragment): x B_hi, then x B_lo0
template <int PASS> __device__ __forceinline__ void x3b_mfma_t(f32x4 &acc, const half8 &a_t, const half8 &b_hi, const half8 &b_lo) {
    static_assert(PASS >= 0 && PASS < 2, "two passes");
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_t, PASS == 1 ? b_lo : b_hi, acc, 0, 0, 0);
}
// tile X (k-steps 6, 7): hi'*hi - from a literal zero at k-step 6 (FROM_ZERO) - then hi'*lo0, lo*hi
template <int PASS, bool FROM_ZERO> __device__ __forceinline__ void x3b_mfma_x(f32x4 &acc, const half8 &a_hi, const half8 &a_lo, const half8 &b_hi, const half8 &b_lo) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PASS == 0) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, FROM_ZERO ? zero4 : acc, 0, 0, 0);
    else x3b_mfma_main<PASS>(acc, a_hi, a_lo, b_hi, b_lo);
}

// ---- channels 48, 49 after k-step 7 ---------------------------------------------------------------------------------------------
// term I of a column tile: I < 4: row I of tile X, xv[I]; I = 4, 5: the centre tap of channel 48, 49, cv[I - 4] (lanes q == 1
// hold rows 4..7 of tile T: hi c0, hi c1, lo c0, lo c1).  One term at a time for the kernel that spreads them over MFMA slots.
template <int I> __device__ __forceinline__ void x3b_tx_term(const f32x4 &accx, const f32x4 &accT, f32x4 &xv, f32x2 &cv) {
    if constexpr (I < 4) xv[I] = accx[I] * X3_INV_SPLIT;
    else cv[I - 4] = (accT[I - 4] + accT[I - 2]) * X3_INV_SPLIT;
}
__device__ __forceinline__ void x3b_tx_terms(const f32x4 &accx, const f32x4 &accT, f32x4 &xv, f32x2 &cv) {
    static_for<6>([&](auto i_c) { x3b_tx_term<decltype(i_c)::value>(accx, accT, xv, cv); });
}
// the nine tap planes at a lane's position, summed in the order pl[0] + pl[1] + ... + pl[8]: step T of that sum
template <int T> __device__ __forceinline__ void x3b_add_plane(f32x2 &s, const f32x2 (&pl)[9]) {
    if constexpr (T == 0) s = pl[0];
    else s = s + pl[T];
}
__device__ __forceinline__ f32x2 x3b_sum_planes(const f32x2 (&pl)[9]) {
    f32x2 s;
    static_for<9>([&](auto t_c) { x3b_add_plane<decltype(t_c)::value>(s, pl); });
    return s;
}

// ---- epilogue of one (output tile, column tile) unit, in fp32 -------------------------------------------------------------------
// KIND 0: conv1, 1: conv2 (not last), 2: last conv.  TT: tile T - lanes q == 0 hold rows hi 48, hi 49, lo 48, lo 49 of the
// gather k-step (+ bias), s49 the sum of the tap planes; rows 4..15 are centre-tap rows / unused.  Scales the accumulator back
// (exactly: a power of two), reloads it with next_bias (2048 x the next conv's bias: scaled on the host), updates the residual
// stream, and returns the value the caller splits and stores: the next conv's activation (split4_planes), for KIND 2 the
// tower output (split4_f16x3).
template <int KIND, bool TT, bool IS_FIRST>
__device__ __forceinline__ f32x4 x3b_epilogue_value(f32x4 &acc, f32x4 &xres, const f32x2 &s49, const f32x4 &sc, const f32x4 &sh, const f32x4 &next_bias, int q) {
    const f32x4 a_in = acc;
    f32x4 v;
    if constexpr (!TT) {
        v = acc * X3_INV_SPLIT;
        acc = next_bias;
    } else {
        v = (f32x4){(acc[0] + acc[2]) * X3_INV_SPLIT, (acc[1] + acc[3]) * X3_INV_SPLIT, 0.f, 0.f};
        if constexpr (!IS_FIRST) {
            v[0] += s49[0];
            v[1] += s49[1];
        }
        if (q != 0) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        acc = q == 0 ? (f32x4){next_bias[0], next_bias[1], 0.f, 0.f} : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (KIND == 0) return __builtin_elementwise_max(v, v * 0.01f);
    else {
        // xres + a / 2048 in one instruction: a / 2048 is exact (a power of two; an accumulator of 2048 x a conv is nowhere near
        // underflow), so the fma has the bits of multiply-then-add
        f32x4 xv;
        if constexpr (!TT) xv = __builtin_elementwise_fma(a_in, (f32x4){X3_INV_SPLIT, X3_INV_SPLIT, X3_INV_SPLIT, X3_INV_SPLIT}, xres);
        else xv = xres + v;
        xres = xv;
        if constexpr (KIND == 2) return xv;
        else {
            const f32x4 t = __builtin_elementwise_fma(sc, xv, sh);
            return __builtin_elementwise_max(t, t * 0.01f);
        }
    }
}
