// az_net_wide.h — the general layer-by-layer PV-net forward (az_net_wide.hip): parameters, constants and launchers shared with
// the host glue in az_net.hip (az_net_create_wide).  Internal; NOT part of the C ABI.
//
// One launch per 3x3 conv, an implicit GEMM on v_mfma_f32_16x16x32_f16: M = output channels, N = (board, position) columns,
// K = (channel chunk of 32, tap, channel) in that fixed order.  Between convs the activations live in HBM as [B][HW][Fpad]:
// the fp32 residual stream and the fp16 operand planes hi (+ lo for the fp32-grade variant).  A workgroup owns whole boards
// (WIDE_NT column tiles of 16, so the 3x3 halo never leaves it) and 64 or 128 output channels; its four waves own 16 or 32
// channels each and every column tile, and share the staged activations in LDS.
#pragma once
#include "az_net_common.h"

#define WIDE_NT 11                     // column tiles per workgroup: floor(176 / HW) whole boards (connect_four: 4 boards, 168 columns)
#define WIDE_ZR (16 * WIDE_NT)         // first of the 16 zero rows of a staged plane (taps off the board read them)
#define WIDE_PLANE_B ((WIDE_ZR + 16) * 64) // one staged plane: rows of 32 channels (64 B), octets swizzled by row (wide_swz)
#define WIDE_CIN0 32                   // channel stride of conv 0's input operand (the <= 4 input planes, zero padded)

struct WideConvParams {
    int W, HW, nbw, n_boards; // board width, cells; boards per workgroup; batch
    int cin, n_chunks;        // channel stride of the input operand (Fpad, or WIDE_CIN0 for conv 0); cin / 32
    int fpad, nmt;            // output channel stride; its 16-row tiles
    int mode;                 // WIDE_MODE_*
    const _Float16 *a_hi, *a_lo; // input operand [B][HW][cin] (a_lo: fp16(a - hi), unscaled)
    const _Float16 *w;        // [n_chunks][9 taps][nmt][hi, lo][64 lanes][8]
    const float *epi;         // [4][fpad]: 1 / (2048 s_co), bias, next bn1 scale, next bn1 shift
    float *x;                 // residual stream [B][HW][fpad]
    _Float16 *o_hi, *o_lo;    // output operand (WIDE_MODE_LAST: the tower output, lo x 2048)
};
#define WIDE_MODE_CONV1 0 // lrelu(conv + bias) -> operand
#define WIDE_MODE_CONV2 1 // x += conv + bias; lrelu(bn1_next(x)) -> operand
#define WIDE_MODE_LAST 2  // x + conv + bias -> tower output

struct WideInputParams {
    int HW, cin, fpad, n_boards;
    const float *obs;                 // [B][cin][HW]
    const float *in_scale, *in_shift; // block-1 bn1 over the input planes [cin]
    const float *skip_w;              // [fpad][4]: block-1 skip (1x1 conv, or identity)
    float *x;                         // residual stream [B][HW][fpad]
    _Float16 *a_hi, *a_lo;            // conv 0's operand [B][HW][WIDE_CIN0]
};

// lds: dynamic LDS bytes of the conv launch (wide_conv_lds)
hipError_t az_launch_wide_input(const WideInputParams &p, hipStream_t st);
hipError_t az_launch_wide_conv(int device, bool x3, const WideConvParams &p, hipStream_t st);
static inline int wide_conv_lds(bool x3) { return 2 * (x3 ? 2 : 1) * WIDE_PLANE_B; }
static inline int wide_mtw(int fpad) { return fpad > 64 ? 2 : 1; } // m-tiles per wave
