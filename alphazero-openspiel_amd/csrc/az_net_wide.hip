// az_net_wide.hip — the general PV-net forward for nets the tuned tower kernels cannot hold (more than 56 filters, conv
// weights of any magnitude, boards that do not fit their LDS): one launch per conv, activations in HBM between convs
// (az_net_wide.h).  Host glue: az_net_create_wide in az_net.hip.
#include "az_net_wide.h"

// Row r of a staged plane keeps its four 16-byte channel octets in the order o ^ wide_swz(r): with 16 consecutive rows per lane
// group, each of ds_read_b128's four lane groups then touches 16 distinct 16-byte bank slots (MI355X LDS lane groups).
__device__ __forceinline__ int wide_swz(int r) { return (-(r >> 2)) & 3; }

// conv 0's operand lrelu(bn1(obs)) (channels past the input planes zero) and the residual stream's start, the block-1 skip.
__global__ __launch_bounds__(256) void az_wide_input_kernel(WideInputParams p) {
    const int nq = p.fpad / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.n_boards * p.HW * nq) return;
    const long bp = idx / nq; // board * HW + position
    const int cq = (int)(idx % nq), b = (int)(bp / p.HW), pos = (int)(bp % p.HW);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < p.cin; c++) v[c] = p.obs[((size_t)b * p.cin + c) * p.HW + pos];
    f32x4 s;
    for (int j = 0; j < 4; j++) {
        float acc = 0.f;
        for (int c = 0; c < p.cin; c++) acc += p.skip_w[(4 * cq + j) * 4 + c] * v[c];
        s[j] = acc;
    }
    *(f32x4 *)(p.x + (size_t)bp * p.fpad + 4 * cq) = s;
    if (cq < WIDE_CIN0 / 4) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < 4; j++) {
            const int c = 4 * cq + j;
            if (c < p.cin) a[j] = lrelu(p.in_scale[c] * v[c] + p.in_shift[c]);
        }
        half4 hi, lo;
        split4_planes(a, hi, lo);
        *(half4 *)(p.a_hi + (size_t)bp * WIDE_CIN0 + 4 * cq) = hi;
        if (p.a_lo) *(half4 *)(p.a_lo + (size_t)bp * WIDE_CIN0 + 4 * cq) = lo;
    }
}

// X3: the fp32-grade variant (operands hi + lo, three MFMAs per product into one accumulator: hi' bh + hi' bl + lo' bh, the
// weights' halves both carrying 2048 s_co).  MTW: 16-row output tiles per wave.
template <bool X3, int MTW>
__global__ __launch_bounds__(256) void az_conv_wide_kernel(WideConvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int NPL = X3 ? 2 : 1; // staged planes per buffer
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, l15 = lane & 15;
    const int b0 = blockIdx.x * p.nbw;
    const int nb = p.n_boards - b0 < p.nbw ? p.n_boards - b0 : p.nbw;
    const int ncols = nb * p.HW, ntiles = (ncols + 15) >> 4;
    const int mt0 = (blockIdx.y * 4 + wave) * MTW;
    const bool active = mt0 < p.nmt; // (wave-uniform) a wave past the channel count only stages
    const size_t col0 = (size_t)b0 * p.HW;

    // zero rows of both buffers' planes
    for (int i = tid; i < 2 * NPL * 64; i += 256)
        *(f32x4 *)(lds + (i >> 6) * WIDE_PLANE_B + WIDE_ZR * 64 + (i & 63) * 16) = (f32x4){0.f, 0.f, 0.f, 0.f};
    // chunk c (32 channels) of the workgroup's columns -> buffer k, by LDS-DMA: one 16-row KiB piece per wave-instruction
    auto stage = [&](int c, int k) {
        for (int piece = wave; piece < NPL * ntiles; piece += 4) {
            const int pl = piece >= ntiles, t = piece - pl * ntiles;
            const int r = 16 * t + (lane >> 2), o = (lane & 3) ^ wide_swz(r);
            const int rr = r < ncols ? r : ncols - 1; // (rows past the boards are never read: any valid address)
            const _Float16 *src = (pl ? p.a_lo : p.a_hi) + (col0 + rr) * p.cin + 32 * c + 8 * o;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(lds + (k * NPL + pl) * WIDE_PLANE_B + t * 1024), 16, 0, 0);
        }
    };
    // per column tile: this lane's column | (taps whose source lies on the board) << 16
    unsigned tinfo[WIDE_NT];
#pragma unroll
    for (int t = 0; t < WIDE_NT; t++) {
        const int col = 16 * t + l15;
        unsigned m = 0;
        if (col < ncols) {
            const int pos = col % p.HW, y = pos / p.W, x = pos % p.W, H = p.HW / p.W;
            for (int tap = 0; tap < 9; tap++) {
                const int ys = y + tap / 3 - 1, xs = x + tap % 3 - 1;
                if (ys >= 0 && ys < H && xs >= 0 && xs < p.W) m |= 1u << tap;
            }
        }
        tinfo[t] = (unsigned)col | m << 16;
    }
    f32x4 acc[MTW][WIDE_NT];
#pragma unroll
    for (int i = 0; i < MTW; i++)
#pragma unroll
        for (int t = 0; t < WIDE_NT; t++) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nks = 9 * p.n_chunks;
    // A fragments of k-step kk (= chunk * 9 + tap) for this wave's tiles; the next k-step's are fetched during this one's MFMAs
    auto load_a = [&](int kk, half8 *ah, half8 *al) {
#pragma unroll
        for (int i = 0; i < MTW; i++) {
            const _Float16 *src = p.w + (((size_t)kk * p.nmt + mt0 + i) * 2) * 512 + lane * 8;
            ah[i] = *(const half8 *)src;
            if constexpr (X3) al[i] = *(const half8 *)(src + 512);
        }
    };
    half8 ah[MTW], al[MTW], nah[MTW], nal[MTW];
    if (active) load_a(0, ah, al);
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kk = 0; kk < nks; kk++) {
        const int c = kk / 9, tap = kk - 9 * c;
        if (tap == 0 && c + 1 < p.n_chunks) stage(c + 1, (c + 1) & 1);
        if (active) {
            if (kk + 1 < nks) load_a(kk + 1, nah, nal);
            const unsigned char *buf = lds + (c & 1) * NPL * WIDE_PLANE_B;
            const int shift = (tap / 3 - 1) * p.W + (tap % 3 - 1);
#pragma unroll
            for (int t = 0; t < WIDE_NT; t++) {
                if (t < ntiles) {
                    const int r = (tinfo[t] >> (16 + tap)) & 1 ? (int)(tinfo[t] & 0xFFFF) + shift : WIDE_ZR;
                    const int off = r * 64 + 16 * (q ^ wide_swz(r));
                    const half8 bh = *(const half8 *)(buf + off);
                    half8 bl;
                    if constexpr (X3) bl = *(const half8 *)(buf + WIDE_PLANE_B + off);
#pragma unroll
                    for (int i = 0; i < MTW; i++) {
                        acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i][t], 0, 0, 0);
                        if constexpr (X3) {
                            acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i][t], 0, 0, 0);
                            acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i][t], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < MTW; i++) {
                ah[i] = nah[i];
                if constexpr (X3) al[i] = nal[i];
            }
        }
        if (tap == 8 && c + 1 < p.n_chunks) { // the next chunk has landed and everybody is done with this one
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (!active) return;
    // epilogue: lane (q, l15) holds channels 16 mt + 4 q .. + 3 of column 16 t + l15
#pragma unroll
    for (int i = 0; i < MTW; i++) {
        const int co = 16 * (mt0 + i) + 4 * q;
        const f32x4 inv = *(const f32x4 *)(p.epi + co), bias = *(const f32x4 *)(p.epi + p.fpad + co);
        const f32x4 sc = *(const f32x4 *)(p.epi + 2 * p.fpad + co), sh = *(const f32x4 *)(p.epi + 3 * p.fpad + co);
#pragma unroll
        for (int t = 0; t < WIDE_NT; t++) {
            const int col = 16 * t + l15;
            if (t >= ntiles || col >= ncols) continue;
            const size_t g = (col0 + col) * p.fpad + co;
            const f32x4 v = acc[i][t] * inv + bias; // (acc * inv is exact: a power of two)
            f32x4 a;
            if (p.mode == WIDE_MODE_CONV1) {
                for (int j = 0; j < 4; j++) a[j] = lrelu(v[j]);
            } else {
                const f32x4 xn = *(const f32x4 *)(p.x + g) + v;
                if (p.mode == WIDE_MODE_LAST) { // the tower output: hi, lo x 2048 (what the head kernels read)
                    half4 hi, lo;
                    if constexpr (X3) {
                        split4_f16x3(xn, hi, lo);
                        *(half4 *)(p.o_lo + g) = lo;
                    } else
                        for (int j = 0; j < 4; j++) hi[j] = (_Float16)xn[j];
                    *(half4 *)(p.o_hi + g) = hi;
                    continue;
                }
                *(f32x4 *)(p.x + g) = xn;
                for (int j = 0; j < 4; j++) a[j] = lrelu(xn[j] * sc[j] + sh[j]);
            }
            half4 hi, lo;
            split4_planes(a, hi, lo);
            *(half4 *)(p.o_hi + g) = hi;
            if constexpr (X3) *(half4 *)(p.o_lo + g) = lo;
        }
    }
}

hipError_t az_launch_wide_input(const WideInputParams &p, hipStream_t st) {
    const long n = (long)p.n_boards * p.HW * (p.fpad / 4);
    hipLaunchKernelGGL(az_wide_input_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    return hipGetLastError();
}

template <bool X3, int MTW> static hipError_t launch_conv(int dv, const WideConvParams &p, hipStream_t st) {
    static bool attr[AZ_MAX_DEVICES] = {false};
    if (dv < 0 || dv >= AZ_MAX_DEVICES || !attr[dv]) {
        hipError_t s = hipFuncSetAttribute((const void *)az_conv_wide_kernel<X3, MTW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           wide_conv_lds(X3));
        if (s != hipSuccess) return s;
        if (dv >= 0 && dv < AZ_MAX_DEVICES) attr[dv] = true;
    }
    const int mb = (p.nmt + 4 * MTW - 1) / (4 * MTW);
    hipLaunchKernelGGL((az_conv_wide_kernel<X3, MTW>), dim3((p.n_boards + p.nbw - 1) / p.nbw, mb), dim3(256), wide_conv_lds(X3), st, p);
    return hipGetLastError();
}
hipError_t az_launch_wide_conv(int device, bool x3, const WideConvParams &p, hipStream_t st) {
    const int mtw = wide_mtw(p.fpad);
    if (x3) return mtw == 2 ? launch_conv<true, 2>(device, p, st) : launch_conv<true, 1>(device, p, st);
    return mtw == 2 ? launch_conv<false, 2>(device, p, st) : launch_conv<false, 1>(device, p, st);
}
