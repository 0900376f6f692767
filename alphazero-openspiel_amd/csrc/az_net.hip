// az_net.hip — the host side of the fused PV-net forward: the C ABI of include/az_net.h.  No kernels live here.
//
// Reference computation: Net.forward / ResidualBlock.forward (network.py) in eval mode.  Two create paths fill one az_net:
//   * az_net_create takes the layouts packed by fusednet.pack_net (<= 56 filters; fp16, or split-fp16 hi / lo pairs for the
//     fp32-grade precision), re-groups them into the weight streams of the tuned tower kernels and records the net's scheme:
//     which of those kernels can run it;
//   * az_net_create_wide takes plain folded fp32 arrays (up to 256 filters, any finite weight) for the general layer-by-layer
//     path (az_net_wide.h), which runs the nets that pack_net or az_net_create refuse.
// plan_forward picks, from the scheme and the batch size alone, the tower kernel of a forward and its launch shape;
// az_net_forward launches it (then the head, unless the tower kernel ran fc1 itself), and az_net_kernel_label and
// az_net_issued_mfma_per_board describe that same plan.
//
// Kernels: az_tower_f16.h, az_tower_f16c.h (fp16 operands), az_tower_x3.h, az_tower_x3b.h, az_tower_x3c.h, az_tower_x3d.h
// (split-fp16 operands: fp32-grade), az_net_wide.h, az_head.h and az_head_fused.h (fc1 + softmax + tanh); shared types and
// launch parameters: az_net_common.h, az_head_params.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include <string>
#include <vector>

#include "../../include/az_engine.h"
#include "../../include/az_net.h"

#include "az_net_common.h"
#include "az_head_params.h"
#include "az_net_wide.h"

#define AZ_X3C_MAX_BOARDS 512 // (set from profiles/r3_tower_vs_boards.txt)
#define AZ_F16C_MAX_BOARDS 512 // the same for the f16 tower (az_tower_f16c.h)
#define AZ_X3C_ONE_PER_WG 256 // up to here a board per workgroup fills fewer CUs than the chip has; above, two boards per workgroup (39 vs 49 us at 512 boards)

// Which tower kernels can run a net, fixed at create; plan_forward picks among them by batch size.
enum class NetScheme {
    F16,     // az_tower_kernel
    F16C,    // az_tower_f16c_kernel up to AZ_F16C_MAX_BOARDS boards, az_tower_kernel above (row-pair board of <= 6 rows, <= 50 filters)
    X3,      // az_tower_x3_kernel
    X3B,     // row-pair board with <= 50 filters: az_tower_x3c_kernel up to AZ_X3C_MAX_BOARDS boards, az_tower_x3b_kernel above
    X3B_X3D, // the same, and the positions pack into whole column tiles: az_tower_x3d_kernel above 128 x xd_nb boards
    X3D,     // the positions pack into whole column tiles, not a row-pair board (8x8): az_tower_x3d_kernel
    WIDE,    // az_net_create_wide: az_conv_wide_kernel per conv
};
// The tower kernel of one forward.  X3C_FUSED_HEAD: az_tower_x3c_kernel also runs fc1 + softmax + tanh for its boards.
enum class TowerKind { F16, F16C, X3, X3B, X3C, X3C_FUSED_HEAD, X3D, WIDE };
constexpr int N_TOWER_KINDS = 8;
// az_net_kernel_label's name of each kind's tower launch (kind_label: + the head kernels, and the conv count of WIDE)
static const char *const TOWER_NAME[N_TOWER_KINDS] = {
    "az_tower_kernel", "az_tower_f16c_kernel", "az_tower_x3_kernel", "az_tower_x3b_kernel", "az_tower_x3c_kernel",
    "az_tower_x3c_kernel (fc1 + softmax + tanh in the same launch)", "az_tower_x3d_kernel", "az_wide_input_kernel + az_conv_wide_kernel"};

// ================================================================================================
struct az_net {
    az_net_desc d;
    std::string err;
    NetScheme scheme = NetScheme::F16;
    _Float16 *conv_w = nullptr, *fc_w = nullptr, *xout = nullptr;
    _Float16 *fc_w_lo = nullptr, *xout_lo = nullptr; // f16x3 only
    float *epi = nullptr, *fc_b = nullptr, *skip_w = nullptr, *logits = nullptr;
    int xc = AZ_NET_XOUT_C, fc_ksteps = 0; // channel stride of xout / k-steps of fc1 (az_net_create)
    float in_affine[16];
    int max_boards = 0;
    int bpw_max = 0, lds_head = 0, n_ot = 0;
    int r3 = 16;                  // 2: <= 50 filters, output-channel tile 3 holds two stored rows (a template argument of the kernels)
    int precision = AZ_NET_PREC_F16;
    // az_tower_x3d_kernel (schemes X3B_X3D, X3D): its variant, boards per workgroup, cells per board region, row stride
    int xd_variant = -1, xd_nb = 0, xd_R = 0, xd_rs = 0;
    _Float16 *conv_w_d = nullptr; // the x3d weight stream (conv_w keeps the stream of the small-batch / fallback kernel)
    uint16_t *xd_pos = nullptr, *xd_sdst = nullptr;
    // the general layer-by-layer path (az_net_create_wide, az_net_wide.h); d then holds the geometry only
    int fpad = 0, nbw = 0;
    std::vector<size_t> w_off;                   // halves from w_wide to conv c's weight stream
    _Float16 *w_wide = nullptr;                  // every conv's [n_chunks][9][nmt][hi, lo][64][8]
    float *epi_wide = nullptr, *in_wide = nullptr; // [n_convs][4][fpad]; [in_scale 4][in_shift 4][skip fpad x 4]
    float *x_wide = nullptr;                     // residual stream [max_boards][HW][fpad]
    _Float16 *opa_hi = nullptr, *opa_lo = nullptr, *opb_hi = nullptr, *opb_lo = nullptr; // operand planes (opb: conv 0's input, then the tower output)
    std::string labels[N_TOWER_KINDS];           // az_net_kernel_label of each kind (finish_create)
};
static std::string g_net_err;

#define NCHK(n, call)                                                        \
    do {                                                                     \
        hipError_t _s = (call);                                              \
        if (_s != hipSuccess) {                                              \
            (n)->err = std::string(#call) + ": " + hipGetErrorString(_s);    \
            return AZ_E_HIP;                                                 \
        }                                                                    \
    } while (0)

extern "C" const char *az_net_last_error(const az_net *n) { return n ? n->err.c_str() : g_net_err.c_str(); }

extern "C" int az_net_destroy(az_net *n) {
    if (!n) return AZ_OK;
    (void)hipSetDevice(n->d.device);
    void *bufs[] = {n->conv_w, n->fc_w,   n->fc_w_lo, n->xout,   n->xout_lo,  n->epi,    n->fc_b,   n->skip_w, n->logits, n->conv_w_d,
                    n->xd_pos, n->xd_sdst, n->w_wide, n->epi_wide, n->in_wide, n->x_wide, n->opa_hi, n->opa_lo, n->opb_hi, n->opb_lo};
    for (void *b : bufs) (void)hipFree(b);
    delete n;
    return AZ_OK;
}

// geometry of one launch: boards per wave, column tiles per wave, k-steps per weight chunk, waves per workgroup, the cell grid
// (az_net_common.h: TowerParams) and the LDS layout
struct TowerGeom {
    int bpw, nt, ck, waves, rcells, zcell, rs, tpb, cells, off_epi, off_act, lds;
    bool rp1; // f16x3: a row-pair board whose lo planes sit at the compile-time distance X3_LOFF_RP1
};
// the f16 tower for a given boards-per-wave
static TowerGeom tower_geom(int bpw, int waves, int H, int W) {
    TowerGeom g = {};
    g.bpw = bpw;
    if (W <= 7) { // row-pair tiles at row stride 8 (conflict-free B reads)
        g.rs = 8;
        g.tpb = (H + 1) / 2;
        g.nt = bpw * g.tpb;
    } else {
        g.rs = W + 1;
        g.tpb = 0;
        g.nt = (bpw * H * W + 15) / 16;
    }
    g.cells = (H + 2) * g.rs + 1;
    int zpad = 2 * (g.rs + 1) + 1;
    g.rcells = (bpw * g.cells + zpad + 15) & ~15;
    g.zcell = bpw * g.cells + (g.rs + 1);
    int wave_act = N_OCT * g.rcells * OCT_B;
    // waves = 8 (512 threads): small tiles only (<= 256 registers/wave), 2 waves per SIMD, so one wave's epilogue / waits
    // overlap another's MFMAs, and the eight share ONE weight stream (two co-resident 4-wave workgroups each pull their
    // own: at 1 board per wave that is ~25 TB/s of L2 reads chip-wide).
    g.waves = waves;
    int act = g.waves * wave_act;
    // 32 KiB weight chunks (half the barriers) when LDS allows; not with 8 waves: the longer unrolled body spills there
    g.ck = (act + 6144 + 2 * 8 * 4096 <= 160 * 1024) ? 8 : 4; // 32 KiB chunks (half the barriers) when LDS allows

    g.off_epi = 2 * g.ck * 4096;
    g.off_act = g.off_epi + 2048 + 8 * 64 * 8; // epilogue ring (2 KiB) + trash slots (8 B per thread, up to 512 threads)
    g.lds = g.off_act + act;
    return g;
}

// bytes of one k-step record of the record streams (conv_stream): output-channel tiles 0..2 + the stored rows of tile 3
static int record_bytes(int r3) { return 3 * 1024 + 4 * (r3 < 16 ? r3 + 1 : 16) * 16; }

// geometry of the f16x3 tower: one board per wave (the cell grid of the f16 tower's), 4 waves, 4-k-step chunks of (hi, lo) records
static TowerGeom x3_geom(int H, int W, int r3) {
    TowerGeom g = tower_geom(1, 4, H, W);
    g.ck = 4;
    g.rp1 = g.tpb && g.rs == 8 && g.tpb <= 3 && g.rcells <= 96;
    const int lo_off = g.rp1 ? X3_LOFF_RP1 : N_OCT * g.rcells * OCT_B;
    const int chunk_s = (4 * 2 * record_bytes(r3) + 1023) & ~1023;
    g.off_epi = 2 * chunk_s;
    g.off_act = g.off_epi + 2048 + 256 * 16;
    g.lds = g.off_act + 4 * 2 * lo_off;
    if (g.nt < 3) g.nt = 3;
    return g;
}

// fp16 bits of conv c's weight W[co][tap][ch] in the interchange (ABI) layout: group g = tap * 7 + ch / 8, element ch % 8
static inline uint16_t abi_weight(const uint16_t *src, int c, int co, int tap, int ch) {
    const int g = tap * 7 + (ch >> 3), oks = g >> 2, olane = (g & 3) * 16 + (co & 15), mt = co >> 4;
    return src[(size_t)c * AZ_NET_KSTEPS * 2048 + ((((size_t)oks * 4 + mt) * 64 + olane) * 8) + (ch & 7)];
}

// K grouping of the device weight streams: which weight is element j of group q (= lane >> 4) of k-step ks of conv c - its tap
// and input channel, or false: a zero.  Conv 0 sees the input planes only (channel octet 0): group g = 4 ks + q < 9 = tap g.
// The 15-k-step convs (<= 50 filters): group g < 54: (tap, octet) = divmod(g, 6), the 48 channels of six full octets; 54, 55:
// zero; k-step 14, the gather k-step: element j of group q < 3 is channel 48 + (j & 1) at tap 4 q + j / 2 (taps > 8: zero).
static bool k_group(int c, int ks, int q, int j, int &tap, int &ch) {
    const int g = 4 * ks + q;
    if (c == 0) tap = g, ch = j;
    else if (ks < X3B::NKS - 1) tap = g / 6, ch = 8 * (g % 6) + j;
    else tap = 4 * q + (j >> 1), ch = 48 + (j & 1);
    return (c && ks == X3B::NKS - 1) ? (q < 3 && tap < 9) : g < (c ? 54 : 9);
}
// its fp16 bits for output channel co, from the interchange layout
static inline uint16_t grouped_weight(const uint16_t *src, int c, int co, int ks, int q, int j) {
    int tap, ch;
    return k_group(c, ks, q, j, tap, ch) ? abi_weight(src, c, co, tap, ch) : 0;
}

// Device weight stream of az_tower_kernel, az_tower_f16c_kernel and az_tower_x3_kernel: [conv 0 compacted to AZ_NET_K0STEPS
// k-steps][conv 1 ..][..], one RECORD per k-step: output-channel tiles 0..2 as in the ABI layout (3 KiB), tile 3 with only its
// stored rows (see WRec).  Conv 0's ABI groups 7 * tap become groups 0..8 of its 4 k-steps.  <= 50 filters (r3 < 16): the K
// dimension is re-grouped into 15 k-steps - channels 48, 49 of the nine taps fit ONE k-step instead of filling the seventh
// channel octet of every tap (k_group).
static void build_records(const unsigned char *src, int r3, int n_convs, std::vector<unsigned char> &dev) {
    const bool l15 = r3 < 16;
    const int nks = l15 ? 15 : AZ_NET_KSTEPS;
    const int rows = r3 < 16 ? r3 + 1 : 16, rec = record_bytes(r3);
    const size_t conv_b = (size_t)AZ_NET_KSTEPS * 4096;
    const size_t n_rec = (size_t)AZ_NET_K0STEPS + (size_t)(n_convs - 1) * nks;
    dev.assign(n_rec * rec, 0);
    auto put_record = [&](unsigned char *dst, const unsigned char *ks4k) { // ks4k: [4 mt][64 lanes][16 B]
        memcpy(dst, ks4k, 3 * 1024);
        for (int q = 0; q < 4; q++)
            for (int r = 0; r < (r3 < 16 ? r3 : 16); r++)
                memcpy(dst + 3 * 1024 + (q * rows + r) * 16, ks4k + 3 * 1024 + (q * 16 + r) * 16, 16);
    };
    std::vector<uint16_t> k4(4096 / 2);
    auto put_grouped = [&](unsigned char *dst, int c, int ks) { // k-step ks of conv c in k_group's grouping
        for (int mt = 0; mt < 4; mt++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++)
                    k4[((size_t)mt * 64 + lane) * 8 + j] = grouped_weight((const uint16_t *)src, c, 16 * mt + (lane & 15), ks, lane >> 4, j);
        put_record(dst, (const unsigned char *)k4.data());
    };
    size_t off = 0;
    for (int ks = 0; ks < AZ_NET_K0STEPS; ks++, off += rec) put_grouped(&dev[off], 0, ks);
    for (int c = 1; c < n_convs; c++)
        for (int ks = 0; ks < nks; ks++, off += rec) {
            if (l15) put_grouped(&dev[off], c, ks);
            else put_record(&dev[off], src + (size_t)c * conv_b + (size_t)ks * 4096);
        }
}
// the records of conv_w (f16x3: per k-step the hi record, then the lo record) + a chunk of padding: the last (short) chunk is
// fetched at full length
static std::vector<unsigned char> conv_stream(const az_net_desc &d, int r3) {
    const int n_convs = 2 * d.n_blocks;
    const size_t pad = 2 * 8 * 4096 + 1024, rec = record_bytes(r3);
    std::vector<unsigned char> hi, lo, dev;
    build_records((const unsigned char *)d.conv_w, r3, n_convs, hi);
    if (d.precision != AZ_NET_PREC_F16X3) {
        hi.resize(hi.size() + pad, 0);
        return hi;
    }
    build_records((const unsigned char *)d.conv_w_lo, r3, n_convs, lo);
    const size_t n_rec = hi.size() / rec;
    dev.assign(2 * n_rec * rec + pad, 0);
    for (size_t r = 0; r < n_rec; r++) {
        memcpy(&dev[2 * r * rec], &hi[r * rec], rec);
        memcpy(&dev[(2 * r + 1) * rec], &lo[r * rec], rec);
    }
    return dev;
}

// Device weight streams of the kernels on the x3b scheme (meaning of tiles T and X: az_tower_x3b.h).  A conv is cut into parts
// (= LDS chunks): the part's k-step records [hi mt 0..2][lo mt 0..2], then the extra fragments of its k-steps in k-step order -
// conv 0: T of every k-step; conv c >= 1: T, Xhi, Xlo of k-steps 6 and 7, T of the gather k-step 14.
//   az_tower_x3b_kernel / az_tower_x3c_kernel (struct X3B): conv 0 = one part; conv c >= 1 = k-steps [0,4) [4,8) [8,12) [12,15)
//   az_tower_x3d_kernel (struct X3D):                        conv 0 = [0,2) [2,4); conv c >= 1 = [0,3) [3,6) [6,8) [8,11) [11,14) [14]
struct X3Stream {
    int n_parts0, ks0_0[2], ks1_0[2];
    size_t off_0[2], c0_b;
    int n_parts, ks0[6], ks1[6];
    size_t off[6], conv_b;
};
static X3Stream x3b_stream_layout() {
    X3Stream L = {};
    L.n_parts0 = 1, L.ks0_0[0] = 0, L.ks1_0[0] = AZ_NET_K0STEPS, L.off_0[0] = 0, L.c0_b = X3B::C0_B;
    L.n_parts = X3B::PARTS, L.conv_b = X3B::CONV_B;
    for (int part = 0; part < X3B::PARTS; part++) {
        L.ks0[part] = part * X3B::CK;
        L.ks1[part] = L.ks0[part] + X3B::CK < X3B::NKS ? L.ks0[part] + X3B::CK : X3B::NKS;
        L.off[part] = X3B::part_off(part);
    }
    return L;
}
static X3Stream x3d_stream_layout() {
    X3Stream L = {};
    L.n_parts0 = X3D::PARTS0, L.c0_b = X3D::C0_B;
    for (int part = 0; part < X3D::PARTS0; part++) L.ks0_0[part] = 2 * part, L.ks1_0[part] = 2 * part + 2, L.off_0[part] = (size_t)part * X3D::C0_PART_B;
    L.n_parts = X3D::PARTS, L.conv_b = X3D::CONV_B;
    for (int part = 0; part < X3D::PARTS; part++)
        L.ks0[part] = X3D::part_ks0(part), L.ks1[part] = X3D::part_ks0(part) + X3D::part_len(part), L.off[part] = X3D::part_off(part);
    return L;
}
// The hi halves go into these streams x 2048 (X3_WSCALE; the lo halves carry that factor in the interchange format already): with
// the activations' lo half unscaled between convs, every product of a split-fp16 multiply is then 2048 x its share and ONE
// accumulator takes all three (az_net_common.h: split_pair_planes).  Exact (a power of two) unless |w| >= 32: -> false.
static bool build_x3_stream(const X3Stream &L, const uint16_t *hi_abi, const uint16_t *lo, int n_convs, std::vector<unsigned char> &dev) {
    std::vector<uint16_t> hi_scaled((size_t)n_convs * AZ_NET_KSTEPS * 2048);
    for (size_t i = 0; i < hi_scaled.size(); i++) {
        _Float16 h;
        memcpy(&h, &hi_abi[i], 2);
        const float f = (float)h * 2048.0f;
        if (!(f > -65520.0f && f < 65520.0f)) return false;
        h = (_Float16)f;
        memcpy(&hi_scaled[i], &h, 2);
    }
    const uint16_t *hi = hi_scaled.data();
    // (+ two convs of zero padding: the kernels' fetch of "chunk + 2" is unconditional)
    dev.assign(L.c0_b + (size_t)(n_convs - 1) * L.conv_b + 2 * L.conv_b, 0);
    constexpr int FR = X3B::FR, REC2 = X3B::REC2;
    // one fragment: 64 lanes x 8 fp16; f(q, l15, j) -> bits
    auto put_frag = [&](size_t off, auto f) {
        uint16_t *o = (uint16_t *)&dev[off];
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 8; j++) o[lane * 8 + j] = f(lane >> 4, lane & 15, j);
    };
    auto put_record = [&](size_t off, int c, int ks) { // [hi mt 0..2][lo mt 0..2]
        for (int part = 0; part < 2; part++)
            for (int mt = 0; mt < 3; mt++)
                put_frag(off + (size_t)(part * 3 + mt) * FR,
                         [&](int q, int l, int j) { return grouped_weight(part ? lo : hi, c, 16 * mt + l, ks, q, j); });
    };
    // tile T: rows 0..3 = hi 48, hi 49, lo 48, lo 49 of a shifted-B k-step (conv 0's k-steps, the gather k-step);
    //         rows 4..7 = hi 48, hi 49, lo 48, lo 49 of the centre tap over input channels 0..47 (k-steps 6, 7)
    auto put_t = [&](size_t off, int c, int ks) {
        put_frag(off, [&](int q, int l, int j) -> uint16_t {
            const bool centre = c > 0 && (ks == 6 || ks == 7);
            const int l0 = centre ? 4 : 0;
            if (l < l0 || l >= l0 + 4) return 0;
            const uint16_t *src = (l - l0) < 2 ? hi : lo;
            const int co = 48 + ((l - l0) & 1);
            if (!centre) return grouped_weight(src, c, co, ks, q, j);
            const int gp = 4 * ks + q; // groups 24..29 = (tap 4, octet 0..5); 30, 31 belong to tap 5: zero rows here
            return gp < 30 ? abi_weight(src, c, co, 4, 8 * (gp - 24) + j) : 0;
        });
    };
    // tile X (k-steps 6, 7): row 2 t + cc = channel 48 + cc at tap tap_of_plane(t), over input channels 0..47, unshifted B
    auto put_x = [&](size_t off, int c, int ks, const uint16_t *src) {
        put_frag(off, [&](int q, int l, int j) -> uint16_t {
            const int gp = 4 * ks + q;
            return gp < 30 ? abi_weight(src, c, 48 + (l & 1), X3B::tap_of_plane(l >> 1), 8 * (gp - 24) + j) : 0;
        });
    };
    for (int part = 0; part < L.n_parts0; part++) {
        size_t off = L.off_0[part];
        for (int ks = L.ks0_0[part]; ks < L.ks1_0[part]; ks++, off += REC2) put_record(off, 0, ks);
        for (int ks = L.ks0_0[part]; ks < L.ks1_0[part]; ks++, off += FR) put_t(off, 0, ks);
    }
    for (int c = 1; c < n_convs; c++) {
        const size_t base = L.c0_b + (size_t)(c - 1) * L.conv_b;
        for (int part = 0; part < L.n_parts; part++) {
            size_t off = base + L.off[part];
            for (int ks = L.ks0[part]; ks < L.ks1[part]; ks++, off += REC2) put_record(off, c, ks);
            for (int ks = L.ks0[part]; ks < L.ks1[part]; ks++) {
                if (ks == 6 || ks == 7) {
                    put_t(off, c, ks);
                    put_x(off + FR, c, ks, hi);
                    put_x(off + 2 * FR, c, ks, lo);
                    off += 3 * FR;
                } else if (ks == X3B::NKS - 1) {
                    put_t(off, c, ks);
                    off += FR;
                }
            }
        }
    }
    return true;
}

// Column layout of az_tower_x3d_kernel (az_tower_x3d.h): x3d_layout, az_x3d_layout.h (plain C++, also built on the host by
// tests/test_x3d_layout_host.py).
static_assert(az_x3d_tap_of_plane(0) == X3D::tap_of_plane(0) && az_x3d_tap_of_plane(3) == X3D::tap_of_plane(3) && az_x3d_tap_of_plane(4) == X3D::tap_of_plane(4) &&
                  az_x3d_tap_of_plane(7) == X3D::tap_of_plane(7),
              "az_x3d_layout.h and az_net_common.h number the tap planes alike");

// fc1 of the ABI layout (AZ_NET_XOUT_C channels per cell) -> xc channels per cell: [ot][k-step][lane][8], k = 32 ks + 8 (lane >> 4) + e,
// row lane & 15
static std::vector<uint16_t> repack_fc(const uint16_t *src, int n_ot, int fc_ksteps, int HW, int xc) {
    const int ks64 = HW * AZ_NET_XOUT_C / 32;
    std::vector<uint16_t> dst((size_t)n_ot * fc_ksteps * 64 * 8, 0);
    for (int ot = 0; ot < n_ot; ot++)
        for (int ks = 0; ks < fc_ksteps; ks++)
            for (int lane = 0; lane < 64; lane++)
                for (int e = 0; e < 8; e++) {
                    const int k = 32 * ks + 8 * (lane >> 4) + e;
                    if (k >= HW * xc) continue;
                    const int k64 = (k / xc) * AZ_NET_XOUT_C + k % xc;
                    dst[(((size_t)ot * fc_ksteps + ks) * 64 + lane) * 8 + e] =
                        src[(((size_t)ot * ks64 + k64 / 32) * 64 + ((k64 % 32) / 8) * 16 + (lane & 15)) * 8 + k64 % 8];
                }
    return dst;
}

// v_mfma instructions of one column tile in a conv on the x3b scheme (conv 0 / a later conv): what its k-steps multiply (X3BK)
template <bool IS_FIRST> static constexpr int x3b_mfma_per_tile() {
    int n = 0;
    for (int ks = 0; ks < X3BK<IS_FIRST, 1>::NKSC; ks++) n += X3BK<IS_FIRST, 1>::n_mfma(ks);
    return n;
}
static_assert(x3b_mfma_per_tile<false>() == 147, "az_tower_x3b.h: 147 against 180");
// v_mfma instructions one wave (= one board) of az_tower_x3_kernel issues (az_tower_x3.h: 3 per product, every tile)
static double x3_mfma_per_wave(int nt, int n_convs, int nks) { return 3.0 * (AZ_NET_K0STEPS + (double)(n_convs - 1) * nks) * 4 * nt; }

// the head kernels of a forward, as az_net_kernel_label names them
static std::string head_label(const az_net *n) {
    const std::string t = n->precision == AZ_NET_PREC_F16X3 ? "<X3>" : "";
    return n->n_ot > OTG ? "az_head_gemm_kernel" + t + " + az_head_softmax_kernel" + t : "az_head_kernel" + t;
}
static std::string kind_label(const az_net *n, TowerKind k) {
    std::string s = TOWER_NAME[(int)k];
    if (k == TowerKind::WIDE) s += std::string(n->precision == AZ_NET_PREC_F16X3 ? "<X3>" : "<F16>") + " x" + std::to_string(2 * n->d.n_blocks);
    return k == TowerKind::X3C_FUSED_HEAD ? s : s + " + " + head_label(n);
}

// ---- what the two create paths share -----------------------------------------------------------------------------------------
template <class Desc> static int check_args(const Desc *desc, az_net **out, const char *desc_name) {
    if (!desc || !out) {
        g_net_err = "null argument";
        return AZ_E_INVALID;
    }
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(Desc)) {
        g_net_err = std::string(desc_name) + ".struct_size mismatch";
        return AZ_E_INVALID;
    }
    return AZ_OK;
}
// once the description passed the path's own checks: the device, and a fresh net on it
static int new_net(int device, az_net **n) {
    const hipError_t s = hipSetDevice(device);
    if (s != hipSuccess) {
        g_net_err = std::string("hipSetDevice: ") + hipGetErrorString(s);
        return AZ_E_HIP;
    }
    *n = new az_net();
    return AZ_OK;
}
// hipMalloc + hipMemcpy of host-built buffers into the net; the first failure sticks (later uploads are skipped)
struct Upload {
    int rc = AZ_OK;
    void fail(int code, const char *msg) {
        if (rc != AZ_OK) return;
        g_net_err = msg;
        rc = code;
    }
    template <class T> void operator()(T *&dst, const void *src, size_t bytes) {
        if (rc == AZ_OK && (hipMalloc((void **)&dst, bytes) != hipSuccess || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess))
            fail(AZ_E_NOMEM, "hipMalloc/hipMemcpy of the net's weights failed");
    }
};
// the end of both create paths: a failed upload frees the net and everything uploaded so far
static int finish_create(az_net *n, const Upload &up, az_net **out) {
    if (up.rc != AZ_OK) {
        az_net_destroy(n);
        return up.rc;
    }
    for (int k = 0; k < N_TOWER_KINDS; k++) n->labels[k] = kind_label(n, (TowerKind)k);
    *out = n;
    return AZ_OK;
}

extern "C" int az_net_create(const az_net_desc *desc, az_net **out) {
    if (int rc = check_args(desc, out, "az_net_desc")) return rc;
    const az_net_desc &d = *desc;
    if (d.rows < 3 || d.cols < 3 || d.rows * d.cols > 64 || d.in_planes < 1 || d.in_planes > 4 || d.n_filters < 1 ||
        d.n_filters > AZ_NET_CPAD || d.n_blocks < 1 || d.num_actions < 1 || !d.conv_w || !d.conv_epi || !d.in_affine ||
        !d.skip_w || !d.fc_w || !d.fc_b) {
        g_net_err = "bad net description (need 3<=rows,cols, rows*cols<=64, in_planes<=4, n_filters<=56, packed buffers)";
        return AZ_E_INVALID;
    }
    if (d.precision != AZ_NET_PREC_F16 && d.precision != AZ_NET_PREC_F16X3) {
        g_net_err = "precision must be AZ_NET_PREC_F16 or AZ_NET_PREC_F16X3";
        return AZ_E_INVALID;
    }
    const bool x3 = d.precision == AZ_NET_PREC_F16X3;
    if (x3 && (!d.conv_w_lo || !d.fc_w_lo)) {
        g_net_err = "AZ_NET_PREC_F16X3 needs conv_w_lo and fc_w_lo";
        return AZ_E_INVALID;
    }
    // the scheme.  <= 50 filters (r3 = 2): output-channel tile 3 holds only channels 48, 49
    const int r3 = d.n_filters <= 50 ? 2 : 16, HW = d.rows * d.cols;
    NetScheme scheme;
    X3DLayout xd;
    if (x3) {
        const TowerGeom g = x3_geom(d.rows, d.cols, r3);
        const bool x3b = g.rp1 && r3 == 2; // row-pair board, channels 48, 49 the only ones past three tiles
        if (!x3b && (g.nt > 4 || g.lds > 160 * 1024)) {
            g_net_err = "board / filter count does not fit the f16x3 tower kernel's LDS budget";
            return AZ_E_INVALID;
        }
        if (r3 == 2) xd = x3d_layout(d.rows, d.cols);
        scheme = xd.variant >= 0 ? (x3b ? NetScheme::X3B_X3D : NetScheme::X3D) : x3b ? NetScheme::X3B : NetScheme::X3;
    } else {
        const TowerGeom gc = tower_geom(1, 1, d.rows, d.cols);
        scheme = r3 == 2 && gc.tpb && gc.rs == 8 && gc.tpb <= 3 ? NetScheme::F16C : NetScheme::F16;
    }
    // boards per wave: at most 4 column tiles per wave (larger tiles spill registers under the hand-scheduled k-loop
    // and measured slower than more, smaller waves) within the 160 KiB LDS
    int best = 0;
    for (int bpw = 1; bpw <= 8; bpw++) {
        TowerGeom g = tower_geom(bpw, 4, d.rows, d.cols);
        if (g.nt > 4 || g.lds > 160 * 1024) break;
        best = bpw;
    }
    if (!best) {
        g_net_err = "board does not fit the tower kernel's LDS budget";
        return AZ_E_INVALID;
    }
    az_net *n;
    if (int rc = new_net(d.device, &n)) return rc;
    n->d = d;
    n->precision = d.precision;
    n->scheme = scheme;
    n->r3 = r3;
    memcpy(n->in_affine, d.in_affine, sizeof n->in_affine);
    n->bpw_max = best;
    n->n_ot = (d.num_actions + 1 + 15) / 16;
    n->lds_head = HEAD_NW * OTG * 64 * 16 + 16 * n->n_ot * 16 * 4;
    // Channel stride of the tower output = K index of fc1.  The descriptor's fc stream is laid out for 64 (AZ_NET_XOUT_C: 50 channels
    // padded to two 32-wide k-steps per cell).  Where fc1 is a real GEMM (az_head_gemm_kernel) the 14 padding channels are 22 % of its
    // MFMAs and bytes: those nets keep 52 channels per cell (8-byte stores stay aligned; H*W even keeps the board rows 16-byte aligned)
    // and the stream is repacked here.  The small heads (az_head_kernel, az_head_fused.h) walk k-steps of (cell, channel half): 64.
    n->xc = (n->n_ot > OTG && HW % 2 == 0 && d.n_filters <= 52) ? 52 : AZ_NET_XOUT_C; // (the reference's nets have 50 filters)
    n->fc_ksteps = (HW * n->xc + 31) / 32;
    Upload up;
    // conv weights: the x3d stream where the positions pack; conv_w holds the x3b stream on the x3b schemes, the records elsewhere
    const int n_convs = 2 * d.n_blocks;
    auto x3_stream = [&](const X3Stream &L, _Float16 *&dst) {
        std::vector<unsigned char> s;
        if (!build_x3_stream(L, d.conv_w, d.conv_w_lo, n_convs, s))
            up.fail(AZ_E_INVALID, "AZ_NET_PREC_F16X3: a conv weight of magnitude >= 32 (the device copy holds the weights x 2048 in fp16)");
        up(dst, s.data(), s.size());
    };
    if (xd.variant >= 0) {
        n->xd_variant = xd.variant, n->xd_nb = xd.nb, n->xd_R = xd.R, n->xd_rs = xd.rs;
        x3_stream(x3d_stream_layout(), n->conv_w_d);
        up(n->xd_pos, xd.pos.data(), xd.pos.size() * 2);
        up(n->xd_sdst, xd.sdst.data(), xd.sdst.size() * 2);
    }
    if (scheme == NetScheme::X3B || scheme == NetScheme::X3B_X3D) x3_stream(x3b_stream_layout(), n->conv_w);
    else {
        const std::vector<unsigned char> s = conv_stream(d, r3);
        up(n->conv_w, s.data(), s.size());
    }
    {   // [conv][3][64] (ABI) -> [conv][4][64] with the NEXT conv's bias in row 3 (what the kernel's ring slot holds; f32x: x 2048)
        std::vector<float> e4((size_t)n_convs * 256, 0.f);
        for (int c = 0; c < n_convs; c++) {
            memcpy(&e4[(size_t)c * 256], d.conv_epi + (size_t)c * 192, 192 * sizeof(float));
            if (c + 1 < n_convs) memcpy(&e4[(size_t)c * 256 + 192], d.conv_epi + (size_t)(c + 1) * 192, 64 * sizeof(float));
            // fp32-grade towers: an accumulator holds 2048 x the conv (X3_WSCALE), so its initial value is 2048 x the bias - scaled here
            // (exact), not by two multiplies per output tile in every epilogue
            if (x3)
                for (int i = 0; i < 64; i++) e4[(size_t)c * 256 + 192 + i] *= X3_WSCALE;
        }
        up(n->epi, e4.data(), e4.size() * sizeof(float));
    }
    const size_t fw = (size_t)n->n_ot * n->fc_ksteps * 64 * 8 * 2;
    for (int lo = 0; lo < (x3 ? 2 : 1); lo++) { // fc1: hi (and lo) halves
        const uint16_t *src = lo ? d.fc_w_lo : d.fc_w;
        std::vector<uint16_t> re;
        if (n->xc != AZ_NET_XOUT_C) re = repack_fc(src, n->n_ot, n->fc_ksteps, HW, n->xc), src = re.data();
        up(lo ? n->fc_w_lo : n->fc_w, src, fw);
    }
    up(n->fc_b, d.fc_b, (size_t)n->n_ot * 16 * 4);
    up(n->skip_w, d.skip_w, 64 * 4 * sizeof(float));
    n->d.conv_w_lo = nullptr;
    n->d.fc_w_lo = nullptr;
    n->d.conv_w = nullptr; // host pointers are not kept
    n->d.conv_epi = nullptr;
    n->d.in_affine = nullptr;
    n->d.skip_w = nullptr;
    n->d.fc_w = nullptr;
    n->d.fc_b = nullptr;
    return finish_create(n, up, out);
}

// ================================================================================================
// The general path (az_net_wide.h): the descriptor holds plain folded fp32 arrays; every device layout is decided here.
// Conv weights: a power-of-two scale s per output channel puts the channel's largest |w| s in [8, 16), so hi' = 2048 fp16(w s) and
// lo' = fp16(2048 (w s - fp16(w s))) are finite for any finite weight; the epilogue multiplies by 1 / (2048 s), exactly.
static int wide_fpad(int f) { return (f + 31) & ~31; }
static int wide_nks(const az_net *n, int conv) { return conv == 0 ? 9 : 9 * n->fpad / 32; }

extern "C" int az_net_create_wide(const az_net_wide_desc *desc, az_net **out) {
    if (int rc = check_args(desc, out, "az_net_wide_desc")) return rc;
    const az_net_wide_desc &d = *desc;
    if (d.rows < 1 || d.cols < 1 || d.rows * d.cols > 64 || d.in_planes < 1 || d.in_planes > 4 || d.n_filters < 1 ||
        d.n_filters > AZ_NET_WIDE_MAX_FILTERS || d.n_blocks < 1 || d.num_actions < 1 || d.num_actions > 768 || !d.conv_w ||
        !d.conv_b || !d.bn1_scale || !d.bn1_shift || !d.skip_w || !d.fc_w || !d.fc_b) {
        g_net_err = "bad wide net description (need rows*cols<=64, 1<=in_planes<=4, 1<=n_filters<=256, A<=768, all buffers)";
        return AZ_E_INVALID;
    }
    if (d.precision != AZ_NET_PREC_F16 && d.precision != AZ_NET_PREC_F16X3) {
        g_net_err = "precision must be AZ_NET_PREC_F16 or AZ_NET_PREC_F16X3";
        return AZ_E_INVALID;
    }
    const int F = d.n_filters, HW = d.rows * d.cols, cin0 = d.in_planes, C = F > cin0 ? F : cin0, nc = 2 * d.n_blocks;
    const int fpad = wide_fpad(F), nmt = fpad / 16, A1 = d.num_actions + 1;
    const size_t n_w = (size_t)nc * F * C * 9;
    for (size_t i = 0; i < n_w; i++)
        if (!std::isfinite(d.conv_w[i])) {
            g_net_err = "az_net_create_wide: a conv weight is not finite";
            return AZ_E_INVALID;
        }
    az_net *n;
    if (int rc = new_net(d.device, &n)) return rc;
    n->d = az_net_desc{};
    n->d.struct_size = sizeof(az_net_desc);
    n->d.rows = d.rows, n->d.cols = d.cols, n->d.in_planes = cin0, n->d.n_filters = F, n->d.n_blocks = d.n_blocks;
    n->d.num_actions = d.num_actions, n->d.device = d.device, n->d.precision = d.precision;
    n->precision = d.precision;
    n->scheme = NetScheme::WIDE;
    n->fpad = fpad;
    n->nbw = 16 * WIDE_NT / HW;
    n->xc = fpad;
    n->n_ot = (A1 + 15) / 16;
    n->fc_ksteps = HW * fpad / 32;
    n->lds_head = HEAD_NW * OTG * 64 * 16 + 16 * n->n_ot * 16 * 4;
    // conv weight streams and epilogue rows
    std::vector<uint16_t> w;
    std::vector<float> epi((size_t)nc * 4 * fpad, 0.f);
    auto h16 = [](double v) {
        _Float16 h = (_Float16)v;
        uint16_t b;
        memcpy(&b, &h, 2);
        return b;
    };
    for (int c = 0; c < nc; c++) {
        n->w_off.push_back(w.size());
        const int cin = c == 0 ? WIDE_CIN0 : fpad, n_ch = cin / 32, cin_real = c == 0 ? cin0 : F;
        const float *wc = d.conv_w + (size_t)c * F * C * 9;
        std::vector<double> sc(fpad, 1.0);
        for (int co = 0; co < F; co++) {
            double m = 0;
            for (int k = 0; k < cin_real * 9; k++) m = std::max(m, (double)std::fabs(wc[((size_t)co * C + k / 9) * 9 + k % 9]));
            int e = 0;
            if (m > 0) {
                (void)std::frexp(m, &e); // m = f 2^e, f in [0.5, 1): m 2^(4 - e) in [8, 16)
                e = std::min(100, std::max(-100, 4 - e));
            }
            sc[co] = std::ldexp(1.0, e);
        }
        const size_t base = w.size();
        w.resize(base + (size_t)n_ch * 9 * nmt * 2 * 512, 0);
        for (int ch = 0; ch < n_ch; ch++)
            for (int tap = 0; tap < 9; tap++)
                for (int mt = 0; mt < nmt; mt++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int j = 0; j < 8; j++) {
                            const int co = 16 * mt + (lane & 15), ci = 32 * ch + 8 * (lane >> 4) + j;
                            if (co >= F || ci >= cin_real) continue;
                            const double v = (double)wc[((size_t)co * C + ci) * 9 + tap] * sc[co];
                            const double hi = (double)(_Float16)v;
                            const size_t o = base + ((((size_t)(ch * 9 + tap) * nmt + mt) * 2) * 512) + lane * 8 + j;
                            w[o] = h16(hi * 2048.0);
                            w[o + 512] = h16((v - hi) * 2048.0);
                        }
        float *e4 = &epi[(size_t)c * 4 * fpad];
        for (int co = 0; co < fpad; co++) e4[co] = (float)(1.0 / (2048.0 * sc[co]));
        for (int co = 0; co < F; co++) {
            e4[fpad + co] = d.conv_b[(size_t)c * F + co];
            if (c % 2 == 1 && c + 1 < nc) { // the next block's bn1
                e4[2 * fpad + co] = d.bn1_scale[(size_t)(c / 2 + 1) * C + co];
                e4[3 * fpad + co] = d.bn1_shift[(size_t)(c / 2 + 1) * C + co];
            }
        }
    }
    std::vector<float> in((size_t)8 + (size_t)fpad * 4, 0.f);
    for (int c = 0; c < cin0; c++) in[c] = d.bn1_scale[c], in[4 + c] = d.bn1_shift[c];
    for (int co = 0; co < F; co++)
        for (int c = 0; c < cin0; c++) in[8 + (size_t)co * 4 + c] = d.skip_w[(size_t)co * cin0 + c];
    // fc1 [A+1][F*HW] (index c*HW + pos) -> the heads' stream [n_ot][ksteps][64][8], k = pos * fpad + c; lo = fp16((w - hi) * 2048)
    const size_t fw = (size_t)n->n_ot * n->fc_ksteps * 512;
    std::vector<uint16_t> fh(fw, 0), fl(fw, 0);
    for (int ot = 0; ot < n->n_ot; ot++)
        for (int ks = 0; ks < n->fc_ksteps; ks++)
            for (int lane = 0; lane < 64; lane++)
                for (int j = 0; j < 8; j++) {
                    const int o = 16 * ot + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + j, pos = k / fpad, c = k % fpad;
                    if (o >= A1 || c >= F) continue;
                    const double v = d.fc_w[(size_t)o * F * HW + (size_t)c * HW + pos], hi = (double)(_Float16)v;
                    const size_t i = (((size_t)ot * n->fc_ksteps + ks) * 64 + lane) * 8 + j;
                    fh[i] = h16(hi);
                    fl[i] = h16((v - hi) * 2048.0);
                }
    std::vector<float> fb((size_t)n->n_ot * 16, 0.f);
    for (int o = 0; o < A1; o++) fb[o] = d.fc_b[o];
    Upload up;
    up(n->w_wide, w.data(), w.size() * 2);
    up(n->epi_wide, epi.data(), epi.size() * 4);
    up(n->in_wide, in.data(), in.size() * 4);
    up(n->fc_w, fh.data(), fw * 2);
    up(n->fc_w_lo, fl.data(), fw * 2);
    up(n->fc_b, fb.data(), fb.size() * 4);
    return finish_create(n, up, out);
}

// v_mfma_f32_16x16x32_f16 per board of a wide forward of n_boards boards: every workgroup runs all of its channel tiles over
// ceil(columns / 16) column tiles for every k-step of every conv (x 3 for f32x), then the head
static double wide_mfma_per_board(const az_net *n, int n_boards) {
    const int HW = n->d.rows * n->d.cols, nc = 2 * n->d.n_blocks, per = n->precision == AZ_NET_PREC_F16X3 ? 3 : 1;
    double ks = 0;
    for (int c = 0; c < nc; c++) ks += wide_nks(n, c);
    const long full = n_boards / n->nbw, rest = n_boards % n->nbw;
    const double tiles = (double)full * ((n->nbw * HW + 15) / 16) + (rest ? (rest * HW + 15) / 16 : 0);
    return per * ks * (n->fpad / 16) * tiles / n_boards + per * (double)n->n_ot * n->fc_ksteps / 16.0;
}
static int wide_reserve(az_net *n, int32_t max_boards) {
    const size_t cells = (size_t)max_boards * n->d.rows * n->d.cols;
    float **fbufs[] = {&n->x_wide, &n->logits};
    for (float **b : fbufs) (void)hipFree(*b), *b = nullptr;
    _Float16 **hbufs[] = {&n->opa_hi, &n->opa_lo, &n->opb_hi, &n->opb_lo};
    for (_Float16 **b : hbufs) (void)hipFree(*b), *b = nullptr;
    n->max_boards = 0;
    NCHK(n, hipMalloc((void **)&n->x_wide, cells * n->fpad * 4));
    for (_Float16 **b : hbufs) {
        if (n->precision != AZ_NET_PREC_F16X3 && (b == &n->opa_lo || b == &n->opb_lo)) continue;
        NCHK(n, hipMalloc((void **)b, cells * n->fpad * 2));
        NCHK(n, hipMemset(*b, 0, cells * n->fpad * 2));
    }
    if (n->n_ot > OTG) NCHK(n, hipMalloc((void **)&n->logits, (size_t)max_boards * n->n_ot * 16 * sizeof(float) * 2));
    n->max_boards = max_boards;
    return AZ_OK;
}
// the wide tower: the input launch, then one launch per conv; the tower output ends in opb
static hipError_t wide_tower(az_net *n, const float *obs, int32_t n_boards, hipStream_t st) {
    const bool x3 = n->precision == AZ_NET_PREC_F16X3;
    const int HW = n->d.rows * n->d.cols, nc = 2 * n->d.n_blocks;
    WideInputParams ip;
    ip.HW = HW, ip.cin = n->d.in_planes, ip.fpad = n->fpad, ip.n_boards = n_boards;
    ip.obs = obs, ip.in_scale = n->in_wide, ip.in_shift = n->in_wide + 4, ip.skip_w = n->in_wide + 8;
    ip.x = n->x_wide, ip.a_hi = n->opb_hi, ip.a_lo = x3 ? n->opb_lo : nullptr;
    hipError_t s = az_launch_wide_input(ip, st);
    for (int c = 0; c < nc && s == hipSuccess; c++) {
        WideConvParams p;
        p.W = n->d.cols, p.HW = HW, p.nbw = n->nbw, p.n_boards = n_boards;
        p.cin = c == 0 ? WIDE_CIN0 : n->fpad, p.n_chunks = p.cin / 32;
        p.fpad = n->fpad, p.nmt = n->fpad / 16;
        p.mode = c % 2 == 0 ? WIDE_MODE_CONV1 : c + 1 < nc ? WIDE_MODE_CONV2 : WIDE_MODE_LAST;
        const bool in_a = c % 2 == 1; // conv c reads what conv c - 1 wrote: even convs write opa, odd ones opb
        p.a_hi = in_a ? n->opa_hi : n->opb_hi, p.a_lo = in_a ? n->opa_lo : n->opb_lo;
        p.o_hi = in_a ? n->opb_hi : n->opa_hi, p.o_lo = in_a ? n->opb_lo : n->opa_lo;
        p.w = n->w_wide + n->w_off[c], p.epi = n->epi_wide + (size_t)c * 4 * n->fpad, p.x = n->x_wide;
        s = az_launch_wide_conv(n->d.device, x3, p, st);
    }
    return s;
}

extern "C" int az_net_reserve(az_net *n, int32_t max_boards) {
    if (!n || max_boards < 1) return AZ_E_INVALID;
    NCHK(n, hipSetDevice(n->d.device));
    if (n->scheme == NetScheme::WIDE) return wide_reserve(n, max_boards);
    if (n->xout) (void)hipFree(n->xout);
    n->xout = nullptr;
    // The cross-board read under the K tail.  With the 52-channel stride K = H*W*52 need not be a multiple of 32 (6x7: 68 k-steps +
    // 24 halves, 6x6: 58 + 16), and the last fc1 k-step of board b then reads the first 8 / 16 halves of board b + 1's row.  The
    // repacked fc stream (repack_fc) holds zeros at k >= K, so what is read there counts for nothing AS LONG AS IT IS FINITE: a NaN
    // or Inf in the first channels of board b + 1 would turn board b's logits into NaN (0 * Inf).  Rows past a forward's n_boards
    // hold what an earlier, larger forward left (finite tower outputs) or the zeros written here; the + 64 bytes are that read for
    // the last row of the buffer.  tests/test_head_kernels_gpu.py::test_a_board_keeps_its_bits pins that a small batch after a
    // larger one of other boards gives the bits of a fresh handle.
    size_t bytes = (size_t)max_boards * n->d.rows * n->d.cols * n->xc * 2 + 64;
    NCHK(n, hipMalloc((void **)&n->xout, bytes));
    NCHK(n, hipMemset(n->xout, 0, bytes));
    if (n->xout_lo) (void)hipFree(n->xout_lo);
    n->xout_lo = nullptr;
    if (n->precision == AZ_NET_PREC_F16X3) {
        NCHK(n, hipMalloc((void **)&n->xout_lo, bytes));
        NCHK(n, hipMemset(n->xout_lo, 0, bytes));
    }
    if (n->logits) (void)hipFree(n->logits);
    n->logits = nullptr;
    if (n->n_ot > OTG) NCHK(n, hipMalloc((void **)&n->logits, (size_t)max_boards * n->n_ot * 16 * sizeof(float) * 2)); // x 2: HG_KSPLIT partial sums (az_head_gemm_kernel)
    n->max_boards = max_boards;
    return AZ_OK;
}

// Work partition of the f16 tower for THIS batch size.  Candidates: boards per wave x {4, 8} waves per workgroup.  One
// workgroup per CU is resident, a launch runs in ceil(WGs / 256) rounds and a round costs ~ (2 * tiles + 1), x1.5 when two
// waves share each SIMD: pick the candidate that minimises rounds x round cost.
static TowerGeom choose_geom(const az_net *n, int n_boards) {
    TowerGeom g = tower_geom(1, 4, n->d.rows, n->d.cols);
    double best_cost = -1;
    for (int bpw = 1; bpw <= n->bpw_max; bpw++)
        for (int waves = 4; waves <= 8; waves += 4) {
            TowerGeom c = tower_geom(bpw, waves, n->d.rows, n->d.cols);
            if (c.lds > 160 * 1024 || (waves == 8 && c.nt > 3)) continue; // 8 waves need <= 256 registers each
            long wgs = (n_boards + waves * bpw - 1) / (waves * bpw);
            long rounds = (wgs + 255) / 256;
            double cost = rounds * (2.0 * (c.nt < 3 ? 3 : c.nt) + 1.0) * (waves == 8 ? 1.5 : 1.0);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                g = c;
            }
        }
    return g;
}

// ================================================================================================
// One forward of n_boards boards: the tower kernel and its launch shape.  A pure function of (net, n_boards) - forwards are
// captured in graphs, so nothing here may keep state; az_net_forward, az_net_kernel_label and az_net_issued_mfma_per_board
// all follow it.
struct ForwardPlan {
    TowerKind kind;
    TowerGeom g = {};    // the launch geometry (ck: k-steps per weight chunk); unused by WIDE
    int per_wg = 0;      // boards per workgroup
    int grid = 0;        // workgroups of the tower launch
    int xd_variant = -1; // X3D: the kernel variant
    bool head = true;    // a separate head launch follows the tower
};
static ForwardPlan plan_forward(const az_net *n, int n_boards) {
    ForwardPlan p;
    const int H = n->d.rows, W = n->d.cols;
    switch (n->scheme) {
    case NetScheme::WIDE:
        p.kind = TowerKind::WIDE;
        return p;
    case NetScheme::F16C:
        if (n_boards <= AZ_F16C_MAX_BOARDS) { // small batch of a row-pair board: a board per four-wave workgroup (az_tower_f16c.h)
            p.kind = TowerKind::F16C;
            p.g = tower_geom(1, 1, H, W);
            // up to a board per CU: 32 KiB weight chunks (half the barriers); above: 16 KiB chunks, so that two workgroups fit a CU's LDS
            p.g.ck = n_boards <= AZ_X3C_ONE_PER_WG ? 8 : 4;
            p.g.off_epi = (p.g.ck == 8 ? 4 : 3) * p.g.ck * 4096; // a ring of four 32-KiB / three 16-KiB weight buffers (147 / 65 KB with the planes)
            p.g.off_act = p.g.off_epi + 2048 + 8 * 64 * 8;
            p.g.lds = p.g.off_act + N_OCT * p.g.rcells * OCT_B;
            p.per_wg = 1;
            break;
        }
        [[fallthrough]];
    case NetScheme::F16:
        p.kind = TowerKind::F16;
        p.g = choose_geom(n, n_boards);
        p.per_wg = p.g.waves * p.g.bpw;
        break;
    default: { // the f16x3 schemes: one board per wave, 4 waves per workgroup
        const bool x3b = n->scheme == NetScheme::X3B || n->scheme == NetScheme::X3B_X3D;
        p.g = x3_geom(H, W, n->r3);
        p.per_wg = 4;
        if (x3b && n_boards <= AZ_X3C_MAX_BOARDS) { // small batch: one board per four waves (az_tower_x3c.h), two per workgroup above 256
            // ... and with a single output tile (connect_four: 7 + 1 outputs) that kernel also runs fc1 + softmax + tanh for its board:
            // at <= 512 boards the head kernel is 7 us of a 49 us tick (profiles/r3_small_generation_kernel_stats.csv).  (The same inside
            // az_tower_x3b_kernel, measured: bit-identical and SLOWER - 1146 vs 1182 games/s in a same-box A/B: at one workgroup per CU
            // the head phase of each of the four rounds, ~5 us, has nothing to hide behind.)  Eight chains x HMAX k-steps; a chain
            // steps 4 columns: az_tower_x3c.h.
            p.head = !(n->n_ot == 1 && n->fc_ksteps <= 96 && W >= 4);
            p.kind = p.head ? TowerKind::X3C : TowerKind::X3C_FUSED_HEAD;
            p.per_wg = n_boards > AZ_X3C_ONE_PER_WG ? 2 : 1;
        } else if (n->scheme == NetScheme::X3D || (n->scheme == NetScheme::X3B_X3D && n_boards > 128 * n->xd_nb)) {
            // packed column tiles (az_tower_x3d.h).  They put xd_nb boards in a workgroup: with eight (6x6) a batch must be large enough
            // to occupy the chip - at 1024 boards 128 workgroups of 4.5 tiles per SIMD lose to 256 of 3 (az_tower_x3b_kernel, one
            // round), from 1280 on they win
            p.kind = TowerKind::X3D;
            p.per_wg = n->xd_nb;
            p.xd_variant = n->xd_variant;
        } else
            p.kind = x3b ? TowerKind::X3B : TowerKind::X3;
    }
    }
    p.grid = (n_boards + p.per_wg - 1) / p.per_wg;
    return p;
}

// launch parameters of the tuned tower kernels
static TowerParams tower_params(const az_net *n, const ForwardPlan &p, const float *obs, float *priors, float *values, int n_boards) {
    TowerParams tp = {};
    tp.H = n->d.rows, tp.W = n->d.cols, tp.HW = tp.H * tp.W, tp.cin = n->d.in_planes, tp.n_convs = 2 * n->d.n_blocks;
    tp.n_boards = n_boards;
    tp.cells = p.g.cells, tp.rs = p.g.rs, tp.tpb = p.g.tpb, tp.bpw = p.g.bpw, tp.rcells = p.g.rcells, tp.zcell = p.g.zcell;
    tp.off_epi = p.g.off_epi, tp.off_act = p.g.off_act;
    tp.conv_w = p.kind == TowerKind::X3D ? n->conv_w_d : n->conv_w;
    tp.epi = n->epi, tp.skip_w = n->skip_w;
    memcpy(tp.in_scale, n->in_affine, 32);
    memcpy(tp.in_shift, n->in_affine + 8, 32);
    tp.obs = obs, tp.xout = n->xout, tp.xout_lo = n->xout_lo, tp.xout_c = n->xc;
    tp.fc_w = p.kind == TowerKind::X3C_FUSED_HEAD ? n->fc_w : nullptr; // set: the tower kernel runs the head
    tp.fc_w_lo = n->fc_w_lo, tp.fc_b = n->fc_b, tp.priors = priors, tp.values = values;
    tp.A = n->d.num_actions, tp.fc_ksteps = n->fc_ksteps;
    tp.xd_nb = n->xd_nb, tp.xd_R = n->xd_R, tp.xd_rs = n->xd_rs, tp.xd_pos = n->xd_pos, tp.xd_sdst = n->xd_sdst;
    return tp;
}
// launch parameters of the head kernels: the tower output of either path
static HeadParams head_params(const az_net *n, float *priors, float *values, int n_boards) {
    const bool wide = n->scheme == NetScheme::WIDE;
    HeadParams hp;
    hp.HW = n->d.rows * n->d.cols, hp.A = n->d.num_actions, hp.n_ot = n->n_ot, hp.K = hp.HW * n->xc, hp.ksteps = n->fc_ksteps;
    hp.n_boards = n_boards;
    hp.x = wide ? n->opb_hi : n->xout, hp.x_lo = wide ? n->opb_lo : n->xout_lo;
    hp.fc_w = n->fc_w, hp.fc_w_lo = n->fc_w_lo, hp.fc_b = n->fc_b;
    hp.priors = priors, hp.values = values;
    return hp;
}

extern "C" int az_net_issued_mfma_per_board(const az_net *n, int32_t n_boards, double *out) {
    if (!n || !out || n_boards < 1) return AZ_E_INVALID;
    const ForwardPlan p = plan_forward(n, n_boards);
    const int n_convs = 2 * n->d.n_blocks, nks = n->r3 < 16 ? 15 : AZ_NET_KSTEPS;
    const double head = (double)n->n_ot * n->fc_ksteps / 16.0; // one MFMA per (output tile, k-step) per 16 boards
    const double per_tile = x3b_mfma_per_tile<true>() + (double)(n_convs - 1) * x3b_mfma_per_tile<false>();
    switch (p.kind) {
    case TowerKind::F16: {
        const int nt = p.g.nt < 3 ? 3 : (p.g.nt > 3 ? 4 : 3);
        *out = (double)(AZ_NET_K0STEPS + (n_convs - 1) * nks) * 4 * nt / p.g.bpw + head;
        break;
    }
    case TowerKind::F16C: // one board per four-wave workgroup: three column tiles x 4 output-channel tiles
        *out = (double)(AZ_NET_K0STEPS + (n_convs - 1) * nks) * 4 * 3 + head;
        break;
    case TowerKind::X3: // one board per wave
        *out = x3_mfma_per_wave(p.g.nt <= 3 ? 3 : 4, n_convs, nks) + 3.0 * head;
        break;
    case TowerKind::X3B: // three tiles per board
    case TowerKind::X3C:
        *out = 3.0 * per_tile + 3.0 * head;
        break;
    case TowerKind::X3C_FUSED_HEAD: // the fused head runs its eight chains once per board or pair of boards
        *out = 3.0 * per_tile + 3.0 * (head * 16.0 / p.per_wg);
        break;
    case TowerKind::X3D: // the workgroup's tiles over its boards.  The count of the SCHEME: the connect_four variant issues fewer -
        // its pure tiles sit out the k-steps of their halo row, (skip_top + skip_bot) x 36 MFMAs per workgroup and later conv
        // (X3BK::n_mfma_pure; 27 per board) - but tests/golden/net_dispatch.json pins this figure as it is
        *out = az_x3d_variant(p.xd_variant).tiles * per_tile / p.per_wg + 3.0 * head;
        break;
    case TowerKind::WIDE:
        *out = wide_mfma_per_board(n, n_boards);
        break;
    }
    return AZ_OK;
}

extern "C" const char *az_net_kernel_label(const az_net *n, int32_t n_boards) {
    if (!n) return "";
    return n->labels[(int)plan_forward(n, n_boards < 1 ? n->max_boards : n_boards).kind].c_str();
}

extern "C" int az_net_forward(az_net *n, const float *obs, float *priors, float *values, int32_t n_boards, void *stream) {
    if (!n || !obs || !priors || !values || n_boards < 1) return AZ_E_INVALID;
    if (n_boards > n->max_boards) {
        n->err = "n_boards exceeds az_net_reserve()";
        return AZ_E_STATE;
    }
    NCHK(n, hipSetDevice(n->d.device)); // the launch must pair `stream` with the device the net lives on
    hipStream_t st = (hipStream_t)stream;
    const ForwardPlan p = plan_forward(n, n_boards);
    const TowerParams tp = tower_params(n, p, obs, priors, values, n_boards);
    const int dv = n->d.device;
    const bool x3 = n->precision == AZ_NET_PREC_F16X3;
    hipError_t s = hipSuccess;
    switch (p.kind) {
    case TowerKind::F16: s = az_launch_tower_f16(dv, p.g.nt, p.g.ck, p.g.waves, n->r3, tp, p.grid, p.g.lds, st); break;
    case TowerKind::F16C: s = az_launch_tower_f16c(dv, p.g.ck, tp, n_boards, p.g.lds, st); break;
    case TowerKind::X3: s = az_launch_tower_x3(dv, p.g.nt, p.g.rp1, n->r3, tp, p.grid, p.g.lds, st); break;
    case TowerKind::X3B: s = az_launch_tower_x3b(dv, tp, p.grid, st); break;
    case TowerKind::X3C:
    case TowerKind::X3C_FUSED_HEAD: s = az_launch_tower_x3c(dv, p.per_wg, tp, n_boards, st); break;
    case TowerKind::X3D: s = az_launch_tower_x3d(dv, p.xd_variant, tp, p.grid, st); break;
    case TowerKind::WIDE: s = wide_tower(n, obs, n_boards, st); break;
    }
    if (s != hipSuccess) {
        n->err = std::string(p.kind == TowerKind::WIDE ? "wide tower launch: " : x3 ? "f16x3 tower launch: " : "tower launch: ") + hipGetErrorString(s);
        return AZ_E_HIP;
    }
    if (p.head) NCHK(n, az_launch_head(dv, x3, head_params(n, priors, values, n_boards), n_boards, n->lds_head, n->logits, st));
    return AZ_OK;
}

extern "C" int az_net_read_tower(az_net *n, float *out, int32_t n_boards) {
    if (!n || !out || n_boards < 1 || n_boards > n->max_boards) return AZ_E_INVALID;
    NCHK(n, hipSetDevice(n->d.device));
    NCHK(n, hipDeviceSynchronize());
    if (n->scheme == NetScheme::WIDE) { // out: [n_boards][H*W][fpad], hi + lo / 2048 of the tower output
        const size_t cnt = (size_t)n_boards * n->d.rows * n->d.cols * n->fpad;
        std::vector<_Float16> h(cnt);
        NCHK(n, hipMemcpy(h.data(), n->opb_hi, cnt * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; i++) out[i] = (float)h[i];
        if (n->precision == AZ_NET_PREC_F16X3) {
            NCHK(n, hipMemcpy(h.data(), n->opb_lo, cnt * 2, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < cnt; i++) out[i] += (float)h[i] * (1.0f / 2048.0f);
        }
        return AZ_OK;
    }
    // out: [n_boards][H*W][AZ_NET_XOUT_C] whatever the stride on the device (channels past it read as zero)
    const size_t cells = (size_t)n_boards * n->d.rows * n->d.cols, cnt = cells * n->xc;
    const int nc = n->xc < AZ_NET_XOUT_C ? n->xc : AZ_NET_XOUT_C;
    std::vector<_Float16> h(cnt);
    NCHK(n, hipMemcpy(h.data(), n->xout, cnt * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cells * AZ_NET_XOUT_C; i++) out[i] = 0.f;
    for (size_t c = 0; c < cells; c++)
        for (int ch = 0; ch < nc; ch++) out[c * AZ_NET_XOUT_C + ch] = (float)h[c * n->xc + ch];
    if (n->precision == AZ_NET_PREC_F16X3) { // hi + lo / 2048
        NCHK(n, hipMemcpy(h.data(), n->xout_lo, cnt * 2, hipMemcpyDeviceToHost));
        for (size_t c = 0; c < cells; c++)
            for (int ch = 0; ch < nc; ch++) out[c * AZ_NET_XOUT_C + ch] += (float)h[c * n->xc + ch] * (1.0f / 2048.0f);
    }
    return AZ_OK;
}
