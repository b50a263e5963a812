// The plan of one conv launch: conv_plan (kernels_gemm.hip) decides everything about it -- kernel, tile, grid, K splits, tile walk,
// epilogue form -- and launch_conv, the query functions of nope_common.h and the runtimes only read the result.  Also the launch parameters
// the conv kernels take by value (conv_gemm_common.h includes this header; internal linkage, the same text in every translation unit).
#pragma once
#include "nope_common.h"

namespace nope {

// FastDiv and ConvParams stay in an anonymous namespace ON PURPOSE: the kernels take ConvParams by value, so its qualified name is part of
// every kernel's symbol; moving it would rename them all (and with them the code objects and the per-kernel register-usage records).  ConvLaunch,
// which crosses translation units, therefore has a member of a type that is formally distinct per unit; every unit reads the same text above
// the same headers, so the layouts are one.  (The kernel launchers of the other files take `const void* params` for the same reason.)
namespace {

// Unsigned division by a launch-time constant, exact for n < 2^31: q = mulhi(n, M) >> sh with
// M = floor(2^(32+sh) / d) + 1, sh = ceil(log2 d) - 1 (d >= 2); M == 0 encodes d == 1.  Replaces the ~35-instruction
// integer-division sequences of the per-row index arithmetic in the conv prologue.
struct FastDiv {
    unsigned M, sh;
    __device__ __forceinline__ unsigned div(unsigned n) const {
        return M ? (unsigned)(((unsigned long long)n * M) >> 32) >> sh : n;
    }
};
static inline FastDiv make_fastdiv(unsigned d) {
    FastDiv f{0u, 0u};
    if (d <= 1) return f;
    unsigned s = 0;
    while ((1ull << s) < d) ++s;                       // s = ceil(log2 d) >= 1
    f.sh = s - 1;
    f.M = (unsigned)(((1ull << (31 + s)) / d) + 1);    // < 2^32 because d > 2^(s-1)
    return f;
}

struct ConvParams {
    const unsigned char* src1; const unsigned char* src2;
    int C1, C2, rep1, rep2;
    int Hs, Ws, Ho, Wo;
    int mode, ntaps;
    const unsigned char* w;
    const float* bias;
    const unsigned char* resid;
    unsigned char* out;
    int Cout, M;
    int out_nchw, out_dt;
    int act;                           // 0 none, 1 ReLU (after bias and residual)
    int tiles_m, tiles_n, xcd_map, wide_out;
    int geglu;                         // host side only: selects the GEGLU-epilogue instantiation (ConvArgs::geglu)
    int nchw_staged;                   // out_nchw through the per-wave LDS panels (epilogue_nchw): whole 64-row blocks inside one sample
    int xcd_gn;                        // (xcd_map: 0 none, 1 one panel per XCD, 2 below, 3 small-tile kernel, 4 any tiles_n) xcd_map == 2: XCD columns the weight panels are split over (tile_coords)
    int variant;                       // tuning switches (NOPE_CONV_VARIANT), 0 in production
    FastDiv d_hw, d_w, d_rep1, d_rep2; // / (Hm*Wm), / Wm, / rep1, / rep2
    unsigned char pos_order[64];       // posmajor: pixel positions by descending number of valid taps
    int persist_iters;                 // > 1: a workgroup walks this many tiles
    unsigned persist_d1, persist_d2;   // byte advance of the A offsets per walked tile (src1 / src2)
    int persist_dm;                    // GEMM rows between the tiles a workgroup of the 128 x 192 kernel walks
    unsigned* timeline;                // tuning only (NOPE_PP_VARIANT & 256): cycle stamps of workgroup 0, see conv3x3_halo_kernel
    int posmajor;                      // 1: GEMM rows ordered (pixel position, sample) instead of (sample, pixel) -- see conv_plan
    FastDiv d_n;                       // / nhyp (posmajor)
    int nhyp;
    int splits;                        // > 1: blockIdx.z owns a K range and writes raw f32 partial sums
    float* split_out;                  // [splits][M][Cout]
    int Hm, Wm;                        // grid the GEMM rows enumerate: output grid, or the SOURCE grid for UP2P
    unsigned w_phase_bytes;            // UP2P: byte stride between the 4 phase weight sets
    float* colstats;                   // optional [M/stat_rows][Cout][2]: per row block column sum / sum of squares
    int stat_rows;                     // 64 (every kernel), 16 / 32 (small-tile kernel only)
    const float* pn_ms; const float* pn_c0; const float* pn_c1;   // optional fused PreNorm (see ConvArgs)
    unsigned bytes1, bytes2, bytesw;   // tensor sizes for the buffer descriptors of the DMA kernel
    const int* x2_scale;               // NOPE_F16X2 (ping-pong kernels): the tail of the packed weights, [0] = E8M0 scale of the A operand, [3] = range shift t
    unsigned* x2_amax;                 // NOPE_F16X2: optional device word, atomicMax of the bits of max |a| over every A element the launch converted (NOPE_X2_KERNEL_AMAX builds)
    int x2_t_zero;                     // NOPE_F16X2: the caller vouches that the layer's range shift (tail word 3) is 0: the tap-resident kernel skips the a * 2^-t multiplies
    int lean;                          // 1: f32 storage, every wave tile of the launch whole and in NHWC row order (see epilogue_wide, LEANM): the kernels' LEAN instantiations
    unsigned* out_amax;                // f32-storage launches with a wide NHWC epilogue: optional range slot (amax_publish) for max |out| of what the launch writes
    int s2_off;                        // STRIDE2: 0 = centre tap at (2 oy, 2 ox) (pad 1), 1 = at (2 oy + 1, 2 ox + 1) (NOPE_CONV_STRIDE2_PAD01: pad (0, 1, 0, 1))
    // GroupNorm tail (ConvArgs::gn_*; the per-tap ping-pong kernel's lean epilogue only: conv_gemm_pp_kernel with PP_GN_TAIL): out = conv + SiLU(GN(resid))
    const float* gn_ms; const float* gn_gamma; const float* gn_beta;
    int gn_G;
    FastDiv d_cpg;                     // / (Cout / gn_G)
    float* tail_stats;                 // optional [nhyp][(HW / 64) * tail_cols][2]: (sum, sum of squares) of what each wave tile wrote
    int tail_cols;                     // 96-column wave tiles across Cout
    // The launch's own GroupNorm (ConvArgs::gn_self; the tap-resident kernel's lean epilogue only): out = SiLU(GN(conv)) [+ emb] [+ resid];
    // gn_gamma / gn_beta / gn_G / d_cpg above, stat_rows = rows per block of the column sums it keeps in LDS (64, or 16 on 16-pixel maps), resid = ConvArgs::gn_resid
    int gn_self;
    int gn_cpg;                        // Cout / gn_G
    float gn_eps;
    const float* gn_emb; int gn_emb_stride;
    int padskip;                       // 1: the tap-resident kernel's form for 4 x 4 maps that stages a tile in (position, sample) order and skips the MFMA blocks that lie wholly in the padding (conv3x3_halo_kernel, PADSKIP)
};

}  // namespace

enum { CONV_REDUCE_NONE = 0, CONV_REDUCE_PLAIN = 1, CONV_REDUCE_STATS = 2 };      // the kernel that follows a split-K launch

struct ConvLaunch {
    int err = NOPE_OK;               // NOPE_OK, or what launch_conv returns without launching: nothing below is meaningful then
    int dt = NOPE_F32;               // element type the kernels see: NOPE_F16X2 as an element type runs as NOPE_BF16X3 on the two-pass weights
    ConvParams p{};                  // (zero except what conv_plan fills; p.splits = K splits, blockIdx.z)
    dim3 grid{1, 1, 1};
    int kind = NOPE_CONV_KERNEL_GENERIC;      // NOPE_CONV_KERNEL_*: what the trace line, nope_conv_launch_info and the dispatch read
    int small = -1;                  // NOPE_CONV_KERNEL_SMALL: the tile of conv_gemm_small_kernel (0 = 64 x 64, 1 = 128 x 128, 2 = 64 x 64 / 6-stage ring, 3 = 64 x 64 by two K groups)
    int bm = 128;                    // rows of a tile
    int reduce = CONV_REDUCE_NONE;
    bool x2 = false;                 // runs the f16 + MX-fp8 (two-pass) tile on ConvArgs::w_x2
    bool posmajor = false;
    bool records_out_amax = false;   // its epilogue can fill a range slot with max |out|, whether or not ConvArgs::out_amax named one ...
    void record_out_amax(unsigned* slot) { if (records_out_amax) p.out_amax = slot; }      // ... a slot chosen after planning
    double flops = 0.0;              // multiply-adds x2 the launch executes (position-major launches skip the taps that lie in the padding)
};

ConvLaunch conv_plan(int dt, const ConvArgs& a);      // pure: no HIP call, no pointer dereferenced, no I/O; reads `a`, `dt` and the NOPE_* switches
int launch_conv(const ConvLaunch& L, hipStream_t s);   // trace line (NOPE_CONV_TRACE), the planned kernel, the reduce kernel of a split launch; L.err when that is set

}  // namespace nope
