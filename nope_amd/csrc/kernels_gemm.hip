// Implicit-GEMM convolution for gfx950 (MI355X): every conv / linear of the NOPE U-Net.
//
//   out[m, n] = sum_{tap, c} A[m, tap, c] * W[n, tap, c] + bias[n] (+ resid[m, n])
//
// m = (hypothesis, oy, ox) over NHWC activations, n = output channel, K = taps x Cin.
// The A operand is never materialised: the loader walks taps and channel chunks directly
// over one or two NHWC sources (virtual torch.cat, u_net.py:186,189,194), optionally through
// a nearest-x2 upsample (HardUpsample, model_utils.py:161-165) or a 2x2 space-to-depth
// (HardDownsample, :168-172; the weight's K axis is re-ordered at pack time so each of the 4
// taps reads a contiguous channel run), and sources may be shared by `rep` consecutive
// hypotheses (the reference embedding feeding all N pose hypotheses, model.py:219).
//
// Tiling (64-wide wavefronts): 128 x 192 output tile per 256-thread workgroup, 4 waves as
// 2(M) x 2(N), each wave 64 x 96 = 4 x 6 MFMA 16x16 tiles (96 accumulator VGPRs).  192
// divides every Cout of the network (192/384/768/1536 and the 384-wide qkv).  K step = 128
// bytes per row (64 bf16 / 32 f32).  LDS rows are 128 B = 8 x 16-B slots, XOR-swizzled by
// (row >> 1) & 7 so the ds_read_b128 fragment reads (16 rows x one slot per lane group) are
// bank-conflict free (MI355X_MICROARCH.md, LDS table).
//
// Two kernels share the MFMA stage / epilogues:
//   conv_gemm_dma_kernel  the fast path: LDS-DMA staging (buffer_load ... lds), two 40 KiB stages,
//                         one barrier per K step; needs Cin (and C1 of a concat) to be a multiple of
//                         the K step.  Used by every conv of the real network.
//   conv_gemm_kernel      any channel count (global -> VGPR -> LDS staging): init conv (Cin = 8) and
//                         the tiny nets of the parity tests.
// Epilogue: accumulators (+bias) are staged per wave through LDS in f32 and written as 16-byte rows
// (epilogue_wide); on the way the per-64-row-block column sums needed by the following GroupNorm are
// emitted (colstats), so no separate statistics pass reads the tensor again.
//
// MFMA: bf16 -> v_mfma_f32_16x16x32_bf16; f32 -> v_mfma_f32_16x16x4_f32 (exact f32 fma
// chain; gfx950 has no xf32).  For f32 each lane's 16-byte fragment holds 4 consecutive
// channels that feed 4 successive 16x16x4 steps - the reduction order inside a 32-channel
// chunk is permuted identically for A and W, which only reorders the fp32 sum.
//
// Workgroup -> tile map is XCD-aware: blocks that land on one XCD (blockIdx % 8) share the
// weight panel (tile_n) and a contiguous run of M tiles (shared 3x3 halo rows stay in that L2).
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "conv_gemm_dma.h"      // (conv_gemm_common.h + epilogue_split; the LDS-DMA kernel itself is instantiated in kernels_gemm_dma_*.hip)

namespace nope {

namespace {

// out = act(sum_z part[z] + bias + resid): NHWC T, or NCHW f32 (out_nchw).
template <class T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int splits, int M, int Cout,
                                                            const float* __restrict__ bias, const T* __restrict__ resid, int act,
                                                            T* __restrict__ out, int out_nchw, int HWo) {
    const size_t MN = (size_t)M * Cout;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < MN; i += (size_t)gridDim.x * 256) {
        const int n = (int)(i % Cout);
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += part[(size_t)z * MN + i];
        if (bias) v += bias[n];
        if (resid) v += Elt<T>::ld(resid + i);
        if (act) v = v > 0.f ? v : 0.f;
        if (out_nchw) {
            const size_t m = i / Cout;
            const size_t b = m / HWo;
            reinterpret_cast<float*>(out)[(b * Cout + n) * HWo + (m - b * HWo)] = v;
        } else Elt<T>::st(out + i, v);
    }
}

// The same reduction for NHWC outputs that feed a GroupNorm: one thread per column walks the `rows` rows of a statistics block
// (rows = min(H W, 64): whole samples or 64-row blocks of one sample), so the (sum, sum of squares) of what it writes -- f32, before the
// rounding to T, like the conv epilogues' -- come for free: colstats[M / rows][Cout][2], one writer per entry.  Grid (M / rows, Cout / 256).
template <class T>
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const float* __restrict__ part, int splits, int M, int Cout,
                                                                  const float* __restrict__ bias, int act, T* __restrict__ out,
                                                                  float* __restrict__ colstats, int rows) {
    // 64 columns x 4 row quarters per workgroup; a thread adds the partials of its rows / 4 rows (all split loads of a row in flight
    // at once), the four quarters of a column are then added in row order by its first thread.  Grid (M / rows, Cout / 64).
    __shared__ float s_s[4][64], s_q[4][64];
    const int c = threadIdx.x & 63, rq = threadIdx.x >> 6;
    const int n = blockIdx.y * 64 + c;
    const size_t MN = (size_t)M * Cout;
    const int rper = rows >> 2;
    const int m0 = blockIdx.x * rows + rq * rper;
    float s = 0.f, q = 0.f;
    if (n < Cout) {
        const float bv = bias ? bias[n] : 0.f;
        for (int r = 0; r < rper; ++r) {
            const size_t i = (size_t)(m0 + r) * Cout + n;
            float pv[16];
#pragma unroll
            for (int z = 0; z < 16; ++z) pv[z] = z < splits ? part[(size_t)z * MN + i] : 0.f;
            float v = 0.f;
#pragma unroll
            for (int z = 0; z < 16; ++z) if (z < splits) v += pv[z];
            v += bv;
            if (act) v = v > 0.f ? v : 0.f;
            Elt<T>::st(out + i, v);
            s += v; q += v * v;
        }
    }
    s_s[rq][c] = s; s_q[rq][c] = q;
    __syncthreads();
    if (rq == 0 && n < Cout) {
        float S = 0.f, Q = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { S += s_s[k][c]; Q += s_q[k][c]; }
        float* cs = colstats + ((size_t)blockIdx.x * Cout + n) * 2;
        cs[0] = S; cs[1] = Q;
    }
}

// Source pixel of output pixel (oy, ox) under tap (dy, dx); false = zero padding / beyond M.
__device__ __forceinline__ bool tap_pixel(const ConvParams& p, int oy, int ox, int dy, int dx, int& iy, int& ix) {
    if (p.mode == NOPE_CONV_DOWN2) { iy = 2 * oy + dy; ix = 2 * ox + dx; return oy >= 0; }
    if (p.mode == NOPE_CONV_STRIDE2) {   // stride 2, pad 1 (3x3) / pad 0 (1x1); s2_off = 1: 3x3 with pad (0, 1, 0, 1) (NOPE_CONV_STRIDE2_PAD01)
        iy = 2 * oy + dy + p.s2_off; ix = 2 * ox + dx + p.s2_off;
        return oy >= 0 && iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
    }
    if (p.mode == NOPE_CONV_UP2P) {   // rows are source pixels; (dy, dx) already include the phase shift
        iy = oy + dy; ix = ox + dx;
        return iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
    }
    if (p.mode == NOPE_CONV_UP2) {
        const int uy = oy + dy, ux = ox + dx;
        iy = uy >> 1; ix = ux >> 1;
        return uy >= 0 && uy < p.Ho && ux >= 0 && ux < p.Wo;
    }
    iy = oy + dy; ix = ox + dx;
    return iy >= 0 && iy < p.Hs && ix >= 0 && ix < p.Ws;
}
__device__ __forceinline__ void tap_delta(const ConvParams& p, int tap, int& dy, int& dx) {
    dy = 0; dx = 0;
    if (p.mode == NOPE_CONV_DOWN2) { dy = tap >> 1; dx = tap & 1; }
    else if (p.mode == NOPE_CONV_UP2P) { dy = (tap >> 1) + ((int)blockIdx.y >> 1) - 1; dx = (tap & 1) + ((int)blockIdx.y & 1) - 1; }
    else if (p.ntaps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
    else if (p.ntaps == 16) { dy = (tap >> 2) - 1; dx = (tap & 3) - 1; }      // 4x4, pad 1 (STRIDE2 only)
}

// ---- generic kernel: global -> VGPR -> LDS staging, any channel counts ----------------------------
template <class T, bool PN>
__global__ __launch_bounds__(NT, 2) void conv_gemm_kernel(ConvParams p) {
    constexpr int VEC = Elt<T>::VEC;
    constexpr int BK = 8 * VEC;
    constexpr int ES = (int)sizeof(T);
    constexpr int LDS_BYTES = (BM + BN) * ROWB > 4 * Ep<T>::WAVE_BYTES ? (BM + BN) * ROWB : 4 * Ep<T>::WAVE_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];   // K-step tile, then the epilogue panels
    unsigned char* ldsA = lds;
    unsigned char* ldsB = lds + BM * ROWB;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int tile_m, tile_n;
    tile_coords(p, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int slot = tid & 7;
    const int rbase = tid >> 3;
    const int HWo = p.Hm * p.Wm;
    const int Cin = p.C1 + p.C2;
    const unsigned char* wbase = p.w + (size_t)blockIdx.y * p.w_phase_bytes;

    int a_s1[A_ITERS], a_s2[A_ITERS], a_oy[A_ITERS], a_ox[A_ITERS];
#pragma unroll
    for (int i = 0; i < A_ITERS; ++i) {
        const int m = m0 + rbase + 32 * i;
        const bool ok = m < p.M;
        const int mm = ok ? m : 0;
        const int b = mm / HWo;
        const int r = mm - b * HWo;
        const int oy = r / p.Wm;
        a_oy[i] = ok ? oy : -100000;   // poisons the bounds test for rows beyond M
        a_ox[i] = r - oy * p.Wm;
        a_s1[i] = b / p.rep1;
        a_s2[i] = b / p.rep2;
    }

    const int kc_per_tap = (Cin + BK - 1) / BK;
    const int nk = p.ntaps * kc_per_tap;

    u32x4 ra[A_ITERS], rb[B_ITERS];
    int ld_tap = 0, ld_kc = 0;

    auto load_step = [&]() {
        const int c = ld_kc * BK + slot * VEC;
        int dy, dx;
        tap_delta(p, ld_tap, dy, dx);
        const bool c_ok = c < Cin;
        const bool first = c < p.C1;
        const unsigned char* sbase = first ? p.src1 : p.src2;
        const int cs = first ? c : c - p.C1;
        const int Cs = first ? p.C1 : p.C2;
#pragma unroll
        for (int i = 0; i < A_ITERS; ++i) {
            int iy, ix;
            const bool ok = tap_pixel(p, a_oy[i], a_ox[i], dy, dx, iy, ix) && c_ok;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ok) {
                const int sb = first ? a_s1[i] : a_s2[i];
                const size_t pix = ((size_t)sb * p.Hs + iy) * p.Ws + ix;
                v = ld16(sbase + (pix * Cs + cs) * ES);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int j = 0; j < B_ITERS; ++j) {
            const int n = n0 + rbase + 32 * j;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (n < p.Cout && c_ok) v = ld16(wbase + (((size_t)n * p.ntaps + ld_tap) * Cin + c) * ES);
            rb[j] = v;
        }
        if (++ld_kc == kc_per_tap) { ld_kc = 0; ++ld_tap; }
    };

    typename Tile<T>::acc_t acc[Tile<T>::MT][Tile<T>::NTL];
#pragma unroll
    for (int i = 0; i < Tile<T>::MT; ++i)
#pragma unroll
        for (int j = 0; j < Tile<T>::NTL; ++j)
#pragma unroll
            for (int r = 0; r < Tile<T>::R; ++r) acc[i][j][r] = 0.f;

    load_step();
    for (int ks = 0; ks < nk; ++ks) {
#pragma unroll
        for (int i = 0; i < A_ITERS; ++i) st16(ldsA + lds_off_rb<ROWB>(rbase + 32 * i, slot), ra[i]);
#pragma unroll
        for (int j = 0; j < B_ITERS; ++j) st16(ldsB + lds_off_rb<ROWB>(rbase + 32 * j, slot), rb[j]);
        __syncthreads();
        if (ks + 1 < nk) load_step();   // global loads for step ks+1 fly under the MFMAs below
        mma_stage<T, ROWB>(ldsA, ldsB, wm, wn, lane, acc);
        __syncthreads();
    }
    if (PN) {
        if (p.wide_out) epilogue_wide<T, true>(p, acc, m0, n0, wm, wn, lane, lds + wave * Ep<T>::WAVE_BYTES);
        else epilogue<T, true>(p, acc, m0, n0, wm, wn, lane);
    } else {
        if (p.wide_out) epilogue_wide<T, false>(p, acc, m0, n0, wm, wn, lane, lds + wave * Ep<T>::WAVE_BYTES);
        else if (p.nchw_staged) epilogue_nchw<T>(p, acc, m0, n0, wm, wn, lane, lds + wave * Ep<T>::WAVE_BYTES);
        else epilogue<T, false>(p, acc, m0, n0, wm, wn, lane);
    }
}

}  // namespace

constexpr int POSMAJOR_MAX_HW = 64;

void launch_conv_dma_f32(const void* params, int bm, dim3 grid, hipStream_t s);            // kernels_gemm_dma_*.hip
void launch_conv_dma_bf16x3(const void* params, dim3 grid, hipStream_t s);
void launch_conv_dma_f16(const void* params, dim3 grid, hipStream_t s);
void launch_conv_dma_bf16(const void* params, dim3 grid, hipStream_t s);
void launch_conv_dma_bf16_variant(const void* params, int bm, dim3 grid, hipStream_t s);
void launch_conv_pp(int dt, const void* params, dim3 grid, hipStream_t s);   // kernels_gemm_pp.hip
void launch_conv_small(int dt, const void* params, int tile, dim3 grid, hipStream_t s);   // kernels_gemm_small.hip
void launch_conv_halo(int dt, const void* params, dim3 grid, hipStream_t s);
void launch_conv_stream(int dt, const void* params, dim3 grid, hipStream_t s);   // kernels_gemm_stream.hip
int conv_halo_max_width();

// ---- the planner's switches: conv_switches is the ONE place that names them; read per plan (tests and tuning sweeps toggle them: nope_tuning_reload),
// ---- each with its default and meaning here, the reasons and measurements with the policy that uses it.  (NOPE_CONV_TRACE is launch_conv's.)
struct OptSwitch { bool set; int val; };      // a switch for which "unset" is not one of its values
#define NOPE_ENV_OPT(name) ({ static ::nope::EnvCache nope_env_c__; const ::nope::EnvVal nope_env_v__ = ::nope::env_lookup(nope_env_c__, name); OptSwitch{nope_env_v__.set, (int)nope_env_v__.val}; })
struct ConvSwitches {
    int pp, variant, small_mode, small_max_tiles, small_1x1_maxk, small_deep_max, small_kg2_max, halo_split_min_chunks, halo_split_max_tiles, halo_min_tiles, halo_persist, up2p_halo;
    int stream, stream_grid, stream_min_iters, persist_grid, geglu_fused;
    bool halo_split, x2_small, x2_pp, geglu_fused_f32, stats16, nchw_staged, xcd_one_panel, xcd_any, persist, lean, halo_padskip;
    OptSwitch small_tile, xcd_gn, pp_variant;
};
static ConvSwitches read_switches(int dt) {      // dt: a base type (the default of NOPE_CONV_PP depends on it)
    ConvSwitches s;
    s.pp = NOPE_ENV("NOPE_CONV_PP", dt != NOPE_F32 ? 3 : 0);                 // bit set: which launches take the ping-pong kernels (choose_kernel)
    s.variant = NOPE_ENV("NOPE_CONV_VARIANT", 0);                            // tuning variants of the 128 x 192 kernel (4: the 256 x 192 / 8-wave tile); ConvParams::variant
    s.small_mode = NOPE_ENV("NOPE_CONV_SMALL", 1);                           // small-tile kernel: 0 never, 1 by tile count, 2 whenever it applies (tests)
    s.small_tile = NOPE_ENV_OPT("NOPE_SMALL_TILE");                          // forces its tile (0..3); unset: small_tile decides
    s.small_max_tiles = NOPE_ENV("NOPE_SMALL_MAX_TILES", 320);               // launches with fewer 128 x 192 tiles take the small-tile kernel
    s.small_1x1_maxk = NOPE_ENV("NOPE_SMALL_1X1_MAXK", 0);                   // 1x1 convs of any size with at most this many K steps take it too (0: off)
    s.small_deep_max = NOPE_ENV("NOPE_SMALL_DEEP_MAX", 0);                   // tile 2 (6-stage ring) for at most this many 64 x 64 tiles (0: off)
    s.small_kg2_max = NOPE_ENV("NOPE_SMALL_KG2_MAX", 256);                   // tile 3 (two K groups) for at most this many 64 x 64 tiles
    s.halo_split = NOPE_ENV("NOPE_HALO_SPLIT", -1) != 0;                     // 0: no K splits on the tap-resident kernel
    s.halo_split_min_chunks = NOPE_ENV("NOPE_HALO_SPLIT_MIN_CHUNKS", 12);    // ... only from this many channel chunks on
    s.halo_split_max_tiles = NOPE_ENV("NOPE_HALO_SPLIT_MAX_TILES", 128);     // ... and up to this many 256 x 192 tiles
    s.halo_min_tiles = NOPE_ENV("NOPE_HALO_MIN_TILES", 128);                 // long 3x3 convs take the tap-resident kernel from this many tiles on
    s.halo_persist = NOPE_ENV("NOPE_HALO_PERSIST", 256);                     // workgroups of its tile walk (0: one tile per workgroup)
    s.up2p_halo = NOPE_ENV("NOPE_UP2P_HALO", 1);                             // phase convs tap-resident: 0 never, 1 two-pass layers, 2 bf16x3 too
    s.halo_padskip = NOPE_ENV("NOPE_HALO_PADSKIP", 1) != 0;                  // 0: 4 x 4 maps in (sample, position) order, every block-tap executed (A/B)
    s.stream = NOPE_ENV("NOPE_CONV_STREAM", 0);                              // streaming 1x1 kernel: bit 0 the 128 x 192 kernel's launches, bit 1 the per-tap ping-pong kernel's
    s.stream_grid = NOPE_ENV("NOPE_STREAM_GRID", 256);                       // its workgroups: one per CU (the tests walk small grids); a multiple of 8, else 256
    if (s.stream_grid < 8 || s.stream_grid % 8) s.stream_grid = 256;
    s.stream_min_iters = NOPE_ENV("NOPE_STREAM_MIN_ITERS", 2);               // ... from this many tiles per workgroup on
    s.x2_small = NOPE_ENV("NOPE_X2_SMALL", 0) != 0;                          // two-pass tile on the small-tile kernel too
    s.x2_pp = NOPE_ENV("NOPE_X2_PP", 1) != 0;                                // 0: two-pass tile on the tap-resident kernel only
    s.geglu_fused = NOPE_ENV("NOPE_GEGLU_FUSED", 1);                         // conv_geglu_fusable: 0 never, 2 only launches the 128 x 192 kernel would get anyway
    s.geglu_fused_f32 = NOPE_ENV("NOPE_GEGLU_FUSED_F32", 1) != 0;            // 0: no GEGLU epilogue on f32 storage (A/B)
    s.stats16 = NOPE_ENV("NOPE_STATS16", -1) != 0;                           // 0: the 128 x 192 / ping-pong kernels leave 16-pixel maps to gn_stats (A/B)
    s.nchw_staged = NOPE_ENV("NOPE_NCHW_STAGED", -1) != 0;                   // 0: NCHW output never through the LDS panels
    s.xcd_one_panel = NOPE_ENV("NOPE_XCD_MAP", -1) == 1;                     // 1: one weight panel per XCD (no map 2)
    s.xcd_gn = NOPE_ENV_OPT("NOPE_XCD_GN");                                  // tests: forces the XCD columns of map 2
    s.xcd_any = NOPE_ENV("NOPE_XCD_ANY", -1) != 0;                           // 0: no map 4 for panel counts outside {1, 2, 4, 8}
    s.persist = NOPE_ENV("NOPE_CONV_PERSIST", 1) != 0;                       // 0: the 128 x 192 kernel walks no tiles
    s.persist_grid = NOPE_ENV("NOPE_PERSIST_GRID", 512) == 256 ? 256 : 512;  // workgroups of that walk (tuning: 256 = one per CU)
    s.lean = NOPE_ENV("NOPE_EPILOGUE_LEAN", 1) != 0;                         // 0: the generic row loop everywhere (A/B)
    s.pp_variant = NOPE_ENV_OPT("NOPE_PP_VARIANT");                          // tuning ablations of the ping-pong kernels: their ConvParams::variant; no GroupNorm tail
    return s;
}
// The switches of a plan: read again whenever nope_tuning_reload has started a new generation, else the calling thread's last reading
// (a plan looks at the generation once instead of at thirty call sites; the U-Net plans ~100 launches per step)
static const ConvSwitches& conv_switches(int dt) {
    thread_local ConvSwitches cached[2];
    thread_local unsigned gen[2] = {0xffffffffu, 0xffffffffu};
    const int k = dt == NOPE_F32 ? 1 : 0;
    const unsigned g = tuning_generation();
    if (gen[k] != g) { cached[k] = read_switches(dt); gen[k] = g; }
    return cached[k];
}

// ---- the pieces conv_plan is built on; conv_stat_rows and conv_splitk_factor, which a caller asks BEFORE it has the scratch a plan needs,
// ---- read the same ones.  `dt` is a base type everywhere below (NOPE_F16X2 plans as NOPE_BF16X3: same storage, same tiles).

// Sizes of a launch, computed once: M = GEMM rows (source pixels for the phase convs of an up-sampling), b1 / b2 / bw = bytes of the two
// sources and of one phase's weights.  (rep < 1 is refused by conv_plan; the pre-queries, which validate nothing, must not divide by it.)
struct ConvSizes { int vec, es, bk, Cin; bool phased; long long M; unsigned long long b1, b2, bw; };
static ConvSizes conv_sizes(int dt, const ConvArgs& a) {
    const int es = dt_es(dt), Cin = a.C1 + a.C2;
    const bool phased = a.mode == NOPE_CONV_UP2P;
    return {dt_vec(dt), es, 8 * dt_vec(dt), Cin, phased, (long long)a.nhyp * (phased ? a.Hs * a.Ws : a.Ho * a.Wo),
            (unsigned long long)cdiv(a.nhyp, a.rep1 < 1 ? 1 : a.rep1) * a.Hs * a.Ws * a.C1 * es, a.C2 ? (unsigned long long)cdiv(a.nhyp, a.rep2 < 1 ? 1 : a.rep2) * a.Hs * a.Ws * a.C2 * es : 0,
            (unsigned long long)a.Cout * a.ntaps * Cin * es};
}

// LDS-DMA kernels: a K step (128 B of channels) never straddles sources and 32-bit offsets suffice
// (the 4x4 stride-2 conv of the non-default soft downsampling runs on the generic kernel: its tap geometry is not a 3x3 mask)
static bool takes_dma(const ConvArgs& a, const ConvSizes& z) {
    const unsigned long long lim = 0x7fffffffULL;
    return !a.force_generic && a.ntaps != 16 && z.Cin % z.bk == 0 && (a.C2 == 0 || (a.C1 % z.bk == 0 && a.mode == NOPE_CONV_PLAIN)) && z.b1 < lim && z.b2 < lim && z.bw < lim;
}

// What the policies below ask about a launch more than once, computed ONCE per plan and per pre-query (conv_facts), so that choose_kernel,
// stat_rows and splitk_factor cannot disagree.  None of it looks at the scratch or at `colstats`.
struct ConvFacts {
    ConvSizes z;
    bool dma;              // takes_dma
    long long tiles256;    // 256 x 192 tiles of one phase
    bool x2_layer;         // a layer whose second weight pack the two-pass tile can run (which kernels run it: plan_kernel)
    int hsplit;            // halo_split_factor: K splits the tap-resident kernel would take (1: none); granted only where the scratch holds them
    int small;             // small_tile: -1, or the tile of the small-tile kernel
};

// Launches that cannot give every CU a 128 x 192 tile take the small-tile kernel (kernels_gemm_small.hip): fewer than
// NOPE_SMALL_MAX_TILES tiles of 128 x 192.  -1, or the tile (ConvLaunch::small).  (Reads f.z, f.dma, f.tiles256.)
static int small_tile(int dt, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f) {
    const ConvSizes& z = f.z;
    if (!f.dma || a.geglu) return -1;          // (GEGLU epilogue: an instantiation of the 128 x 192 kernel only)
    if (s.small_mode == 0 || a.mode == NOPE_CONV_UP2 || a.ntaps == 16 || a.force_generic) return -1;
    if (a.out_nchw && a.pn_ms) return -1;      // (the small-tile kernel's NCHW epilogue has no fused PreNorm: the 128 x 192 kernel's generic epilogue does)
    if (s.small_mode == 1 && (s.pp & 8)) return -1;      // bit 3 = "ping-pong kernels at ANY tile count" (their tests)
    const int ph = z.phased ? 4 : 1, nk1 = z.Cin / z.bk;
    const long long tiles128 = (long long)cdiv((int)z.M, BM) * cdiv(a.Cout, BN) * ph;
    // Short-K 1x1 convs of ANY size (NOPE_SMALL_1X1_MAXK = K steps, default 0 = off): their 128 x 192 launches are bound by the epilogue
    // of a three-K-step tile, not by HBM (192 -> 384 at 32 x 32 x 512: 604 MB in 221 us = 2.7 TB/s); the 128 x 128 small tile has a one-pass
    // epilogue.
    if (s.small_mode == 1 && a.mode == NOPE_CONV_PLAIN && a.ntaps == 1 && !a.out_nchw && nk1 <= s.small_1x1_maxk && tiles128 >= s.small_max_tiles)
        return s.small_tile.set ? s.small_tile.val : 1;      // (as given: not clamped here)
    if (s.small_mode == 1 && tiles128 >= s.small_max_tiles) return -1;
    if (s.small_mode == 1 && dt != NOPE_F32 && a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && a.Ws <= conv_halo_max_width() && a.rep1 == 1 && !a.out_nchw &&
        !a.pn_ms && a.Cout % z.vec == 0 && 9 * nk1 >= 54 && f.tiles256 >= 128)
        return -1;       // the tap-resident kernel has its 128 tiles of 256 rows (measured at 16 x 16 x 64: 60.6 / 83 us against 83 / 116 us on 64 x 64 tiles)
    if (s.small_tile.set) return s.small_tile.val < 0 || s.small_tile.val > 3 ? 0 : s.small_tile.val;
    const long long tiles64 = (long long)cdiv((int)z.M, 64) * cdiv(a.Cout, 64) * ph;
    if (tiles64 > 1536) return 1;
    // (tile 2, the 6-stage ring, for launches of at most NOPE_SMALL_DEEP_MAX tiles with a K loop of >= 8 steps: with 512 -- launches that
    //  the 48 KiB ring runs two workgroups per CU -- measured SLOWER than the 3-stage ring, 26 / 64 templates 4.16 / 4.95 ms against
    //  4.04 / 4.81, profiles/r04e_small_bank_sweep.txt; off by default)
    const int nk = a.ntaps * nk1;
    if (tiles64 <= s.small_deep_max && nk >= 8) return 2;
    // at most one workgroup per CU and a long K: two wave groups per tile on alternate K steps (tile 3)
    return (tiles64 <= s.small_kg2_max && nk >= 12) ? 3 : 0;
}

// 3x3 convs with FEW 256 x 192 tiles and a LONG K (the 4 x 4 / 8 x 8 levels of the U-Net at a few dozen pose hypotheses: 16-64 tiles
// of 100-200 K steps) run on the tap-resident kernel with the channel chunks split over blockIdx.z (f32 partials + the fixed-order
// reduce): its 256-row tiles move a third of the L2 -> LDS bytes per flop of the 128 x 192 kernel, which is what bounds these
// launches (profiles/r04b: 51 us for 1536 -> 1536 at 4 x 4 x 64 on the 128 x 192 kernel split 8 ways = 1.9 us per K step, 111 us on 64 x 64
// tiles).  Returns the number of splits (1: does not apply).  NOPE_HALO_SPLIT=0 turns it off.
static int halo_split_factor(const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f) {      // (reads f.z, f.tiles256)
    const ConvSizes& z = f.z;
    if (!s.halo_split || !(s.pp & 1) || (s.pp & 16)) return 1;
    if (a.mode != NOPE_CONV_PLAIN || a.ntaps != 9 || a.Ws > conv_halo_max_width() || a.rep1 != 1 || a.out_nchw || a.pn_ms ||
        a.force_generic || a.Cout % z.vec || z.Cin % z.bk || (a.C2 && a.C1 % z.bk)) return 1;
    const int nchunks = z.Cin / z.bk;
    const long long tiles = f.tiles256;
    // 128 tiles split in two fill the 256 CUs in one round (256 hypotheses at the 4 x 4 level: 11.35 -> 10.76 ms per step, run t); above that a
    // split needs a second round of workgroups and loses (176 tiles, 341 hypotheses: 14.8 -> 15.3 ms)
    if (tiles < 1 || tiles > s.halo_split_max_tiles || nchunks < s.halo_split_min_chunks) return 1;      // (tiles < 1: the empty launch of a pre-query that validates nothing)
    // as many splits as fit ONE round of 256 workgroups (one per CU: 158 KiB of LDS each): 88 tiles x 3 = 264 would run a second
    // round for 8 of them
    int S = (int)(256 / tiles);
    if (S > nchunks) S = nchunks;
    if (S > 16) S = 16;
    return S < 2 ? 1 : S;
}

static ConvFacts conv_facts(int dt, const ConvArgs& a, const ConvSwitches& s) {
    ConvFacts f;
    f.z = conv_sizes(dt, a);
    f.dma = takes_dma(a, f.z);
    f.tiles256 = (long long)cdiv((int)f.z.M, 256) * cdiv(a.Cout, BN);
    f.x2_layer = a.w_x2 && !a.pn_ms && !a.geglu && f.z.Cin % 32 == 0;
    f.hsplit = halo_split_factor(a, s, f);
    f.small = small_tile(dt, a, s, f);
    return f;
}

// Split-K factor for a conv that would otherwise leave most of the 256 CUs idle (few output tiles, long K):
// enough K slices to reach ~2 workgroups per CU, at least 4 K steps each.  1 = do not split.
static int splitk_factor(const ConvArgs& a, const ConvFacts& f) {
    const ConvSizes& z = f.z;
    if (f.hsplit > 1) return f.hsplit;      // long 3x3 convs with few tiles: split-K on the tap-resident kernel (its reduce kernel also serves a colstats request)
    if (a.colstats || a.gn_self || a.pn_ms || a.mode == NOPE_CONV_UP2P || a.mode == NOPE_CONV_UP2) return 1;      // (gn_self: planned as the launch with fused statistics it replaces)
    if (z.Cin % z.bk) return 1;
    if (f.small >= 0) return 1;          // the small-tile kernel has enough workgroups without splitting K
    const long long tiles = (long long)cdiv((int)z.M, BM) * cdiv(a.Cout, BN);
    const int nk = a.ntaps * (z.Cin / z.bk);
    if (tiles > 128 || nk < 8) return 1;
    int S = (int)((512 + tiles - 1) / tiles);
    if (S > nk / 4) S = nk / 4;
    if (S > 16) S = 16;
    return S < 2 ? 1 : S;
}
int conv_splitk_factor(int dt, const ConvArgs& a) { return splitk_factor(a, conv_facts(dt_base(dt), a, conv_switches(dt_base(dt)))); }

// Fused GroupNorm column statistics, rows per block (0: this conv cannot emit them): 64 wherever samples are whole 64-row blocks; 16 on
// 16-pixel maps (the 4 x 4 level: per-sample blocks, every LDS-DMA kernel's wide epilogue, the small-tile kernel, the split-K reduce) -- which
// removes that level's gn_stats passes; 32 on 32-pixel maps from the small-tile kernel and the split-K reduce.
static int stat_rows(const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f) {
    const ConvSizes& z = f.z;
    if (z.phased || a.resid || a.out_nchw || a.Cout % z.vec || a.Cout > 2048) return 0;
    const long long HW = (long long)a.Ho * a.Wo;
    if (HW % 64 == 0) return 64;
    // 16-pixel maps (the 4 x 4 level): per-sample blocks of 16 rows -- every kernel with the wide epilogue, the small-tile kernel and the
    // split-K reduce emit them; 32-pixel maps only the latter two ("small or split" whether or not a scratch will hold the split)
    const bool small_or_split = f.hsplit > 1 || f.small >= 0;
    if (HW == 16 && z.M % 16 == 0 && (small_or_split || (s.stats16 && f.dma))) return 16;
    if (HW == 32 && z.M % 32 == 0 && small_or_split) return 32;
    return 0;
}
int conv_stat_rows(int dt, const ConvArgs& a) { const ConvSwitches& s = conv_switches(dt_base(dt)); return stat_rows(a, s, conv_facts(dt_base(dt), a, s)); }
int conv_tail_stat_blocks(int HW, int Cout) { return HW / 64 * cdiv(Cout, 96); }

// Which kernel a conv asks for.  NOPE_CONV_PP (tuning; default 3): bit 0 = the 256 x 192 ping-pong kernels for launches with
// at least one 256-row tile per CU, bit 1 = also for the small-map 3x3 convs that would otherwise run position-major on
// the 128 x 192 kernel (they then run in standard row order, all 9 taps, on the tap-resident kernel: 239 vs 257 us for
// 1536 -> 1536 at 4 x 4 x 512 although it executed the 31 % of MACs the position-major order skips; since then the tap-resident kernel's PADSKIP form,
// plan_epilogue, leaves out those that are padding for a whole 32-row block of a (position, sample) stage, 1/6 of the K loop), bit 2 = those run position-major on the
// ping-pong kernel (needs nhyp % 256 == 0), bit 3 = no minimum tile count (tests: small shapes on the ping-pong kernel),
// bit 4 = 3x3 convs per tap on the ping-pong kernel instead of the tap-resident (halo) kernel.
struct KernelChoice { bool pp, posmajor, halo; int small; int hsplit; bool stream; };      // hsplit > 1: tap-resident kernel with that many K splits; stream: asked for -- plan_walks keeps it only if the grid fits
static KernelChoice choose_kernel(int dt, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f) {
    // (the default of NOPE_CONV_PP: f32 -- the parity mode -- stays on the 128 x 192 kernel unless asked: its MFMA phase is
    //  16x longer per K step, loads were never its bound, and two workgroups per CU beat one: 126 vs 135 ms per 512-template step)
    const ConvSizes& z = f.z;
    const int pp_mode = s.pp, variant = s.variant;
    KernelChoice pl{false, false, false, -1, 1, false};
    if (!f.dma || a.geglu) return pl;          // (GEGLU epilogue: an instantiation of the 128 x 192 kernel only)
    if (a.splitk_ws && f.hsplit > 1 && (size_t)f.hsplit * (size_t)z.M * a.Cout * 4 <= a.splitk_bytes) { pl.pp = pl.halo = true; pl.hsplit = f.hsplit; return pl; }      // the split only where the scratch holds it
    pl.small = f.small;
    if (pl.small >= 0) return pl;
    const bool small3x3 = a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && !a.colstats && !a.gn_self && !a.pn_ms && !a.out_nchw && !a.splitk_ws &&
                          a.Hs * a.Ws <= POSMAJOR_MAX_HW;
    const bool posmajor128 = small3x3 && a.nhyp % BM == 0 && !(variant & 8) && variant != 4;
    // (short K loops -- the 1x1 convs around the attention blocks, 2-3 K steps per tile -- stay on the 128 x 192 kernel, whose two
    //  workgroups per CU cover each other's prologue and epilogue: measured 193 vs 234 us for 192 -> 384 at 32 x 32)
    // (long 3x3 launches take the tap-resident kernel from 128 tiles on -- NOPE_HALO_MIN_TILES: the 768 -> 768 convs of the 4 x 4
    //  level at 512 hypotheses have 128 tiles of 108 K steps; on half the CUs they still beat the position-major 128 x 192 launch,
    //  one workgroup per CU: 20.26 -> 20.19 ms per step, profiles/r03d_defaults_ab.txt)
    const long long min_tiles = (a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && a.ntaps * (z.Cin / z.bk) >= 54) ? s.halo_min_tiles : 256;
    const bool pp_shape = (a.mode == NOPE_CONV_PLAIN || a.mode == NOPE_CONV_DOWN2 || z.phased) && !a.out_nchw && a.Cout % z.vec == 0 &&
                          ((pp_mode & 8) || a.ntaps * (z.Cin / z.bk) >= 12) &&
                          ((pp_mode & 8) || f.tiles256 * (z.phased ? 4 : 1) >= min_tiles) && variant == 0;
    if (pp_shape && (pp_mode & 1)) {
        if (!posmajor128) pl.pp = true;
        else if ((pp_mode & 4) && a.nhyp % 256 == 0) { pl.pp = true; pl.posmajor = true; }
        else if (pp_mode & 2) pl.pp = true;
    }
    if (!pl.pp) pl.posmajor = posmajor128;
    // 3x3 convs in standard row order on the ping-pong schedule keep their A operand in LDS across the 9 taps (bit 4 = off)
    // (the first source must not be broadcast: its A offsets are linear in the flat pixel index; a broadcast second source is fine)
    pl.halo = pl.pp && !pl.posmajor && a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && a.Ws <= conv_halo_max_width() && a.rep1 == 1 &&
              !(pp_mode & 16);
    // ... and so do the four phase convs of an up-sampling (conv3x3_halo_kernel<..., UP>: the stage is the 3 x 3 neighbourhood the phases' 2 x 2 taps
    // come from) under the two-pass tile, whose per-tap launches are bound by staging 256 f32 rows per tap and splitting them in registers at every
    // read: 512-hypothesis launches 0.77 / 0.72 / 0.67 -> ~0.59 ms, step -1.2 % (profiles/r06w_up2p_tap_resident_ab.txt).  As bf16x3 (three MFMA
    // passes per step: the per-tap kernel's LOAD phase is hidden) it is +-2 % per launch: per tap stays.  NOPE_UP2P_HALO: 0 = per tap, 2 = bf16x3 too.
    if (pl.pp && z.phased && !pl.posmajor && a.ntaps == 4 && dt == NOPE_BF16X3 && a.C2 == 0 && a.Ws <= 30 && a.rep1 == 1 && !(pp_mode & 16) &&      // (Ws <= 30: at most five A pieces per wave)
        (s.up2p_halo == 2 || (s.up2p_halo == 1 && f.x2_layer)))
        pl.halo = true;
    // The streaming 1x1 kernel (kernels_gemm_stream.hip: one persistent workgroup per CU, the activations through a five-stage ring that runs
    // across tile boundaries) for 1x1 convs with thousands of 128 x 192 tiles.  OFF by default: built on the premise that these HBM-bound
    // launches wait for memory round trips, measured 20-25 % SLOWER than the 128 x 192 kernel they would leave (profiles/r06h_stream_bench_*.txt,
    // r06l_*): what bounds them is the epilogue -- its instruction stream (the lean form of epilogue_wide took 12 % off) and, on gfx9, a wave's
    // stores draining through the same in-order vmcnt as its loads (r06i ablations: stores alone 166 us + MFMA 100 us + loads 96 us ~ the
    // launch's 375 us) -- and two workgroups per CU overlap that better than one.  NOPE_CONV_STREAM: bit 0 = the launches the 128 x 192 kernel
    // would take, bit 1 = also the long 1x1 convs of the per-tap ping-pong kernel; NOPE_STREAM_MIN_ITERS = tiles per workgroup from which on.
    const long long tm = z.M / BM, tn = cdiv(a.Cout, BN);
    if (s.stream && dt != NOPE_F32 && a.mode == NOPE_CONV_PLAIN && a.ntaps == 1 && !pl.posmajor && !a.out_nchw && a.Cout % z.vec == 0 && a.w &&
        a.rep1 == 1 && a.rep2 == 1 && variant == 0 && (!pl.pp || (s.stream & 2)) && z.M % BM == 0 && (tn == 1 || tn == 2 || tn == 4 || tn == 8) &&
        tm % 8 == 0 && (tm * tn) % s.stream_grid == 0 && (tm * tn) / s.stream_grid >= s.stream_min_iters) {
        pl.stream = true; pl.pp = false; pl.halo = false;
    }
    return pl;
}

// ---- conv_plan in stages, called in this order; each returns NOPE_OK or the error that refuses the launch (the order of the checks is the order of
// ---- the error codes), reads the switches `s` and the facts `f`, and fills its part of the ConvLaunch.

// The two argument rewrites, and what is wrong with the arguments by themselves
static int plan_arguments(int& dt, ConvArgs& a) {
    if (a.mode == NOPE_CONV_STRIDE2_PAD01) {      // Downsample2D(padding=0) / CompVis Downsample: pad (0, 1, 0, 1), 3x3, stride 2, no padding --
        // the STRIDE2 tiles with the centre tap one source pixel down and right; the bottom / right taps of the last row / column read the padding
        if (a.ntaps != 9 || a.C2 != 0 || a.s2_off != 0) return NOPE_ERR_ARG;
        a.mode = NOPE_CONV_STRIDE2; a.s2_off = 1;
    }
    if (a.s2_off && (a.mode != NOPE_CONV_STRIDE2 || a.ntaps != 9 || a.s2_off != 1)) return NOPE_ERR_ARG;
    if (dt == NOPE_F16X2) {      // as an element type (nope_op_conv): `w` is in the NOPE_F16X2 layout, which only the ping-pong kernels read
        if (a.w_x2) return NOPE_ERR_ARG;
        a.w_x2 = a.w; a.w = nullptr;
        dt = NOPE_BF16X3;
    }
    if (a.w_x2 && dt != NOPE_BF16X3) return NOPE_ERR_ARG;
    if (!a.src1 || (!a.w && !a.w_x2) || !a.out || a.C1 <= 0 || a.Cout <= 0 || a.nhyp <= 0) return NOPE_ERR_ARG;
    if (a.C2 > 0 && !a.src2) return NOPE_ERR_ARG;
    if (!dt_is_compute(dt)) return NOPE_ERR_UNSUPPORTED;
    if (a.C1 % dt_vec(dt) || a.C2 % dt_vec(dt)) return NOPE_ERR_UNSUPPORTED;
    if (dt == NOPE_BF16X3 && (a.C1 % 8 || a.C2 % 8)) return NOPE_ERR_UNSUPPORTED;     // (hi, lo) weight groups hold 8 channels
    if (a.rep1 < 1 || a.rep2 < 1) return NOPE_ERR_ARG;
    const bool same = a.Hs == a.Ho && a.Ws == a.Wo, up = a.Ho == 2 * a.Hs && a.Wo == 2 * a.Ws, down = a.Hs == 2 * a.Ho && a.Ws == 2 * a.Wo;
    if (!(a.mode == NOPE_CONV_PLAIN ? (a.ntaps == 1 || a.ntaps == 9) && same
          : a.mode == NOPE_CONV_UP2 ? a.ntaps == 9 && up
          : a.mode == NOPE_CONV_DOWN2 ? a.ntaps == 4 && down
          : a.mode == NOPE_CONV_UP2P ? a.ntaps == 4 && up && a.C2 == 0 && !a.out_nchw
          : a.mode == NOPE_CONV_STRIDE2 && (a.ntaps == 1 || a.ntaps == 9 || a.ntaps == 16) && down && a.C2 == 0)) return NOPE_ERR_ARG;
    return NOPE_OK;
}

// ... and with its sizes: the row count, and what a fused PreNorm, the column statistics and the GroupNorm tail ask of the arguments
static int plan_requests(const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f) {
    if (f.z.M > 0x7fffffffLL) return NOPE_ERR_UNSUPPORTED;
    const bool wide_out = !a.out_nchw && a.Cout % f.z.vec == 0;
    if (a.pn_ms && (!a.pn_c0 || !a.pn_c1 || a.mode != NOPE_CONV_PLAIN || a.ntaps != 1 || a.colstats)) return NOPE_ERR_ARG;
    // (act: the epilogues take the statistics before an activation, the split-K reduce after it -- nobody needs the pair)
    if (a.colstats && (!wide_out || f.z.phased || a.resid || a.act || a.stat_rows != stat_rows(a, s, f))) return NOPE_ERR_ARG;
    // GroupNorm tail on the residual (ConvArgs::gn_*): complete arguments here; that the launch is one whose epilogue has the tail, in plan_epilogue
    // (gn_G >= 1 is also what makes epilogue_wide's `tz` -- conv_gemm_common.h: a zero formed from `gn_G <= 0` -- a zero)
    if ((a.gn_ms || a.tail_stats) && (!a.gn_ms || !a.gn_gamma || !a.gn_beta || !a.resid || a.gn_G < 1 || a.Cout % a.gn_G || a.act || a.pn_ms || a.colstats ||
                                      ((uintptr_t)a.gn_ms & 7))) return NOPE_ERR_ARG;
    // The launch's own GroupNorm (ConvArgs::gn_self): complete arguments, none of the forms it replaces or cannot sit next to
    if (a.gn_self && (!a.gn_gamma || !a.gn_beta || a.gn_G < 1 || a.Cout % a.gn_G || a.gn_ms || a.tail_stats || a.resid || a.colstats || a.act || a.pn_ms || a.geglu ||
                      a.out_nchw || (a.gn_emb && a.gn_emb_stride < a.Cout))) return NOPE_ERR_ARG;
    return NOPE_OK;
}

// Kernel, tile, precision
static int plan_kernel(ConvLaunch& L, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f, KernelChoice& pick) {
    const int dt = L.dt;
    pick = choose_kernel(dt, a, s, f);
    L.small = pick.small;
    L.posmajor = pick.posmajor;
    // the f16 + MX-fp8 tile: launches of a layer that carries the second pack on a ping-pong kernel (tap-resident or per-tap) or -- round 6 -- on the
    // small-tile kernel (reference-sized banks, an 8-way shard).  NOPE_X2_PP=0: tap-resident only.  NOPE_X2_SMALL=1: also on the small-tile kernel
    // -- built, bit-identical to the ping-pong kernels, measured SLOWER than its bf16x3 form there (26 / 64 / 91 templates 7.29 / 9.13 / 11.47 ms
    // against 6.52 / 8.59 / 11.05, same box, profiles/r06c_small_tile_x2_ab.txt: a 64 x 64 tile's wave holds ONE accumulator, so its three MFMAs per
    // K step are a dependent chain either way and the register split costs more VALU than the third pass costs matrix time): off by default
    L.x2 = f.x2_layer && (pick.small >= 0 ? s.x2_small : pick.pp && (pick.halo || s.x2_pp));
    if (!L.x2 && !a.w) return NOPE_ERR_UNSUPPORTED;       // (NOPE_F16X2 as an element type on a shape the ping-pong kernels do not take)
    // ConvArgs::geglu: a plain 1x1 conv on the 128 x 192 LDS-DMA kernel's wide epilogue (no residual / statistics / PreNorm / activation / split):
    // 16-bit storage on the packed path, column pairs whole inside a lane's 8-column chunk and 8-byte output rows; f32 storage (round 6; NOPE_GEGLU_FUSED_F32=0:
    // A/B switch) in the generic row loop, two pairs per 4-column chunk
    if (a.geglu && !((f.z.es == 2 || s.geglu_fused_f32) && a.mode == NOPE_CONV_PLAIN && a.ntaps == 1 && !a.resid && !a.colstats && !a.pn_ms && !a.out_nchw &&
                     !a.act && !a.splitk_ws && a.Cout % 16 == 0 && f.dma && !pick.pp && pick.small < 0 && !pick.posmajor && s.variant == 0))
        return NOPE_ERR_UNSUPPORTED;
    if (a.colstats && a.stat_rows == 32 && pick.small < 0 && pick.hsplit <= 1) return NOPE_ERR_ARG;   // 32-row blocks: small-tile kernel or split-K reduce only
    if (a.colstats && a.stat_rows == 16 && pick.small < 0 && pick.hsplit <= 1 && (!f.dma || pick.posmajor)) return NOPE_ERR_ARG;
    // NOPE_CONV_VARIANT=4 selects the 256x192 / 8-wave tile (measured on par with the default 128x192 / 4-wave
    // tile in round 1; kept for tuning, see DESIGN.md section 4 for the other variants that were tried).
    L.bm = pick.small >= 0 ? (pick.small == 1 ? 128 : 64)
           : (pick.pp || (f.dma && s.variant == 4 && f.z.M >= 256 * 256 && (dt == NOPE_F32 || dt == NOPE_BF16))) ? 256 : BM;
    return NOPE_OK;
}

// The kernels' parameters: the arguments, the tile counts, the position-major row order
static int plan_params(ConvLaunch& L, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f, const KernelChoice& pick) {
    ConvParams& p = L.p;
    const ConvSizes& z = f.z;
    const bool phased = z.phased, dma = f.dma;
    const long long M = z.M;
    p.src1 = (const unsigned char*)a.src1; p.src2 = (const unsigned char*)a.src2;
    p.C1 = a.C1; p.C2 = a.C2; p.rep1 = a.rep1; p.rep2 = a.rep2;
    p.Hs = a.Hs; p.Ws = a.Ws; p.Ho = a.Ho; p.Wo = a.Wo;
    p.Hm = phased ? a.Hs : a.Ho; p.Wm = phased ? a.Ws : a.Wo;
    p.mode = a.mode; p.ntaps = a.ntaps; p.s2_off = a.s2_off;
    p.w = (const unsigned char*)a.w; p.bias = a.bias; p.resid = (const unsigned char*)a.resid;
    p.out = (unsigned char*)a.out; p.Cout = a.Cout; p.M = (int)M;
    p.out_nchw = a.out_nchw; p.out_dt = a.out_dt;
    p.act = a.act;
    p.wide_out = !a.out_nchw && a.Cout % z.vec == 0 ? 1 : 0;
    p.nchw_staged = (a.out_nchw && !a.resid && !a.pn_ms && M % 64 == 0 && ((long long)a.Ho * a.Wo) % 64 == 0 && s.nchw_staged) ? 1 : 0;
    p.colstats = a.colstats;
    p.stat_rows = a.stat_rows;
    p.pn_ms = a.pn_ms; p.pn_c0 = a.pn_c0; p.pn_c1 = a.pn_c1;
    p.w_phase_bytes = phased ? (unsigned)z.bw : 0u;
    p.x2_amax = L.x2 ? a.x2_amax : nullptr; p.x2_t_zero = L.x2 ? a.x2_t_zero : 0;
    if (L.x2) { p.w = (const unsigned char*)a.w_x2; p.x2_scale = reinterpret_cast<const int*>(p.w + z.bw * (phased ? 4 : 1)); }
    p.geglu = a.geglu;
    p.bytes1 = (unsigned)(dma ? z.b1 : 0); p.bytes2 = (unsigned)(dma ? z.b2 : 0); p.bytesw = (unsigned)(dma ? z.bw : 0);
    p.variant = s.variant;
    p.d_hw = make_fastdiv((unsigned)(p.Hm * p.Wm)); p.d_w = make_fastdiv((unsigned)p.Wm);
    p.d_rep1 = make_fastdiv((unsigned)p.rep1); p.d_rep2 = make_fastdiv((unsigned)p.rep2);
    p.tiles_m = cdiv((int)M, L.bm); p.tiles_n = cdiv(a.Cout, pick.small >= 0 ? (pick.small == 1 ? 128 : 64) : BN);
    if ((long long)p.tiles_m * p.tiles_n > 0x7fffffffLL) return NOPE_ERR_UNSUPPORTED;
    // Position-major row order for small images: with 4x4 / 8x8 maps 31 % / 16 % of the 3x3 taps fall into the padding;
    // grouping the rows of a tile by pixel position makes those taps invalid for whole tiles, whose K steps then vanish.
    p.nhyp = a.nhyp; p.d_n = make_fastdiv((unsigned)a.nhyp);
    p.posmajor = pick.posmajor ? 1 : 0;
    if (p.posmajor) {       // positions sorted by descending valid-tap count (stable)
        int cnt[64], n = a.Hs * a.Ws;
        for (int i = 0; i < n; ++i) {
            const int y = i / a.Ws, x = i % a.Ws;
            cnt[i] = ((y > 0) + 1 + (y + 1 < a.Hs)) * ((x > 0) + 1 + (x + 1 < a.Ws));
            p.pos_order[i] = (unsigned char)i;
        }
        for (int i = 1; i < n; ++i)      // insertion sort, n <= 64
            for (int j = i; j > 0 && cnt[p.pos_order[j]] > cnt[p.pos_order[j - 1]]; --j) {
                const unsigned char tmp = p.pos_order[j]; p.pos_order[j] = p.pos_order[j - 1]; p.pos_order[j - 1] = tmp;
            }
    }
    return NOPE_OK;
}

// K splits and the reduce kernel: the tap-resident kernel's (chosen with the kernel), or the 128 x 192 kernel's where the scratch holds them
static void plan_splits(ConvLaunch& L, const ConvArgs& a, const ConvFacts& f, const KernelChoice& pick) {
    ConvParams& p = L.p;
    p.splits = 1;
    const int want_splits = (f.dma && !pick.pp && a.splitk_ws) ? splitk_factor(a, f) : 1;
    if (pick.hsplit > 1) p.splits = pick.hsplit;
    else if ((size_t)want_splits * (size_t)f.z.M * a.Cout * 4 <= a.splitk_bytes) p.splits = want_splits;
    if (p.splits > 1) p.split_out = (float*)a.splitk_ws;
    L.reduce = p.splits <= 1 ? CONV_REDUCE_NONE : a.colstats ? CONV_REDUCE_STATS : CONV_REDUCE_PLAIN;      // (statistics: the tap-resident split only)
    // the wide NHWC epilogue (epilogue_wide) of a 4-byte element type, whole launch in one pass: the 128 x 192 LDS-DMA kernel and the ping-pong kernels
    // (a 128 x 192 launch that WANTED to split but whose scratch was short records nothing either)
    L.records_out_amax = f.z.es == 4 && f.dma && pick.small < 0 && pick.hsplit <= 1 && !a.out_nchw && !a.geglu && a.Cout % 4 == 0 && (pick.pp || want_splits <= 1);
    p.out_amax = L.records_out_amax ? a.out_amax : nullptr;
}

// Workgroup -> tile map (ConvParams::xcd_map, xcd_gn: tile_coords)
static void plan_tile_map(ConvLaunch& L, const ConvSwitches& s, const ConvFacts& f, const KernelChoice& pick) {
    ConvParams& p = L.p;
    const ConvSizes& z = f.z;
    const int tn = p.tiles_n;
    p.xcd_map = pick.small < 0 && (tn == 1 || tn == 2 || tn == 4 || tn == 8) && (p.tiles_m % (8 / tn) == 0) ? 1 : 0;
    // LDS-DMA launches with several weight panels: split the panels over gn XCD columns and the M tiles over 8 / gn XCD rows
    // so that the bytes crossing the fabric, gn x activations + (8 / gn) x weights, are fewest (tile_coords, map 2).
    // NOPE_XCD_MAP=1 keeps one panel per XCD (gn = tiles_n).
    p.xcd_gn = tn;
    const double abytes = (double)z.b1 + (double)z.b2, wbytes = (double)z.bw * (z.phased ? 4 : 1);
    if (pick.small >= 0) {
        // small tiles: an (8 / gn) x gn XCD grid over (runs of M tiles) x (groups of weight panels), gn chosen like below; at small
        // M the weights are most of the bytes, so they usually cross the fabric once (gn = 8) and the activations 8 times
        double best = -1.0;
        for (int gn = 1; gn <= 8; gn *= 2)
            if (p.tiles_m % (8 / gn) == 0 && p.tiles_n % gn == 0 && (best < 0 || gn * abytes + (8 / gn) * wbytes < best)) {
                best = gn * abytes + (8 / gn) * wbytes; p.xcd_gn = gn; p.xcd_map = 3;
            }
    }
    if (f.dma && p.xcd_map && p.xcd_map != 3 && tn > 1 && !s.xcd_one_panel) {
        double best = tn * abytes + (8 / tn) * wbytes;
        for (int gn = 1; gn < tn; gn *= 2)
            if (p.tiles_m % (8 / gn) == 0 && gn * abytes + (8 / gn) * wbytes < best) { best = gn * abytes + (8 / gn) * wbytes; p.xcd_gn = gn; }
        const int gn = s.xcd_gn.val;            // tests: force the split
        if (s.xcd_gn.set && gn >= 1 && gn <= tn && (gn & (gn - 1)) == 0 && p.tiles_m % (8 / gn) == 0) p.xcd_gn = gn;
        if (p.xcd_gn != tn) p.xcd_map = 2;
    }
    // Panel counts outside {1, 2, 4, 8} (no launch of the default U-Net; the LDM variant's linears): map 4 of tile_coords.  NOPE_XCD_ANY=0: off.
    if (!p.xcd_map && pick.small < 0 && tn > 1 && p.tiles_m % 8 == 0 && s.xcd_any) p.xcd_map = 4;
}

// Tile walks (128 x 192, tap-resident, streaming) and the grid; a launch that asked for the streaming kernel keeps it (pick.stream) only if its walk fits
static void plan_walks(ConvLaunch& L, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f, KernelChoice& pick) {
    ConvParams& p = L.p;
    const int dt = L.dt, es = f.z.es, tn = p.tiles_n;
    const long long M = f.z.M, nblocks = (long long)p.tiles_m * p.tiles_n;
    // Persistent walk: 512 workgroups (2 per CU), each `iters` tiles 64 / span tile_m apart (same XCD, same weight panel; span =
    // panels an XCD interleaves under map 2).
    p.persist_iters = 1;
    unsigned gx = (unsigned)nblocks;
    const long long hw = (long long)a.Hs * a.Ws;
    const int span = p.xcd_map == 2 ? tn / p.xcd_gn : 1;     // workgroups of one XCD that share an M tile
    const auto walk128 = [&](int g) {      // g workgroups of the 128-row tiles, each walking tiles g / 8 / span tile_m apart
        p.persist_iters = (int)(nblocks / g);
        p.persist_dm = (g / 8 / span) * BM;
        p.persist_d1 = (unsigned)((long long)p.persist_dm * a.C1 * es);
        p.persist_d2 = (unsigned)((long long)p.persist_dm * a.C2 * es);
        gx = (unsigned)g;
    };
    const int pg = s.persist_grid;
    if (s.persist && f.dma && pick.small < 0 && L.bm == BM && dt != NOPE_F32 && a.mode == NOPE_CONV_PLAIN && !p.posmajor && p.splits == 1 && p.xcd_map && p.xcd_map != 4 &&
        p.wide_out && a.rep1 == 1 && a.rep2 == 1 && M % BM == 0 && nblocks > pg && nblocks % pg == 0 && (pg / 8) % span == 0 &&
        ((long long)(pg / 8 / span) * BM) % hw == 0 && !(s.variant & 2))
        walk128(pg);
    // The tap-resident kernel walks tiles too (bf16): one workgroup per CU, tiles gx / 8 apart inside the XCD's run of M tiles,
    // the next tile's prologue in flight under the epilogue.  NOPE_HALO_PERSIST = workgroups (default 256, 0 = one tile per
    // workgroup; the tests use small grids).
    if (pick.halo && !f.z.phased && dt != NOPE_F32 && p.xcd_map && p.xcd_map != 4 && p.splits == 1) {      // (the split-K instantiation returns after its first tile; the phase-conv form walks no tiles)
        const int want = s.halo_persist;
        if (want >= 8 && want % (8 * span) == 0 && nblocks > want && nblocks % want == 0 && ((long long)(want / 8 / span) * 256) % hw == 0) {
            gx = (unsigned)want;
            p.persist_iters = (int)(nblocks / want);
        }
    }
    // The streaming 1x1 kernel: 256 workgroups (one per CU), each `iters` tiles 32 / span tile_m apart (same XCD, same weight panel).
    // A launch that asked for it keeps the 128 x 192 kernel unless it is unsplit, on map 1 or 2, and the grid divides.
    const int sgrid = s.stream_grid;
    pick.stream = pick.stream && p.splits == 1 && (p.xcd_map == 1 || p.xcd_map == 2) && nblocks % sgrid == 0 && (sgrid / 8) % span == 0;
    if (pick.stream) walk128(sgrid);
    L.grid = dim3(gx, f.z.phased ? 4u : 1u, (unsigned)p.splits);
}

// Epilogue form: the lean row walk, and the GroupNorm tail that lives in it
static int plan_epilogue(ConvLaunch& L, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f, const KernelChoice& pick) {
    ConvParams& p = L.p;
    const int dt = L.dt, bm = L.bm;
    const bool dma = f.dma, phased = f.z.phased;
    const long long M = f.z.M;
    // The lean wide epilogue (epilogue_wide, LEANM = 1): f32 storage on the 32 x 32 tiles, EVERY wave tile of the launch whole along M and in whole 32-column passes along N, rows in NHWC order,
    // one sample per wave tile under a fused PreNorm, 32-bit byte offsets.  NOPE_EPILOGUE_LEAN=0: the generic row loop everywhere (A/B).
    p.lean = (dt == NOPE_BF16X3 && dma && pick.small < 0 && p.wide_out && !p.posmajor && !phased && p.splits == 1 && !a.geglu && M % bm == 0 && a.Cout % 32 == 0 &&
              (!a.pn_ms || ((long long)p.Hm * p.Wm) % 64 == 0) && (unsigned long long)M * a.Cout * 4ull < 0xffffffffull && s.lean) ? 1 : 0;
    if (a.gn_ms) {
        // the tail lives in ONE epilogue: the lean row walk of the per-tap ping-pong kernel (conv_gemm_pp_kernel with PP_GN_TAIL), a wave tile inside one sample (one
        // (mean, rstd) per group and pass), a lane's 4-channel chunk inside one group.  Any other launch is refused, never run without the tail.
        const long long HW = (long long)p.Hm * p.Wm;
        const int cpg = a.Cout / a.gn_G;
        if (!(pick.pp && !pick.halo && !pick.stream && p.lean && a.mode == NOPE_CONV_PLAIN && HW % 64 == 0 && cpg % 4 == 0 && s.variant == 0 && !s.pp_variant.set))
            return NOPE_ERR_UNSUPPORTED;
        if (a.tail_stats && conv_tail_stat_blocks((int)HW, a.Cout) > 64) return NOPE_ERR_UNSUPPORTED;      // (the runtimes' partial buffers hold 64 entries per hypothesis)
        p.gn_ms = a.gn_ms; p.gn_gamma = a.gn_gamma; p.gn_beta = a.gn_beta; p.gn_G = a.gn_G;
        p.d_cpg = make_fastdiv((unsigned)cpg);
        p.tail_stats = a.tail_stats; p.tail_cols = cdiv(a.Cout, 96);
    }
    if (a.gn_self) {
        // the launch's own GroupNorm lives in ONE epilogue too: the lean row walk of the tap-resident kernel, where a 256-row tile holds
        // whole samples (maps of 16, 64 or 256 pixels) and a 192-column tile whole groups of whole 4-channel chunks, in one launch (no split-K); on 16-pixel maps the
        // column sums take the LDS a tile walk's next prologue would write, so one tile per workgroup there.  Any other launch is refused, never run without it.
        const long long HW = (long long)p.Hm * p.Wm;
        const int cpg = a.Cout / a.gn_G;
        if (!(pick.halo && !phased && p.lean && a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && p.splits == 1 && (HW == 16 || HW == 64 || HW == 256) && M % 256 == 0 &&
              cpg % 4 == 0 && BN % cpg == 0 && (HW != 16 || p.persist_iters == 1) && s.variant == 0 && !s.pp_variant.set))
            return NOPE_ERR_UNSUPPORTED;
        p.gn_self = 1; p.gn_gamma = a.gn_gamma; p.gn_beta = a.gn_beta; p.gn_G = a.gn_G; p.gn_cpg = cpg; p.gn_eps = a.gn_eps;
        p.d_cpg = make_fastdiv((unsigned)cpg);
        p.gn_emb = a.gn_emb; p.gn_emb_stride = a.gn_emb_stride;
        p.resid = (const unsigned char*)a.gn_resid;
        p.stat_rows = HW == 16 ? 16 : 64;
    }
    // The tap-resident kernel's padding-skipping form (conv3x3_halo_kernel, PADSKIP) for the 4 x 4 level: a 256-row tile of 16 whole samples staged in
    // (position, sample) order, 12 of the 72 MFMA block-taps of a channel chunk -- those that lie wholly in the zero padding -- not executed, the
    // accumulators exchanged through LDS before the unchanged lean epilogue (so one tile per workgroup: the exchange takes the LDS a walk's next
    // prologue would write).  A flag of the same launch kind; results are the sample-major form's.  NOPE_HALO_PADSKIP=0: that form (A/B).
    p.padskip = (s.halo_padskip && pick.halo && !phased && p.lean && a.mode == NOPE_CONV_PLAIN && a.ntaps == 9 && a.Hs == 4 && a.Ws == 4 && M % 256 == 0 && p.splits == 1 &&
                 p.persist_iters == 1 && a.rep1 == 1 && !(a.C2 > 0 && a.rep2 > 1) && s.variant == 0 && !s.pp_variant.set) ? 1 : 0;
    return NOPE_OK;
}

// What the dispatch, the trace line and the queries call the launch, and the flops it executes
static void plan_kind(ConvLaunch& L, const ConvArgs& a, const ConvSwitches& s, const ConvFacts& f, const KernelChoice& pick) {
    L.kind = pick.small >= 0 ? NOPE_CONV_KERNEL_SMALL : pick.stream ? NOPE_CONV_KERNEL_STREAM : pick.halo ? NOPE_CONV_KERNEL_HALO256 : pick.pp ? NOPE_CONV_KERNEL_PP256
             : f.dma ? NOPE_CONV_KERNEL_DMA128 : NOPE_CONV_KERNEL_GENERIC;
    if ((L.kind == NOPE_CONV_KERNEL_HALO256 || L.kind == NOPE_CONV_KERNEL_PP256) && s.pp_variant.set) L.p.variant = s.pp_variant.val;      // tuning ablations of the ping-pong kernel
    // executed multiply-adds x2 (position-major launches skip the taps that lie in the padding: (3H-2)(3W-2) of the 9 H W tap instances remain)
    const double taps = L.posmajor ? (double)(3 * a.Hs - 2) * (3 * a.Ws - 2) / ((double)a.Hs * a.Ws) : (double)a.ntaps;
    L.flops = 2.0 * (double)a.nhyp * a.Ho * a.Wo * a.Cout * taps * f.z.Cin;
}

static ConvLaunch plan(int dt, const ConvArgs& a0, const ConvSwitches& s) {
    ConvLaunch L;
    ConvArgs a = a0;
    ConvFacts f;            // (filled once the arguments are sound)
    KernelChoice pick;      // (filled by plan_kernel)
    L.err = plan_arguments(dt, a);
    L.dt = dt;
    if (L.err == NOPE_OK) { f = conv_facts(dt, a, s); L.err = plan_requests(a, s, f); }
    if (L.err == NOPE_OK) L.err = plan_kernel(L, a, s, f, pick);
    if (L.err == NOPE_OK) L.err = plan_params(L, a, s, f, pick);
    if (L.err != NOPE_OK) return L;
    plan_splits(L, a, f, pick);
    plan_tile_map(L, s, f, pick);
    plan_walks(L, a, s, f, pick);
    L.err = plan_epilogue(L, a, s, f, pick);
    if (L.err == NOPE_OK) plan_kind(L, a, s, f, pick);
    return L;
}
ConvLaunch conv_plan(int dt, const ConvArgs& a) { return plan(dt, a, conv_switches(dt_base(dt))); }

// ---- the queries: what would launch_conv do with this layer?  Each reads the plan (of a launch conv_plan rejects: false / generic / 0).
// Asked per compute mode, as they always were: NOPE_F16X2 is answered as NOPE_BF16X3 (the runtimes launch under that type, with ConvArgs::w_x2).
static ConvLaunch query(int dt, const ConvArgs& a) { return conv_plan(dt_base(dt), a); }
bool conv_is_posmajor(int dt, const ConvArgs& a) { return query(dt, a).posmajor; }
int conv_kernel_kind(int dt, const ConvArgs& a) { return query(dt, a).kind; }
bool conv_takes_x2(int dt, const ConvArgs& a) { return query(dt, a).x2; }
bool conv_records_out_amax(int dt, const ConvArgs& a) { return query(dt, a).p.out_amax != nullptr; }
double conv_executed_flops(int dt, const ConvArgs& a) { return query(dt, a).flops; }
bool conv_geglu_fusable(int dt, const ConvArgs& a0) {
    const ConvSwitches& s = conv_switches(dt_base(dt));
    const int mode = s.geglu_fused;      // (A/B switch of the CALLER's choice; 2: only launches the 128 x 192 kernel would get anyway)
    if (mode == 0) return false;
    if (mode == 2) { const int k = plan(dt_base(dt), a0, s).kind; if (k == NOPE_CONV_KERNEL_PP256 || k == NOPE_CONV_KERNEL_HALO256 || k == NOPE_CONV_KERNEL_SMALL) return false; }
    ConvArgs a = a0;
    a.geglu = 1;
    return plan(dt_base(dt), a, s).err == NOPE_OK;
}

// one line per launch (NOPE_CONV_TRACE: tuning aid, and what the tests read)
static void trace_conv(const ConvLaunch& L) {
    static const char* const names[] = {"generic", "dma128", "pp256", "halo256", "small", "stream128"};
    const ConvParams& p = L.p;
    const int Cin = p.C1 + p.C2;
    if (L.kind == NOPE_CONV_KERNEL_SMALL) fprintf(stderr, "conv small%d mode %d taps %d Cin %d Cout %d M %lld tiles %dx%d grid %u,%u,%u xcd %d/%d\n", L.small, p.mode, p.ntaps, Cin, p.Cout, (long long)p.M,
                                                 p.tiles_m, p.tiles_n, L.grid.x, L.grid.y, L.grid.z, p.xcd_map, p.xcd_gn);
    else fprintf(stderr, "conv %s mode %d taps %d Cin %d Cout %d M %lld tiles %dx%d grid %u,%u,%u posmajor %d persist %d xcd %d/%d%s%s%s\n",
                 names[L.kind], p.mode, p.ntaps, Cin, p.Cout, (long long)p.M, p.tiles_m, p.tiles_n, L.grid.x, L.grid.y, L.grid.z,
                 p.posmajor, p.persist_iters, p.xcd_map, p.xcd_gn, p.padskip ? " padskip" : "", p.geglu ? " geglu" : L.x2 ? " x2" : "", p.gn_ms ? " lean gn-tail" : p.gn_self ? " lean gn-self" : p.lean ? " lean" : "");
}

// fn((T*)nullptr) with T the type a tensor of `dt` is stored in (the reduce kernels of a split launch write it)
template <class F>
static void by_storage_type(int dt, F fn) { if (dt_es(dt) == 4) fn((float*)nullptr); else if (dt == NOPE_F16) fn((f16_t*)nullptr); else fn((bf16_t*)nullptr); }

#define LAUNCH_GENERIC(T) \
    do { if (p.pn_ms) hipLaunchKernelGGL((conv_gemm_kernel<T, true>), grid, block, 0, s, p); else hipLaunchKernelGGL((conv_gemm_kernel<T, false>), grid, block, 0, s, p); } while (0)
int launch_conv(const ConvLaunch& L, hipStream_t s) {
    if (L.err != NOPE_OK) return L.err;
    if (NOPE_ENV_SET("NOPE_CONV_TRACE")) trace_conv(L);
    const ConvParams& p = L.p;
    const int dt = L.dt;
    const dim3 grid = L.grid, block(NT);
    if (L.kind == NOPE_CONV_KERNEL_SMALL) launch_conv_small(dt, &p, L.small, grid, s);
    else if (L.kind == NOPE_CONV_KERNEL_STREAM) launch_conv_stream(dt, &p, grid, s);
    else if (L.kind == NOPE_CONV_KERNEL_HALO256) launch_conv_halo(L.x2 ? NOPE_F16X2 : dt, &p, grid, s);
    else if (L.kind == NOPE_CONV_KERNEL_PP256) launch_conv_pp(L.x2 ? NOPE_F16X2 : dt, &p, grid, s);
    else if (L.kind == NOPE_CONV_KERNEL_DMA128) {
        if (dt == NOPE_F32) launch_conv_dma_f32(&p, L.bm, grid, s);
        else if (dt == NOPE_BF16X3) launch_conv_dma_bf16x3(&p, grid, s);
        else if (dt == NOPE_F16) launch_conv_dma_f16(&p, grid, s);
        else if (L.bm == 256 || (p.variant & 2)) launch_conv_dma_bf16_variant(&p, L.bm, grid, s);
        else launch_conv_dma_bf16(&p, grid, s);
    } else if (dt == NOPE_F32) LAUNCH_GENERIC(float);      // any channel counts: the register-staged kernel
    else if (dt == NOPE_BF16X3) LAUNCH_GENERIC(f32s_t);
    else if (dt == NOPE_F16) LAUNCH_GENERIC(f16_t);
    else LAUNCH_GENERIC(bf16_t);
    NOPE_CHECK_LAUNCH();
    if (L.reduce == CONV_REDUCE_STATS) {
        const dim3 rg((unsigned)(p.M / p.stat_rows), (unsigned)cdiv(p.Cout, 64));      // (splits <= 16, stat_rows in {16, 32, 64})
        by_storage_type(dt, [&](auto* out) {
            using T = std::remove_pointer_t<decltype(out)>;
            hipLaunchKernelGGL((splitk_reduce_stats_kernel<T>), rg, dim3(256), 0, s, p.split_out, p.splits, p.M, p.Cout, p.bias, p.act, (T*)p.out, p.colstats, p.stat_rows);
        });
        NOPE_CHECK_LAUNCH();
    } else if (L.reduce == CONV_REDUCE_PLAIN) {
        const size_t MN = (size_t)p.M * p.Cout;
        const dim3 rg((unsigned)((MN + 255) / 256 < 4096 ? (MN + 255) / 256 : 4096));
        const int HWo = p.Ho * p.Wo;
        by_storage_type(dt, [&](auto* out) {
            using T = std::remove_pointer_t<decltype(out)>;
            hipLaunchKernelGGL((splitk_reduce_kernel<T>), rg, dim3(256), 0, s, p.split_out, p.splits, p.M, p.Cout, p.bias, (const T*)p.resid, p.act, (T*)p.out, p.out_nchw, HWo);
        });
        NOPE_CHECK_LAUNCH();
    }
    return NOPE_OK;
}
#undef LAUNCH_GENERIC

int launch_conv(int dt, const ConvArgs& a, hipStream_t s) { return launch_conv(conv_plan(dt, a), s); }

}  // namespace nope
