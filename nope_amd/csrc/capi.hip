// extern "C" entry points of libnope_hip.so that are thin argument checks over the kernel
// launchers (the U-Net entry points live in unet_runtime.hip).  See include/nope_hip.h.
#include "conv_plan.h"      // (nope_common.h; ConvLaunch)

#include <atomic>
#include <cstdlib>
#include <mutex>

using namespace nope;

namespace nope {
static std::atomic<unsigned> g_tuning_gen{0};
static std::mutex g_env_mu;
unsigned tuning_generation() { return g_tuning_gen.load(std::memory_order_acquire); }
EnvVal env_lookup(EnvCache& c, const char* name) {
    const unsigned g = tuning_generation();
    if (c.gen.load(std::memory_order_acquire) != g) {  // first use of this site, or a reload since: read the variable (rare path, serialised)
        std::lock_guard<std::mutex> lock(g_env_mu);
        const char* v = getenv(name);
        c.set.store(v != nullptr, std::memory_order_relaxed);
        c.val.store(v ? atoll(v) : 0, std::memory_order_relaxed);
        c.gen.store(g, std::memory_order_release);
    }
    return EnvVal{c.set.load(std::memory_order_relaxed), c.val.load(std::memory_order_relaxed)};
}
}  // namespace nope

extern "C" {

int nope_abi_version(void) { return NOPE_ABI_VERSION; }
void nope_tuning_reload(void) { g_tuning_gen.fetch_add(1, std::memory_order_acq_rel); }

const char* nope_strerror(int code) {
    switch (code) {
        case NOPE_OK: return "ok";
        case NOPE_ERR_RANGE: return "f16x2: activations outside a layer's accurate range (shifts adjusted: run again)";
        case NOPE_ERR_RANGE_F16: return "f16x2: non-finite activations (run as bf16x3)";
        case NOPE_ERR_ARG: return "invalid argument";
        case NOPE_ERR_LAUNCH: return "HIP launch/runtime error";
        case NOPE_ERR_WORKSPACE: return "workspace too small";
        case NOPE_ERR_WEIGHT: return "missing or mis-shaped state-dict tensor";
        case NOPE_ERR_ALLOC: return "device allocation failed";
        case NOPE_ERR_UNSUPPORTED: return "unsupported size or dtype";
        default: return "unknown error";
    }
}

int nope_similarity(const float* q, const void* bank, int bank_dtype, float* scores, int B, int N, int C, int H, int W,
                    int64_t bank_stride_b, int score_ld, nope_stream_t stream) {
    if (H <= 0 || W <= 0) return NOPE_ERR_ARG;
    return launch_similarity(q, bank, bank_dtype, scores, B, N, C, H * W, (long long)bank_stride_b, score_ld, (hipStream_t)stream);
}

int nope_topk(const float* scores, int64_t* idx, float* vals, int B, int N, int k, int score_ld, nope_stream_t stream) {
    return launch_topk(scores, (long long*)idx, vals, B, N, k, score_ld, (hipStream_t)stream);
}

int nope_gather_topk(const float* gathered, int n_ranks, int B, int n_total, float* scores, int64_t* idx, float* vals, int k, nope_stream_t stream) {
    return launch_gather_topk(gathered, n_ranks, B, n_total, scores, (long long*)idx, vals, k, (hipStream_t)stream);
}

int nope_topk_merge(const float* cand_vals, const int64_t* cand_idx, int64_t* idx, float* vals, int B, int M, int k, nope_stream_t stream) {
    if (!cand_idx) return NOPE_ERR_ARG;
    return launch_topk(cand_vals, (long long*)idx, vals, B, M, k, M, (hipStream_t)stream, (const long long*)cand_idx);
}

int nope_op_geodesic(const double* poses, int64_t pose_stride_b, int N, const int64_t* idx, const double* gt, const int* symmetry,
                     double* err_rad, int* status, int B, int k, nope_stream_t stream) {
    return launch_geodesic(poses, (long long)pose_stride_b, N, (const long long*)idx, gt, symmetry, err_rad, status, B, k, (hipStream_t)stream);
}

int nope_op_refine_init(const float* all_relativeR, int64_t N, const int64_t* idx, double* dR, double* dR_init, float* poses, int* status,
                        int B, int k, double fd_step, nope_stream_t stream) {
    return launch_refine_init(all_relativeR, (long long)N, (const long long*)idx, dR, dR_init, poses, status, B, k, fd_step, (hipStream_t)stream);
}

size_t nope_op_refine_normal_eq_workspace_bytes(int B, int k, int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return refine_normal_eq_workspace_bytes(B, k, H * W);
}

int nope_op_refine_normal_eq(const float* q, const float* maps, double* normal_eq, int B, int k, int C, int H, int W, double fd_step,
                             void* workspace, size_t workspace_bytes, nope_stream_t stream) {
    if (H <= 0 || W <= 0) return NOPE_ERR_ARG;
    return launch_refine_normal_eq(q, maps, normal_eq, B, k, C, H * W, fd_step, workspace, workspace_bytes, (hipStream_t)stream);
}

int nope_op_refine_step(const double* normal_eq, double* dR, float* poses, int* status, int B, int k, double fd_step, double max_step_rad,
                        double damping, nope_stream_t stream) {
    return launch_refine_step(normal_eq, dR, poses, status, B, k, fd_step, max_step_rad, damping, (hipStream_t)stream);
}

int nope_op_refine_select(const double* dR, const double* dR_init, const float* score_refined, const float* similarity, int64_t similarity_ld,
                          int64_t N, const int64_t* idx, const double* template_poses, int64_t template_stride_b, int64_t n_templates,
                          double* out_dR, float* out_6d, float* out_score, float* out_score_init, int* out_accepted, int64_t* out_order,
                          double* pred_R, int B, int k, nope_stream_t stream) {
    return launch_refine_select(dR, dR_init, score_refined, similarity, (long long)similarity_ld, (long long)N, (const long long*)idx,
                                template_poses, (long long)template_stride_b, (long long)n_templates, out_dR, out_6d, out_score, out_score_init,
                                out_accepted, (long long*)out_order, pred_R, B, k, (hipStream_t)stream);
}

size_t nope_op_render_depth_workspace_bytes(int P, int max_faces) { return render_depth_workspace_bytes(P, max_faces); }

int nope_op_render_depth(const float* verts, int V, const int* faces, int F, const int* face_off, const int* face_cnt, int max_faces,
                         const double* poses, const double* K, int P, int H, int W, float* depth, uint32_t* skipped, void* workspace,
                         size_t workspace_bytes, nope_stream_t stream) {
    return launch_render_depth(verts, V, faces, F, face_off, face_cnt, max_faces, poses, K, P, H, W, depth, skipped, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

size_t nope_op_vsd_workspace_bytes(int B, int k, int H, int W) { return vsd_workspace_bytes(B, k, H, W); }

int nope_op_vsd(const float* depth_test, const float* depth_gt, const float* depth_est, const double* K, int B, int k, int H, int W,
                double delta, double tau, int cost_type, int visib_mode, double* err, void* workspace, size_t workspace_bytes,
                nope_stream_t stream) {
    return launch_vsd(depth_test, depth_gt, depth_est, K, B, k, H, W, delta, tau, cost_type, visib_mode, err, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

int nope_op_vis_grid(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, void* grid_f16, nope_stream_t stream) {
    return launch_vis_grid(cols, n_cols, B, F, H, W, static_cast<f16_t*>(grid_f16), (hipStream_t)stream);
}

int nope_op_vis_sheet(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, int tile, int nrow, int padding,
                      void* sheet_u8, nope_stream_t stream) {
    return launch_vis_sheet(cols, n_cols, B, F, H, W, tile, nrow, padding, static_cast<unsigned char*>(sheet_u8), (hipStream_t)stream);
}

int nope_op_nchw_to_nhwc(int dtype, const float* x, void* y, int n, int C, int HW, nope_stream_t s) {
    return launch_nchw_to_nhwc(dtype, x, y, n, C, HW, (hipStream_t)s);
}
int nope_op_nhwc_to_nchw(int dtype, const void* x, float* y, int n, int C, int HW, nope_stream_t s) {
    return launch_nhwc_to_nchw_f32(dtype, x, y, n, C, HW, (hipStream_t)s);
}
int nope_op_pack_conv_weight(int dtype, const float* w, void* packed, int Cout, int Cin, int ntaps, int mode, nope_stream_t s) {
    return launch_pack_conv_w(dtype, w, packed, Cout, Cin, ntaps, mode, (hipStream_t)s);
}

static void fill_conv_args(ConvArgs& a, const void* src1, int C1, int rep1, const void* src2, int C2, int rep2, int Hs, int Ws, int mode, int ntaps,
                           const void* w_packed, const float* bias, const void* resid, void* out, int Cout, int n_hyp, int out_nchw,
                           int out_dtype, int act_relu) {
    a.src1 = src1; a.C1 = C1; a.rep1 = rep1; a.src2 = src2; a.C2 = C2; a.rep2 = rep2 > 0 ? rep2 : 1;
    a.Hs = Hs; a.Ws = Ws; a.mode = mode; a.ntaps = ntaps;
    const bool up = mode == NOPE_CONV_UP2 || mode == NOPE_CONV_UP2P;
    const bool half = mode == NOPE_CONV_DOWN2 || mode == NOPE_CONV_STRIDE2 || mode == NOPE_CONV_STRIDE2_PAD01;
    a.Ho = up ? 2 * Hs : (half ? Hs / 2 : Hs);
    a.Wo = up ? 2 * Ws : (half ? Ws / 2 : Ws);
    a.act = act_relu ? 1 : 0;
    a.w = w_packed; a.bias = bias; a.resid = resid; a.out = out; a.Cout = Cout; a.nhyp = n_hyp;
    a.out_nchw = out_nchw; a.out_dt = out_dtype;
}

int nope_op_conv_ws(int dtype, const void* src1, int C1, int rep1, const void* src2, int C2, int rep2, int Hs, int Ws, int mode,
                    int ntaps, const void* w_packed, const float* bias, const void* resid, void* out, int Cout, int n_hyp,
                    int out_nchw, int out_dtype, int act_relu, void* splitk_ws, size_t splitk_bytes, nope_stream_t s) {
    ConvArgs a;
    fill_conv_args(a, src1, C1, rep1, src2, C2, rep2, Hs, Ws, mode, ntaps, w_packed, bias, resid, out, Cout, n_hyp, out_nchw, out_dtype, act_relu);
    if ((mode == NOPE_CONV_DOWN2 || mode == NOPE_CONV_STRIDE2 || mode == NOPE_CONV_STRIDE2_PAD01) && ((Hs | Ws) & 1)) return NOPE_ERR_ARG;
    a.splitk_ws = splitk_ws; a.splitk_bytes = splitk_ws ? splitk_bytes : 0;
    return launch_conv(dtype, a, (hipStream_t)s);
}

int nope_op_conv(int dtype, const void* src1, int C1, int rep1, const void* src2, int C2, int rep2, int Hs, int Ws, int mode,
                 int ntaps, const void* w_packed, const float* bias, const void* resid, void* out, int Cout, int n_hyp,
                 int out_nchw, int out_dtype, int act_relu, nope_stream_t s) {
    return nope_op_conv_ws(dtype, src1, C1, rep1, src2, C2, rep2, Hs, Ws, mode, ntaps, w_packed, bias, resid, out, Cout, n_hyp, out_nchw,
                           out_dtype, act_relu, nullptr, 0, s);
}

size_t nope_op_conv_splitk_bytes(int dtype, int C1, int C2, int rep1, int Hs, int Ws, int mode, int ntaps, int Cout, int n_hyp) {
    ConvArgs a;
    static const int dummy = 0;
    fill_conv_args(a, &dummy, C1, rep1, C2 ? &dummy : nullptr, C2, 1, Hs, Ws, mode, ntaps, &dummy, nullptr, nullptr, (void*)&dummy, Cout, n_hyp, 0, NOPE_F32, 0);
    if (!dt_is_compute(dtype)) return 0;
    const int S = conv_splitk_factor(dtype, a);
    return S > 1 ? (size_t)S * (size_t)n_hyp * a.Ho * a.Wo * Cout * 4 : 0;
}

int nope_op_stem_conv(int dtype, const float* image, const float* w, const float* scale, const float* shift, float* w_scratch,
                      void* out, int n_img, int H, int W, nope_stream_t s) {
    int e = launch_stem_pack(w, scale, w_scratch, (hipStream_t)s);      // w_scratch: 147 * 64 floats
    if (e) return e;
    return launch_stem_conv(dtype, image, w_scratch, shift, out, n_img, H, W, (hipStream_t)s);
}

int nope_op_gn_chunks(int dtype, int HW, int C) { return gn_stats_chunks(HW, C, dtype); }

int nope_op_group_norm(int dtype, const void* x, void* y, float* partial, const float* gamma, const float* beta, int n_hyp, int HW,
                       int C, int G, int act_silu, const float* emb, int emb_stride, const void* resid, nope_stream_t s) {
    const int nch = gn_stats_chunks(HW, C, dtype);
    int e = launch_gn_stats(dtype, x, partial, n_hyp, HW, C, G, nch, (hipStream_t)s);
    if (e) return e;
    GnApplyArgs a;
    a.x = x; a.y = y; a.partial = partial; a.nchunk = nch; a.gamma = gamma; a.beta = beta;
    a.nhyp = n_hyp; a.HW = HW; a.C = C; a.G = G; a.act = act_silu; a.emb = emb; a.emb_stride = emb_stride; a.resid = resid;
    return launch_gn_apply(dtype, a, (hipStream_t)s);
}

// ---- (ABI 11) the fused GroupNorm statistics plumbing, one launcher each: nothing below computes, refuses or repairs anything itself ----
int nope_op_amax_slot_words(void) { return kX2SlotWords; }

// the range slot of a launch -> one float: fold the slot's lines (launch_amax_reduce zeroes them again); the word IS the bit pattern of max |.|
static int amax_decode(uint32_t* slot, float* amax_out, hipStream_t s) { return launch_amax_reduce(slot, 1, reinterpret_cast<unsigned*>(amax_out), s); }

int nope_op_absmax_f32(const float* x, size_t n, uint32_t* amax_slot, float* amax_out, nope_stream_t s) {
    if (!amax_slot || !amax_out) return NOPE_ERR_ARG;
    if (hipMemsetAsync(amax_slot, 0, (size_t)kX2SlotWords * 4, (hipStream_t)s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch_absmax_f32(x, n, amax_slot, (hipStream_t)s)) return e;
    return amax_decode(amax_slot, amax_out, (hipStream_t)s);
}

int nope_op_conv_stat_rows(int dtype, int C1, int C2, int rep1, int Hs, int Ws, int mode, int ntaps, int Cout, int n_hyp, int has_resid,
                           int out_nchw, int act_relu) {
    ConvArgs a;
    static const int dummy = 0;
    fill_conv_args(a, &dummy, C1, rep1, C2 ? &dummy : nullptr, C2, 1, Hs, Ws, mode, ntaps, &dummy, nullptr, has_resid ? &dummy : nullptr, (void*)&dummy,
                   Cout, n_hyp, out_nchw, NOPE_F32, act_relu);
    if (!dt_is_compute(dtype) || act_relu) return 0;      // (launch_conv refuses statistics behind an activation)
    return conv_stat_rows(dtype, a);
}

int nope_op_conv_ex(int dtype, const void* src1, int C1, int rep1, const void* src2, int C2, int rep2, int Hs, int Ws, int mode,
                    int ntaps, const void* w_packed, const float* bias, const void* resid, void* out, int Cout, int n_hyp,
                    int out_nchw, int out_dtype, int act_relu, void* splitk_ws, size_t splitk_bytes, float* colstats, int stat_rows,
                    const float* pn_ms, const float* pn_c0, const float* pn_c1, uint32_t* amax_slot, float* amax_out, int* amax_recorded,
                    nope_stream_t s) {
    ConvArgs a;
    fill_conv_args(a, src1, C1, rep1, src2, C2, rep2, Hs, Ws, mode, ntaps, w_packed, bias, resid, out, Cout, n_hyp, out_nchw, out_dtype, act_relu);
    if ((mode == NOPE_CONV_DOWN2 || mode == NOPE_CONV_STRIDE2 || mode == NOPE_CONV_STRIDE2_PAD01) && ((Hs | Ws) & 1)) return NOPE_ERR_ARG;
    if ((amax_slot != nullptr) != (amax_out != nullptr)) return NOPE_ERR_ARG;
    a.splitk_ws = splitk_ws; a.splitk_bytes = splitk_ws ? splitk_bytes : 0;
    a.colstats = colstats;
    if (colstats) a.stat_rows = stat_rows;
    a.pn_ms = pn_ms; a.pn_c0 = pn_c0; a.pn_c1 = pn_c1;
    a.out_amax = amax_slot;
    const ConvLaunch L = conv_plan(dtype, a);
    if (amax_recorded) *amax_recorded = L.p.out_amax ? 1 : 0;      // (of the launch that runs: a slot was given and its epilogue fills it)
    if (amax_slot && hipMemsetAsync(amax_slot, 0, (size_t)kX2SlotWords * 4, (hipStream_t)s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch_conv(L, (hipStream_t)s)) return e;
    return amax_slot ? amax_decode(amax_slot, amax_out, (hipStream_t)s) : NOPE_OK;
}

int nope_op_gn_apply_blocks(int dtype, int HW, int C, int n_hyp) { return gn_apply_blocks(HW, C, dtype, n_hyp); }

int nope_op_gn_finalize(const float* partial, float* ms, int n_hyp, int nchunk, float count, float eps, nope_stream_t s) {
    return launch_gn_finalize(partial, ms, n_hyp, nchunk, count, eps, (hipStream_t)s);
}

int nope_op_group_norm_ex(int dtype, const void* x, void* y, float* partial, const float* colstats, int stat_blocks, int fold_launch,
                          const float* gamma, const float* beta, int n_hyp, int HW, int C, int G, int act_silu, const float* emb,
                          int emb_stride, const float* film, int film_stride, const void* resid, int x_rep, int resid_rep, float* out_stats,
                          float eps, int fast_silu, uint32_t* amax_slot, float* amax_out, nope_stream_t s) {
    if (x_rep < 1 || n_hyp <= 0 || n_hyp % x_rep || (amax_slot != nullptr) != (amax_out != nullptr)) return NOPE_ERR_ARG;
    GnApplyArgs a;
    a.partial = partial;
    if (colstats && fold_launch) {           // the separate fold launch + the partial path (what the runtimes do under NOPE_GN_FOLD_INLINE)
        if (const int e = launch_gn_fold(colstats, partial, n_hyp / x_rep, stat_blocks, C, G, (hipStream_t)s)) return e;
    } else if (colstats) {                   // every gn_apply workgroup folds its sample's column statistics itself
        a.colstats = colstats; a.stat_blocks = stat_blocks;
    } else {
        a.nchunk = gn_stats_chunks(HW, C, dtype);
        if (const int e = launch_gn_stats(dtype, x, partial, n_hyp / x_rep, HW, C, G, a.nchunk, (hipStream_t)s)) return e;
    }
    a.x = x; a.y = y; a.gamma = gamma; a.beta = beta;
    a.nhyp = n_hyp; a.HW = HW; a.C = C; a.G = G; a.act = act_silu; a.emb = emb; a.emb_stride = emb_stride;
    a.film = film; a.film_stride = film_stride; a.resid = resid; a.x_rep = x_rep; a.resid_rep = resid_rep;
    a.out_stats = out_stats; a.eps = eps; a.fast_silu = fast_silu; a.amax_out = amax_slot;
    if (amax_slot && hipMemsetAsync(amax_slot, 0, (size_t)kX2SlotWords * 4, (hipStream_t)s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch_gn_apply(dtype, a, (hipStream_t)s)) return e;
    return amax_slot ? amax_decode(amax_slot, amax_out, (hipStream_t)s) : NOPE_OK;
}

int nope_op_group_norm_shared(int dtype, const void* x, void* y, float* partial, const float* sh_s, int sh_rep, const float* sh_e, int H, int W,
                              const float* gamma, const float* beta, int n_hyp, int C, int G, int act_silu, const float* emb, int emb_stride,
                              const void* resid, int resid_rep, float* out_stats, float eps, int fast_silu, uint32_t* amax_slot, float* amax_out,
                              nope_stream_t s) {
    if (n_hyp <= 0 || H <= 0 || W <= 0 || (amax_slot != nullptr) != (amax_out != nullptr) || !partial) return NOPE_ERR_ARG;
    if (!sh_s && !sh_e) return NOPE_ERR_ARG;          // (nope_op_group_norm_ex is the entry without a shared addend)
    GnApplyArgs a;
    a.x = x; a.y = y; a.partial = partial; a.gamma = gamma; a.beta = beta;
    a.nhyp = n_hyp; a.HW = H * W; a.C = C; a.G = G; a.act = act_silu; a.emb = emb; a.emb_stride = emb_stride;
    a.resid = resid; a.resid_rep = resid_rep; a.out_stats = out_stats; a.eps = eps; a.fast_silu = fast_silu; a.amax_out = amax_slot;
    a.sh_s = sh_s; a.sh_rep = sh_rep; a.sh_e = sh_e; a.sh_H = H; a.sh_W = W;
    a.nchunk = gn_stats_chunks(a.HW, C, dtype);
    if (const int e = launch_gn_stats_shared(dtype, a, partial, a.nchunk, (hipStream_t)s)) return e;
    if (amax_slot && hipMemsetAsync(amax_slot, 0, (size_t)kX2SlotWords * 4, (hipStream_t)s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch_gn_apply(dtype, a, (hipStream_t)s)) return e;
    return amax_slot ? amax_decode(amax_slot, amax_out, (hipStream_t)s) : NOPE_OK;
}

// ---- (ABI 16) the GroupNorm tail of the per-tap ping-pong kernel's lean epilogue, as Fwd::res_tail (unet_runtime.hip) launches it
int nope_op_conv_tail_stat_blocks(int HW, int Cout) { return conv_tail_stat_blocks(HW, Cout); }

int nope_op_conv_gn_tail(int dtype, const void* src1, int C1, const void* src2, int C2, int Hs, int Ws, const void* w_packed, const float* bias,
                         const void* resid, void* out, int Cout, int n_hyp, const float* colstats, int stat_blocks, const float* gamma,
                         const float* beta, int G, float eps, float* ms, float* tail_stats, uint32_t* amax_slot, float* amax_out, nope_stream_t s) {
    if ((amax_slot != nullptr) != (amax_out != nullptr)) return NOPE_ERR_ARG;
    ConvArgs a;
    fill_conv_args(a, src1, C1, 1, src2, C2, 1, Hs, Ws, NOPE_CONV_PLAIN, 1, w_packed, bias, resid, out, Cout, n_hyp, 0, NOPE_F32, 0);
    a.gn_ms = ms; a.gn_gamma = gamma; a.gn_beta = beta; a.gn_G = G; a.tail_stats = tail_stats;
    a.out_amax = amax_slot;
    const ConvLaunch L = conv_plan(dtype, a);
    if (L.err != NOPE_OK) return L.err;      // (before the statistics launch: a refused combination launches nothing)
    if (const int e = launch_gn_colstats_finalize(colstats, ms, n_hyp, stat_blocks, Cout, G, Hs * Ws, eps, (hipStream_t)s)) return e;
    if (amax_slot && hipMemsetAsync(amax_slot, 0, (size_t)kX2SlotWords * 4, (hipStream_t)s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch_conv(L, (hipStream_t)s)) return e;
    return amax_slot ? amax_decode(amax_slot, amax_out, (hipStream_t)s) : NOPE_OK;
}

int nope_op_conv_class_weights(const float* w, float* out, int Cout, int Cin, nope_stream_t s) {
    return launch_pack_conv_classes(w, out, Cout, Cin, (hipStream_t)s);
}

int nope_op_linear_attention(int dtype, const void* qkv, void* out, int n_hyp, int HW, int heads, int dim_head, nope_stream_t s) {
    return launch_linattn(dtype, qkv, out, n_hyp, HW, heads, dim_head, (hipStream_t)s);
}
int nope_op_attention(int dtype, const void* qkv, void* out, int n_hyp, int HW, int heads, int dim_head, nope_stream_t s) {
    return launch_attn(dtype, qkv, out, n_hyp, HW, heads, dim_head, (hipStream_t)s);
}
int nope_op_layer_norm(int dtype, const void* x, void* y, const float* gamma, const float* beta, int64_t M, int C, float eps, nope_stream_t s) {
    return launch_layernorm(dtype, x, y, gamma, beta, (long long)M, C, eps, (hipStream_t)s);
}
int nope_op_geglu(int dtype, const void* in, void* out, int64_t M, int D, nope_stream_t s) {
    return launch_geglu(dtype, in, out, (long long)M, D, (hipStream_t)s);
}
int nope_op_token_attention(int dtype, const void* qkv, void* out, int n, int N, int C, int dim_head, nope_stream_t s) {
    return launch_token_attention(dtype, qkv, out, n, N, C, dim_head, (hipStream_t)s);
}
int nope_op_wide_attention(int dtype, const void* qkv, void* out, int n, int N, int C, nope_stream_t s) {
    return launch_wide_attention(dtype, qkv, out, n, N, C, (hipStream_t)s);
}
int nope_op_warp_perspective(const void* src, int src_is_u8, int Hs, int Ws, int C, const float* minv9_host, float* dst_chw, int Hd, int Wd,
                             float scale, float shift, nope_stream_t s) {
    return launch_warp_perspective(src, src_is_u8, Hs, Ws, C, minv9_host, dst_chw, Hd, Wd, scale, shift, (hipStream_t)s);
}
int nope_op_crop_frames(const void* frames, int F, int Hs, int Ws, int Cs, const float* minv, float* dst, int Hd, int Wd, float scale, float shift,
                        int round_u8, nope_stream_t s) {
    return launch_crop_frames(frames, F, Hs, Ws, Cs, minv, dst, Hd, Wd, scale, shift, round_u8, (hipStream_t)s);
}
int nope_op_linear(const float* in, const float* w, const float* bias, float* out, int M, int N, int K, int act_in, nope_stream_t s) {
    return launch_linear_naive(in, w, bias, out, M, N, K, act_in, N, (hipStream_t)s);
}

}  // extern "C"
