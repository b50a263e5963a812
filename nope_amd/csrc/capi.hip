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

// ---- the operator entries that take their arguments by name (nope_conv_op, nope_gn_op): nothing below computes, refuses or repairs anything
// ---- a launcher would not; each piece exists once
template <class Op>
static bool sized(const Op* op) { return op && op->struct_size == sizeof(Op); }      // a binding built against another layout is refused, not read past its end

// the range slot of a launch -> one float: fold the slot's lines (launch_amax_reduce zeroes them again); the word IS the bit pattern of max |.|
static int amax_decode(uint32_t* slot, float* amax_out, hipStream_t s) { return launch_amax_reduce(slot, 1, reinterpret_cast<unsigned*>(amax_out), s); }

// the range-slot tail of an entry: clear the slot, launch, decode (no slot: just launch)
template <class Launch>
static int with_amax(uint32_t* slot, float* amax_out, hipStream_t s, Launch launch) {
    if (slot && hipMemsetAsync(slot, 0, (size_t)kX2SlotWords * 4, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (const int e = launch()) return e;
    return slot ? amax_decode(slot, amax_out, s) : NOPE_OK;
}

// nope_conv_op -> ConvArgs (always filled: the query answers for a launch the entry would refuse), and what the entry refuses before it plans
static int conv_args(const nope_conv_op& op, ConvArgs& a) {
    a.src1 = op.src1; a.C1 = op.C1; a.rep1 = op.rep1 > 0 ? op.rep1 : 1; a.src2 = op.src2; a.C2 = op.C2; a.rep2 = op.rep2 > 0 ? op.rep2 : 1;
    a.Hs = op.Hs; a.Ws = op.Ws; a.mode = op.mode; a.ntaps = op.ntaps;
    const bool up = op.mode == NOPE_CONV_UP2 || op.mode == NOPE_CONV_UP2P;
    const bool half = op.mode == NOPE_CONV_DOWN2 || op.mode == NOPE_CONV_STRIDE2 || op.mode == NOPE_CONV_STRIDE2_PAD01;
    a.Ho = up ? 2 * op.Hs : (half ? op.Hs / 2 : op.Hs);
    a.Wo = up ? 2 * op.Ws : (half ? op.Ws / 2 : op.Ws);
    a.act = op.act_relu ? 1 : 0;
    a.w = op.w_packed; a.bias = op.bias; a.resid = op.resid; a.out = op.out; a.Cout = op.Cout; a.nhyp = op.n_hyp;
    a.out_nchw = op.out_nchw; a.out_dt = op.out_dtype;
    a.splitk_ws = op.splitk_ws; a.splitk_bytes = op.splitk_ws ? op.splitk_bytes : 0;
    a.colstats = op.colstats;
    if (op.colstats) a.stat_rows = op.stat_rows;
    a.pn_ms = op.pn_ms; a.pn_c0 = op.pn_c0; a.pn_c1 = op.pn_c1;
    a.gn_ms = op.gn_ms; a.gn_gamma = op.gn_gamma; a.gn_beta = op.gn_beta; a.gn_G = op.gn_G; a.tail_stats = op.tail_stats;
    a.out_amax = op.amax_slot;
    if (op.gn_self) {      // the conv's own GroupNorm: resid is added behind it
        a.gn_self = 1; a.gn_eps = op.gn_eps; a.gn_emb = op.gn_emb; a.gn_emb_stride = op.gn_emb_stride; a.gn_resid = op.resid; a.resid = nullptr;
    }
    if (half && ((op.Hs | op.Ws) & 1)) return NOPE_ERR_ARG;
    if ((op.amax_slot != nullptr) != (op.amax_out != nullptr)) return NOPE_ERR_ARG;
    if (op.gn_gamma && !op.gn_self && (!op.gn_ms || !op.tail_colstats)) return NOPE_ERR_ARG;      // (conv_plan takes a launch without gn_ms for one without the tail)
    if (op.gn_self && op.gn_resid_rep > 1) return NOPE_ERR_UNSUPPORTED;      // (the launch reads one residual sample per output sample)
    return NOPE_OK;
}

// nope_gn_op -> GnApplyArgs but for the statistics source (nope_op_group_norm), and the entry's own argument checks
static int gn_args(const nope_gn_op& op, GnApplyArgs& a) {
    a.x = op.x; a.y = op.y; a.partial = op.partial; a.gamma = op.gamma; a.beta = op.beta;
    a.nhyp = op.n_hyp; a.HW = op.H * op.W; a.C = op.C; a.G = op.G; a.act = op.act_silu; a.emb = op.emb; a.emb_stride = op.emb_stride;
    a.film = op.film; a.film_stride = op.film_stride; a.resid = op.resid;
    a.x_rep = op.x_rep ? op.x_rep : 1; a.resid_rep = op.resid_rep ? op.resid_rep : 1;
    a.out_stats = op.out_stats; a.eps = op.eps; a.fast_silu = op.fast_silu; a.amax_out = op.amax_slot;
    a.sh_s = op.sh_s; a.sh_rep = op.sh_rep ? op.sh_rep : 1; a.sh_e = op.sh_e; a.sh_H = op.H; a.sh_W = op.W;
    if (op.n_hyp <= 0 || op.H <= 0 || op.W <= 0 || a.x_rep < 1 || op.n_hyp % a.x_rep) return NOPE_ERR_ARG;
    if ((op.amax_slot != nullptr) != (op.amax_out != nullptr)) return NOPE_ERR_ARG;
    return NOPE_OK;
}

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

int nope_op_pose_modes(const float* similarity, int64_t similarity_ld, const double* template_poses, int64_t pose_stride_b, int N,
                       const int* symmetry, double temperature, double radius_rad, int max_modes, int fill, float* prob, int64_t prob_ld,
                       float* entropy, int64_t* mode_idx, float* mode_score, float* mode_mass, int* mode_count, int* n_modes, int* status,
                       int B, nope_stream_t stream) {
    return launch_pose_modes(similarity, (long long)similarity_ld, template_poses, (long long)pose_stride_b, N, symmetry, temperature, radius_rad,
                             max_modes, fill, prob, (long long)prob_ld, entropy, (long long*)mode_idx, mode_score, mode_mass, mode_count, n_modes,
                             status, B, (hipStream_t)stream);
}

int nope_op_c2f_expand(const double* template_poses, int64_t pose_stride_b, int N, const int* stage_of, int max_stage, uint8_t* state,
                       const int64_t* seeds, int n_seeds, double radius_rad, int dist_kind, const float* all_relativeR, int capacity, int* cand,
                       int* n_cand, int* n_dropped, float* rows, int* status, int B, nope_stream_t stream) {
    return launch_c2f_expand(template_poses, (long long)pose_stride_b, N, stage_of, max_stage, state, (const long long*)seeds, n_seeds, radius_rad,
                             dist_kind, all_relativeR, capacity, cand, n_cand, n_dropped, rows, status, B, (hipStream_t)stream);
}

int nope_op_c2f_commit(const float* scores, const int* cand, int capacity, int N, float* similarity, int64_t similarity_ld, int B,
                       nope_stream_t stream) {
    return launch_c2f_commit(scores, cand, capacity, N, similarity, (long long)similarity_ld, B, (hipStream_t)stream);
}

int nope_op_multiref_prepare(const double* template_poses, int64_t pose_stride_b, int N, const double* ref_poses, int R, const int* n_refs,
                             int weighting, double tau_rad, int dist_kind, float* all_relativeR, float* weights, double* dist, int* status, int B,
                             nope_stream_t stream) {
    return launch_multiref_prepare(template_poses, (long long)pose_stride_b, N, ref_poses, R, n_refs, weighting, tau_rad, dist_kind, all_relativeR,
                                   weights, dist, status, B, (hipStream_t)stream);
}

int nope_multiref_similarity(const float* q, const void* bank, int bank_dtype, const float* weights, float* scores, int B, int R, int N, int C,
                             int H, int W, int score_ld, nope_stream_t stream) {
    if (H <= 0 || W <= 0) return NOPE_ERR_ARG;
    return launch_multiref_similarity(q, bank, bank_dtype, weights, scores, B, R, N, C, H * W, score_ld, (hipStream_t)stream);
}

int nope_op_multiref_fuse_scores(const float* per_ref, const float* weights, float* scores, int B, int R, int N, int64_t score_ld,
                                 nope_stream_t stream) {
    return launch_multiref_fuse_scores(per_ref, weights, scores, B, R, N, (long long)score_ld, (hipStream_t)stream);
}

int nope_op_multiref_select(const double* template_poses, int64_t pose_stride_b, int N, const double* ref_poses, int R, const int* n_refs,
                            const int* cand, int S, int M, int weighting, double tau_rad, int dist_kind, int* src, float* all_relativeR, float* weights,
                            double* dist, int* status, int B, nope_stream_t stream) {
    return launch_multiref_select(template_poses, (long long)pose_stride_b, N, ref_poses, R, n_refs, cand, S, M, weighting, tau_rad, dist_kind, src,
                                  all_relativeR, weights, dist, status, B, (hipStream_t)stream);
}

int nope_op_multiref_gather(const float* reference_feats, const int* src, float* out, int B, int R, int J, int64_t L, nope_stream_t stream) {
    return launch_multiref_gather(reference_feats, src, out, B, R, J, (long long)L, (hipStream_t)stream);
}

int nope_robust_similarity(const float* q, const void* bank, int bank_dtype, const uint8_t* mask, float trim, float* scores, int B, int N, int C,
                           int H, int W, int64_t bank_stride_b, int score_ld, nope_stream_t stream) {
    if (H <= 0 || W <= 0) return NOPE_ERR_ARG;
    return launch_robust_similarity(q, bank, bank_dtype, mask, trim, scores, B, N, C, H * W, (long long)bank_stride_b, score_ld, (hipStream_t)stream);
}

int nope_op_residual_maps(const float* q, const void* bank, int bank_dtype, const int64_t* idx, float* out, int B, int N, int k, int C, int H,
                          int W, int64_t bank_stride_b, nope_stream_t stream) {
    if (H <= 0 || W <= 0) return NOPE_ERR_ARG;
    return launch_residual_maps(q, bank, bank_dtype, (const long long*)idx, out, B, N, k, C, H * W, (long long)bank_stride_b, (hipStream_t)stream);
}

int nope_op_pool_mask(const void* cover, int is_u8, int B, int S_h, int S_w, int H, int W, int64_t min_sum_u8, float min_mean_f32, uint8_t* mask,
                      nope_stream_t stream) {
    return launch_pool_mask(cover, is_u8, B, S_h, S_w, H, W, (long long)min_sum_u8, min_mean_f32, mask, (hipStream_t)stream);
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

size_t nope_op_pose_errors_workspace_bytes(int P, int max_verts, int max_syms) { return pose_errors_workspace_bytes(P, max_verts, max_syms); }

int nope_op_pose_errors(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* syms, int S_total,
                        const int* sym_off, const int* sym_cnt, int max_syms, const double* pose_est, const double* pose_gt, const double* K,
                        int P, double* mssd, double* mspd, double* add, double* adi, int* status, void* workspace, size_t workspace_bytes,
                        nope_stream_t stream) {
    return launch_pose_errors(verts, V, vert_off, vert_cnt, max_verts, syms, S_total, sym_off, sym_cnt, max_syms, pose_est, pose_gt, K, P, mssd,
                              mspd, add, adi, status, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t nope_op_mesh_diameter_workspace_bytes(int n_obj, int max_verts) { return mesh_diameter_workspace_bytes(n_obj, max_verts); }

int nope_op_mesh_diameter(const float* verts, int V, const int* vert_off, const int* vert_cnt, int n_obj, int max_verts, double* diameter,
                          void* workspace, size_t workspace_bytes, nope_stream_t stream) {
    return launch_mesh_diameter(verts, V, vert_off, vert_cnt, n_obj, max_verts, diameter, workspace, workspace_bytes, (hipStream_t)stream);
}

int nope_op_fit_translation(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* R, const double* K,
                            const double* box, int P, int max_iters, double tol_scale, double tol_px, double* t, double* residual, int* iters,
                            int* status, nope_stream_t stream) {
    return launch_fit_translation(verts, V, vert_off, vert_cnt, max_verts, R, K, box, P, max_iters, tol_scale, tol_px, t, residual, iters, status,
                                  (hipStream_t)stream);
}

int nope_op_mask_boxes(const unsigned char* mask, int B, int H, int W, double* box, int* count, nope_stream_t stream) {
    return launch_mask_boxes(mask, B, H, W, box, count, (hipStream_t)stream);
}

size_t nope_op_depth_shift_workspace_bytes(int B, int k, int H, int W) { return depth_shift_workspace_bytes(B, k, H, W); }

int nope_op_depth_shift(const float* depth_test, const float* depth_est, const unsigned char* mask, int B, int k, int H, int W, double tau,
                        double* shift, int* count, void* workspace, size_t workspace_bytes, nope_stream_t stream) {
    return launch_depth_shift(depth_test, depth_est, mask, B, k, H, W, tau, shift, count, workspace, workspace_bytes, (hipStream_t)stream);
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

int nope_op_conv(const nope_conv_op* op, int* amax_recorded, nope_stream_t stream) {
    if (!sized(op)) return NOPE_ERR_ARG;
    ConvArgs a;
    if (const int e = conv_args(*op, a)) return e;
    hipStream_t s = (hipStream_t)stream;
    const ConvLaunch L = conv_plan(op->dtype, a);
    if (amax_recorded) *amax_recorded = L.p.out_amax ? 1 : 0;      // (of the launch that runs: a slot was given and its epilogue fills it)
    if (op->gn_gamma && !op->gn_self) {      // the GroupNorm tail of the per-tap ping-pong kernel's lean epilogue, as Fwd::res_tail (unet_runtime.hip) launches it
        if (L.err != NOPE_OK) return L.err;      // (before the statistics launch: a refused combination launches nothing)
        if (const int e = launch_gn_colstats_finalize(op->tail_colstats, op->gn_ms, a.nhyp, op->tail_stat_blocks, a.Cout, a.gn_G, a.Hs * a.Ws,
                                                      op->gn_eps, s)) return e;
    }
    return with_amax(op->amax_slot, op->amax_out, s, [&] { return launch_conv(L, s); });
}

int nope_op_conv_query(const nope_conv_op* op, nope_conv_op_info* info) {
    if (!sized(op) || !info) return NOPE_ERR_ARG;
    ConvArgs a;
    const int e = conv_args(*op, a);
    // (the pre-queries validate nothing: keep them from dividing by an empty tile count)
    const bool ask = dt_is_compute(op->dtype) && a.C1 > 0 && a.C2 >= 0 && a.Cout > 0 && a.nhyp > 0 && a.Hs > 0 && a.Ws > 0 && a.Ho > 0 && a.Wo > 0;
    const int S = ask ? conv_splitk_factor(op->dtype, a) : 1;
    info->splitk_bytes = S > 1 ? (size_t)S * (size_t)a.nhyp * a.Ho * a.Wo * a.Cout * 4 : 0;
    info->stat_rows = ask && !a.act ? conv_stat_rows(op->dtype, a) : 0;      // (launch_conv refuses statistics behind an activation)
    info->tail_stat_blocks = ask ? conv_tail_stat_blocks(a.Ho * a.Wo, a.Cout) : 0;
    const ConvLaunch L = conv_plan(op->dtype, a);
    info->records_out_amax = L.err == NOPE_OK && L.records_out_amax ? 1 : 0;
    info->err = e ? e : L.err;
    return NOPE_OK;
}

int nope_op_stem_conv(int dtype, const float* image, const float* w, const float* scale, const float* shift, float* w_scratch,
                      void* out, int n_img, int H, int W, nope_stream_t s) {
    int e = launch_stem_pack(w, scale, w_scratch, (hipStream_t)s);      // w_scratch: 147 * 64 floats
    if (e) return e;
    return launch_stem_conv(dtype, image, w_scratch, shift, out, n_img, H, W, (hipStream_t)s);
}

int nope_op_gn_chunks(int dtype, int HW, int C) { return gn_stats_chunks(HW, C, dtype); }

int nope_op_gn_apply_blocks(int dtype, int HW, int C, int n_hyp) { return gn_apply_blocks(HW, C, dtype, n_hyp); }

int nope_op_group_norm(const nope_gn_op* op, nope_stream_t stream) {
    if (!sized(op)) return NOPE_ERR_ARG;
    GnApplyArgs a;
    if (const int e = gn_args(*op, a)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int dt = op->dtype, nx = a.nhyp / a.x_rep;
    if (op->sh_s || op->sh_e) {              // the shared addend: a statistics pass forms x_eff, the apply pass forms it again
        if (!op->partial) return NOPE_ERR_ARG;
        if (op->colstats) return NOPE_ERR_UNSUPPORTED;
        a.nchunk = gn_stats_chunks(a.HW, a.C, dt);
        if (const int e = launch_gn_stats_shared(dt, a, op->partial, a.nchunk, s)) return e;
    } else if (op->colstats && op->fold_launch) {      // the separate fold launch + the partial path (what the runtimes do under NOPE_GN_FOLD_INLINE)
        if (const int e = launch_gn_fold(op->colstats, op->partial, nx, op->stat_blocks, a.C, a.G, s)) return e;
    } else if (op->colstats) {               // every gn_apply workgroup folds its sample's column statistics itself
        a.colstats = op->colstats; a.stat_blocks = op->stat_blocks;
    } else {
        a.nchunk = gn_stats_chunks(a.HW, a.C, dt);
        if (const int e = launch_gn_stats(dt, op->x, op->partial, nx, a.HW, a.C, a.G, a.nchunk, s)) return e;
    }
    return with_amax(op->amax_slot, op->amax_out, s, [&] { return launch_gn_apply(dt, a, s); });
}

int nope_op_gn_finalize(const float* partial, float* ms, int n_hyp, int nchunk, float count, float eps, nope_stream_t s) {
    return launch_gn_finalize(partial, ms, n_hyp, nchunk, count, eps, (hipStream_t)s);
}

int nope_op_amax_slot_words(void) { return kX2SlotWords; }

int nope_op_absmax_f32(const float* x, size_t n, uint32_t* amax_slot, float* amax_out, nope_stream_t s) {
    if (!amax_slot || !amax_out) return NOPE_ERR_ARG;
    return with_amax(amax_slot, amax_out, (hipStream_t)s, [&] { return launch_absmax_f32(x, n, amax_slot, (hipStream_t)s); });
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
