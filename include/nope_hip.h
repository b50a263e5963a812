/* nope_hip.h -- C ABI of libnope_hip.so: the MI355X (gfx950) implementation of the NOPE
 * inference hot path (template encoder + pose-conditioned U-Net template generation +
 * template-bank scoring).
 *
 * The reference (nv-nguyen/nope) is pure Python on torch ops and has no FFI of its own; the
 * drop-in boundary is its Python operator interface (src/model/model.py, u_net.py), mirrored
 * by `nope_amd/` on top of THIS library.  Each entry point names the reference code whose
 * arithmetic it replaces (paths relative to the reference tree).  See INTEGRATION.md for the
 * ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller owns all buffers; only nope_unet_create / nope_encoder_create allocate device memory
 *     (packed weights), and nope_encoder_forward keeps host-side hipGraph objects in its handle;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - no global state; calls with different handles, or with one U-Net handle and different workspaces, may
 *     run on different streams; returns 0 or a negative NOPE_ERR_* code;
 *   - nothing here ever falls back to the host: without a GPU the calls fail.
 */
#ifndef NOPE_HIP_H
#define NOPE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { NOPE_F32 = 0, NOPE_BF16 = 1,
       NOPE_F16 = 2,   /* IEEE half: storage type of the template bank (nope_similarity's bank_dtype, nope_unet_forward's out_dtype,
                          BASELINE configs[4]) and a compute mode of the networks: f16 storage + f16 MFMA, f32 accumulate / statistics
                          -- the MFMA rate of NOPE_BF16 with 3 more mantissa bits; stores saturate at +-65504 (no inf; a NaN is stored as -65504) */
       NOPE_BF16X3 = 3,/* compute mode only: f32 storage, every conv / linear as three bf16 MFMA passes over (hi, lo) bf16 splits of
                          both operands (hi*hi + hi*lo + lo*hi, f32 accumulate): ~2^-17 relative per product instead of bf16's 2^-9
                          at 3/16 of the exact-f32 MFMA cost -- meets the 1e-4 score tolerance */
       NOPE_F16X2 = 4  /* compute mode only: NOPE_BF16X3 (f32 storage, same kernels) except that the convolutions the ping-pong kernels run --
                          the tap-resident 3x3 kernel, 9/10 of the U-Net's work, and the per-tap kernel's long 1x1 / space-to-depth / phase
                          convs -- cost TWO pass equivalents instead of three: a_hi w_hi on the f16 MFMA
                          (hi = f16 part) plus ONE MX-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, twice the f16 rate) for both
                          cross terms, K-concatenated: [e4m3(a_lo) | e4m3(a)] x [e4m3(w) ; e4m3(w_lo)], power-of-two pre-scales undone by
                          the instruction's block scale.  The cross terms carry <= 2^-11 of the result, so 4-bit operands leave ~2^-15
                          per product -- the fast mode that meets the 1e-4 score tolerance.  As an element type of nope_op_conv /
                          nope_op_pack_conv_weight it names those kernels and their weight layout (modes PLAIN 1x1 / 3x3, DOWN2, UP2P;
                          Cin % 32 == 0; nope_op_conv refuses a launch whose shape no ping-pong kernel takes).
                          RANGE.  The tile forms its activation operands from a' = a * 2^-t, t a per-layer shift (0 at create time and for
                          nope_op_conv): f16(a') (saturates at 65504), e4m3(a'_lo * 2^9), e4m3(a' * 2^-2) (saturates at |a'| = 1792; four significant
                          bits down to |a'| = 2^-4); the accumulators hold 2^-t x the convolution and the epilogue multiplies by 2^t -- all
                          exact.  Full accuracy while the LARGEST |a| of a launch lies in [2^(t - 4), 1792 * 2^t] (t = 0: 0.06 .. 1792); outside,
                          the cross terms of the saturated / flushed elements are lost: plain-f16 accuracy (~2^-11 per product) there.  The
                          producers of a layer's inputs record max |a|; every forward is judged on the device and an out-of-range forward's
                          output is NaN (nope_unet_x2_poll / _range_check re-centre t and say so; nope_amd's U-Net repeats the call on request),
                          so the mode is never silently outside its accuracy at any magnitude an f32 tensor can hold */ };
/* Tap geometries of nope_op_conv.  UP2P is UP2 (nearest-x2 upsample + 3x3, pad 1) rewritten as four
 * 2x2 convolutions over the un-upsampled input, one per output-pixel parity, with the 3x3 weights that
 * fall on the same source pixel pre-summed at pack time: same function, 4/9 of the multiply-adds. */
enum { NOPE_CONV_PLAIN = 0, NOPE_CONV_UP2 = 1, NOPE_CONV_DOWN2 = 2, NOPE_CONV_UP2P = 3,
       NOPE_CONV_STRIDE2 = 4 /* stride 2: 3x3 pad 1 or 1x1 pad 0 (ResNet Bottleneck, encoder/resnet.py:64-65,122-123), 4x4 pad 1 (Downsample, model_utils.py:129-136) */,
       NOPE_CONV_STRIDE2_PAD01 = 5 /* (ABI 8) 3x3 stride 2 after a (0, 1, 0, 1) zero pad, no padding of its own: output (oy, ox) reads source rows / columns
                                      2 oy .. 2 oy + 2 (the Stable Diffusion VAE's Downsample, u_net/ldm/model.py:57-74; diffusers' Downsample2D(padding=0)).
                                      3x3 only, one source, even source size; weights packed as NOPE_CONV_STRIDE2's */ };
enum {
    NOPE_OK = 0,
    NOPE_ERR_ARG = -1,        /* bad argument (null pointer, unsupported size/dtype) */
    NOPE_ERR_LAUNCH = -2,     /* HIP reported a launch error */
    NOPE_ERR_WORKSPACE = -3,  /* workspace too small */
    NOPE_ERR_WEIGHT = -4,     /* missing / mis-shaped state-dict entry */
    NOPE_ERR_ALLOC = -5,
    NOPE_ERR_UNSUPPORTED = -6,
    NOPE_ERR_RANGE = -7,      /* nope_unet_x2_range_check: a NOPE_F16X2 launch saw activations outside its layer's window; the shifts were moved -- run the forward again */
    NOPE_ERR_RANGE_F16 = -8   /* ... non-finite activations (inf): no shift repairs that; nope_unet_x2_enable(net, 0) runs the NOPE_BF16X3 kernels, which propagate them as f32 does */
};

typedef void* nope_stream_t;

/* Bumped whenever a struct of this header changes layout or an enum gains a meaning (2: nope_unet_config.soft_up_down;
 * 3: NOPE_F16 / NOPE_BF16X3 compute modes, 4x4 STRIDE2, nope_ldm_config.transformer_depth;
 * 4: nope_op_geodesic, nope_unet_graph_limit -- hipGraph replay became opt-in;
 * 5: NOPE_F16X2, nope_tuning_reload, nope_gather_topk, nope_topk_merge;
 * 6: nope_unet_x2_poll / _x2_range_check / _x2_enable / _x2_shifts, NOPE_ERR_RANGE*;
 * 7: nope_ldm_config.head_channels / resblock_updown / conv_resample, nope_op_token_attention dim_head 64 / 128;
 * 8: NOPE_CONV_STRIDE2_PAD01, nope_op_wide_attention, nope_vae_*;
 * 9: nope_op_render_depth, nope_op_vsd, NOPE_VSD_* / NOPE_VISIB_*;
 * 10: nope_gd_config, nope_gd_*;
 * 11: nope_op_conv_stat_rows, nope_op_conv_ex, nope_op_group_norm_ex, nope_op_gn_apply_blocks, nope_op_gn_finalize, nope_op_absmax_f32,
 *     nope_op_amax_slot_words -- the fused GroupNorm statistics / PreNorm / range-slot plumbing at operator level;
 * 12: nope_vis_column, nope_op_vis_grid, nope_op_vis_sheet, NOPE_VIS_*;
 * 13: nope_op_crop_frames;
 * 14: nope_op_group_norm_shared, nope_op_conv_class_weights;
 * 15: nope_op_refine_init / _normal_eq / _normal_eq_workspace_bytes / _step / _select, NOPE_REFINE_*;
 * 16: nope_op_conv_gn_tail, nope_op_conv_tail_stat_blocks;
 * 17: nope_conv_op / nope_op_conv / nope_op_conv_query and nope_gn_op / nope_op_group_norm take their arguments by name and replace
 *     nope_op_conv_ws, nope_op_conv_ex, nope_op_conv_gn_tail, nope_op_conv_splitk_bytes, nope_op_conv_stat_rows, nope_op_conv_tail_stat_blocks,
 *     nope_op_group_norm_ex and nope_op_group_norm_shared);
 * 18: nope_op_pose_modes;
 * 19: nope_conv_op gains gn_emb, gn_emb_stride, gn_self, gn_resid_rep (the conv's own GroupNorm);
 * 20: nope_op_c2f_expand, nope_op_c2f_commit;
 * 21: nope_op_multiref_prepare, nope_multiref_similarity, nope_op_multiref_fuse_scores;
 * 22: nope_op_multiref_select, nope_op_multiref_gather;
 * 23: nope_robust_similarity, nope_op_residual_maps, nope_op_pool_mask;
 * 24: nope_op_pose_errors, nope_op_mesh_diameter and their _workspace_bytes, NOPE_POSE_ERR_*;
 * 25: nope_op_fit_translation, nope_op_mask_boxes, nope_op_depth_shift and its _workspace_bytes, NOPE_FIT_*.  Callers compare
 * nope_abi_version() against the header they were built with before passing any struct (nope_amd/hip.py does at load time). */
#define NOPE_ABI_VERSION 25
const char* nope_strerror(int code);
int nope_abi_version(void);
/* The library reads its tuning / test switches (NOPE_* environment variables: launch policies, A/B switches, traces) once per call site and
 * caches them.  A caller that changes one of them after its first call into the library calls this to have them read again (the Python
 * binding does so by itself).  No reference counterpart: the reference has no tuning switches. */
void nope_tuning_reload(void);

/* ------------------------------------------------------------------------------------------
 * Template-bank scoring.  Replaces PoseConditional.retrieval's "l2" metric,
 * src/model/model.py:257-262:
 *     score[b,n] = - sum_{h,w} sqrt( sum_c (q[b,c,h,w] - t[b,n,c,h,w])^4 )
 * without materialising the repeated query (model.py:258).
 *   q       (B,C,H,W) f32, contiguous
 *   bank    (B,N,C,H,W) of `bank_dtype` (NOPE_F32 | NOPE_BF16 | NOPE_F16); sample stride `bank_stride_b`
 *           ELEMENTS (0 = one bank shared by every query)
 *   scores  f32, row b at scores + b*score_ld  (score_ld >= N; lets a rank write its
 *           N/G slice of a gathered (B,N) matrix in place)
 * HW*sizeof(elt) must be a multiple of 16 bytes. */
int nope_similarity(const float* q, const void* bank, int bank_dtype, float* scores, int B, int N, int C, int H,
                    int W, int64_t bank_stride_b, int score_ld, nope_stream_t stream);

/* Top-k over each row.  Replaces `similarity.topk(k=5, dim=1)`, model.py:265.
 * Order: descending score; ties -> lowest index (argmax semantics); NaN ranks highest.
 *   idx   (B,k) int64;  vals (B,k) f32 or NULL.   1 <= k <= 16, k <= N. */
int nope_topk(const float* scores, int64_t* idx, float* vals, int B, int N, int k, int score_ld,
              nope_stream_t stream);

/* Template-sharded banks (north_star: "partition [the bank] across the 8 GPUs of one node with an RCCL all-gather of per-shard top-k
 * scores"; the reference has no collective on this path).  Rank r of G holds the contiguous slice [lo_r, hi_r) of the N
 * templates (balanced: the first N % G ranks one more) and scores it into a padded (B, nmax) buffer, nmax = ceil(N / G); the collective
 * itself stays with the caller (torch.distributed / RCCL).  Two ways to finish the step, each ONE launch behind the collective:
 *   nope_gather_topk  gathered (G,B,nmax) f32 = the all-gathered slices -> scores (B,N) f32, the full similarity `retrieval` returns and the
 *                     harness saves (model.py:323,369-375), AND its top-k (model.py:265; k = 0: scores only, idx / vals may be NULL);
 *   nope_topk_merge   cand_vals / cand_idx (B,M) = the all-gathered per-shard top-k lists (M = G k values with their GLOBAL template
 *                     indices, shards in rank order) -> the global top-k.  Same order as nope_topk on the full row: descending score, ties
 *                     -> lowest global index, compared on the index each candidate CARRIES (then on list position, for two entries with
 *                     the same index).  A pad fills a list that holds fewer than k real candidates: score -inf, index INT64_MAX.  It
 *                     ranks behind every real candidate, a real -inf score included (INT64_MAX is the highest index), and comes back
 *                     only when the lists hold fewer than k real candidates together.  For callers that do not need the
 *                     full similarity: 12 k bytes per query and rank cross the fabric instead of 4 N / G. */
int nope_gather_topk(const float* gathered, int n_ranks, int B, int n_total, float* scores, int64_t* idx, float* vals, int k,
                     nope_stream_t stream);
int nope_topk_merge(const float* cand_vals, const int64_t* cand_idx, int64_t* idx, float* vals, int B, int M, int k, nope_stream_t stream);

/* Geodesic error of the retrieved poses against the ground truth (row f2).  Replaces `pred_R = template_poses[nearest_idx]`,
 * src/model/model.py:352-354, and GeodesicError's per-element arithmetic, src/model/loss.py:14-75 (so3_relative_angle_with_symmetry:
 * symmetry 0 = none, 1 = 180 degrees about Y, 2 = circular) with pytorch3d's so3_relative_angle(eps = 1e-2) restated from its
 * published formula (acos_linear_extrapolation, bound 1 - 1e-4).  float64 throughout, as loss.py:87,103 casts.
 *   poses     (B, N, 3, 3) f64, sample stride `pose_stride_b` elements (0 = one grid shared by every query)
 *   idx       (B, k) int64 rows of `poses` to score (nope_topk's output), or NULL: score poses[b, 0..k)
 *   gt        (B, 3, 3) f64;  symmetry (B) int32 in {0, 1, 2} or NULL (all 0)
 *   err_rad   (B, k) f64 radians
 *   status    one device int: bit 0 = a trace left [-1 - eps, 3 + eps] (pytorch3d raises ValueError there: the caller must),
 *             bit 1 = an index outside [0, N). */
int nope_op_geodesic(const double* poses, int64_t pose_stride_b, int N, const int64_t* idx, const double* gt, const int* symmetry,
                     double* err_rad, int* status, int B, int k, nope_stream_t stream);

/* (ABI 18) Pose distribution and distinct pose modes from the retrieval scores.  No reference counterpart: the
 * reference stops at `similarity.topk(k=5)` (src/model/model.py:265), one grid vertex and four of its neighbours.  One workgroup per query,
 * no workspace, nothing read by the host, no floating-point atomics: bit-identical from run to run.
 *   similarity      (B, N) f32, row stride similarity_ld >= N; columns >= N are never read
 *   template_poses  (B|1, N, 3, 3) f64, sample stride pose_stride_b elements (0 = one grid for every query, as nope_op_geodesic)
 *   symmetry        (B) int32 in {0, 1, 2} or NULL (all 0)
 * Distribution, per row: p[n] = exp((s[n] - max s) / temperature) / Z and entropy = -sum p ln p (nats, 0 ln 0 = 0); exponentials, sums and
 * the entropy in f64, rounded once to f32.  -inf is an ordinary score (p = 0, ranks last).  A row whose maximum is NaN or +-inf is
 * undefined: its prob row and entropy are NaN, n_modes = 0, every slot mode_idx = -1 / mode_score = NaN / mode_mass = 0 / mode_count = 0,
 * and *status (one device int, zeroed by the call) gets bit 0; the other rows are not affected.
 * Modes, greedy suppression: all N templates start alive; slot m = 0, 1, ...: the seed is the alive template with the highest score (ties ->
 * the lowest index, nope_topk's rule), its members are the alive templates n with d(poses[n], poses[seed]) <= radius_rad (the seed always, a
 * NaN distance never); mode_idx = seed, mode_score = s[seed], mode_mass = sum of p over the members (f64 sum), mode_count = their number;
 * the members leave.  It stops when nothing is alive; n_modes[b] = the slots filled this way.  Left-over slots: fill = 0: mode_idx = -1,
 * mode_score = -inf, mass 0, count 0; fill = 1 (needs max_modes <= N): the best-scoring templates not yet listed, in nope_topk order, with
 * mass 0 and count 0 -- a caller that needs exactly max_modes valid candidates always gets them.  max_modes = 0: the distribution only.
 * The distance d is this op's own, f64: theta(A, B) = acos(clamp((tr(A B^T) - 1) / 2, -1, 1)); symmetry 0: theta(A, B); 1: min(theta(A, B),
 * theta(diag(-1, 1, -1) A, B)); 2: the clamped acos of the cosine between the viewing axes -inv(P)[2, :] (norms floored at 1e-8).  Unlike
 * nope_op_geodesic it does not reproduce the reference's f32 round trips, pytorch3d's linear extrapolation of acos (a self-distance of
 * 0.0071 rad) or the unclamped acos of the circular branch (NaN between viewpoints of equal elevation): right for a reported metric, wrong
 * for a membership decision.  The two differ by <= 0.0071 rad, near 0 and pi only.
 *   prob (B, N) f32, row stride prob_ld, or NULL;  entropy (B) f32;  mode_idx (B, max_modes) int64;  mode_score, mode_mass (B, max_modes)
 *   f32;  mode_count (B, max_modes) int32;  n_modes (B) int32.
 * NOPE_ERR_ARG, before anything is launched or written: temperature not finite or not > 0; radius_rad NaN or < 0; max_modes outside
 * [0, 64]; N < 1; fill with max_modes > N; a missing pointer.  The alive flags live in LDS: N <= 262144, NOPE_ERR_UNSUPPORTED beyond. */
int nope_op_pose_modes(const float* similarity, int64_t similarity_ld, const double* template_poses, int64_t pose_stride_b, int N,
                       const int* symmetry, double temperature, double radius_rad, int max_modes, int fill, float* prob, int64_t prob_ld,
                       float* entropy, int64_t* mode_idx, float* mode_score, float* mode_mass, int* mode_count, int* n_modes, int* status,
                       int B, nope_stream_t stream);

/* (ABI 20) Coarse-to-fine pose retrieval over nested viewpoint grids.  No reference counterpart: the reference
 * scores every pose of the grid (src/model/model.py:313,323).  Icosphere levels are nested, so a query can be scored in stages: the coarsest
 * level, then the finer-level neighbours of its best few poses, and so on.  The caller's loop (nope_amd/search.py: coarse_to_fine_search):
 *     nope_op_c2f_expand (no seeds);  scores of `rows` (nope_unet_forward + nope_similarity);  nope_op_c2f_commit
 *     stages x { nope_topk of the sparse row -> seeds;  nope_op_c2f_expand;  scores of `rows`;  nope_op_c2f_commit };  nope_topk
 * The sparse score row holds -inf where nothing was evaluated: an ordinary input to nope_topk, nope_op_pose_modes and nope_op_refine_select.
 * Both entries: one workgroup per query, no workspace, nothing read by the host, no floating-point atomics, plain vector stores only, and
 * byte-identical output from run to run (the slot of a candidate comes from a block-wide prefix scan, never from thread timing).
 *
 * nope_op_c2f_expand chooses this stage's candidates and gathers their pose rows.
 *   template_poses  (B|1, N, 3, 3) f64, sample stride pose_stride_b elements (0 = one grid for every query, as nope_op_pose_modes)
 *   stage_of        (N) int32: the first stage at which a pose is eligible; shared by the batch
 *   state           (B, N) uint8, in/out: 0 = not evaluated, 1 = evaluated or chosen
 *   seeds           (B, n_seeds) int64, as nope_topk writes them; n_seeds in [0, 16] (0: may be NULL)
 *   all_relativeR   (B, N, 6) f32
 * A pose p is eligible when stage_of[p] <= max_stage and state[b, p] == 0.  n_seeds == 0 (stage 0): every eligible pose is a candidate, in
 * ascending index order.  Otherwise, for each seed in the given order: the eligible poses p != seed with d(poses[p], poses[seed]) <=
 * radius_rad (a NaN distance never qualifies), in ascending index order; a pose is a candidate once, under the first seed that reaches it.
 * The seed itself is never a candidate of its own pass: it is already evaluated.  The first `capacity` candidates of that sequence are
 * emitted and get state = 1; the rest are dropped: their state stays 0 and n_dropped[b] counts each of them once.
 * The distance d is f64.  dist_kind 0, rotation: theta(A, B) = acos(clamp((tr(A B^T) - 1) / 2, -1, 1)), exactly nope_op_pose_modes'.
 * dist_kind 1, viewpoint: the clamped acos of the cosine between the third ROWS P[2, :] (norms floored at 1e-8) -- the camera's optical
 * axis in the object frame.  It is NOT nope_op_pose_modes' symmetry class 2, whose axis -inv(P)[2, :] is the third column and depends on
 * the elevation only.
 *   cand       (B, capacity) int32: the candidates in emission order, then -1
 *   n_cand, n_dropped  (B) int32
 *   rows       (B, capacity, 6) f32: the exact bits of all_relativeR[b, cand].  A padded slot carries the row of the query's first valid
 *              seed (n_seeds == 0, or no valid seed: the row of pose 0): the U-Net sees a finite pose, and its score is discarded.
 *   status     one device int, zeroed by the call: bit 0 = a query overflowed `capacity`, bit 1 = a seed outside [0, N) (it is skipped).
 * NOPE_ERR_ARG, before anything is launched or written: N < 1; capacity < 1; n_seeds outside [0, 16]; radius_rad NaN or < 0 with
 * n_seeds > 0; dist_kind not 0 or 1; a missing pointer.  "Reached by an earlier seed" is a flag in LDS, laid out as nope_op_pose_modes'
 * alive flags: N <= 262144, NOPE_ERR_UNSUPPORTED beyond.
 *
 * nope_op_c2f_commit writes scores[b, j] ((B, capacity) f32) into similarity[b, cand[b, j]] ((B, N) f32, row stride similarity_ld >= N)
 * for every 0 <= cand < N, bit for bit (NaN included); -1 is skipped; nothing else is touched, columns >= N included. */
int nope_op_c2f_expand(const double* template_poses, int64_t pose_stride_b, int N, const int* stage_of, int max_stage, uint8_t* state,
                       const int64_t* seeds, int n_seeds, double radius_rad, int dist_kind, const float* all_relativeR, int capacity, int* cand,
                       int* n_cand, int* n_dropped, float* rows, int* status, int B, nope_stream_t stream);
int nope_op_c2f_commit(const float* scores, const int* cand, int capacity, int N, float* similarity, int64_t similarity_ld, int B,
                       nope_stream_t stream);

/* (ABI 21) Multi-reference pose retrieval: several posed reference views of one object fused into one score row.
 * No reference counterpart: the reference has one reference image per object (src/model/model.py:313,323).  Per sample b: one query, R
 * references (1 <= R <= 8) with their object-to-camera rotations P[b, r] in the object frame of the template grid T[n], and optionally
 * n_refs[b] <= R: references r >= n_refs[b] are padding.  The caller's sequence:
 *     nope_op_multiref_prepare;  nope_unet_forward on the B R sources with all_relativeR viewed as (B R, N, 6) -> bank (B, R, N, C, H, W);
 *     feature fusion: nope_multiref_similarity      or  score fusion: nope_similarity of the bank viewed as (B, R N, C, H, W), then
 *     nope_op_multiref_fuse_scores;  nope_topk
 * The fused (B, N) row is an ordinary input to nope_topk, nope_op_pose_modes and nope_op_refine_select.
 *
 * nope_op_multiref_prepare: the relative poses and the blend weights.  One launch, f64 arithmetic, nothing read by the host, no atomics
 * (the status word has one writer), plain vector stores only, byte-identical from run to run.
 *   template_poses  (B|1, N, 3, 3) f64, sample stride pose_stride_b elements (0 = one grid for every query, as nope_op_pose_modes)
 *   ref_poses       (B, R, 3, 3) f64
 *   n_refs          (B) int32 or NULL (all R)
 * The distance d[b, r, n] between T[n] and P[b, r] is nope_op_c2f_expand's: dist_kind 0, rotation: acos(clamp((tr(T P^T) - 1) / 2, -1, 1));
 * dist_kind 1, viewpoint: the clamped acos of the cosine between the third rows, norms floored at 1e-8.
 *   all_relativeR   (B, R, N, 6) f32 or NULL: the first two rows of T[n] P[b, r]^T, computed in f64 and rounded once to f32 -- the
 *                   reference's R_q R_ref^-1 (src/dataloader/shapeNet.py:243-245) for an orthonormal P; orthonormality is not checked.
 *                   A padded reference carries the rows of reference 0: the U-Net sees a finite pose.
 *   weights         (B, R, N) f32.  weighting 0, uniform: 1 / n_refs[b].  1, softmax: exp(-(d_r - d_min) / tau_rad) / sum_r exp(-(d_r -
 *                   d_min) / tau_rad), the sum over the valid references in ascending r, f64, rounded once to f32.  2, nearest: 1 at the
 *                   valid reference with the smallest d (ties -> the lowest r), 0 elsewhere.  Padded references get 0.
 *   dist            (B, R, N) f64 or NULL: d; +inf at a padded reference.
 *   status          one device int, written by the call: bit 0 = a valid reference pose has a non-finite entry, bit 1 = n_refs[b] outside
 *                   [1, R].  In either case EVERY weight of that sample is NaN, so its fused row is NaN and ranks first in nope_topk:
 *                   visible, never silently wrong.  The other samples are not affected.
 * NOPE_ERR_ARG, before anything is launched or written: R outside [1, 8]; N < 1; tau_rad not finite or not > 0 under softmax; an unknown
 * weighting or dist_kind; a missing pointer (template_poses, ref_poses, weights, status).
 *
 * nope_multiref_similarity: the score against the blend of the R banks, in one streaming pass; the blend is never materialised.
 *   q (B, C, H, W) f32;  bank (B, R, N, C, H, W) of bank_dtype (NOPE_F32 | NOPE_BF16 | NOPE_F16), contiguous;  weights (B, R, N) f32;
 *   scores f32, row b at scores + b * score_ld (score_ld >= N).
 * Per element: tbar = 0.0f; for r = 0 .. R - 1 in that order: if (w[b, r, n] != 0) tbar = fma(w[b, r, n], float(t[b, r, n, c, p]), tbar), in
 * f32 -- one fused multiply-add per term on the device.  (The host interpreter build of the test suite has no fused multiply-add and
 * rounds the product and the sum separately.)  Then score[b, n] = - sum_p sqrt(sum_c (q - tbar)^4) with nope_similarity's arithmetic per
 * bank type: the correctly rounded sqrtf for f32 banks, the hardware square root for the 16-bit ones.  A term whose weight is exactly 0
 * contributes nothing whatever its bank entries hold, NaN and inf included: it is discarded by a select, never multiplied.  NaN is not 0:
 * a NaN weight gives a NaN score.  R = 1 with weight 1 is nope_similarity's definition (another kernel: the two agree to the last bits of
 * the sums, not bit for bit).  Shape limits are nope_similarity's: H W a multiple of 4 (f32)
 * or 8 (16-bit); the generic form (taken when H W / (4 | 8) does not divide 256, or C > 16) needs C H W <= 16384; NOPE_ERR_UNSUPPORTED
 * beyond.  NOPE_ERR_ARG: R outside [1, 8], a missing pointer, a size < 1, score_ld < N.
 *
 * nope_op_multiref_fuse_scores: late fusion.  per_ref, weights (B, R, N) f32 -> scores[b, n] = f32(sum_r f64(w) f64(s)), ascending r,
 * terms with w == 0 skipped (a -inf or NaN score under a zero weight does not poison the row), row stride score_ld >= N; columns >= N
 * are not touched.  The per-reference scores need no entry of their own: nope_similarity of the bank viewed as (B, R N, C, H, W). */
int nope_op_multiref_prepare(const double* template_poses, int64_t pose_stride_b, int N, const double* ref_poses, int R, const int* n_refs,
                             int weighting, double tau_rad, int dist_kind, float* all_relativeR, float* weights, double* dist, int* status, int B,
                             nope_stream_t stream);
int nope_multiref_similarity(const float* q, const void* bank, int bank_dtype, const float* weights, float* scores, int B, int R, int N, int C,
                             int H, int W, int score_ld, nope_stream_t stream);
int nope_op_multiref_fuse_scores(const float* per_ref, const float* weights, float* scores, int B, int R, int N, int64_t score_ld,
                                 nope_stream_t stream);

/* (ABI 22) Multi-reference retrieval from the M nearest references per pose.  No reference counterpart.  The ABI 21
 * sequence runs the U-Net on every (reference, pose) pair, B R N hypotheses; here the caller decides per (sample, pose), before the U-Net
 * runs, which M <= R references that pose is generated from, and the U-Net runs on B M S hypotheses whatever R is.  The caller's sequence:
 *     nope_op_multiref_select;  nope_op_multiref_gather -> sources (B M S, C, H, W);  nope_unet_forward on those sources, one pose each
 *     (x_rep = 1), with all_relativeR viewed as (B M S, 6) -> bank (B, M, S, C, H, W);
 *     M > 1: nope_multiref_similarity or nope_similarity + nope_op_multiref_fuse_scores with R := M;  M = 1: nope_similarity;  nope_topk
 * With a candidate list the S slots are the candidates of a coarse-to-fine stage (nope_op_c2f_expand's cand; scores back through
 * nope_op_c2f_commit) or the k candidates of a refinement (nope_topk's indices as int32).
 *
 * nope_op_multiref_select: the M nearest references of every slot.  One launch, f64 arithmetic, one thread per (b, slot), nothing read by
 * the host, no atomics (the status word has one writer), plain vector stores only, byte-identical from run to run.
 *   template_poses, pose_stride_b, ref_poses, n_refs, weighting, tau_rad, dist_kind: as nope_op_multiref_prepare
 *   cand            (B, S) int32 or NULL.  NULL: S = N (the argument S is ignored) and slot s is pose s.  Otherwise slot s is pose
 *                   cand[b, s], laid out as nope_op_c2f_expand writes it: candidates, then -1.
 *   M               in [1, R]
 * Per valid slot: d[r], nope_op_multiref_prepare's distance (the same bits), of the valid references; ordered by (d, r) ascending, a NaN
 * after every number; the first Mv = min(M, n_refs[b]) are kept.
 *   src             (B, M, S) int32: the kept reference of slot m
 *   all_relativeR   (B, M, S, 6) f32 or NULL: the first two rows of T[p] P[b, src]^T, f64 rounded once (nope_op_multiref_prepare's bits)
 *   weights         (B, M, S) f32.  uniform: 1 / Mv.  softmax, over the KEPT references only: exp(-(d_m - d_0) / tau_rad) / sum_m exp(-(d_m -
 *                   d_0) / tau_rad), the sum in ascending m, f64 rounded once.  nearest: 1 at m = 0, 0 elsewhere.
 *   dist            (B, M, S) f64 or NULL
 * Slots m >= Mv: weight exactly 0, src and pose rows of slot 0, dist +inf.  A padded candidate (cand == -1): all M weights 0, src 0, the rows
 * of pose 0 against reference 0, dist +inf.  A cand entry below -1 or >= N: as padding, and status bit 2.  Status bits 0 and 1 are
 * nope_op_multiref_prepare's, and so is their rule: EVERY weight of such a sample is NaN (padded slots included), src stays inside [0, R).
 * NOPE_ERR_ARG, before anything is launched or written: nope_op_multiref_prepare's cases; M outside [1, R]; S < 1 with cand given; a
 * missing src, weights or status.
 *
 * nope_op_multiref_gather: out[b, j, :] = reference_feats[b, src[b, j], :], j in [0, J) (J = M S), both f32, rows of L = C H W elements, L a
 * multiple of 4: 16-byte copies, bit for bit (NaN payloads survive).  reference_feats (B, R, L), src (B, J) int32, out (B, J, L).  A src
 * entry outside [0, R) fills its row with NaN: visible, never a wild read.  NOPE_ERR_ARG: L % 4, a missing pointer, a size < 1. */
int nope_op_multiref_select(const double* template_poses, int64_t pose_stride_b, int N, const double* ref_poses, int R, const int* n_refs,
                            const int* cand, int S, int M, int weighting, double tau_rad, int dist_kind, int* src, float* all_relativeR, float* weights,
                            double* dist, int* status, int B, nope_stream_t stream);
int nope_op_multiref_gather(const float* reference_feats, const int* src, float* out, int B, int R, int J, int64_t L, nope_stream_t stream);

/* (ABI 23) Occlusion-robust scoring: masked and trimmed template scores.  No reference counterpart: the reference
 * scores every pixel of the latent map (src/model/model.py:257-262), so one covered region of a query crop adds a large term to the score
 * of the CORRECT template.  Two mechanisms, usable together: a mask (the caller knows which latent pixels show the object: only those are
 * scored) and a trim (nobody knows where the occluder is: per hypothesis the largest per-pixel terms are dropped, as a fraction of the
 * scored pixels -- a least-trimmed sum, which is scale-free).  Off by default everywhere; an addition next to the "l2" metric.
 *
 * With d[b,n,p] = sqrt( sum_c (q[b,c,p] - t[b,n,c,p])^4 ) in nope_similarity's arithmetic per bank type (f32 accumulation; sqrtf for f32
 * banks, the hardware square root for the 16-bit banks):
 *     A[b]  = { p : mask[b,p] != 0 }   (mask NULL: all H W pixels),  a = |A[b]|
 *     t     = min(a - 1, (int)floorf(trim * (float)a))               trim f32 in [0, 1): one f32 product, then floor
 *     m     = a - t                                                  (m >= 1 whenever a >= 1)
 *     score[b,n] = - ( sum of the m smallest values of { d[b,n,p] : p in A[b] } )
 * The sum of the m smallest is a multiset quantity: ties need no rule.  It is formed as s_less + (m - c_less) v, v the m-th smallest value
 * (an exact bitwise selection on the f32 patterns, which are ordered because d >= 0), s_less and c_less the sum and the count of the values
 * strictly below v; the second term is added only when m - c_less > 0 (an infinite v never meets a factor 0).
 *   - a pixel outside A[b] is a select: its bank and query values do not enter, NaN or inf there does not leak;
 *   - any NaN among the d of A[b] makes the score NaN (NaNs are never trimmed away as "the largest"); +inf is an ordinary largest value:
 *     trimmed it leaves a finite score, kept it gives -inf;
 *   - a == 0: the whole row is NaN;  all kept terms zero: the score is -0.0, as a planted match scores in nope_similarity;
 *   - trim == 0 with mask == NULL is nope_similarity's definition from another kernel: the two agree to the last bits of the sums, not bit
 *     for bit (the statement made for nope_multiref_similarity);  trim == 0 skips the selection: a plain masked sum;
 *   - fixed-shape reductions, no floating-point atomics: bit-identical from run to run.
 *   q, bank, bank_dtype, bank_stride_b (0 = one shared bank), scores, score_ld and the shape limits: as nope_similarity
 *   mask    (B, H, W) uint8 or NULL
 * NOPE_ERR_ARG: trim outside [0, 1) or NaN, and nope_similarity's cases.
 *
 * nope_op_residual_maps: the d planes of chosen hypotheses -- where a match disagrees.  out[b, j, p] = d[b, idx[b, j], p], (B, k, H, W) f32;
 * idx (B, k) int64 or NULL (templates 0..k, k <= N).  An index outside [0, N) gives a NaN plane, never a wild read.  Any H, W >= 1.
 *
 * nope_op_pool_mask: an image-resolution coverage plane (B, S_h, S_w) -> the latent mask (B, H, W) uint8 in {0, 1}; S_h % H == 0 and
 * S_w % W == 0 (else NOPE_ERR_ARG); a cell is (S_h / H) x (S_w / W) pixels.
 *   is_u8 != 0: cover is uint8 alpha; mask = 1 where the cell's integer byte sum is >= min_sum_u8 (exact).
 *   is_u8 == 0: cover is an f32 visibility in [0, 1]; mask = 1 where the cell's f32 sum, taken in row-major order within the cell, divided
 *               by the f32 area is >= min_mean_f32 (a NaN never is). */
int nope_robust_similarity(const float* q, const void* bank, int bank_dtype, const uint8_t* mask, float trim, float* scores, int B, int N, int C,
                           int H, int W, int64_t bank_stride_b, int score_ld, nope_stream_t stream);
int nope_op_residual_maps(const float* q, const void* bank, int bank_dtype, const int64_t* idx, float* out, int B, int N, int k, int C, int H,
                          int W, int64_t bank_stride_b, nope_stream_t stream);
int nope_op_pool_mask(const void* cover, int is_u8, int B, int S_h, int S_w, int H, int W, int64_t min_sum_u8, float min_mean_f32, uint8_t* mask,
                      nope_stream_t stream);

/* (ABI 15) Sub-grid pose refinement: Gauss-Newton on SO(3) through the U-Net.  No reference counterpart: the reference's prediction is
 * template_poses[nearest_idx] (src/model/model.py:352-354), a vertex of the template grid (26 templates: ~32 degrees apart).  The U-Net is a
 * smooth function of a continuous rotation and its training loss is the distance between its output and the query's embedding
 * (model.py:96-111), so a caller can descend on || u_net(reference_feat, dR) - query_feat ||^2 from the retrieved candidates.  There is no
 * autograd behind this ABI: the Jacobian is a central difference over left-multiplied tangent steps, six extra hypotheses per candidate.
 * A candidate (b, j) carries dR (3 x 3 row-major f64).  The caller's loop (nope_amd/model.py: PoseConditional.refine_from_feat):
 *     nope_op_refine_init                                  dR = GramSchmidt(all_relativeR[b, idx[b, j]]), first seven poses
 *     iters x { nope_unet_forward on poses (B, 7k, 6) -> maps (B, k, 7, C, h, w) f32;  nope_op_refine_normal_eq;  nope_op_refine_step }
 *     nope_unet_forward on the k base poses;  nope_similarity of those maps;  nope_op_refine_select
 * Nothing in it is read by the host.  The seven poses of a candidate, as 6-D f32 rows (the first two matrix rows, the U-Net's pose input,
 * src/poses/rotation_conversions.py:490-503), h = fd_step radians:
 *     [dR, exp(+h e_x) dR, exp(-h e_x) dR, exp(+h e_y) dR, exp(-h e_y) dR, exp(+h e_z) dR, exp(-h e_z) dR]
 * Everything below is f64 arithmetic on the device and run-to-run deterministic. */
enum { NOPE_REFINE_NONFINITE = 1,  /* step: a normal-equation entry (or the solution) is not finite: no step */
       NOPE_REFINE_SINGULAR = 2,   /* step: det(A + damping diag A) <= 0: no step */
       NOPE_REFINE_ZERO_STEP = 3,  /* step: the solution is exactly 0 (g = 0): no step */
       NOPE_REFINE_CLAMPED = 4,    /* step: taken, |w| was cut to max_step_rad (direction kept) */
       NOPE_REFINE_BAD_INDEX = 5   /* init: idx outside [0, N) (clamped into it) */ };
/*   all_relativeR (B, N, 6) f32;  idx (B, k) int64 (nope_topk's);  fd_step > 0
 *   dR, dR_init   (B, k, 3, 3) f64 out: the Gram-Schmidt matrix (b1 = a1 / |a1|, b2 = normalised a2 - (b1 . a2) b1, b3 = b1 x b2), twice
 *   poses         (B, 7k, 6) f32 out, candidate-major: row (j * 7 + m) of sample b
 *   status        (B, k) int32 out: 0 or NOPE_REFINE_BAD_INDEX */
int nope_op_refine_init(const float* all_relativeR, int64_t N, const int64_t* idx, double* dR, double* dR_init, float* poses, int* status,
                        int B, int k, double fd_step, nope_stream_t stream);
/*   q (B, C, h, w) f32;  maps (B, k, 7, C, h, w) f32, the U-Net's outputs for `poses`
 *   normal_eq (B, k, 10) f64 out: A00 A01 A02 A11 A12 A22 | g0 g1 g2 | cost, with r = t0 - q, J_a = (t_{+a} - t_{-a}) / (2 fd_step),
 *             A = J^T J, g = J^T r, cost = r^T r.  Differences, products and sums in f64; sums of (t+ - t-) products, scaled once.
 *   workspace nope_op_refine_normal_eq_workspace_bytes(B, k, h, w) bytes: the per-(candidate, pixel slice) partial sums, folded in slice order.
 * h * w must be a multiple of 16 (NOPE_ERR_UNSUPPORTED otherwise; every network here needs that already); pointers 16-byte aligned. */
size_t nope_op_refine_normal_eq_workspace_bytes(int B, int k, int H, int W);
int nope_op_refine_normal_eq(const float* q, const float* maps, double* normal_eq, int B, int k, int C, int H, int W, double fd_step,
                             void* workspace, size_t workspace_bytes, nope_stream_t stream);
/*   Solves (A + damping diag A) w = -g, scales w to |w| = max_step_rad when it is longer, dR <- GramSchmidt(exp(w) dR) (exp: Rodrigues),
 *   writes the next seven poses and status (B, k) int32: 0, NOPE_REFINE_CLAMPED (step taken), or NOPE_REFINE_NONFINITE / _SINGULAR /
 *   _ZERO_STEP: no step, dR stays as it is bit for bit (the poses are written again all the same). */
int nope_op_refine_step(const double* normal_eq, double* dR, float* poses, int* status, int B, int k, double fd_step, double max_step_rad,
                        double damping, nope_stream_t stream);
/*   score_refined (B, k) f32: nope_similarity of the query against the maps of the k refined poses (the reference's metric, model.py:257-262)
 *   similarity    (B, N) f32, row stride similarity_ld: the retrieval scores; candidate j's is similarity[b, idx[b, j]]
 *   A refined pose is kept iff score_refined > that score (Gauss-Newton minimises the plain L2 distance, the score is quartic: without this
 *   guard a step could lower it); a NaN on either side is never an improvement.  A candidate that is not kept reverts to dR_init and its
 *   retrieval score.  The candidates are then ordered by final score, descending; ties -> the lower retrieval rank; a NaN first, as nope_topk.
 *   Outputs, all in the final order: out_dR (B, k, 3, 3) f64, out_6d (B, k, 6) f32 (its first two rows), out_score / out_score_init (B, k) f32,
 *   out_accepted (B, k) int32, out_order (B, k) int64 (the retrieval rank of each entry), and -- with template_poses (B, N_t, 3, 3) f64, sample
 *   stride template_stride_b elements (0 = one grid for every query), or both NULL --
 *       pred_R (B, k, 3, 3) f64 = (dR dR_init^T) template_poses[b, idx[b, j]]   (a reverted candidate: the grid pose itself, bit for bit)
 *   which nope_op_geodesic scores as a per-sample pose table (pose_stride_b = 9k, idx = NULL).  1 <= k <= 16. */
int nope_op_refine_select(const double* dR, const double* dR_init, const float* score_refined, const float* similarity, int64_t similarity_ld,
                          int64_t N, const int64_t* idx, const double* template_poses, int64_t template_stride_b, int64_t n_templates,
                          double* out_dR, float* out_6d, float* out_score, float* out_score_init, int* out_accepted, int64_t* out_order,
                          double* pred_R, int B, int k, nope_stream_t stream);

/* (ABI 9) Depth rendering of object meshes for the VSD evaluation.  Replaces pyrenderer, src/poses/vsd.py:25-54 (pyrender's OpenGL
 * OffscreenRenderer with an IntrinsicsCamera, znear 0.05, zfar 100000, DEPTH_ONLY), as called by vsd_obj, vsd.py:79-90.
 *   verts     (V, 3) f32, all meshes concatenated (mm);  faces (F, 3) int32 indices into verts
 *   face_off, face_cnt  (P) int32: pose p draws faces [face_off[p], face_off[p] + face_cnt[p]); max_faces >= every face_cnt[p]
 *   poses     (P, 4, 4) f64 object-to-camera, OpenCV axes (x right, y down, z forward);  K (P, 3, 3) f64 (fx, fy, cx, cy are read)
 *   depth     (P, H, W) f32: camera-frame Z of the nearest surface at the image point (x + 0.5, y + 0.5), 1/Z interpolated in screen
 *             space; 0 where nothing is hit.  No face culling; deterministic.
 *   skipped   (P) uint32: triangles of each pose with a vertex at Z <= znear (not clipped: skipped; the caller reports a non-zero count)
 *   workspace nope_op_render_depth_workspace_bytes(P, max_faces) bytes.
 * Bad sizes, null pointers: NOPE_ERR_ARG; a short workspace: NOPE_ERR_WORKSPACE. */
size_t nope_op_render_depth_workspace_bytes(int P, int max_faces);
int nope_op_render_depth(const float* verts, int V, const int* faces, int F, const int* face_off, const int* face_cnt, int max_faces,
                         const double* poses, const double* K, int P, int H, int W, float* depth, uint32_t* skipped, void* workspace,
                         size_t workspace_bytes, nope_stream_t stream);

/* (ABI 9) Visible Surface Discrepancy of k estimated poses per query.  Replaces vsd_obj's per-pose loop, src/poses/vsd.py:91-132, with
 * depth_im_to_dist_im_fast, _estimate_visib_mask and estimate_visib_mask_gt / _est of src/poses/vsd_utils.py:41-134 (bop_toolkit).
 *   depth_test (B, H, W), depth_gt (B, H, W), depth_est (B, k, H, W) f32 in mm (0 = no depth);  K (B, 3, 3) f64;  1 <= k <= 16
 *   delta, tau  the misalignment / visibility tolerances (vsd.py:59-60: 15, 20);  cost_type NOPE_VSD_STEP | NOPE_VSD_TLINEAR;
 *   visib_mode  NOPE_VISIB_BOP19 | NOPE_VISIB_BOP18
 *   err        (B, k) f64: (cost + |union| - |intersection|) / |union|, 1.0 for an empty union
 * Arithmetic of the reference: distance images in f64 from integer pixel coordinates, the visibility test f32(d_model) - f32(d_test)
 * <= delta in f32, integer counts; the tlinear sum in a fixed order (the same bits on every run, not numpy's pairwise order).
 * Test and gt pixels are read once for all k.  workspace: nope_op_vsd_workspace_bytes(B, k, H, W) bytes. */
enum { NOPE_VSD_STEP = 0, NOPE_VSD_TLINEAR = 1 };
enum { NOPE_VISIB_BOP19 = 0, NOPE_VISIB_BOP18 = 1 };
size_t nope_op_vsd_workspace_bytes(int B, int k, int H, int W);
int nope_op_vsd(const float* depth_test, const float* depth_gt, const float* depth_est, const double* K, int B, int k, int H, int W,
                double delta, double tau, int cost_type, int visib_mode, double* err, void* workspace, size_t workspace_bytes,
                nope_stream_t stream);

/* (ABI 24) The BOP pose errors besides VSD: MSSD, MSPD, ADD and ADI (ADD-S) of P pose pairs.  No reference
 * counterpart: the reference reads models_info.json (dataloader/baseBOP.py:284) but evaluates VSD alone.  The definitions are those of
 * the BOP toolkit (pose_error.py: mssd, mspd, add, adi), restated here; they are the contract.
 *   verts     (V, 3) f32, all meshes concatenated (mm), as nope_op_render_depth takes them
 *   vert_off, vert_cnt  (P) int32 on the device: pose p reads the vertices x_i, i < V_p = vert_cnt[p], at vert_off[p] + i;
 *             max_verts (host) >= every vert_cnt[p]
 *   syms      (S_total, 4, 4) f64 row-major rigid transforms (R_s | t_s), the symmetry sets of all objects concatenated
 *   sym_off, sym_cnt    (P) int32 on the device: pose p uses the symmetries s < S_p = sym_cnt[p] at sym_off[p] + s (the identity is entry 0 of
 *             every set nope_amd.bop builds; the kernels do not rely on it);  max_syms (host) >= every sym_cnt[p]
 *   pose_est, pose_gt   (P, 4, 4) f64 object-to-camera (Re | te), (Rg | tg): OpenCV axes, mm;  K (P, 3, 3) f64
 *   mssd, mspd, add, adi  (P) f64 each, or NULL: a NULL output's metric is not computed (ADI is the expensive one)
 *   status    (P) int32: 0 or a sum of NOPE_POSE_ERR_* bits
 * With Xe_i = Re x_i + te and Xg_i^s = Rg (R_s x_i + t_s) + tg:
 *   ADD  = (1 / V_p) sum_i |Xe_i - (Rg x_i + tg)|
 *   ADI  = (1 / V_p) sum_i min_j |Xe_i - (Rg x_j + tg)|, searched in the ground truth's object frame: y_i = Rg^T (Xe_i - tg),
 *          min_j |y_i - x_j|  (Rg is taken to be a rotation)
 *   MSSD = min_s max_i |Xe_i - Xg_i^s|                                        (mm)
 *   MSPD = min_s max_i |pi(Xe_i) - pi(Xg_i^s)|, pi(X) = (K X)_{0,1} / (K X)_2 with the whole K, as the toolkit's project_pts    (pixels)
 * Arithmetic: f64 on the f32-stored vertices, no contraction, every 3-term dot product summed left to right; min / max are taken on
 * squared distances and sqrt once (sqrt is monotone and correctly rounded: the same bits).  The means are summed in a fixed order (per lane,
 * butterfly, waves, then blocks of NOPE_POSE_ERR_POINT_BLOCK vertices in order); no floating-point atomics: the same bits on every run.
 * Edge rules:
 *   a NaN or inf anywhere in pose_est[p], pose_gt[p] or K[p]: all outputs of p are NaN, NOPE_POSE_ERR_NONFINITE.  The maxima and minima keep
 *     a NaN of any operand (a NaN vertex gives NaN, not the maximum of the others)
 *   a vertex with (K X)_2 <= 0 under the estimate or under any symmetric ground truth: mspd[p] is NaN, NOPE_POSE_ERR_BEHIND; mssd, add,
 *     adi are unaffected
 *   vert_cnt[p] <= 0, > max_verts, or a range outside [0, V): all outputs of p are NaN, NOPE_POSE_ERR_VERT_RANGE; nothing is read
 *   sym_cnt[p] <= 0, > max_syms, or a range outside [0, S_total): the same with NOPE_POSE_ERR_SYM_RANGE
 *   all four outputs NULL, a missing input pointer, V, S_total, P, max_verts or max_syms < 1, P > 65535: NOPE_ERR_ARG; a short workspace:
 *     NOPE_ERR_WORKSPACE; both before anything is launched or written
 * workspace: nope_op_pose_errors_workspace_bytes(P, max_verts, max_syms) bytes. */
enum { NOPE_POSE_ERR_NONFINITE = 1, NOPE_POSE_ERR_BEHIND = 2, NOPE_POSE_ERR_VERT_RANGE = 4, NOPE_POSE_ERR_SYM_RANGE = 8 };
/* the sizes at which the kernels take another path (tests name their shapes from these) */
enum { NOPE_POSE_ERR_POINT_BLOCK = 512, /* vertices whose ADD / ADI terms one workgroup owns */
       NOPE_POSE_ERR_TILE = 1024,       /* vertices per LDS tile of the ADI / diameter search */
       NOPE_POSE_ERR_SYM_CHUNK = 8      /* symmetries one workgroup walks */ };
size_t nope_op_pose_errors_workspace_bytes(int P, int max_verts, int max_syms);
int nope_op_pose_errors(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* syms, int S_total,
                        const int* sym_off, const int* sym_cnt, int max_syms, const double* pose_est, const double* pose_gt, const double* K,
                        int P, double* mssd, double* mspd, double* add, double* adi, int* status, void* workspace, size_t workspace_bytes,
                        nope_stream_t stream);

/* (ABI 24) Diameter of n_obj objects: diameter[o] = max_{i,j} |x_i - x_j| over the vertex range of object o, f64 on the f32 vertices, the
 * ADI tiling with a maximum over the block pairs i <= j; bit-identical from run to run.  An empty or bad range gives NaN (nothing is read),
 * a NaN vertex gives NaN.  n_obj <= 65535.  workspace: nope_op_mesh_diameter_workspace_bytes(n_obj, max_verts) bytes. */
size_t nope_op_mesh_diameter_workspace_bytes(int n_obj, int max_verts);
int nope_op_mesh_diameter(const float* verts, int V, const int* vert_off, const int* vert_cnt, int n_obj, int max_verts, double* diameter,
                          void* workspace, size_t workspace_bytes, nope_stream_t stream);

/* (ABI 25) Translation of P poses from a rotation, the model and a 2D box: the t under which the projected box of the model's vertices is
 * the given one.  No reference counterpart: the reference predicts no translation (src/poses/vsd.py:84-87 takes the
 * ground truth's).
 *   verts, V, vert_off, vert_cnt, max_verts   as nope_op_pose_errors takes them: pose p reads x_i, i < V_p
 *   R         (P, 3, 3) f64 row-major;  K (P, 3, 3) f64: fx = K[0], cx = K[2], fy = K[4], cy = K[5] are read, as nope_op_render_depth reads them
 *   box       (P, 4) f64 (u0, v0, u1, v1) in pixels, the rasteriser's image coordinates: image point u falls in pixel floor(u)
 *   max_iters >= 0;  tol_scale, tol_px >= 0
 *   t (P, 3) f64, residual (P) f64 (pixels), iters (P) int32, status (P) int32: 0 or a sum of NOPE_FIT_* bits
 * The contract is this sequence of f64 operations on the f32-stored vertices, without contraction, every 3-term product summed left to
 * right; min / max run over the V_p vertices and keep a NaN of any operand:
 *   y_i = R x_i = ((R[3r] x + R[3r+1] y) + R[3r+2] z)_r;   bw = u1 - u0, bh = v1 - v0, cu = 0.5 (u0 + u1), cv = 0.5 (v0 + v1)
 *   ax0 / ax1 = min / max y_i.x,  ay0 / ay1 = min / max y_i.y
 *   z = 0.5 ((fx (ax1 - ax0)) / bw + (fy (ay1 - ay0)) / bh)
 *   t = (((cu - cx) / fx) z - 0.5 (ax0 + ax1), ((cv - cy) / fy) z - 0.5 (ay0 + ay1), z);  n = 0
 *   loop:
 *     Z_i = y_i.z + t_z;  if not (min Z_i > 0): NOPE_FIT_BEHIND, t and residual NaN, iters = n, stop
 *     u_i = fx ((y_i.x + t_x) / Z_i) + cx,  v_i = fy ((y_i.y + t_y) / Z_i) + cy;  pu0 / pu1 = min / max u_i,  pv0 / pv1 = min / max v_i
 *     s = 0.5 ((pu1 - pu0) / bw + (pv1 - pv0) / bh);  du = cu - 0.5 (pu0 + pu1);  dv = cv - 0.5 (pv0 + pv1)
 *     residual = max(max(max(|pu0 - u0|, |pu1 - u1|), |pv0 - v0|), |pv1 - v1|)
 *     if |s - 1| <= tol_scale and |du| <= tol_px and |dv| <= tol_px: iters = n, stop (status 0)
 *     if n == max_iters: NOPE_FIT_NOT_CONVERGED, t and residual as they stand, iters = n, stop
 *     z' = t_z s;  t = (t_x s + (du z') / fx, t_y s + (dv z') / fy, z');  n = n + 1
 * max_iters = 0 returns the initial guess and its residual.  Minima and maxima do not depend on the order they are taken in and nothing is
 * summed over the vertices: the same bits on every run and from any reduction tree (the one freedom is the sign of an extreme that is
 * zero, which reaches an output only where both extremes of an axis are zero).  One workgroup of NOPE_FIT_THREADS lanes per pose; the
 * vertices are read and rotated again in every pass.
 * Edge rules:
 *   a NaN or inf in R[p], K[p] or box[p]: t, residual NaN, iters 0, NOPE_FIT_NONFINITE
 *   a finite box with not (bw > 0) or not (bh > 0): the same with NOPE_FIT_BAD_BOX
 *   vert_cnt[p] <= 0, > max_verts, or a range outside [0, V): the same with NOPE_FIT_VERT_RANGE; nothing is read
 *   a NaN vertex: it stays in the extremes, z and Z_i are NaN, so the first pass stops at its test with NaN outputs (and NOPE_FIT_BEHIND)
 *   a missing pointer, V, P or max_verts < 1, max_iters < 0, a negative or NaN tolerance: NOPE_ERR_ARG before anything is launched or written */
enum { NOPE_FIT_NONFINITE = 1, NOPE_FIT_BAD_BOX = 2, NOPE_FIT_VERT_RANGE = 4, NOPE_FIT_BEHIND = 8, NOPE_FIT_NOT_CONVERGED = 16 };
enum { NOPE_FIT_THREADS = 256 /* lanes per pose: vertex i is lane i mod NOPE_FIT_THREADS's (tests name their shapes from it) */ };
int nope_op_fit_translation(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* R, const double* K,
                            const double* box, int P, int max_iters, double tol_scale, double tol_px, double* t, double* residual, int* iters,
                            int* status, nope_stream_t stream);

/* (ABI 25) Boxes of B masks, in the coordinates nope_op_fit_translation takes: with xmin .. xmax, ymin .. ymax the extreme non-zero pixels of
 * mask[b], box[b] = (xmin, ymin, xmax + 1, ymax + 1) and count[b] the number of non-zero pixels; an empty mask: a NaN box and count 0.
 *   mask (B, H, W) uint8;  box (B, 4) f64;  count (B) int32.  Integer min / max and an integer count, one workgroup per image.
 * A missing pointer, B, H or W < 1, H W > 2^30: NOPE_ERR_ARG. */
int nope_op_mask_boxes(const unsigned char* mask, int B, int H, int W, double* box, int* count, nope_stream_t stream);

/* (ABI 25) Mean depth difference between a test image and k rendered estimates over their inliers: the correction of an estimate's distance.
 *   depth_test (B, H, W) f32, depth_est (B, k, H, W) f32 in mm (0 = no depth), mask (B, H, W) uint8 or NULL;  tau >= 0 (mm);  1 <= k <= 16
 *   a pixel is an inlier of estimate j when test > 0, est > 0, mask != 0 (if given) and |f64(test) - f64(est)| <= tau; a NaN compares false
 *   count (B, k) int32 inliers;  shift (B, k) f64 = (sum over the inliers of f64(test) - f64(est)) / count, NaN where count = 0
 * The sum's order is fixed: with nblk = the workgroups per image (a function of H W alone), lane l of workgroup w adds pixels
 * (w + j nblk) 256 + l, j = 0, 1, ..., in that order; then the butterfly over the wave (xor 32, 16, ..., 1), the four waves left to right,
 * the workgroups in order.  No floating-point atomics: the same bits on every run.
 * A missing pointer, B, H or W < 1, B > 65535, H W > 2^30, k outside 1 .. 16, a negative or NaN tau: NOPE_ERR_ARG; a short workspace:
 * NOPE_ERR_WORKSPACE; both before anything is launched or written.  workspace: nope_op_depth_shift_workspace_bytes(B, k, H, W) bytes. */
size_t nope_op_depth_shift_workspace_bytes(int B, int k, int H, int W);
int nope_op_depth_shift(const float* depth_test, const float* depth_est, const unsigned char* mask, int B, int k, int H, int W, double tau,
                        double* shift, int* count, void* workspace, size_t workspace_bytes, nope_stream_t stream);

/* (ABI 12) Visualisation pictures: the contact sheets PoseConditional saves as PNGs and the `vis_imgs` grid of its predictions file.
 * A picture is n_cols (1 .. NOPE_VIS_MAX_COLS) columns; a column is one stack of f32 NCHW images, read where it lies -- nothing is copied
 * or repeated on the host.  `cols` is a HOST array (it travels as kernel arguments); the pointers inside it are device pointers. */
enum { NOPE_VIS_MAX_COLS = 8 };
enum { NOPE_VIS_UNNORMALIZE = 1, /* (x + 1) * 0.5 first, in f32 */
       NOPE_VIS_CLAMP = 2        /* then clamp to [0, 1]; both = unnormalize_to_zero_to_one, src/model/utils.py:12-15 */ };
typedef struct {
    const float* data;      /* (..., 3, H, W) f32 planes: sample b of frame f at data + b * stride_b + f * stride_f */
    int64_t stride_b;       /* elements between samples b */
    int64_t stride_f;       /* elements between frames f; 0 = the same images in every frame */
    const int64_t* index;   /* NULL, or device indices: sample b of every frame reads frame index[b * index_stride]
                               (gt_templates[b, nearest_idx[b, 0]], src/model/model.py:331-333) */
    int64_t index_stride;
    int64_t index_limit;    /* indices are clamped into [0, index_limit) on the device: a bad index never reads out of bounds */
    int flags;              /* NOPE_VIS_UNNORMALIZE | NOPE_VIS_CLAMP */
} nope_vis_column;

/* The full-size f16 grid with its margin column.  Replaces put_image_to_grid(list_imgs, adding_margin=True),
 * src/utils/visualization_utils.py:43-57 (and the unnormalize_to_zero_to_one calls on its inputs, src/model/model.py:215-218,292-296,
 * 334-338), for F pictures in one launch.
 *   grid_f16  (F, B * (n_cols + 1), 3, H, W) f16: image b * (n_cols + 1) + i is column i of sample b, image b * (n_cols + 1) + n_cols is
 *             zero.  The flags run in f32, then ONE round-to-nearest-even cast to f16.
 * 1 <= n_cols <= 8; B, H, W > 0; B * (n_cols + 1) <= 65535; 0 <= F <= 65535, F = 0 is a no-op that succeeds; non-null pointers when F > 0;
 * index_limit >= 1 wherever index is set: otherwise NOPE_ERR_ARG, and nothing is launched. */
int nope_op_vis_grid(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, void* grid_f16, nope_stream_t stream);

/* The bytes of the PNG.  Replaces, per picture, put_image_to_grid + clone + F.interpolate(grid, (tile, tile), mode="bilinear",
 * align_corners=False) + torchvision.utils.save_image(grid, path, nrow=nrow) up to the file encoder (src/model/model.py:231-240,297-306,
 * 339-348; the reference: tile 64, nrow 4 * (n_cols + 1), padding 2), for F pictures in one launch; frames are independent.
 *   sheet_u8  (F, Hs, Ws, 3) u8, HWC, any byte alignment.  n_img = B * (n_cols + 1), xmaps = min(nrow, n_img), ymaps = ceil(n_img / xmaps),
 *             Hs = (tile + padding) * ymaps + padding, Ws = (tile + padding) * xmaps + padding (make_grid); image k has its corner at
 *             ((k / xmaps) * (tile + padding) + padding, (k % xmaps) * (tile + padding) + padding); padding, margin images and the empty
 *             slots of a ragged last row are 0.
 * Per byte, in the arithmetic the reference's f16 grid goes through: column flags in f32 -> f16; bilinear resample (scale = (float)H / tile,
 * src = max(scale * (o + 0.5f) - 0.5f, 0), i0 = min((int)src, H - 1), i1 = min(i0 + 1, H - 1), l1 = src - i0, l0 = 1 - l1; H and W
 * independently) as l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d) in f32 on the four f16 taps -> f16; save_image's
 * mul(255).add_(0.5).clamp_(0, 255).to(uint8) with an f16 rounding after the product and after the sum.
 * Checks as nope_op_vis_grid (n_img is not limited to 65535 here), and tile, nrow > 0, padding >= 0, Hs <= 65535. */
int nope_op_vis_sheet(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, int tile, int nrow, int padding,
                      void* sheet_u8, nope_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pose-conditioned U-Net.  Replaces UNet.__init__/forward,
 * src/model/u_net/denoising_diffusion_pytorch/u_net.py:27-198 and the blocks of
 * model_utils.py:161-172,198-279,367-418.
 */
typedef struct nope_unet nope_unet;

typedef struct {
    const char* name;      /* host: reference state-dict key, e.g. "downs.0.0.block1.proj.weight" */
    const float* data;     /* device: f32, contiguous, torch layout (Conv2d: [Cout,Cin,kh,kw]) */
    int ndim;
    int64_t shape[4];
} nope_tensor_desc;

typedef struct {
    int u_net_dim;         /* 192  (configs/model/template_base.yaml:4) */
    int channels;          /* encoder.latent_dim, 8 (u_net.py:45) */
    int out_dim;           /* = channels (u_net.py:50) */
    int pose_dim;          /* rot_representation_dim, 6 */
    int n_levels;          /* len(dim_mults) = 4 */
    int dim_mults[8];      /* (1,2,4,8) */
    int groups;            /* resnet_block_groups = 8 */
    int heads, dim_head;   /* 4, 32 (model_utils.py:368,394) */
    int pose_mlp_layers;   /* 1 = "single_layer", 2 = "two_layers" (u_net.py:63-72) */
    int compute_dtype;     /* NOPE_F32: f32 storage + f32-input MFMA (bit-faithful fp32 sums);
                              NOPE_BF16 / NOPE_F16: 16-bit storage + 16-bit MFMA, f32 accumulate / statistics;
                              NOPE_BF16X3 / NOPE_F16X2: f32 storage, split-precision MFMA (see the enum) */
    int soft_up_down;      /* 0: use_hard_up_down = True, the shipped configuration (HardDownsample / HardUpsample, u_net.py:54-56);
                              1: use_hard_up_down = False -- Downsample = Conv2d(4, stride 2, pad 1) at "downs.l.3.weight",
                              Upsample = ConvTranspose2d(4, stride 2, pad 1) at "ups.l.3.weight" (model_utils.py:119-136) */
} nope_unet_config;

/* Validates and repacks the reference state dict for the device (the only allocating call). */
int nope_unet_create(const nope_unet_config* cfg, const nope_tensor_desc* tensors, int n_tensors,
                     nope_stream_t stream, nope_unet** out);
void nope_unet_destroy(nope_unet* net);

size_t nope_unet_workspace_bytes(const nope_unet* net, int n_hyp, int n_src, int H, int W);

/* out[j] = UNet(x[j / x_rep], pose[j])  for j in [0, n_hyp).
 *   x     (n_src, channels, H, W) f32 NCHW, n_src * x_rep == n_hyp.  x_rep = 1 is
 *         UNet.forward(x, pose) (u_net.py:160); x_rep = N evaluates N pose hypotheses per
 *         reference embedding, the batched form of the template loop (model.py:212-222).
 *   pose  (n_hyp, pose_dim) f32
 *   out   (n_hyp, out_dim, H, W) NCHW of `out_dtype` -- i.e. directly a slice of the
 *         (B,N,C,h,w) template bank.
 * H and W must be divisible by 2^(n_levels-1). */
int nope_unet_forward(const nope_unet* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp,
                      int H, int W, void* out, int out_dtype, void* workspace, size_t workspace_bytes,
                      nope_stream_t stream);

/* hipGraph replay of SMALL forwards, opt-in (no reference counterpart): with max_hyp_pixels > 0, forwards of at most that many
 * n_hyp * H * W replay a captured launch sequence (x, pose and the output are staged through the head of the workspace so the
 * caller's pointers stay out of the graph; one graph per (workspace, shape, out_dtype), cache guarded by a mutex).  0 (the default;
 * NOPE_UNET_GRAPH in the environment at create time overrides) = always launch directly.  Results are bit-identical either way
 * (tests/test_gpu_configs.py::test_unet_graph_replay_matches_direct); a 64-hypothesis pass measured +-0 on MI355X, which is why it is
 * off.  nope_unet_graph_replays: forwards served by a replay since create. */
int nope_unet_graph_limit(nope_unet* net, long long max_hyp_pixels);

/* NOPE_F16X2 activation ranges (no reference counterpart: the reference computes in fp32, model_utils.py:240-252,271-279 see whatever
 * magnitude the residual stream has).  Every nope_unet_forward of a NOPE_F16X2 net ends with a verdict formed ON THE DEVICE: the largest
 * |activation| each two-pass layer read (recorded by the producers of its inputs) against the layer's window.  A forward with a layer outside
 * its window leaves NaNs in `out` -- inaccurate values never pass for accurate ones -- and no host synchronisation is involved.
 *   nope_unet_x2_poll         reads, WITHOUT synchronising, the verdicts that have reached the host since the previous poll, re-centres the
 *                             shifts of the layers that were out of (or within two binades of an end of) their windows -- the new shifts are
 *                             enqueued on `stream` -- and returns NOPE_OK, NOPE_ERR_RANGE (a judged forward was out of range: its output is
 *                             NaN, issue it again) or NOPE_ERR_RANGE_F16 (an activation was infinite: no shift helps; nope_unet_x2_enable(net, 0)
 *                             makes every launch NOPE_BF16X3 -- same weights, the three-pass kernels).  nope_unet_forward polls at entry.
 *   nope_unet_x2_range_check  synchronises `stream` first: the verdict of every forward issued on it so far.
 * n_out_of_range / n_adjusted / max_abs (each may be null): layers out of range in the judged forwards, layers whose shift moved, largest
 * |a| seen.  A net created in another mode: NOPE_OK, nothing to check.  nope_unet_x2_shifts: the current per-layer shifts (creation order). */
int nope_unet_x2_poll(nope_unet* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_unet_x2_range_check(nope_unet* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_unet_x2_enable(nope_unet* net, int on);
int nope_unet_x2_shifts(const nope_unet* net, int* shifts, int max, int* n);
int nope_unet_graph_replays(const nope_unet* net);

/* Measurement aid (bench.py roofline leg, no reference counterpart): while enabled, every
 * launch of the implicit-GEMM conv kernel made by nope_unet_forward is bracketed by HIP events on
 * the caller's stream; _read synchronises them and returns the launch count, the summed kernel
 * time, the summed executed flops (2*M*Cout*taps*Cin) and the summed algorithmic HBM bytes (each input,
 * weight and output element once).  Adds two event records per launch:
 * keep it off in timed regions. */
int nope_unet_profile(nope_unet* net, int enable);
int nope_unet_profile_read(nope_unet* net, int* n_launches, double* total_ms, double* total_flops, double* total_bytes);
/* ... and launch by launch, in issue order: which kernel took the launch, its shape, its HIP-event time.  `flops` counts the
 * convolution's multiply-adds x 2 as executed (NOPE_BF16X3 issues three MFMA passes per product: mfma_passes = 3).  Writes at
 * most `max` records and the total number of recorded launches to *n. */
enum { NOPE_CONV_KERNEL_GENERIC = 0, NOPE_CONV_KERNEL_DMA128 = 1, NOPE_CONV_KERNEL_PP256 = 2, NOPE_CONV_KERNEL_HALO256 = 3, NOPE_CONV_KERNEL_SMALL = 4, NOPE_CONV_KERNEL_STREAM = 5 };
typedef struct {
    double ms, flops, bytes;
    int kernel;            /* NOPE_CONV_KERNEL_* */
    int mode, ntaps, Cin, Cout, Hs, Ws, n_hyp, mfma_passes, posmajor;
} nope_conv_launch_info;
int nope_unet_profile_launches(nope_unet* net, nope_conv_launch_info* out, int max, int* n);

/* ------------------------------------------------------------------------------------------
 * LDM cross-attention U-Net variant.  Replaces UNetModelPose.__init__/forward,
 * src/model/u_net/ldm/adapt_openaimodel.py:14-158 (over UNetModel, ldm/openaimodel.py:428-760; ResBlock :177-288, Downsample /
 * Upsample :93-174; SpatialTransformer / BasicTransformerBlock / CrossAttention / GEGLU, ldm/attention.py:37-277): the variant
 * whose pose conditioning is cross-attention against context = pose_mlp(pose).  Tensor names are UNetModelPose's own
 * state-dict keys ("input_blocks.1.1.transformer_blocks.0.attn2.to_v.weight", "middle_block.0.in_layers.2.weight", ...).
 * Supported: use_spatial_transformer = true with transformer_depth >= 1 and attention heads 32, 64 or 128 channels wide, per level
 * (num_head_channels / num_heads, openaimodel.py:560-580; the shipped configs/model/vae_cin_ldm.yaml has 32 everywhere), conv_resample on
 * or off (Downsample / Upsample with or without their conv, :94-175), resblock_updown on or off (ResBlocks with up / down, :177-288),
 * ResBlocks with or without use_scale_shift_norm (FiLM, openaimodel.py:277-281); pose_mlp "single_layer" / "two_layers";
 * injecting_condition_twice on or off. */
typedef struct nope_ldm nope_ldm;
typedef struct {
    int in_channels;        /* 4 in vae_cin_ldm.yaml (any count: the input conv's K axis is zero-padded to a multiple of 8 at pack time) */
    int model_channels;     /* 256 */
    int out_channels;       /* 4 */
    int num_res_blocks;     /* 2 */
    int n_levels;           /* len(channel_mult) = 3 */
    int channel_mult[8];    /* (1,2,4) */
    int attn_levels[8];     /* 1 where the level's downsampling factor is in attention_resolutions: (1,1,1) */
    int num_head_channels;  /* 32; 0 = per level, from head_channels (ABI 7) */
    int context_dim;        /* 512 */
    int pose_dim;           /* rot_representation_dim, 6 */
    int pose_mlp_layers;    /* 1 = "single_layer", 2 = "two_layers" */
    int injecting_condition_twice;   /* 0: timestep embedding is zeros; 1: emb = pose_mlp_timesteps(pose) */
    int compute_dtype;      /* NOPE_F32 | NOPE_BF16 | NOPE_F16 | NOPE_BF16X3 | NOPE_F16X2 (= NOPE_BF16X3 here: its layers carry no second weight pack), as nope_unet_config */
    int use_scale_shift_norm;        /* 1: ResBlocks apply out_norm(h) * (1 + scale) + shift with (scale, shift) = emb_layers(emb) */
    int transformer_depth;           /* BasicTransformerBlocks per SpatialTransformer (attention.py:232-262); 1 in vae_cin_ldm.yaml; 0 reads as 1 */
    int head_channels[8];   /* (ABI 7) attention head width of each level's SpatialTransformers, 32 / 64 / 128, heads * head_channels = the level's
                             * channels; the middle block uses the last level's.  Read when num_head_channels = 0 (else every level has num_head_channels) */
    int resblock_updown;    /* (ABI 7) 1: the resampling slots are ResBlocks with down / up (avg_pool 2x2 / nearest x2 on h and x, openaimodel.py:177-288) */
    int conv_resample;      /* (ABI 7) 1 (vae_cin_ldm.yaml): Downsample = conv 3x3 stride 2, Upsample = nearest x2 + conv 3x3; 0: avg_pool 2x2 / nearest x2
                             * alone (:94-175).  Ignored under resblock_updown */
} nope_ldm_config;

int nope_ldm_create(const nope_ldm_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_ldm** out);
void nope_ldm_destroy(nope_ldm* net);
size_t nope_ldm_workspace_bytes(const nope_ldm* net, int n_hyp, int n_src, int H, int W);
/* out[j] = UNetModelPose(x[j / x_rep], pose[j]); arguments as nope_unet_forward. */
int nope_ldm_forward(const nope_ldm* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp, int H, int W,
                     void* out, int out_dtype, void* workspace, size_t workspace_bytes, nope_stream_t stream);
/* NOPE_F16X2 in the LDM variant: the 3x3 convolutions (ResBlock in_layers.2 / out_layers.3, openaimodel.py:205-243, and the nearest-x2
 * up-sampling convs :95-118) on the two-pass tile, everything else as NOPE_BF16X3; activation ranges exactly as nope_unet_x2_poll /
 * nope_unet_x2_range_check / nope_unet_x2_enable above (device-side verdict, NaN output for an out-of-range forward, poll at every forward). */
int nope_ldm_x2_poll(nope_ldm* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_ldm_x2_range_check(nope_ldm* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_ldm_x2_enable(nope_ldm* net, int on);

/* ------------------------------------------------------------------------------------------
 * (ABI 10) Guided-diffusion U-Net variant.  Replaces UNetModelPose.__init__/forward, src/model/u_net/guided_diffusion/adapt_u_net.py:13-97
 * (over UNetModel, guided_diffusion/u_net.py:389-; ResBlock :141-253, AttentionBlock :255-300, QKVAttentionLegacy / QKVAttention
 * :323-386, Downsample / Upsample :78-138): the variant whose pose conditioning is emb = pose_mlp(pose) in place of the timestep
 * embedding, read by every ResBlock's emb_layers.  The reference's forward calls module(h, emb, emb), which TimestepEmbedSequential
 * does not accept; this runs the one reading that type-checks, module(h, emb).  Tensor names are UNetModelPose's own state-dict keys
 * ("input_blocks.4.1.qkv.weight" [3C][C][1], "middle_block.1.proj_out.weight" [C][C][1], "output_blocks.2.2.in_layers.2.weight", ...);
 * time_embed.* is never read.  AttentionBlock = GroupNorm(32) -> qkv 1x1 -> softmax attention over the H*W tokens of a sample
 * (nope_op_token_attention: heads 32 / 64 / 128 channels wide; the legacy (head, q|k|v, ch) rows of qkv are permuted to [q | k | v] at
 * create time) -> proj_out 1x1 + x.  Supported: conv_resample, resblock_updown and use_scale_shift_norm on or off; pose_mlp
 * "single_layer" / "two_layers" / "posEncoding". */
typedef struct nope_gd nope_gd;
enum { NOPE_GD_POSE_SINGLE = 1, NOPE_GD_POSE_TWO_LAYERS = 2, NOPE_GD_POSE_ENCODING = 3 };
typedef struct {
    int in_channels;        /* 4 in vae_guidedDiffusion.yaml (any count: the input conv's K axis is zero-padded to a multiple of 8) */
    int model_channels;     /* 256; a multiple of 32 */
    int out_channels;       /* 4 */
    int num_res_blocks;     /* 2 */
    int n_levels;           /* len(channel_mult) = 6 */
    int channel_mult[8];    /* (1,1,2,2,4,4) */
    int attn_levels[8];     /* 1 where the level's downsampling factor is in attention_resolutions: (0,0,0,1,1,1) */
    int head_channels_in[8];   /* head width of level l's input-side AttentionBlocks (num_heads / num_head_channels, u_net.py:444-445, 474-482) */
    int head_channels_out[8];  /* ... of its output-side ones (num_heads_upsample, :580) */
    int head_channels_mid;     /* ... of the middle block's (num_heads at the last level's channels) */
    int pose_dim;           /* rot_representation_dim, 6 */
    int pose_mlp;           /* NOPE_GD_POSE_*: Linear; Linear, GELU (erf), Linear; SinusoidalPosEmb(emb / 6) (pose_dim 6) */
    int new_attention_order;   /* 0: QKVAttentionLegacy, qkv rows (head, q|k|v, ch); 1: QKVAttention, rows (q|k|v, head, ch) */
    int resblock_updown;    /* 1 (the yaml): the resampling slots are ResBlocks with down / up (avg_pool 2x2 / nearest x2 on h and x) */
    int conv_resample;      /* 1: Downsample = conv 3x3 stride 2, Upsample = nearest x2 + conv 3x3; 0: avg_pool 2x2 / nearest x2 alone. Ignored under resblock_updown */
    int use_scale_shift_norm;  /* 1 (the yaml): ResBlocks apply out_norm(h) * (1 + scale) + shift with (scale, shift) = emb_layers(emb) */
    int compute_dtype;      /* NOPE_F32 | NOPE_BF16 | NOPE_F16 | NOPE_BF16X3 | NOPE_F16X2, as nope_ldm_config */
} nope_gd_config;

int nope_gd_create(const nope_gd_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_gd** out);
void nope_gd_destroy(nope_gd* net);
size_t nope_gd_workspace_bytes(const nope_gd* net, int n_hyp, int n_src, int H, int W);
/* out[j] = UNetModelPose(x[j / x_rep], pose[j]); arguments as nope_ldm_forward; H and W multiples of 2^(n_levels - 1). */
int nope_gd_forward(const nope_gd* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp, int H, int W,
                    void* out, int out_dtype, void* workspace, size_t workspace_bytes, nope_stream_t stream);
/* NOPE_F16X2: the 3x3 convolutions on the two-pass tile, everything else as NOPE_BF16X3; activation ranges as nope_ldm_x2_*. */
int nope_gd_x2_poll(nope_gd* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_gd_x2_range_check(nope_gd* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs);
int nope_gd_x2_enable(nope_gd* net, int on);

/* ------------------------------------------------------------------------------------------
 * Template encoder.  Replaces FeatureExtractor.encode_image, src/model/encoder/template.py:47-53
 * (ResNet-50 trunk src/model/encoder/resnet.py:92-152 with eval-mode BatchNorm, then the
 * ReLU/1x1/ReLU/1x1 projector template.py:33-38).  Tensor names are the FeatureExtractor's own
 * state-dict keys ("backbone.conv1.weight", "backbone.layer1.0.bn1.running_mean", "projector.1.weight", ...).
 */
typedef struct nope_encoder nope_encoder;
typedef struct {
    int descriptor_size;   /* 8 (configs/model/template_base.yaml:10) */
    int compute_dtype;     /* NOPE_F32 | NOPE_BF16 | NOPE_F16 | NOPE_BF16X3 | NOPE_F16X2 (its 3x3 convs on the two-pass tile, the rest as NOPE_BF16X3), as nope_unet_config */
    float bn_eps;          /* BatchNorm2d eps; <= 0 selects the torch default 1e-5 */
} nope_encoder_config;

int nope_encoder_create(const nope_encoder_config* cfg, const nope_tensor_desc* tensors, int n_tensors,
                        nope_stream_t stream, nope_encoder** out);
void nope_encoder_destroy(nope_encoder* enc);
size_t nope_encoder_workspace_bytes(const nope_encoder* enc, int n_img, int H, int W);
/* image (n_img, 3, H, W) f32 NCHW in [-1, 1], H and W multiples of 8 -> out (n_img, descriptor_size, H/8, W/8) f32 NCHW.
 * The launch sequence of a pass (~85 small kernels) is captured into a hipGraph the first time a
 * (workspace, n_img, H, W) combination is seen and replayed afterwards (image / out are staged through the
 * workspace, so they may change from call to call); if stream capture is unavailable the kernels are launched
 * directly.  The graph cache lives in the handle: calls on ONE handle must come from one host thread at a time,
 * and concurrent passes on different streams need different workspaces. */
int nope_encoder_forward(const nope_encoder* enc, const float* image, int n_img, int H, int W, float* out,
                         void* workspace, size_t workspace_bytes, nope_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (NHWC activations of `dtype`), exported so that each block of
 * model_utils.py can be parity-tested in isolation.  Weights for nope_op_conv are packed
 * [Cout][ntaps][Cin] by nope_op_pack_conv_weight.
 */
int nope_op_nchw_to_nhwc(int dtype, const float* x_nchw, void* y_nhwc, int n, int C, int HW, nope_stream_t s);
int nope_op_nhwc_to_nchw(int dtype, const void* x_nhwc, float* y_nchw, int n, int C, int HW, nope_stream_t s);
int nope_op_pack_conv_weight(int dtype, const float* w, void* packed, int Cout, int Cin, int ntaps, int mode,
                             nope_stream_t s);
/* RANGE SLOTS (nope_conv_op, nope_gn_op, nope_op_absmax_f32).  `amax_slot` is a scratch of nope_op_amax_slot_words() 32-bit words (the
 * entries clear it), `amax_out` one device float that receives max |.| of what the launch wrote, folded from the slot; both NULL = no
 * request, one without the other is NOPE_ERR_ARG. */
int nope_op_amax_slot_words(void);
/* conv3x3(pad1) / conv1x1 / nearest-x2+conv3x3 (HardUpsample, model_utils.py:161-165) /
 * space-to-depth+conv1x1 (HardDownsample, :168-172) / stride-2 conv (encoder) over a virtual channel concat
 * (torch.cat((x, skip), dim=1), u_net.py:186,189,194) as one implicit GEMM, with the fusion plumbing the network runtimes launch around it
 * (no reference counterpart: the reference runs Conv2d, GroupNorm and PreNorm as separate torch ops, model_utils.py:226-252).  The entry
 * returns whatever the launcher returns: a combination the launcher refuses is refused here.
 * Arguments by name: zero-initialise, set struct_size, fill in what the launch has.  A zero / NULL optional field means "absent". */
typedef struct nope_conv_op {
    uint32_t struct_size; int dtype;      /* struct_size: sizeof(nope_conv_op); anything else is NOPE_ERR_ARG before another field is read */
    const void* src1; int C1; int rep1;      /* NHWC, C1 channels, shared by rep1 consecutive hypotheses (0 reads as 1) */
    const void* src2; int C2; int rep2;      /* the second half of the virtual concat, or NULL with C2 = 0; rep2 as rep1 */
    int Hs, Ws;                /* source map; NOPE_CONV_DOWN2 / _STRIDE2 / _STRIDE2_PAD01 need both even (NOPE_ERR_ARG) */
    int mode, ntaps;           /* NOPE_CONV_* */
    const void* w_packed;      /* nope_op_pack_conv_weight's */
    const float* bias;         /* [Cout] or NULL */
    const void* resid;         /* NHWC of the output's shape, added after the bias, or NULL */
    void* out; int Cout, n_hyp;
    int out_nchw, out_dtype;   /* 1: NCHW output of element type out_dtype; 0: NHWC of dtype's storage type */
    int act_relu;              /* 1: ReLU after bias and residual */
    void* splitk_ws; size_t splitk_bytes;      /* scratch for a deterministic split-K launch (f32 partials + fixed-order reduce) when the launcher wants one
                                * for the shape: nope_op_conv_query says how many bytes it would use; a smaller or NULL scratch = no split */
    float* colstats; int stat_rows;      /* [M / stat_rows][Cout][2] f32 (sum, sum of squares) of the f32 results (accumulator + bias) per block of stat_rows
                                * output rows, or NULL; stat_rows must be nope_op_conv_query's answer (NOPE_ERR_ARG otherwise, and for a shape whose kernel
                                * has no such form) */
    const float* pn_ms; const float* pn_c0; const float* pn_c1;      /* pn_ms [n_hyp][2] (mean, rstd), pn_c0 / pn_c1 [Cout]: fused PreNorm of a 1x1
                                * NOPE_CONV_PLAIN conv whose packed weights carry gamma, out[m, n] = rstd[b] (acc[m, n] - mean[b] c1[n]) + c0[n] + bias[n],
                                * c0 = W beta, c1 = the row sums of the packed W gamma; or NULL */
    /* The GroupNorm tail (gn_gamma set): the end of a ResnetBlock with a res_conv as the U-Net runtime launches it in the split-precision modes,
     *     out[m, n] = conv1x1(src1 [cat src2])[m, n] + bias[n] + SiLU(GroupNorm(gn_G)(resid)[m, n] gn_gamma[n] + gn_beta[n]),
     *   in two launches: (mean, rstd) [n_hyp][gn_G][2] of resid from its producer's column statistics tail_colstats
     *   [n_hyp][tail_stat_blocks][Cout][2] (rows of 64; `colstats` of the launch that wrote resid) into gn_ms, then the conv, whose epilogue
     *   normalises and activates each residual vector on its way in.  Same arithmetic as nope_op_group_norm (fast_silu = 1, that colstats,
     *   act_silu = 1) with the conv's output as ITS residual: bit-identical.  resid may be `out` (in place).  NOPE_BF16X3 / NOPE_F16X2 only, and
     *   only a launch the policy in force puts on the per-tap ping-pong kernel with the lean epilogue, H W a multiple of 64, (Cout / gn_G) a
     *   multiple of 4, at most 64 tail_stats entries per hypothesis: NOPE_ERR_UNSUPPORTED otherwise -- never a launch without the tail, and
     *   nothing is launched for a refused combination.  gn_ms or tail_colstats missing: NOPE_ERR_ARG. */
    const float* tail_colstats; int tail_stat_blocks;
    const float* gn_gamma; const float* gn_beta; int gn_G; float gn_eps; float* gn_ms;
    float* tail_stats;         /* [n_hyp][nope_conv_op_info.tail_stat_blocks][2] or NULL: (sum, sum of squares) of the values written per 64-row x
                                * 96-column tile, for nope_op_gn_finalize */
    uint32_t* amax_slot; float* amax_out;      /* RANGE SLOTS above */
    /* The conv's OWN GroupNorm (gn_self = 1, with gn_gamma / gn_beta / gn_G / gn_eps; gn_ms, tail_colstats, tail_stats, colstats, the PreNorm and
     *   act_relu unset): a ResnetBlock's conv3x3 -> GroupNorm -> SiLU [-> + emb] [-> + x] in ONE launch,
     *     out[m, n] = SiLU(GroupNorm(gn_G)(conv3x3(src1 [cat src2]) + bias)[m, n] gn_gamma[n] + gn_beta[n]) [+ gn_emb[sample of m][n]] [+ resid[m, n]],
     *   the statistics formed inside the launch by the workgroup that owns the samples.  `resid` is added LAST here.  Same column sums, fold order
     *   and arithmetic as the conv with `colstats` followed by nope_op_group_norm (fast_silu = 1, act_silu = 1, that colstats, emb, resid):
     *   bit-identical to those two launches.  NOPE_BF16X3 / NOPE_F16X2 only, and only a launch the policy in force puts on the tap-resident 3x3
     *   kernel with the lean epilogue and no split-K, H W in {16, 64, 256}, n_hyp H W a multiple of 256, (Cout / gn_G) a multiple of 4 that divides
     *   192, gn_resid_rep 0 or 1: NOPE_ERR_UNSUPPORTED otherwise -- never a launch without the GroupNorm, nothing launched for a refused combination. */
    const float* gn_emb; int gn_emb_stride;      /* [n_hyp][gn_emb_stride] (columns [0, Cout) of row s) or NULL */
    int gn_self;
    int gn_resid_rep;          /* hypotheses that share a sample of resid under gn_self (0 reads as 1) */
} nope_conv_op;
/* amax_recorded (host int, may be NULL): 1 when this launch's kernel records max |out| (f32 storage, the wide NHWC epilogue of the
 * 128 x 192 / ping-pong / tap-resident kernels, no split-K), else 0: amax_out is then 0. */
int nope_op_conv(const nope_conv_op* op, int* amax_recorded, nope_stream_t s);
/* What nope_op_conv would do with `op`, without a launch: a pure host call; pointer fields count as NULL / non-NULL only and are never
 * dereferenced.  Follows the launch policy in force (NOPE_* tuning variables), as the launch itself does. */
typedef struct nope_conv_op_info {
    size_t splitk_bytes;       /* bytes of splitk_ws the launcher would use (0: this shape is never split, or not a compute dtype) */
    int stat_rows;             /* rows per block of the column statistics a conv of this shape can emit (64; 16 / 32 on 16- / 32-pixel maps from the kernels
                                *   that have that form; 0 = none: residual, NCHW output, ReLU, NOPE_CONV_UP2P, Cout not in whole 16-byte vectors or > 2048,
                                *   not a compute dtype) */
    int tail_stat_blocks;      /* entries per hypothesis of tail_stats: one per 64-row x 96-column tile of the output map */
    int records_out_amax;      /* nope_op_conv's amax_recorded, had amax_slot been given */
    int err;                   /* NOPE_OK, or what nope_op_conv returns for `op` before anything launches */
} nope_conv_op_info;
int nope_op_conv_query(const nope_conv_op* op, nope_conv_op_info* info);
/* conv1 of the encoder trunk: 7x7 / stride 2 / pad 3 on an NCHW f32 image, + per-channel scale (folded into the
 * weights) and shift + ReLU -> NHWC (n_img, H/2, W/2, 64).  w (64,3,7,7), scale/shift (64). */
int nope_op_stem_conv(int dtype, const float* image, const float* w, const float* scale, const float* shift, float* w_scratch,
                      void* out, int n_img, int H, int W, nope_stream_t s);
/* GroupNorm(G, C) [+ SiLU] [+ emb[hyp, c]] [+ resid]: Block.norm/act (model_utils.py:241-252), the conditioning add (:274-276), PreNorm
 * (:226-234) and Residual (:198-204), with the fusion plumbing the network runtimes launch around it:
 *     y[j] = act(GN(x_eff[j / x_rep]) (1 + scale[j]) + shift[j]) + emb[j] + resid[j / resid_rep],   j in [0, n_hyp).
 * Arguments by name, as nope_conv_op.  The statistics come from, in this order of precedence:
 *   sh_s / sh_e     a pass over x_eff (the shared form below) into `partial`: n_hyp * nope_op_gn_chunks() * G * 2 floats;
 *   colstats        [n_hyp / x_rep][stat_blocks][C][2], a conv's column statistics, folded by every workgroup itself (fold_launch = 0; C <= 2048,
 *                   no FiLM) or by a fold launch into `partial` ((n_hyp / x_rep) * G * 2 floats) first (fold_launch = 1): same bits either way;
 *   otherwise       a pass over x into `partial`: (n_hyp / x_rep) * nope_op_gn_chunks() * G * 2 floats.
 * Refused with NOPE_ERR_ARG: n_hyp <= 0, H <= 0, W <= 0, x_rep < 0, an n_hyp that x_rep does not divide; in the shared form a missing `partial`. */
int nope_op_gn_chunks(int dtype, int HW, int C);
int nope_op_gn_apply_blocks(int dtype, int HW, int C, int n_hyp);
typedef struct nope_gn_op {
    uint32_t struct_size; int dtype;      /* struct_size: sizeof(nope_gn_op); anything else is NOPE_ERR_ARG before another field is read */
    const void* x;             /* NHWC [n_hyp / x_rep][H W][C] */
    void* y;                   /* NHWC [n_hyp][H W][C] */
    float* partial; const float* colstats; int stat_blocks; int fold_launch;
    const float* gamma; const float* beta;
    int n_hyp, H, W;           /* H, W: the map; only H W counts outside the shared form */
    int C, G, act_silu;
    const float* emb; int emb_stride;        /* rows of C floats, emb_stride floats apart, or NULL */
    const float* film; int film_stride;      /* [scale (C) | shift (C)] rows, film_stride floats apart per hypothesis (0: one row for all), or NULL */
    const void* resid; int x_rep, resid_rep;      /* a rep of 0 reads as 1, as sh_rep */
    float* out_stats;          /* [n_hyp][nope_op_gn_apply_blocks()][2]: (sum, sum of squares) of the values each workgroup wrote, or NULL (not with FiLM) */
    float eps;                 /* no default: 0 is 0 */
    int fast_silu;             /* f32 storage only, SiLU on the hardware exp / rcp (what the split-precision modes run; the 16-bit types always do) -- the
                                * only form that records a range maximum: with the libm SiLU or FiLM amax_out stays 0 */
    /* The shared addend (sh_s or sh_e set): the value that is normalised is
     *     x_eff[j][p][c] = x[j][p][c] + sh_s[j / sh_rep][p][c] + sh_e[j][cls(p)][c],   j in [0, n_hyp), p = y W + x,
     *   cls(p) = 3 (y == 0 ? 0 : y == H - 1 ? 2 : 1) + (x == 0 ? 0 : x == W - 1 ? 2 : 1), the border class of the pixel; sh_s f32 NHWC
     *   [n_hyp / sh_rep][H W][C], sh_e f32 [n_hyp][9][C], both 16-byte aligned.  Two forms exist, the ones the U-Net's schedule launches under
     *   NOPE_SHARED_SPLIT: sh_s + sh_e with x = NULL (H, W >= 2), and x + sh_s with sh_e = NULL; SiLU on (act_silu = 1), x_rep = 1, no colstats, no
     *   FiLM; any other combination is refused (NOPE_ERR_ARG where the statistics pass refuses it, else NOPE_ERR_UNSUPPORTED).  x_eff is never
     *   stored: the statistics pass forms it into `partial`, the apply pass forms it again and continues as without the addend (emb, resid /
     *   resid_rep, out_stats, fast_silu, the range maximum). */
    const float* sh_s; int sh_rep; const float* sh_e;
    uint32_t* amax_slot; float* amax_out;      /* RANGE SLOTS above */
} nope_gn_op;
int nope_op_group_norm(const nope_gn_op* op, nope_stream_t s);
/* (mean, rstd) [n_hyp][2] of whole samples from nchunk (sum, sum of squares) pairs each (out_stats, tail_stats), count = HW * C. */
int nope_op_gn_finalize(const float* partial, float* ms, int n_hyp, int nchunk, float count, float eps, nope_stream_t s);
/* w [Cout][Cin][3][3] f32 -> out [9][Cout][Cin] f32, out[cls][co][ci] = the sum of w[co][ci] over the taps a zero-padded 3x3 conv has inside
 * the map at a pixel of border class cls: conv(u + e 1) = conv(u) + out[cls(p)] e for e constant over the map. */
int nope_op_conv_class_weights(const float* w, float* out, int Cout, int Cin, nope_stream_t s);
/* max |x[i]| over n f32 values (NaNs ignored; 0 for n = 0 or all zeros): what the runtimes run over conv-produced tensors in NOPE_F16X2. */
int nope_op_absmax_f32(const float* x, size_t n, uint32_t* amax_slot, float* amax_out, nope_stream_t s);
/* LinearAttention core (model_utils.py:403-416) and Attention core (:376-389) on a fused
 * qkv tensor [n_hyp][HW][3*heads*dim_head]; out [n_hyp][HW][heads*dim_head]. */
int nope_op_linear_attention(int dtype, const void* qkv, void* out, int n_hyp, int HW, int heads, int dim_head,
                             nope_stream_t s);
int nope_op_attention(int dtype, const void* qkv, void* out, int n_hyp, int HW, int heads, int dim_head,
                      nope_stream_t s);
/* out[m, n] = sum_k act(in[m,k]) * w[n,k] + bias[n]  (f32; act_in: 0 none, 1 SiLU, 2 GELU):
 * pose_mlp (u_net.py:63-72) and ResnetBlock.mlp (model_utils.py:261-265). */
int nope_op_linear(const float* in, const float* w, const float* bias, float* out, int M, int N, int K, int act_in,
                   nope_stream_t s);

/* Dataset-side crop (caller of the hot path): cv2.warpPerspective(img, M, (Wd, Hd)) of crop_frame, src/poses/utils.py:262-270
 * (bilinear, zero border), fused with the loader's image transform (dataloader/shapeNet.py:64-69):
 *   dst[c,y,x] = scale * bilinear(src, Minv (x,y,1)) + shift.   src (Hs,Ws,C) uint8 (src_is_u8 = 1, or 2: the interpolated value
 *   is rounded and clamped to [0, 255] first, as cv2's uint8 destination does) or f32 (src_is_u8 = 0), HWC;
 *   minv9_host: HOST pointer to the 3x3 inverse map, row-major; dst (C,Hd,Wd) f32. */
int nope_op_warp_perspective(const void* src, int src_is_u8, int Hs, int Ws, int C, const float* minv9_host, float* dst_chw, int Hd, int Wd,
                             float scale, float shift, nope_stream_t s);
/* (ABI 13) The test loader's chain for a STACK of decoded frames in one launch: paste on black through the alpha channel, crop, image transform
 * (dataloader/shapeNet.py:184-210,167-182,64-69; bop.py:212-232 with the mask image as the alpha channel).
 *   frames (F, Hs, Ws, Cs) uint8, Cs = 3 (RGB) or 4 (RGBA; 4-byte aligned); minv (F, 9) f32 ON THE DEVICE: one row-major inverse map per frame
 *   (output pixel -> source pixel); dst (F, 3, Hd, Wd) f32; scale, shift, round_u8 (0 / 1) as nope_op_warp_perspective's (src_is_u8 = 1 / 2).
 * Cs = 4: every source tap is composited on black first, round(c * a / 255) in integers (PIL's Image.paste(img, mask=alpha) onto black), and the
 * composited taps are interpolated -- the reference's order, paste then warp.  Interpolation, zero border, rounding, scale and shift are
 * nope_op_warp_perspective's arithmetic, operation for operation: frame f equals that call on the pasted frame f bit for bit (Cs = 3: on the raw frame).
 * NOPE_ERR_ARG: null pointers, non-positive sizes; NOPE_ERR_UNSUPPORTED: any other Cs. */
int nope_op_crop_frames(const void* frames, int F, int Hs, int Ws, int Cs, const float* minv, float* dst, int Hd, int Wd, float scale, float shift,
                        int round_u8, nope_stream_t s);
/* Token-space operators of the LDM variant (ldm/attention.py), tokens = NHWC pixels [M][C]:
 * LayerNorm over C (:210-212); GEGLU in [M][2D] -> out [M][D] (:37-44); softmax self-attention over the N tokens of each
 * sample on a fused [n][N][3C] q|k|v tensor, heads of dim_head = 32, 64 or 128 channels, C % dim_head = 0 (:168-189).  dtype = a storage code; nope_op_token_attention also takes the
 * compute tags NOPE_BF16X3 / NOPE_F16X2 (f32 tensors, every product as three bf16 MFMA passes over (hi, lo) splits: what the LDM runtime
 * launches in those modes; NOPE_F32 = all-f32 VALU arithmetic, the parity mode). */
int nope_op_layer_norm(int dtype, const void* x, void* y, const float* gamma, const float* beta, int64_t M, int C, float eps, nope_stream_t s);
int nope_op_geglu(int dtype, const void* in, void* out, int64_t M, int D, nope_stream_t s);
int nope_op_token_attention(int dtype, const void* qkv, void* out, int n, int N, int C, int dim_head, nope_stream_t s);
/* (ABI 8) ONE attention head as wide as the channels, C = 256 or 512, on the same fused [n][N][3C] q|k|v layout, scale C^-1/2: the mid-block
 * AttnBlock of the Stable Diffusion VAE (u_net/ldm/model.py:144-187; diffusers 0.14 AttentionBlock with one head).  dtype as
 * nope_op_token_attention.  Every mode runs the all-f32 VALU kernel of nope_op_token_attention with the head split over 8 / 16 lanes, on
 * the mode's storage type: the 16-bit modes read bf16 / f16 q, k, v and compute in f32 (more accurate than their matrix-core kernels, slower).
 * Other C: NOPE_ERR_ARG. */
int nope_op_wide_attention(int dtype, const void* qkv, void* out, int n, int N, int C, nope_stream_t s);

/* ------------------------------------------------------------------------------------------
 * Stable Diffusion VAE (ABI 8).  Replaces VAE_StableDiffusion.encode_image / decode_latent, src/model/encoder/AutoencoderKL.py:28-47, over
 * diffusers' AutoencoderKL (the CompVis Encoder / Decoder, src/model/u_net/ldm/model.py:77-448: ResnetBlock, AttnBlock, Downsample,
 * Upsample).  Tensor names are AutoencoderKL's own state-dict keys in the diffusers 0.14 spelling ("encoder.down_blocks.0.resnets.0.conv1.weight",
 * "encoder.mid_block.attentions.0.query.weight" [C][C], "quant_conv.weight", "decoder.up_blocks.0.upsamplers.0.conv.weight", ...).
 * Supported: every down block DownEncoderBlock2D, every up block UpDecoderBlock2D, act_fn silu, one mid-block attention head as wide as the
 * last level's channels (32 / 64 / 128: nope_op_token_attention's kernels; 256 / 512: nope_op_wide_attention).
 * NHWC activations; GroupNorm + SiLU and the 3x3 / 1x1 convolutions on the kernels of the U-Nets; Downsample as NOPE_CONV_STRIDE2_PAD01,
 * Upsample as the NOPE_CONV_UP2P phase conv; 0.18215 and its inverse folded into quant_conv / post_quant_conv at create time. */
typedef struct nope_vae nope_vae;
typedef struct {
    int in_channels;            /* 3 (any count: the input convs' K axis is zero-padded to a multiple of 8 at pack time) */
    int out_channels;           /* 3 */
    int n_levels;               /* len(block_out_channels) = 4 */
    int block_out_channels[8];  /* (128, 256, 512, 512); multiples of 32 */
    int layers_per_block;       /* 2: ResnetBlock2Ds per down block (an up block has one more) */
    int latent_channels;        /* 4 */
    int norm_num_groups;        /* 32 */
    int compute_dtype;          /* NOPE_F32 | NOPE_BF16 | NOPE_F16 | NOPE_BF16X3 | NOPE_F16X2 (= NOPE_BF16X3 here: no second weight pack, no range tracking) */
    float gn_eps;               /* GroupNorm eps; <= 0 selects 1e-6 (model.py:35-38) */
} nope_vae_config;

int nope_vae_create(const nope_vae_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_vae** out);
void nope_vae_destroy(nope_vae* vae);
/* Workspace of ONE chunk of n_img samples: decode = 0 -> encode of (n_img, in_channels, H, W) images; decode = 1 -> decode of (n_img,
 * latent_channels, H, W) latents.  0 for an unsupported size. */
size_t nope_vae_workspace_bytes(const nope_vae* vae, int decode, int n_img, int H, int W);
/* image (n_img, in_channels, H, W) f32 NCHW, H and W multiples of 2^(n_levels - 1) -> latent (n_img, latent_channels, H / f, W / f) f32 NCHW:
 * quant_conv(Encoder(image))[:, :latent_channels] * 0.18215 (the mode of the latent distribution, AutoencoderKL.py:33-34).
 * The batch runs in chunks of the largest sample count whose workspace fits workspace_bytes (NOPE_ERR_WORKSPACE if one sample does not). */
int nope_vae_encode(const nope_vae* vae, const float* image, int n_img, int H, int W, float* latent, void* workspace, size_t workspace_bytes,
                    nope_stream_t stream);
/* latent (n_img, latent_channels, h, w) f32 NCHW -> image (n_img, out_channels, f h, f w) f32 NCHW: Decoder(post_quant_conv(latent / 0.18215))
 * (AutoencoderKL.py:44-47); unnormalize = 1: (image + 1) / 2 (unnormalize_to_zero_to_one, PoseConditional.sample), folded into the output
 * conv's weights and bias.  Chunked as nope_vae_encode. */
int nope_vae_decode(const nope_vae* vae, const float* latent, int n_img, int h, int w, float* image, int unnormalize, void* workspace,
                    size_t workspace_bytes, nope_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NOPE_HIP_H */
