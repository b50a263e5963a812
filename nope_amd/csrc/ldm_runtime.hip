// Host-side runtime of the LDM cross-attention U-Net variant: `UNetModelPose`
// (src/model/u_net/ldm/adapt_openaimodel.py:14-158 over openaimodel.py:428-760 and attention.py:149-277) -- the variant whose
// pose conditioning is the cross-attention `context = pose_mlp(pose).unsqueeze(1)` north_star names.
//
// Op order follows UNetModelPose.forward exactly; the execution model is the one of unet_runtime.hip (NHWC activations = token
// major, every conv / linear on the implicit-GEMM MFMA kernels, all pose hypotheses of a reference latent as one batch, bump
// arena over caller-provided workspace).  What the MI355X schedule does differently from the module tree, same arithmetic:
//   * SpatialTransformer tokens are the NHWC activations themselves: the two `rearrange`s are no-ops;
//   * attn1's to_q / to_k / to_v are one GEMM against the row-concatenated weights;
//   * attn2 is cross-attention against ONE context token: softmax over a single key is exactly 1, so its output is
//     to_out(to_v(context)) for every query; to_q, to_k and norm2 never influence the result and are not evaluated (their
//     weights are still validated at create time).  Two linear maps in a row are one: W_out W_v is formed at create time, the
//     products of ALL transformer blocks are stacked, and a forward computes every block's per-sample row in ONE small
//     linear launch (context -> sum of the blocks' channels), each block adding its slice to its tokens;
//   * with injecting_condition_twice = false the timestep embedding is zeros, so emb_layers(emb) is its bias: folded into the
//     bias of in_layers' conv at create time (use_scale_shift_norm: that bias row is the FiLM (scale | shift) of every sample);
//   * FiLM (use_scale_shift_norm) costs no pass: out_norm(h) * (1 + scale) + shift is folded into the per-channel affine the
//     GroupNorm-apply kernel evaluates anyway (kernels_norm.hip);
//   * th.cat((h, skip)) is materialised (GroupNorm(32) groups of the following ResBlock can straddle the two halves).
//
// Loader core, arena, conv / GroupNorm launches and the entry-point bodies: runtime_common.h; ResBlocks and resampling: resblock_runtime.h.
#include "resblock_runtime.h"

using namespace nope;
using namespace nope::rb;

namespace {

struct LTB { NormW ln1, ln3; PackedConv qkv, out1, ff1, ff2; int u_off = 0; };         // one BasicTransformerBlock; u_off: its slice of nope_ldm::u_w
struct LST { NormW norm; PackedConv proj_in, proj_out; std::vector<LTB> blocks; int C = 0, dh = 32; };      // dh: attention head width (dim_head)
// has_resample: a Downsample / Upsample slot -- its conv (conv_resample), or with resample.w = null avg_pool 2x2 / nearest x2 alone; under
// resblock_updown the input-block slot holds a ResBlock (res.updown = RES_DOWN), the output block's slot one in `up` (RES_UP)
struct LBlock { bool has_res = false, has_st = false, has_resample = false; LRes res, up; LST st; PackedConv resample; };     // up: an output block's ResBlock(up=True)

}  // namespace

struct nope_ldm : RtNet {      // (dt / sdt / x2 / x2r / allocs / emb_dim: RtNet, resblock_runtime.h)
    nope_ldm_config cfg;
    PackedConv conv_in, conv_out;
    NormW norm_out;
    std::vector<LBlock> input_blocks, output_blocks;     // input_blocks[0] is conv_in
    LRes mid1, mid2;
    LST mid_st;
    std::vector<int> skip_ch;                            // channels pushed by each input block
    float *pose_w0 = nullptr, *pose_b0 = nullptr, *pose_w2 = nullptr, *pose_b2 = nullptr;
    float *tw = nullptr, *tb = nullptr;                  // pose_mlp_timesteps (injecting_condition_twice)
    float *u_w = nullptr, *u_b = nullptr;                // stacked attn2 maps to_out.0 o to_v of every transformer block: [u_total][context_dim], [u_total]
    int u_total = 0;
};

namespace {

struct Loader : LoaderBase {
    nope_ldm* ldm;
    Loader(nope_ldm* n, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors) : LoaderBase(n, s_, tensors, n_tensors), ldm(n) {}
    struct UPart { float* comb; float* bias; int C, off; };
    std::vector<UPart> u_parts;
    int u_total = 0;
    // GEGLU's projection (attention.py:37-44: `x, gate = proj(x).chunk(2, dim=-1)`): rows (x_j, gate_j) interleaved, so that a lane of the conv
    // epilogue holds whole pairs (ConvArgs::geglu); the unfused path reads the same layout (launch_geglu(..., interleaved))
    PackedConv conv_geglu(const std::string& pfx, int Cin, int D) {
        PackedConv c;
        c.Cin = Cin; c.Cout = 2 * D; c.mode = NOPE_CONV_PLAIN; c.ntaps = 1;
        const nope_tensor_desc* d = get(pfx + "weight", {2 * D, Cin});
        const nope_tensor_desc* bd = get(pfx + "bias", {2 * D});
        if (!d || !bd) return c;
        float* wi = (float*)tmalloc((size_t)2 * D * Cin * 4);
        c.w = dmalloc((size_t)2 * D * Cin * (size_t)dt_es(net->dt));
        c.bias = (float*)dmalloc((size_t)2 * D * 4);
        if (!wi || !c.w || !c.bias) return c;
        const size_t rb = (size_t)Cin * 4;
        const float* w0 = (const float*)d->data;
        const float* b0 = (const float*)bd->data;
        bool ok = hipMemcpy2DAsync(wi, 2 * rb, w0, rb, rb, D, hipMemcpyDeviceToDevice, s) == hipSuccess &&
                  hipMemcpy2DAsync(wi + Cin, 2 * rb, w0 + (size_t)D * Cin, rb, rb, D, hipMemcpyDeviceToDevice, s) == hipSuccess &&
                  hipMemcpy2DAsync(c.bias, 8, b0, 4, 4, D, hipMemcpyDeviceToDevice, s) == hipSuccess &&
                  hipMemcpy2DAsync(c.bias + 1, 8, b0 + D, 4, 4, D, hipMemcpyDeviceToDevice, s) == hipSuccess;
        if (!ok) { chk(NOPE_ERR_LAUNCH); return c; }
        chk(launch_pack_conv_w(net->dt, wi, c.w, 2 * D, Cin, 1, NOPE_CONV_PLAIN, s));
        return c;
    }
    LST st(const std::string& p, int C, int dh) {
        LST T;
        T.C = C; T.dh = dh;
        const int ctx = ldm->cfg.context_dim;
        T.norm = norm(p + "norm.", C);
        T.proj_in = conv(p + "proj_in.", C, C, 1, NOPE_CONV_PLAIN, true);
        const int depth = ldm->cfg.transformer_depth > 0 ? ldm->cfg.transformer_depth : 1;
        for (int d = 0; d < depth; ++d) {                      // attention.py:251-258: `depth` blocks in sequence
        LTB t;
        const std::string b = p + "transformer_blocks." + std::to_string(d) + ".";
        t.ln1 = norm(b + "norm1.", C);
        t.ln3 = norm(b + "norm3.", C);
        get(b + "norm2.weight", {C}); get(b + "norm2.bias", {C});                     // validated, provably without effect (see header)
        get(b + "attn2.to_q.weight", {C, C}); get(b + "attn2.to_k.weight", {C, ctx});
        // attn1: q, k, v as one [3C][C] weight
        const nope_tensor_desc* wq = get(b + "attn1.to_q.weight", {C, C});
        const nope_tensor_desc* wk = get(b + "attn1.to_k.weight", {C, C});
        const nope_tensor_desc* wv = get(b + "attn1.to_v.weight", {C, C});
        t.qkv.Cin = C; t.qkv.Cout = 3 * C; t.qkv.ntaps = 1;
        if (wq && wk && wv) {
            float* cat = (float*)tmalloc((size_t)3 * C * C * 4);
            const size_t es = (size_t)dt_es(net->dt);
            t.qkv.w = dmalloc((size_t)3 * C * C * es);
            if (cat && t.qkv.w) {
                copy_d2d(cat, wq->data, (size_t)C * C * 4);
                copy_d2d(cat + (size_t)C * C, wk->data, (size_t)C * C * 4);
                copy_d2d(cat + (size_t)2 * C * C, wv->data, (size_t)C * C * 4);
                chk(launch_pack_conv_w(net->dt, cat, t.qkv.w, 3 * C, C, 1, NOPE_CONV_PLAIN, s));
            }
        }
        t.out1 = conv(b + "attn1.to_out.0.", C, C, 1, NOPE_CONV_PLAIN, true, true);
        {   // attn2: W = to_out.0.weight x to_v.weight, [C][ctx] (see the header)
            const nope_tensor_desc* wv2 = get(b + "attn2.to_v.weight", {C, ctx});
            const nope_tensor_desc* wo2 = get(b + "attn2.to_out.0.weight", {C, C});
            float* o2_b = copy_f32(b + "attn2.to_out.0.bias", {C});
            float* vT = (float*)dmalloc((size_t)ctx * C * 4);
            float* comb = (float*)dmalloc((size_t)C * ctx * 4);
            if (wv2 && wo2 && vT && comb) {
                chk(launch_nhwc_to_nchw_f32(NOPE_F32, wv2->data, vT, 1, ctx, C, s));                 // to_v.weight^T: [ctx][C]
                chk(launch_linear_naive(wo2->data, vT, nullptr, comb, C, ctx, C, 0, ctx, s));        // comb[c][j] = sum_k Wout[c][k] Wv[k][j]
            }
            t.u_off = u_total;
            u_parts.push_back(UPart{comb, o2_b, C, u_total});
            u_total += C;
        }
        t.ff1 = conv_geglu(b + "ff.net.0.proj.", C, 4 * C);
        t.ff2 = conv(b + "ff.net.2.", 4 * C, C, 1, NOPE_CONV_PLAIN, true, true);
        T.blocks.push_back(t);
        }
        T.proj_out = conv(p + "proj_out.", C, C, 1, NOPE_CONV_PLAIN, true);
        return T;
    }
};

struct Fwd : FwdBase {
    const nope_ldm* ldm;
    const float* ctx = nullptr;       // (nhyp, context_dim)
    const float* u_all = nullptr;     // (nhyp, u_total): every transformer block's to_out(to_v(context)) row
    // SpatialTransformer.forward, attention.py:264-277: GroupNorm, proj_in, `depth` BasicTransformerBlocks (:192-212), proj_out + x
    void st(const LST& T, const Act& x, void* out) {
        const int HW = x.H * x.W, C = T.C;
        const long long M = (long long)nhyp * HW;
        const size_t mark = ar.off;
        void* xn = alloc_act((size_t)M * C);
        void* tok = alloc_act((size_t)M * C);
        void* qkv = alloc_act((size_t)M * 3 * C);
        void* o = alloc_act((size_t)M * C);
        void* tok1 = alloc_act((size_t)M * C);
        void* g = alloc_act((size_t)M * 8 * C);
        void* gg = alloc_act((size_t)M * 4 * C);
        gn(T.norm, 32, x.p, xn, HW, 0, 1e-6f);
        conv(T.proj_in, Act{xn, C, x.H, x.W}, tok, x.H, x.W);
        for (const LTB& B : T.blocks) {
            // attn1 (self-attention) + residual
            void* a = xn;                                    // reuse: LN1(tok)
            if (live()) chk(launch_layernorm(net->sdt, tok, a, B.ln1.gamma, B.ln1.beta, M, C, 1e-5f, s));
            conv(B.qkv, Act{a, C, x.H, x.W}, qkv, x.H, x.W);
            if (live()) chk(launch_token_attention(net->dt, qkv, o, nhyp, HW, C, T.dh, s));
            conv(B.out1, Act{o, C, x.H, x.W}, tok1, x.H, x.W, with_resid(tok));
            // attn2 against the single pose token: + to_out(to_v(context)) for every token -- this block's slice of u_all
            if (live()) chk(launch_add_rowvec(net->sdt, tok1, tok1, u_all + B.u_off, M, HW, C, s, ldm->u_total));
            // feed-forward (GEGLU) + residual
            void* f = o;                                     // reuse: LN3(tok1)
            if (live()) chk(launch_layernorm(net->sdt, tok1, f, B.ln3.gamma, B.ln3.beta, M, C, 1e-5f, s));
            // (x_j, gate_j) column pairs: x * gelu(gate) in the projection's epilogue where the launch qualifies (16-bit modes on the
            //  128 x 192 kernel), else the projection as stored + geglu_kernel on the same layout -- bit-identical results
            if (live()) {
                ConvArgs ca;
                ca.src1 = f; ca.C1 = C; ca.Hs = ca.Ho = x.H; ca.Ws = ca.Wo = x.W; ca.ntaps = 1; ca.w = B.ff1.w; ca.bias = B.ff1.bias;
                ca.Cout = 8 * C; ca.nhyp = nhyp; ca.out = gg;
                if (conv_geglu_fusable(net->dt, ca)) {
                    ca.geglu = 1;
                    chk(launch_conv(net->dt, ca, s));
                } else {
                    conv(B.ff1, Act{f, C, x.H, x.W}, g, x.H, x.W);
                    chk(launch_geglu(net->sdt, g, gg, M, 4 * C, s, 1));
                }
            }
            conv(B.ff2, Act{gg, 4 * C, x.H, x.W}, tok, x.H, x.W, with_resid(tok1));      // (tok is dead after the attn1 residual: the block's output)
        }
        conv(T.proj_out, Act{tok, C, x.H, x.W}, out, x.H, x.W, with_resid(x.p));
        ar.off = mark;
    }
};

int run_forward(const nope_ldm* net, const FwdReq& q, void* ws, size_t ws_bytes, hipStream_t s, bool dry = false, size_t* peak = nullptr) {
    const nope_ldm_config& cfg = net->cfg;
    const int n_src = q.n_src, n_hyp = q.n_hyp, H = q.H, W = q.W;
    Fwd f;
    f.begin(net, n_hyp, ws, ws_bytes, s, dry);
    f.ldm = net;
    const int HW = H * W;
    const int cin_k = net->conv_in.Cin;          // in_channels rounded up to a whole 16-byte vector
    void* x_in = f.alloc_act((size_t)n_src * HW * cin_k);
    float* ctx = f.alloc_f32((size_t)n_hyp * cfg.context_dim);
    float* ctx2 = f.alloc_f32((size_t)n_hyp * cfg.context_dim);
    float* emb = cfg.injecting_condition_twice ? f.alloc_f32((size_t)n_hyp * net->emb_dim) : nullptr;
    float* u_all = f.alloc_f32((size_t)n_hyp * (net->u_total > 0 ? net->u_total : 1));
    f.u_all = u_all;
    f.gn_partial = f.alloc_f32((size_t)n_hyp * 16 * 32 * 2);
    if (f.err) return f.err;
    if (f.live()) {
        f.chk(launch_nchw_to_nhwc(net->sdt, q.x, x_in, n_src, cin_k, HW, s, cfg.in_channels));
        // context = pose_mlp(pose), adapt_openaimodel.py:105-116,145
        f.chk(launch_linear_naive(q.pose, net->pose_w0, net->pose_b0, ctx, n_hyp, cfg.context_dim, cfg.pose_dim, 0, cfg.context_dim, s));
        if (cfg.pose_mlp_layers == 2) {
            f.chk(launch_linear_naive(ctx, net->pose_w2, net->pose_b2, ctx2, n_hyp, cfg.context_dim, cfg.context_dim, 2, cfg.context_dim, s));
            f.ctx = ctx2;
        } else f.ctx = ctx;
        if (net->u_total > 0)     // attn2 of every transformer block at once (see the header)
            f.chk(launch_linear_naive(f.ctx, net->u_w, net->u_b, u_all, n_hyp, net->u_total, cfg.context_dim, 0, net->u_total, s));
        if (emb) {     // emb = pose_mlp_timesteps(pose), :119-123,141-142
            f.chk(launch_linear_naive(q.pose, net->tw, net->tb, emb, n_hyp, net->emb_dim, cfg.pose_dim, 0, net->emb_dim, s));
            f.emb = emb;
        }
    } else if (emb) f.emb = emb;

    // persistent skip stack
    std::vector<Act> hs;
    int curH = H, curW = W;
    // input_blocks[0]: the input conv, evaluated once per hypothesis from the shared latent (source broadcast)
    Act h{f.alloc_act((size_t)n_hyp * HW * net->conv_in.Cout), net->conv_in.Cout, H, W};
    f.conv(net->conv_in, Act{x_in, cin_k, H, W, q.x_rep}, h.p, H, W);
    hs.push_back(h);
    for (size_t b = 1; b < net->input_blocks.size(); ++b) {
        const LBlock& B = net->input_blocks[b];
        Act nxt;
        if (B.has_resample) {            // Downsample: conv 3x3, stride 2, pad 1 (openaimodel.py:143-174), or (no conv_resample) avg_pool 2x2
            nxt = Act{f.alloc_act((size_t)n_hyp * (curH / 2) * (curW / 2) * h.C), h.C, curH / 2, curW / 2};
            if (B.resample.w) f.conv(B.resample, h, nxt.p, curH / 2, curW / 2);
            else f.pool(h, nxt.p);
            curH /= 2; curW /= 2;
        } else if (B.res.updown == RES_DOWN) {      // resblock_updown: ResBlock(down=True) in the Downsample slot
            nxt = Act{f.alloc_act((size_t)n_hyp * (curH / 2) * (curW / 2) * B.res.Cout), B.res.Cout, curH / 2, curW / 2};
            f.res(B.res, h, nxt.p);
            curH /= 2; curW /= 2;
        } else {
            nxt = Act{f.alloc_act((size_t)n_hyp * curH * curW * B.res.Cout), B.res.Cout, curH, curW};
            if (B.has_st) {
                const size_t mark = f.ar.off;
                void* t = f.alloc_act((size_t)n_hyp * curH * curW * B.res.Cout);
                f.res(B.res, h, t);
                f.st(B.st, Act{t, B.res.Cout, curH, curW}, nxt.p);
                f.ar.off = mark;
            } else f.res(B.res, h, nxt.p);
        }
        h = nxt;
        hs.push_back(h);
    }
    // middle block
    {
        const size_t e = (size_t)n_hyp * curH * curW * h.C;
        Act a{f.alloc_act(e), h.C, curH, curW}, b{f.alloc_act(e), h.C, curH, curW}, c{f.alloc_act(e), h.C, curH, curW};
        f.res(net->mid1, h, a.p);
        f.st(net->mid_st, a, b.p);
        f.res(net->mid2, b, c.p);
        h = c;
    }
    // output blocks
    for (size_t b = 0; b < net->output_blocks.size(); ++b) {
        const LBlock& B = net->output_blocks[b];
        const Act sk = hs.back();
        hs.pop_back();
        const long long M = (long long)n_hyp * curH * curW;
        Act cat{f.alloc_act((size_t)M * (h.C + sk.C)), h.C + sk.C, curH, curW};
        if (f.live()) {
            f.chk(launch_copy_cols(net->sdt, h.p, cat.p, M, h.C, cat.C, 0, s));
            f.chk(launch_copy_cols(net->sdt, sk.p, cat.p, M, sk.C, cat.C, h.C, s));
        }
        Act r{f.alloc_act((size_t)M * B.res.Cout), B.res.Cout, curH, curW};
        f.res(B.res, cat, r.p);
        if (B.has_st) {
            Act t{f.alloc_act((size_t)M * B.res.Cout), B.res.Cout, curH, curW};
            f.st(B.st, r, t.p);
            r = t;
        }
        if (B.has_resample) {            // Upsample: nearest x2 + conv 3x3 (openaimodel.py:93-124) as four 2x2 phase convs; nearest x2 alone
            Act u{f.alloc_act((size_t)M * 4 * r.C), r.C, curH * 2, curW * 2};      // without conv_resample; resblock_updown: ResBlock(up=True)
            if (B.up.updown == RES_UP) f.res(B.up, r, u.p);
            else if (B.resample.w) f.conv(B.resample, r, u.p, curH * 2, curW * 2);
            else f.up2(r, u.p);
            curH *= 2; curW *= 2;
            r = u;
        }
        h = r;
    }
    // out: GroupNorm32 + SiLU + conv 3x3 (openaimodel.py:733-737) straight into the NCHW output
    {
        void* t = f.alloc_act((size_t)n_hyp * HW * h.C);
        f.gn(net->norm_out, 32, h.p, t, HW, 1, 1e-5f);
        f.conv(net->conv_out, Act{t, h.C, H, W}, q.out, H, W, to_nchw(q.out_dtype));
    }
    if (f.tracking())      // the forward's verdict; NaNs over the output of a forward whose layers left their windows (x2_range.h)
        f.chk(f.x2.finish(q.out, (size_t)n_hyp * net->cfg.out_channels * HW * (size_t)(q.out_dtype == NOPE_F32 ? 4 : 2), q.out_dtype));
    if (peak) *peak = f.ar.peak;
    return f.err;
}

int check_shape(const nope_ldm* net, int n_hyp, int n_src, int x_rep, int H, int W) {
    if (!net || n_hyp <= 0 || n_src <= 0 || x_rep <= 0 || (long long)n_src * x_rep != n_hyp || H <= 0 || W <= 0) return NOPE_ERR_ARG;
    const int f = 1 << (net->cfg.n_levels - 1);
    if (H % f || W % f) return NOPE_ERR_UNSUPPORTED;
    return NOPE_OK;
}

}  // namespace

extern "C" {

int nope_ldm_create(const nope_ldm_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_ldm** out) {
    if (!cfg || !tensors || !out || n_tensors <= 0) return NOPE_ERR_ARG;
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->num_res_blocks < 1) return NOPE_ERR_UNSUPPORTED;
    for (int l = 0; l < cfg->n_levels; ++l) {          // attention head widths the kernels have (kernels_ldm.hip): heads * width = the level's channels
        if (!cfg->attn_levels[l] && l != cfg->n_levels - 1) continue;          // (the middle block attends at the last level's width)
        const int dh = cfg->num_head_channels > 0 ? cfg->num_head_channels : cfg->head_channels[l];
        if ((dh != 32 && dh != 64 && dh != 128) || (cfg->channel_mult[l] * cfg->model_channels) % dh) return NOPE_ERR_UNSUPPORTED;
    }
    if (!dt_is_compute(cfg->compute_dtype)) return NOPE_ERR_UNSUPPORTED;
    if (cfg->pose_mlp_layers != 1 && cfg->pose_mlp_layers != 2) return NOPE_ERR_UNSUPPORTED;
    if (cfg->model_channels % 32 || cfg->in_channels < 1 || cfg->context_dim <= 0 || cfg->transformer_depth < 0 || cfg->transformer_depth > 16) return NOPE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    nope_ldm* net = new nope_ldm();
    net->cfg = *cfg;
    net->x2 = cfg->compute_dtype == NOPE_F16X2;
    net->dt = dt_base(cfg->compute_dtype);
    net->sdt = dt_storage(net->dt);
    net->emb_dim = cfg->model_channels * 4;
    net->film = cfg->use_scale_shift_norm != 0;
    net->emb_zero = !cfg->injecting_condition_twice;
    const int mc = cfg->model_channels;
    auto dh = [&](int level) { return cfg->num_head_channels > 0 ? cfg->num_head_channels : cfg->head_channels[level]; };
    Loader ld(net, s, tensors, n_tensors);

    net->pose_w0 = ld.copy_f32("pose_mlp.0.weight", {cfg->context_dim, cfg->pose_dim});
    net->pose_b0 = ld.copy_f32("pose_mlp.0.bias", {cfg->context_dim});
    if (cfg->pose_mlp_layers == 2) {
        net->pose_w2 = ld.copy_f32("pose_mlp.2.weight", {cfg->context_dim, cfg->context_dim});
        net->pose_b2 = ld.copy_f32("pose_mlp.2.bias", {cfg->context_dim});
    }
    if (cfg->injecting_condition_twice) {
        net->tw = ld.copy_f32("pose_mlp_timesteps.0.weight", {net->emb_dim, cfg->pose_dim});
        net->tb = ld.copy_f32("pose_mlp_timesteps.0.bias", {net->emb_dim});
    }
    // openaimodel.py:511-612 -- input blocks
    net->conv_in = ld.conv("input_blocks.0.0.", cfg->in_channels, mc, 3, NOPE_CONV_PLAIN, true, false, (cfg->in_channels + 7) / 8 * 8);
    net->input_blocks.emplace_back();
    std::vector<int> chans{mc};
    int ch = mc, idx = 1;
    for (int level = 0; level < cfg->n_levels; ++level) {
        for (int r = 0; r < cfg->num_res_blocks; ++r) {
            LBlock B;
            const std::string p = "input_blocks." + std::to_string(idx) + ".";
            B.has_res = true;
            B.res = ld.res(p + "0.", ch, cfg->channel_mult[level] * mc);
            ch = cfg->channel_mult[level] * mc;
            if (cfg->attn_levels[level]) { B.has_st = true; B.st = ld.st(p + "1.", ch, dh(level)); }
            net->input_blocks.push_back(B);
            chans.push_back(ch);
            ++idx;
        }
        if (level != cfg->n_levels - 1) {
            LBlock B;
            const std::string p = "input_blocks." + std::to_string(idx) + ".0.";
            if (cfg->resblock_updown) { B.has_res = true; B.res = ld.res(p, ch, ch, RES_DOWN); }
            else {
                B.has_resample = true;
                if (cfg->conv_resample) B.resample = ld.conv(p + "op.", ch, ch, 3, NOPE_CONV_STRIDE2, true);
            }
            net->input_blocks.push_back(B);
            chans.push_back(ch);
            ++idx;
        }
    }
    // :618-648 -- middle block
    net->mid1 = ld.res("middle_block.0.", ch, ch);
    net->mid_st = ld.st("middle_block.1.", ch, dh(cfg->n_levels - 1));
    net->mid2 = ld.res("middle_block.2.", ch, ch);
    // :651-731 -- output blocks
    idx = 0;
    for (int level = cfg->n_levels - 1; level >= 0; --level) {
        for (int i = 0; i <= cfg->num_res_blocks; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            LBlock B;
            const std::string p = "output_blocks." + std::to_string(idx) + ".";
            B.has_res = true;
            B.res = ld.res(p + "0.", ch + ich, mc * cfg->channel_mult[level]);
            ch = mc * cfg->channel_mult[level];
            int sub = 1;
            if (cfg->attn_levels[level]) { B.has_st = true; B.st = ld.st(p + std::to_string(sub++) + ".", ch, dh(level)); }
            if (level && i == cfg->num_res_blocks) {
                B.has_resample = true;
                if (cfg->resblock_updown) B.up = ld.res(p + std::to_string(sub) + ".", ch, ch, RES_UP);
                else if (cfg->conv_resample) B.resample = ld.conv(p + std::to_string(sub) + ".conv.", ch, ch, 3, NOPE_CONV_UP2P, true);
            }
            net->output_blocks.push_back(B);
            ++idx;
        }
    }
    net->norm_out = ld.norm("out.0.", ch);
    net->conv_out = ld.conv("out.2.", mc, cfg->out_channels, 3, NOPE_CONV_PLAIN, true);
    if (ch != mc) ld.fail("out.2.weight");

    // stack the attn2 maps of all transformer blocks (in load order: LST::u_off)
    net->u_total = ld.u_total;
    if (ld.err == NOPE_OK && ld.u_total > 0) {
        const int ctx = cfg->context_dim;
        net->u_w = (float*)ld.dmalloc((size_t)ld.u_total * ctx * 4);
        net->u_b = (float*)ld.dmalloc((size_t)ld.u_total * 4);
        if (net->u_w && net->u_b)
            for (const auto& up : ld.u_parts) {
                if (!up.comb || !up.bias) continue;
                ld.copy_d2d(net->u_w + (size_t)up.off * ctx, up.comb, (size_t)up.C * ctx * 4);
                ld.copy_d2d(net->u_b + up.off, up.bias, (size_t)up.C * 4);
            }
    }
    ld.init_x2();
    return finish_create(ld, "nope_ldm_create", net, nope_ldm_destroy, out);
}

void nope_ldm_destroy(nope_ldm* net) {
    if (!net) return;
    free_device(net->allocs, &net->x2r);
    delete net;
}

// NOPE_F16X2 activation ranges of the LDM variant: as nope_unet_x2_poll / _x2_range_check / _x2_enable (include/nope_hip.h)
int nope_ldm_x2_poll(nope_ldm* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return x2_poll(net, stream, n_out_of_range, n_adjusted, max_abs); }
int nope_ldm_x2_range_check(nope_ldm* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return x2_range_check(net, stream, n_out_of_range, n_adjusted, max_abs); }
int nope_ldm_x2_enable(nope_ldm* net, int on) { return x2_enable(net, on); }

size_t nope_ldm_workspace_bytes(const nope_ldm* net, int n_hyp, int n_src, int H, int W) {
    if (!net || n_src <= 0 || n_hyp % n_src) return 0;
    if (check_shape(net, n_hyp, n_src, n_hyp / n_src, H, W) != NOPE_OK) return 0;
    FwdReq q; q.n_src = n_src; q.x_rep = n_hyp / n_src; q.n_hyp = n_hyp; q.H = H; q.W = W;
    size_t peak = 0;
    run_forward(net, q, nullptr, 0, nullptr, true, &peak);
    return align_up(peak, 256) + 256;
}

int nope_ldm_forward(const nope_ldm* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp, int H, int W, void* out,
                     int out_dtype, void* workspace, size_t workspace_bytes, nope_stream_t stream) {
    int e = check_shape(net, n_hyp, n_src, x_rep, H, W);
    if (e) return e;
    if (!x || !pose || !out || !workspace) return NOPE_ERR_ARG;
    if (out_dtype != NOPE_F32 && out_dtype != NOPE_BF16 && out_dtype != NOPE_F16) return NOPE_ERR_UNSUPPORTED;
    unsigned char* base;
    size_t cap;
    if (!workspace_base(workspace, workspace_bytes, base, cap)) return NOPE_ERR_WORKSPACE;
    x2_poll_before_forward(net, stream);
    FwdReq q; q.x = x; q.pose = pose; q.out = out; q.out_dtype = out_dtype;
    q.n_src = n_src; q.x_rep = x_rep; q.n_hyp = n_hyp; q.H = H; q.W = W;
    return run_forward(net, q, base, cap, (hipStream_t)stream);
}

}  // extern "C"
