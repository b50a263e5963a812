// Host-side runtime of the guided-diffusion U-Net variant: `UNetModelPose`
// (src/model/u_net/guided_diffusion/adapt_u_net.py:13-97 over guided_diffusion/u_net.py:389-, ResBlock :141-253, AttentionBlock
// :255-300, QKVAttentionLegacy / QKVAttention :323-386) -- the variant whose pose conditioning is `emb = pose_mlp(pose)` in place of
// the timestep embedding.
//
// The reference's forward calls `module(h, emb, emb)`, which TimestepEmbedSequential.forward(x, emb) does not accept (every call
// raises TypeError); the one reading that type-checks is `module(h, emb)`, and that is what runs here: emb feeds every ResBlock's
// emb_layers (SiLU -> Linear), added to h or, with use_scale_shift_norm, applied as FiLM by the out_layers GroupNorm.
//
// ResBlocks and resampling are the LDM runtime's (resblock_runtime.h); the loader core, the arena, the conv / GroupNorm launches with the
// NOPE_F16X2 range tracking and the entry-point bodies are every network runtime's (runtime_common.h).  What is new:
//   * AttentionBlock: GroupNorm(32, eps 1e-5) -> qkv (a 1x1 conv over the NHWC tokens) -> softmax attention over the H*W tokens of a
//     sample on the LDM token-attention kernels -> proj_out (1x1 conv) with the residual x in its epilogue.  The legacy order's qkv rows
//     (head, q|k|v, ch) are permuted to [q | k | v] (head-major inside each) at create time, which is QKVAttention's order already;
//     the reference scales q and k by ch^-1/4 each, the kernels scale the product by ch^-1/2: equal up to rounding;
//   * the embedding is never zero: no emb_layers bias is folded; the pose MLP (Linear; Linear, GELU, Linear; or the sinusoidal
//     encoding) runs once per forward, each ResBlock's emb_layers once per ResBlock, on all hypotheses at once;
//   * time_embed.* is never evaluated (the reference does not call it either) and is not read.
#include "resblock_runtime.h"

using namespace nope;
using namespace nope::rb;

namespace {

struct LAttn { NormW norm; PackedConv qkv, proj; int C = 0, dh = 32; };             // AttentionBlock; dh: head width
// has_resample: a Downsample / Upsample slot -- its conv (conv_resample), or with resample.w = null avg_pool 2x2 / nearest x2 alone; under
// resblock_updown the input-block slot holds a ResBlock (res.updown = RES_DOWN), the output block's slot one in `up` (RES_UP)
struct GBlock { bool has_res = false, has_attn = false, has_resample = false; LRes res, up; LAttn attn; PackedConv resample; };

}  // namespace

struct nope_gd : RtNet {       // (dt / sdt / x2 / x2r / allocs / emb_dim: RtNet, resblock_runtime.h)
    nope_gd_config cfg;
    PackedConv conv_in, conv_out;
    NormW norm_out;
    std::vector<GBlock> input_blocks, output_blocks;     // input_blocks[0] is conv_in
    LRes mid1, mid2;
    LAttn mid_attn;
    float *pose_w0 = nullptr, *pose_b0 = nullptr, *pose_w2 = nullptr, *pose_b2 = nullptr;
};

namespace {

struct Loader : LoaderBase {
    nope_gd* gd;
    Loader(nope_gd* n, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors) : LoaderBase(n, s_, tensors, n_tensors), gd(n) {}
    // conv_nd(1, Cin, Cout, 1) (weight [Cout][Cin][1]) as a 1x1 conv over the NHWC tokens; perm_heads > 0: the legacy qkv order, rows
    // (head, q|k|v, ch) with ch = Cout / 3 / perm_heads, reordered to (q|k|v, head, ch) -- weights and bias
    PackedConv conv1d(const std::string& pfx, int Cin, int Cout, int perm_heads = 0) {
        PackedConv c;
        c.Cin = Cin; c.Cout = Cout; c.mode = NOPE_CONV_PLAIN; c.ntaps = 1;
        const nope_tensor_desc* d = get(pfx + "weight", {Cout, Cin, 1});
        const nope_tensor_desc* bd = get(pfx + "bias", {Cout});
        if (!d || !bd) return c;
        c.w = dmalloc((size_t)Cout * Cin * (size_t)dt_es(net->dt));
        c.bias = (float*)dmalloc((size_t)Cout * 4);
        if (!c.w || !c.bias) return c;
        const float* w0 = (const float*)d->data;
        const float* b0 = (const float*)bd->data;
        if (perm_heads > 0) {
            float* wp = (float*)tmalloc((size_t)Cout * Cin * 4);
            if (!wp) return c;
            const int C = Cout / 3, ch = C / perm_heads;
            for (int h = 0; h < perm_heads; ++h)
                for (int part = 0; part < 3; ++part) {
                    const size_t src = (size_t)h * 3 * ch + (size_t)part * ch, dst = (size_t)part * C + (size_t)h * ch;
                    copy_d2d(wp + dst * Cin, w0 + src * Cin, (size_t)ch * Cin * 4);
                    copy_d2d(c.bias + dst, b0 + src, (size_t)ch * 4);
                }
            chk(launch_pack_conv_w(net->dt, wp, c.w, Cout, Cin, 1, NOPE_CONV_PLAIN, s));
        } else {
            copy_d2d(c.bias, b0, (size_t)Cout * 4);
            chk(launch_pack_conv_w(net->dt, w0, c.w, Cout, Cin, 1, NOPE_CONV_PLAIN, s));
        }
        return c;
    }
    LAttn attn(const std::string& p, int C, int dh) {
        LAttn A;
        A.C = C; A.dh = dh;
        A.norm = norm(p + "norm.", C);
        A.qkv = conv1d(p + "qkv.", C, 3 * C, gd->cfg.new_attention_order ? 0 : C / dh);
        A.proj = conv1d(p + "proj_out.", C, C);
        return A;
    }
};

struct Fwd : FwdBase {
    // AttentionBlock._forward, u_net.py:294-299: x + proj_out(attention(qkv(norm(x))))
    void attn(const LAttn& A, const Act& x, void* out) {
        const int HW = x.H * x.W, C = A.C;
        const size_t M = (size_t)nhyp * HW;
        const size_t mark = ar.off;
        void* xn = alloc_act(M * C);
        void* qkv = alloc_act(M * 3 * C);
        void* o = alloc_act(M * C);
        gn(A.norm, 32, x.p, xn, HW, 0, 1e-5f);
        conv(A.qkv, Act{xn, C, x.H, x.W}, qkv, x.H, x.W);
        if (live()) chk(launch_token_attention(net->dt, qkv, o, nhyp, HW, C, A.dh, s));
        if (tracking()) x2.overwritten(o);
        conv(A.proj, Act{o, C, x.H, x.W}, out, x.H, x.W, with_resid(x.p));
        ar.off = mark;
    }
};

int run_forward(const nope_gd* net, const FwdReq& q, void* ws, size_t ws_bytes, hipStream_t s, bool dry = false, size_t* peak = nullptr) {
    const nope_gd_config& cfg = net->cfg;
    const int n_src = q.n_src, n_hyp = q.n_hyp, H = q.H, W = q.W;
    Fwd f;
    f.begin(net, n_hyp, ws, ws_bytes, s, dry);
    const int HW = H * W;
    const int cin_k = net->conv_in.Cin;          // in_channels rounded up to a whole 16-byte vector
    const int E = net->emb_dim;
    void* x_in = f.alloc_act((size_t)n_src * HW * cin_k);
    float* emb = f.alloc_f32((size_t)n_hyp * E);
    float* e1 = cfg.pose_mlp == NOPE_GD_POSE_TWO_LAYERS ? f.alloc_f32((size_t)n_hyp * E) : nullptr;
    f.gn_partial = f.alloc_f32((size_t)n_hyp * 16 * 32 * 2);
    f.emb = emb;
    if (f.err) return f.err;
    if (f.live()) {
        f.chk(launch_nchw_to_nhwc(net->sdt, q.x, x_in, n_src, cin_k, HW, s, cfg.in_channels));
        // emb = pose_mlp(pose), adapt_u_net.py:62-78,87
        if (cfg.pose_mlp == NOPE_GD_POSE_ENCODING) f.chk(launch_pos_emb(q.pose, emb, n_hyp, cfg.pose_dim, E, s));
        else if (cfg.pose_mlp == NOPE_GD_POSE_TWO_LAYERS) {
            f.chk(launch_linear_naive(q.pose, net->pose_w0, net->pose_b0, e1, n_hyp, E, cfg.pose_dim, 0, E, s));
            f.chk(launch_linear_naive(e1, net->pose_w2, net->pose_b2, emb, n_hyp, E, E, 2, E, s));          // GELU (erf) on its input
        } else f.chk(launch_linear_naive(q.pose, net->pose_w0, net->pose_b0, emb, n_hyp, E, cfg.pose_dim, 0, E, s));
    }

    std::vector<Act> hs;
    int curH = H, curW = W;
    // input_blocks[0]: the input conv, evaluated once per hypothesis from the shared latent (source broadcast)
    Act h{f.alloc_act((size_t)n_hyp * HW * net->conv_in.Cout), net->conv_in.Cout, H, W};
    f.conv(net->conv_in, Act{x_in, cin_k, H, W, q.x_rep}, h.p, H, W);
    hs.push_back(h);
    for (size_t b = 1; b < net->input_blocks.size(); ++b) {
        const GBlock& B = net->input_blocks[b];
        Act nxt;
        if (B.has_resample) {            // Downsample: conv 3x3, stride 2, pad 1, or (no conv_resample) avg_pool 2x2 (u_net.py:112-138)
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
            if (B.has_attn) {
                const size_t mark = f.ar.off;
                void* t = f.alloc_act((size_t)n_hyp * curH * curW * B.res.Cout);
                f.res(B.res, h, t);
                f.attn(B.attn, Act{t, B.res.Cout, curH, curW}, nxt.p);
                f.ar.off = mark;
            } else f.res(B.res, h, nxt.p);
        }
        h = nxt;
        hs.push_back(h);
    }
    // middle block: ResBlock, AttentionBlock, ResBlock
    {
        const size_t e = (size_t)n_hyp * curH * curW * h.C;
        Act a{f.alloc_act(e), h.C, curH, curW}, b{f.alloc_act(e), h.C, curH, curW}, c{f.alloc_act(e), h.C, curH, curW};
        f.res(net->mid1, h, a.p);
        f.attn(net->mid_attn, a, b.p);
        f.res(net->mid2, b, c.p);
        h = c;
    }
    // output blocks: th.cat([h, hs.pop()]) -> ResBlock [-> AttentionBlock] [-> Upsample / ResBlock(up=True)]
    for (size_t b = 0; b < net->output_blocks.size(); ++b) {
        const GBlock& B = net->output_blocks[b];
        const Act sk = hs.back();
        hs.pop_back();
        const long long M = (long long)n_hyp * curH * curW;
        Act cat{f.alloc_act((size_t)M * (h.C + sk.C)), h.C + sk.C, curH, curW};
        if (f.live()) {
            f.chk(launch_copy_cols(net->sdt, h.p, cat.p, M, h.C, cat.C, 0, s));
            f.chk(launch_copy_cols(net->sdt, sk.p, cat.p, M, sk.C, cat.C, h.C, s));
        }
        if (f.tracking()) f.x2.overwritten(cat.p);
        Act r{f.alloc_act((size_t)M * B.res.Cout), B.res.Cout, curH, curW};
        f.res(B.res, cat, r.p);
        if (B.has_attn) {
            Act t{f.alloc_act((size_t)M * B.res.Cout), B.res.Cout, curH, curW};
            f.attn(B.attn, r, t.p);
            r = t;
        }
        if (B.has_resample) {            // Upsample: nearest x2 + conv 3x3 as four 2x2 phase convs; nearest x2 alone without conv_resample;
            Act u{f.alloc_act((size_t)M * 4 * r.C), r.C, curH * 2, curW * 2};      // resblock_updown: ResBlock(up=True)
            if (B.up.updown == RES_UP) f.res(B.up, r, u.p);
            else if (B.resample.w) f.conv(B.resample, r, u.p, curH * 2, curW * 2);
            else f.up2(r, u.p);
            curH *= 2; curW *= 2;
            r = u;
        }
        h = r;
    }
    // out: GroupNorm32 + SiLU + conv 3x3 straight into the NCHW output
    {
        void* t = f.alloc_act((size_t)n_hyp * HW * h.C);
        f.gn(net->norm_out, 32, h.p, t, HW, 1, 1e-5f);
        f.conv(net->conv_out, Act{t, h.C, H, W}, q.out, H, W, to_nchw(q.out_dtype));
    }
    if (f.tracking())      // the forward's verdict; NaNs over the output of a forward whose layers left their windows (x2_range.h)
        f.chk(f.x2.finish(q.out, (size_t)n_hyp * cfg.out_channels * HW * (size_t)(q.out_dtype == NOPE_F32 ? 4 : 2), q.out_dtype));
    if (peak) *peak = f.ar.peak;
    return f.err;
}

int check_shape(const nope_gd* net, int n_hyp, int n_src, int x_rep, int H, int W) {
    if (!net || n_hyp <= 0 || n_src <= 0 || x_rep <= 0 || (long long)n_src * x_rep != n_hyp || H <= 0 || W <= 0) return NOPE_ERR_ARG;
    const int f = 1 << (net->cfg.n_levels - 1);
    if (H % f || W % f) return NOPE_ERR_UNSUPPORTED;
    return NOPE_OK;
}

bool head_ok(int C, int dh) { return (dh == 32 || dh == 64 || dh == 128) && C % dh == 0; }

}  // namespace

extern "C" {

int nope_gd_create(const nope_gd_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_gd** out) {
    if (!cfg || !tensors || !out || n_tensors <= 0) return NOPE_ERR_ARG;
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->num_res_blocks < 1) return NOPE_ERR_UNSUPPORTED;
    const int mc = cfg->model_channels;
    for (int l = 0; l < cfg->n_levels; ++l) {          // attention head widths the kernels have (kernels_ldm.hip): 32 / 64 / 128 dividing the channels
        if (cfg->channel_mult[l] < 1) return NOPE_ERR_UNSUPPORTED;
        if (cfg->attn_levels[l] && (!head_ok(cfg->channel_mult[l] * mc, cfg->head_channels_in[l]) || !head_ok(cfg->channel_mult[l] * mc, cfg->head_channels_out[l])))
            return NOPE_ERR_UNSUPPORTED;
    }
    if (!head_ok(cfg->channel_mult[cfg->n_levels - 1] * mc, cfg->head_channels_mid)) return NOPE_ERR_UNSUPPORTED;
    if (!dt_is_compute(cfg->compute_dtype)) return NOPE_ERR_UNSUPPORTED;
    if (cfg->pose_mlp < NOPE_GD_POSE_SINGLE || cfg->pose_mlp > NOPE_GD_POSE_ENCODING || cfg->pose_dim < 1) return NOPE_ERR_UNSUPPORTED;
    if (cfg->pose_mlp == NOPE_GD_POSE_ENCODING && (4 * mc) % (2 * cfg->pose_dim)) return NOPE_ERR_UNSUPPORTED;
    if (mc % 32 || cfg->in_channels < 1 || cfg->out_channels < 1) return NOPE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    nope_gd* net = new nope_gd();
    net->cfg = *cfg;
    net->x2 = cfg->compute_dtype == NOPE_F16X2;
    net->dt = dt_base(cfg->compute_dtype);
    net->sdt = dt_storage(net->dt);
    net->emb_dim = mc * 4;
    net->film = cfg->use_scale_shift_norm != 0;
    net->emb_zero = false;
    Loader ld(net, s, tensors, n_tensors);

    const int E = net->emb_dim;
    if (cfg->pose_mlp != NOPE_GD_POSE_ENCODING) {       // adapt_u_net.py:62-73
        net->pose_w0 = ld.copy_f32("pose_mlp.0.weight", {E, cfg->pose_dim});
        net->pose_b0 = ld.copy_f32("pose_mlp.0.bias", {E});
    }
    if (cfg->pose_mlp == NOPE_GD_POSE_TWO_LAYERS) {
        net->pose_w2 = ld.copy_f32("pose_mlp.2.weight", {E, E});
        net->pose_b2 = ld.copy_f32("pose_mlp.2.bias", {E});
    }
    // u_net.py:480-530 -- input blocks
    const int ch0 = cfg->channel_mult[0] * mc;
    net->conv_in = ld.conv("input_blocks.0.0.", cfg->in_channels, ch0, 3, NOPE_CONV_PLAIN, true, false, (cfg->in_channels + 7) / 8 * 8);
    net->input_blocks.emplace_back();
    std::vector<int> chans{ch0};
    int ch = ch0, idx = 1;
    for (int level = 0; level < cfg->n_levels; ++level) {
        for (int r = 0; r < cfg->num_res_blocks; ++r) {
            GBlock B;
            const std::string p = "input_blocks." + std::to_string(idx) + ".";
            B.has_res = true;
            B.res = ld.res(p + "0.", ch, cfg->channel_mult[level] * mc);
            ch = cfg->channel_mult[level] * mc;
            if (cfg->attn_levels[level]) { B.has_attn = true; B.attn = ld.attn(p + "1.", ch, cfg->head_channels_in[level]); }
            net->input_blocks.push_back(B);
            chans.push_back(ch);
            ++idx;
        }
        if (level != cfg->n_levels - 1) {
            GBlock B;
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
    // :532-558 -- middle block
    net->mid1 = ld.res("middle_block.0.", ch, ch);
    net->mid_attn = ld.attn("middle_block.1.", ch, cfg->head_channels_mid);
    net->mid2 = ld.res("middle_block.2.", ch, ch);
    // :560-603 -- output blocks
    idx = 0;
    for (int level = cfg->n_levels - 1; level >= 0; --level) {
        for (int i = 0; i <= cfg->num_res_blocks; ++i) {
            const int ich = chans.back();
            chans.pop_back();
            GBlock B;
            const std::string p = "output_blocks." + std::to_string(idx) + ".";
            B.has_res = true;
            B.res = ld.res(p + "0.", ch + ich, mc * cfg->channel_mult[level]);
            ch = mc * cfg->channel_mult[level];
            int sub = 1;
            if (cfg->attn_levels[level]) { B.has_attn = true; B.attn = ld.attn(p + std::to_string(sub++) + ".", ch, cfg->head_channels_out[level]); }
            if (level && i == cfg->num_res_blocks) {
                B.has_resample = true;
                if (cfg->resblock_updown) B.up = ld.res(p + std::to_string(sub) + ".", ch, ch, RES_UP);
                else if (cfg->conv_resample) B.resample = ld.conv(p + std::to_string(sub) + ".conv.", ch, ch, 3, NOPE_CONV_UP2P, true);
            }
            net->output_blocks.push_back(B);
            ++idx;
        }
    }
    // :605-609 -- out
    net->norm_out = ld.norm("out.0.", ch);
    net->conv_out = ld.conv("out.2.", ch0, cfg->out_channels, 3, NOPE_CONV_PLAIN, true);
    if (ch != ch0) ld.fail("out.2.weight");

    ld.init_x2();
    return finish_create(ld, "nope_gd_create", net, nope_gd_destroy, out);
}

void nope_gd_destroy(nope_gd* net) {
    if (!net) return;
    free_device(net->allocs, &net->x2r);
    delete net;
}

// NOPE_F16X2 activation ranges of the guided-diffusion variant: as nope_ldm_x2_poll / _x2_range_check / _x2_enable
int nope_gd_x2_poll(nope_gd* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return x2_poll(net, stream, n_out_of_range, n_adjusted, max_abs); }
int nope_gd_x2_range_check(nope_gd* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return x2_range_check(net, stream, n_out_of_range, n_adjusted, max_abs); }
int nope_gd_x2_enable(nope_gd* net, int on) { return x2_enable(net, on); }

size_t nope_gd_workspace_bytes(const nope_gd* net, int n_hyp, int n_src, int H, int W) {
    if (!net || n_src <= 0 || n_hyp % n_src) return 0;
    if (check_shape(net, n_hyp, n_src, n_hyp / n_src, H, W) != NOPE_OK) return 0;
    FwdReq q; q.n_src = n_src; q.x_rep = n_hyp / n_src; q.n_hyp = n_hyp; q.H = H; q.W = W;
    size_t peak = 0;
    run_forward(net, q, nullptr, 0, nullptr, true, &peak);
    return align_up(peak, 256) + 256;
}

int nope_gd_forward(const nope_gd* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp, int H, int W, void* out,
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
