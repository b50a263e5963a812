// Host-side runtime of the Stable Diffusion VAE: `VAE_StableDiffusion.encode_image` / `decode_latent` (src/model/encoder/AutoencoderKL.py:28-47)
// over diffusers' AutoencoderKL, i.e. the CompVis Encoder / Decoder of src/model/u_net/ldm/model.py:77-448 (ResnetBlock, AttnBlock, Downsample,
// Upsample) plus quant_conv / post_quant_conv.  Tensor names are AutoencoderKL's state-dict keys in the diffusers 0.14 spelling.
//
// Execution model of ldm_runtime.hip: NHWC activations, every convolution on the implicit-GEMM MFMA kernels, GroupNorm + SiLU as
// gn_stats + gn_apply, a bump arena over the caller's workspace, weights packed once at create time.  What differs from the module tree,
// same arithmetic:
//   * Downsample (pad (0, 1, 0, 1), 3x3 stride 2) is ONE conv launch of geometry NOPE_CONV_STRIDE2_PAD01: no padded copy;
//   * Upsample (nearest x2 + 3x3) is the NOPE_CONV_UP2P phase conv (four 2x2 convs over the un-upsampled input);
//   * the ResnetBlock's residual add (x or its 1x1 conv_shortcut) is conv2's epilogue, AttnBlock's is proj_attn's;
//   * AttnBlock's q / k / v are one GEMM against the row-concatenated weights into the fused [n][N][3C] layout of the attention kernels
//     (one head of C channels: nope_op_token_attention's kernels at C <= 128, nope_op_wide_attention's at 256 / 512);
//   * encode: only the first latent_channels rows of quant_conv are evaluated (the mode of the latent distribution is its mean, the first
//     half of the moments), with 0.18215 folded into them; decode: 1 / 0.18215 folded into post_quant_conv's weights;
//   * decode with unnormalize: (x + 1) / 2 folded into a second pack of conv_out (weights / 2, bias / 2 + 1 / 2);
//   * latent and image channel counts are zero-padded to a multiple of 8 in the NHWC tensors (16-byte vectors of the 16-bit modes).
//
// Loader core, arena, the conv / GroupNorm launches and the entry-point bodies are the shared ones (runtime_common.h); this file keeps its
// ResnetBlock / AttnBlock / mid block, the two-slot ping-pong, and one chunk loop under nope_vae_encode / nope_vae_decode.
#include "runtime_common.h"

using namespace nope;
using namespace nope::rt;

namespace {

constexpr float kScale = 0.18215f;      // AutoencoderKL.py:34,45

struct VRes { NormW n1, n2; PackedConv c1, c2, sc; bool has_sc = false; int Cin = 0, Cout = 0; };
struct VAttn { NormW norm; PackedConv qkv, proj; int C = 0; };
struct VLevel { std::vector<VRes> res; bool has_resample = false; PackedConv resample; };

int pad8(int c) { return (c + 7) / 8 * 8; }

}  // namespace

struct nope_vae : Net {      // (dt / sdt / allocs: rt::Net; NOPE_F16X2 runs as NOPE_BF16X3: x2 stays false, no layer takes a second pack)
    nope_vae_config cfg;
    float eps = 1e-6f;
    int cin_p = 8, zp = 8, mp = 8;      // padded channel counts: image in, latent, encoder moments (2 z)
    // encoder
    PackedConv e_conv_in, e_conv_out, quant;
    std::vector<VLevel> e_down;
    VRes e_mid1, e_mid2;
    VAttn e_attn;
    NormW e_norm_out;
    // decoder
    PackedConv post_quant, d_conv_in, d_conv_out, d_conv_out_un;
    std::vector<VLevel> d_up;
    VRes d_mid1, d_mid2;
    VAttn d_attn;
    NormW d_norm_out;
};

namespace {

struct Loader : LoaderCore {
    nope_vae* net;
    Loader(nope_vae* n, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors) : LoaderCore(n->allocs, n->dt, s_, tensors, n_tensors), net(n) {}
    // conv with bias, packed for the implicit-GEMM kernels; Cin_pad > Cin: zero weights for the padded input channels
    // (NOPE_CONV_STRIDE2_PAD01 differs from NOPE_CONV_STRIDE2 in the launch geometry only: the weights are packed as the latter's)
    PackedConv conv(const std::string& pfx, int Cin, int Cout, int ksz, int mode, int Cin_pad = 0) {
        const nope_tensor_desc* d = get(pfx + "weight", {Cout, Cin, ksz, ksz});
        return pack_conv(d, pfx, Cin, Cin_pad > Cin ? Cin_pad : Cin, Cout, mode == NOPE_CONV_UP2P ? 4 : ksz * ksz, mode, true, false, 0,
                         mode == NOPE_CONV_STRIDE2_PAD01 ? NOPE_CONV_STRIDE2 : mode);
    }
    // the small convs at the latent end, rewritten on the host at create time: rows [0, rows) of the stored conv, scaled (w * ws, b * bs + ba),
    // zero rows up to Cout_pad and zero input channels up to Cin_pad
    PackedConv conv_host(const std::string& pfx, int Cin, int Cout, int ksz, int rows, int Cin_pad, int Cout_pad, float ws, float bs, float ba) {
        PackedConv c;
        c.Cin = Cin_pad; c.Cout = Cout_pad; c.mode = NOPE_CONV_PLAIN; c.ntaps = ksz * ksz;
        const nope_tensor_desc* d = get(pfx + "weight", {Cout, Cin, ksz, ksz});
        const nope_tensor_desc* bd = get(pfx + "bias", {Cout});
        if (!d || !bd || err) return c;
        const size_t per = (size_t)Cin * ksz * ksz;
        std::vector<float> w((size_t)Cout * per), b(Cout);
        if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(w.data(), d->data, w.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(b.data(), bd->data, b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { chk(NOPE_ERR_LAUNCH); return c; }
        std::vector<float> wp((size_t)Cout_pad * per, 0.f), bp(Cout_pad, 0.f);
        for (int r = 0; r < rows; ++r) {
            for (size_t i = 0; i < per; ++i) wp[(size_t)r * per + i] = w[(size_t)r * per + i] * ws;
            bp[r] = b[r] * bs + ba;
        }
        float* wt = (float*)tmalloc(wp.size() * 4);
        c.w = dmalloc((size_t)Cout_pad * c.ntaps * Cin_pad * dt_es(net->dt));
        c.bias = (float*)dmalloc((size_t)Cout_pad * 4);
        if (!wt || !c.w || !c.bias) return c;
        if (hipMemcpy(wt, wp.data(), wp.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(c.bias, bp.data(), bp.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { chk(NOPE_ERR_LAUNCH); return c; }
        chk(launch_pack_conv_w(net->dt, wt, c.w, Cout_pad, Cin_pad, c.ntaps, NOPE_CONV_PLAIN, s, nullptr, nullptr, Cin));
        return c;
    }
    // ResnetBlock2D (temb None, output_scale_factor 1): model.py:77-134
    VRes res(const std::string& p, int Cin, int Cout) {
        VRes r;
        r.Cin = Cin; r.Cout = Cout;
        r.n1 = norm(p + "norm1.", Cin);
        r.c1 = conv(p + "conv1.", Cin, Cout, 3, NOPE_CONV_PLAIN);
        r.n2 = norm(p + "norm2.", Cout);
        r.c2 = conv(p + "conv2.", Cout, Cout, 3, NOPE_CONV_PLAIN);
        r.has_sc = Cin != Cout;
        if (r.has_sc) r.sc = conv(p + "conv_shortcut.", Cin, Cout, 1, NOPE_CONV_PLAIN);
        return r;
    }
    // AttentionBlock with one head (diffusers 0.14 names; AttnBlock, model.py:144-187): query / key / value / proj_attn as Linear [C][C]
    VAttn attn(const std::string& p, int C) {
        VAttn a;
        a.C = C;
        a.norm = norm(p + "group_norm.", C);
        const nope_tensor_desc* wq = get(p + "query.weight", {C, C});
        const nope_tensor_desc* wk = get(p + "key.weight", {C, C});
        const nope_tensor_desc* wv = get(p + "value.weight", {C, C});
        const nope_tensor_desc* bq = get(p + "query.bias", {C});
        const nope_tensor_desc* bk = get(p + "key.bias", {C});
        const nope_tensor_desc* bv = get(p + "value.bias", {C});
        a.qkv.Cin = C; a.qkv.Cout = 3 * C; a.qkv.ntaps = 1;
        if (wq && wk && wv && bq && bk && bv) {
            float* cat = (float*)tmalloc((size_t)3 * C * C * 4);
            a.qkv.w = dmalloc((size_t)3 * C * C * dt_es(net->dt));
            a.qkv.bias = (float*)dmalloc((size_t)3 * C * 4);
            if (cat && a.qkv.w && a.qkv.bias) {
                copy_d2d(cat, wq->data, (size_t)C * C * 4);
                copy_d2d(cat + (size_t)C * C, wk->data, (size_t)C * C * 4);
                copy_d2d(cat + (size_t)2 * C * C, wv->data, (size_t)C * C * 4);
                copy_d2d(a.qkv.bias, bq->data, (size_t)C * 4);
                copy_d2d(a.qkv.bias + C, bk->data, (size_t)C * 4);
                copy_d2d(a.qkv.bias + 2 * C, bv->data, (size_t)C * 4);
                chk(launch_pack_conv_w(net->dt, cat, a.qkv.w, 3 * C, C, 1, NOPE_CONV_PLAIN, s));
            }
        }
        a.proj.Cin = C; a.proj.Cout = C; a.proj.ntaps = 1;
        const nope_tensor_desc* wo = get(p + "proj_attn.weight", {C, C});
        if (wo) {
            a.proj.w = dmalloc((size_t)C * C * dt_es(net->dt));
            if (a.proj.w) chk(launch_pack_conv_w(net->dt, (const float*)wo->data, a.proj.w, C, C, 1, NOPE_CONV_PLAIN, s));
        }
        a.proj.bias = copy_f32(p + "proj_attn.bias", {C});
        return a;
    }
};

struct Fwd : FwdCore<nope_vae> {
    Act act(int C, int H, int W) { return Act{alloc_act((size_t)nhyp * H * W * C), C, H, W}; }
    // conv of `a` into `out` (NHWC of the storage type, or NCHW f32 with to_nchw); output size from the geometry
    void conv(const PackedConv& c, const Act& a, void* out, const ConvOpts& o = ConvOpts()) {
        const int up = c.mode == NOPE_CONV_UP2P, down = c.mode == NOPE_CONV_STRIDE2_PAD01;
        FwdCore::conv(c, a, out, up ? 2 * a.H : down ? a.H / 2 : a.H, up ? 2 * a.W : down ? a.W / 2 : a.W, o);
    }
    // y = [silu](GroupNorm(norm_num_groups, eps)(x))
    void gn(const NormW& nm, const Act& x, void* y, int act) { FwdCore::gn(nm, net->cfg.norm_num_groups, x.p, y, x.H * x.W, act, net->eps); }
    // ResnetBlock: out = shortcut(x) + conv2(silu(norm2(conv1(silu(norm1(x))))))
    void res(const VRes& R, const Act& x, void* out) {
        const size_t mark = ar.off;
        Act t = act(R.Cin, x.H, x.W), h = act(R.Cout, x.H, x.W), t2 = act(R.Cout, x.H, x.W);
        gn(R.n1, x, t.p, 1);
        conv(R.c1, t, h.p);
        gn(R.n2, h, t2.p, 1);
        const void* resid = x.p;
        if (R.has_sc) {
            Act sk = act(R.Cout, x.H, x.W);
            conv(R.sc, x, sk.p);
            resid = sk.p;
        }
        conv(R.c2, t2, out, with_resid(resid));
        ar.off = mark;
    }
    // AttnBlock: out = x + proj_attn(softmax(q k^T / sqrt(C)) v), q | k | v = Linear(GroupNorm(x))
    void attn(const VAttn& A, const Act& x, void* out) {
        const size_t mark = ar.off;
        const int C = A.C, HW = x.H * x.W;
        Act t = act(C, x.H, x.W), qkv = act(3 * C, x.H, x.W), o = act(C, x.H, x.W);
        gn(A.norm, x, t.p, 0);
        conv(A.qkv, t, qkv.p);
        if (live()) chk(C <= 128 ? launch_token_attention(net->dt, qkv.p, o.p, nhyp, HW, C, C, s) : launch_wide_attention(net->dt, qkv.p, o.p, nhyp, HW, C, s));
        conv(A.proj, o, out, with_resid(x.p));
        ar.off = mark;
    }
    // the network's activations alternate between two slots sized for the largest one (block temporaries sit above them): out = other(in)
    void* slot[2] = {nullptr, nullptr};
    void alloc_slots(size_t elems_per_sample) {
        for (int i = 0; i < 2; ++i) slot[i] = alloc_act((size_t)nhyp * elems_per_sample);
    }
    void* other(const Act& a) const { return a.p == slot[0] ? slot[1] : slot[0]; }
    Act res_next(const VRes& R, const Act& x) { Act o{other(x), R.Cout, x.H, x.W}; res(R, x, o.p); return o; }
    Act mid(const VRes& r1, const VAttn& a, const VRes& r2, const Act& x) {
        Act b = res_next(r1, x);
        Act c{other(b), b.C, b.H, b.W};
        attn(a, b, c.p);
        return res_next(r2, c);
    }
    // Set-up of an encode / decode pass over n samples whose full-resolution side is H x W: the arena, the GroupNorm partials and the two
    // slots.  A level's blocks run at its own width or (its first block's input) its predecessor's: the finer level's in the encoder, the
    // coarser one's in the decoder.  in_elems: the padded network input per sample.  false: the workspace does not hold even that.
    bool start(const nope_vae* vae, int decode, int n, int H, int W, size_t in_elems, void* ws, size_t ws_bytes, hipStream_t s_, bool dry) {
        begin(vae, n, ws, ws_bytes, s_, dry);
        gn_partial = (float*)ar.alloc((size_t)n * 16 * 64 * 2 * 4);
        if (!gn_partial) return false;
        const int* boc = net->cfg.block_out_channels;
        const int L = net->cfg.n_levels;
        size_t big = in_elems;                              // largest activation per sample
        for (int l = 0; l < L; ++l) {
            const int nb = decode ? (l + 1 < L ? l + 1 : l) : (l ? l - 1 : 0);
            const size_t e = (size_t)(boc[nb] > boc[l] ? boc[nb] : boc[l]) * (H >> l) * (W >> l);
            if (e > big) big = e;
        }
        alloc_slots(big);
        return true;
    }
    int finish(size_t* peak) const {
        if (peak) *peak = ar.peak;
        return err;
    }
};

int run_encode(const nope_vae* net, const float* image, int n, int H, int W, float* latent, void* ws, size_t ws_bytes, hipStream_t s, bool dry,
               size_t* peak) {
    const nope_vae_config& cfg = net->cfg;
    Fwd f;
    if (!f.start(net, 0, n, H, W, (size_t)net->cin_p * H * W, ws, ws_bytes, s, dry)) return NOPE_ERR_WORKSPACE;
    Act x{f.slot[0], net->cin_p, H, W};
    if (f.live()) f.chk(launch_nchw_to_nhwc(net->sdt, image, x.p, n, net->cin_p, H * W, s, cfg.in_channels));
    Act h{f.other(x), net->e_conv_in.Cout, H, W};
    f.conv(net->e_conv_in, x, h.p);
    for (const VLevel& L : net->e_down) {
        for (const VRes& R : L.res) h = f.res_next(R, h);
        if (L.has_resample) {
            Act o{f.other(h), h.C, h.H / 2, h.W / 2};
            f.conv(L.resample, h, o.p);
            h = o;
        }
    }
    h = f.mid(net->e_mid1, net->e_attn, net->e_mid2, h);
    Act t = f.act(h.C, h.H, h.W);
    f.gn(net->e_norm_out, h, t.p, 1);
    Act m = f.act(net->mp, h.H, h.W);
    f.conv(net->e_conv_out, t, m.p);
    f.conv(net->quant, m, latent, to_nchw(NOPE_F32));          // first latent_channels moments x 0.18215, NCHW f32
    return f.finish(peak);
}

int run_decode(const nope_vae* net, const float* latent, int n, int h, int w, float* image, int unnorm, void* ws, size_t ws_bytes, hipStream_t s,
               bool dry, size_t* peak) {
    const nope_vae_config& cfg = net->cfg;
    Fwd f;
    const int up = cfg.n_levels - 1;
    if (!f.start(net, 1, n, h << up, w << up, (size_t)net->zp * h * w, ws, ws_bytes, s, dry)) return NOPE_ERR_WORKSPACE;
    Act z{f.slot[0], net->zp, h, w};
    if (f.live()) f.chk(launch_nchw_to_nhwc(net->sdt, latent, z.p, n, net->zp, h * w, s, cfg.latent_channels));
    Act zq{f.other(z), net->zp, h, w};
    f.conv(net->post_quant, z, zq.p);                  // (latent / 0.18215) through post_quant_conv
    Act x{f.other(zq), net->d_conv_in.Cout, h, w};
    f.conv(net->d_conv_in, zq, x.p);
    x = f.mid(net->d_mid1, net->d_attn, net->d_mid2, x);
    for (const VLevel& V : net->d_up) {
        for (const VRes& R : V.res) x = f.res_next(R, x);
        if (V.has_resample) {
            Act o{f.other(x), x.C, 2 * x.H, 2 * x.W};
            f.conv(V.resample, x, o.p);
            x = o;
        }
    }
    Act t = f.act(x.C, x.H, x.W);
    f.gn(net->d_norm_out, x, t.p, 1);
    f.conv(unnorm ? net->d_conv_out_un : net->d_conv_out, t, image, to_nchw(NOPE_F32));
    return f.finish(peak);
}

int run(const nope_vae* net, int decode, const float* in, int n, int H, int W, float* out, int unnorm, void* ws, size_t ws_bytes, hipStream_t s, bool dry,
        size_t* peak) {
    return decode ? run_decode(net, in, n, H, W, out, unnorm, ws, ws_bytes, s, dry, peak) : run_encode(net, in, n, H, W, out, ws, ws_bytes, s, dry, peak);
}

// arena bytes a chunk of n samples uses (0: unsupported); the caller's workspace adds up to 255 bytes of base alignment (nope_vae_workspace_bytes)
size_t peak_bytes(const nope_vae* net, int decode, int n, int H, int W) {
    size_t peak = 0;
    return run(net, decode, nullptr, n, H, W, nullptr, 0, nullptr, 0, nullptr, true, &peak) ? 0 : peak;
}

int check_size(const nope_vae* net, int decode, int n, int H, int W) {
    if (!net || n <= 0 || H <= 0 || W <= 0) return NOPE_ERR_ARG;
    const int f = 1 << (net->cfg.n_levels - 1);
    if (!decode && (H % f || W % f)) return NOPE_ERR_UNSUPPORTED;
    const long long pix = decode ? (long long)n * (H * f) * (W * f) : (long long)n * H * W;      // GEMM rows of the largest convolution
    if (pix > 0x7fffffffLL) return NOPE_ERR_UNSUPPORTED;
    return NOPE_OK;
}

// the largest chunk of samples whose workspace fits (0: not even one)
int chunk_for(const nope_vae* net, int decode, int n, int H, int W, size_t bytes) {
    const size_t one = peak_bytes(net, decode, 1, H, W);
    if (!one || one > bytes) return 0;
    int lo = 1, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        const size_t b = peak_bytes(net, decode, mid, H, W);
        if (b && b <= bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// nope_vae_encode / nope_vae_decode: the batch in the largest chunks the workspace holds.  H x W: the input's size (image or latent)
int run_chunks(const nope_vae* vae, int decode, const float* in, int n_img, int H, int W, float* out, int unnorm, void* workspace, size_t workspace_bytes,
               nope_stream_t stream) {
    int e = check_size(vae, decode, n_img, H, W);
    if (e) return e;
    if (!in || !out || !workspace) return NOPE_ERR_ARG;
    unsigned char* base;
    size_t cap;
    if (!workspace_base(workspace, workspace_bytes, base, cap)) return NOPE_ERR_WORKSPACE;
    const int chunk = chunk_for(vae, decode, n_img, H, W, cap);
    if (chunk < 1) return NOPE_ERR_WORKSPACE;
    const int f = 1 << (vae->cfg.n_levels - 1);
    const size_t img_px = decode ? (size_t)(H * f) * (W * f) : (size_t)H * W, lat_px = decode ? (size_t)H * W : (size_t)(H / f) * (W / f);
    const size_t in_per = decode ? vae->cfg.latent_channels * lat_px : vae->cfg.in_channels * img_px;
    const size_t out_per = decode ? vae->cfg.out_channels * img_px : vae->cfg.latent_channels * lat_px;
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int c = n_img - i0 < chunk ? n_img - i0 : chunk;
        e = run(vae, decode, in + (size_t)i0 * in_per, c, H, W, out + (size_t)i0 * out_per, unnorm, base, cap, (hipStream_t)stream, false, nullptr);
        if (e) return e;
    }
    return NOPE_OK;
}

}  // namespace

extern "C" {

int nope_vae_create(const nope_vae_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream, nope_vae** out) {
    if (!cfg || !tensors || !out || n_tensors <= 0) return NOPE_ERR_ARG;
    const int L = cfg->n_levels;
    if (L < 1 || L > 8 || cfg->layers_per_block < 1 || cfg->in_channels < 1 || cfg->out_channels < 1 || cfg->latent_channels < 1) return NOPE_ERR_UNSUPPORTED;
    if (cfg->norm_num_groups < 1 || cfg->norm_num_groups > 64) return NOPE_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l) {
        const int c = cfg->block_out_channels[l];
        if (c <= 0 || c % 32 || c % cfg->norm_num_groups || c > 2048) return NOPE_ERR_UNSUPPORTED;
    }
    const int Cm = cfg->block_out_channels[L - 1];      // the mid blocks' width: one attention head as wide
    if (Cm != 32 && Cm != 64 && Cm != 128 && Cm != 256 && Cm != 512) return NOPE_ERR_UNSUPPORTED;
    if (!dt_is_compute(cfg->compute_dtype)) return NOPE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    nope_vae* net = new nope_vae();
    net->cfg = *cfg;
    net->dt = dt_base(cfg->compute_dtype);
    net->sdt = dt_storage(net->dt);
    net->eps = cfg->gn_eps > 0.f ? cfg->gn_eps : 1e-6f;
    const int z = cfg->latent_channels;
    net->cin_p = pad8(cfg->in_channels);
    net->zp = pad8(z);
    net->mp = pad8(2 * z);
    const int* boc = cfg->block_out_channels;
    const int lpb = cfg->layers_per_block;
    Loader ld(net, s, tensors, n_tensors);

    // encoder: conv_in, down blocks (resnets + Downsample but on the last level), mid block, norm + SiLU + conv_out, quant_conv
    net->e_conv_in = ld.conv("encoder.conv_in.", cfg->in_channels, boc[0], 3, NOPE_CONV_PLAIN, net->cin_p);
    int ch = boc[0];
    for (int l = 0; l < L; ++l) {
        VLevel V;
        const std::string p = "encoder.down_blocks." + std::to_string(l) + ".";
        for (int j = 0; j < lpb; ++j) {
            V.res.push_back(ld.res(p + "resnets." + std::to_string(j) + ".", ch, boc[l]));
            ch = boc[l];
        }
        if (l != L - 1) { V.has_resample = true; V.resample = ld.conv(p + "downsamplers.0.conv.", ch, ch, 3, NOPE_CONV_STRIDE2_PAD01); }
        net->e_down.push_back(V);
    }
    net->e_mid1 = ld.res("encoder.mid_block.resnets.0.", Cm, Cm);
    net->e_attn = ld.attn("encoder.mid_block.attentions.0.", Cm);
    net->e_mid2 = ld.res("encoder.mid_block.resnets.1.", Cm, Cm);
    net->e_norm_out = ld.norm("encoder.conv_norm_out.", Cm);
    net->e_conv_out = ld.conv_host("encoder.conv_out.", Cm, 2 * z, 3, 2 * z, Cm, net->mp, 1.f, 1.f, 0.f);
    net->quant = ld.conv_host("quant_conv.", 2 * z, 2 * z, 1, z, net->mp, z, kScale, kScale, 0.f);
    // decoder: post_quant_conv (x 1 / 0.18215 on the weights), conv_in, mid block, up blocks (resnets + Upsample but on the last), norm + SiLU + conv_out
    net->post_quant = ld.conv_host("post_quant_conv.", z, z, 1, z, net->zp, net->zp, 1.f / kScale, 1.f, 0.f);
    net->d_conv_in = ld.conv("decoder.conv_in.", z, Cm, 3, NOPE_CONV_PLAIN, net->zp);
    net->d_mid1 = ld.res("decoder.mid_block.resnets.0.", Cm, Cm);
    net->d_attn = ld.attn("decoder.mid_block.attentions.0.", Cm);
    net->d_mid2 = ld.res("decoder.mid_block.resnets.1.", Cm, Cm);
    ch = Cm;
    for (int i = 0; i < L; ++i) {
        VLevel V;
        const int co = boc[L - 1 - i];
        const std::string p = "decoder.up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j <= lpb; ++j) {
            V.res.push_back(ld.res(p + "resnets." + std::to_string(j) + ".", ch, co));
            ch = co;
        }
        if (i != L - 1) { V.has_resample = true; V.resample = ld.conv(p + "upsamplers.0.conv.", ch, ch, 3, NOPE_CONV_UP2P); }
        net->d_up.push_back(V);
    }
    net->d_norm_out = ld.norm("decoder.conv_norm_out.", ch);
    net->d_conv_out = ld.conv_host("decoder.conv_out.", ch, cfg->out_channels, 3, cfg->out_channels, ch, cfg->out_channels, 1.f, 1.f, 0.f);
    net->d_conv_out_un = ld.conv_host("decoder.conv_out.", ch, cfg->out_channels, 3, cfg->out_channels, ch, cfg->out_channels, 0.5f, 0.5f, 0.5f);

    return finish_create(ld, "nope_vae_create", net, nope_vae_destroy, out);
}

void nope_vae_destroy(nope_vae* vae) {
    if (!vae) return;
    free_device(vae->allocs);
    delete vae;
}

size_t nope_vae_workspace_bytes(const nope_vae* vae, int decode, int n_img, int H, int W) {
    if (check_size(vae, decode, n_img, H, W) != NOPE_OK) return 0;
    const size_t peak = peak_bytes(vae, decode, n_img, H, W);
    return peak ? align_up(peak, 256) + 256 : 0;
}

int nope_vae_encode(const nope_vae* vae, const float* image, int n_img, int H, int W, float* latent, void* workspace, size_t workspace_bytes,
                    nope_stream_t stream) {
    return run_chunks(vae, 0, image, n_img, H, W, latent, 0, workspace, workspace_bytes, stream);
}

int nope_vae_decode(const nope_vae* vae, const float* latent, int n_img, int h, int w, float* image, int unnormalize, void* workspace,
                    size_t workspace_bytes, nope_stream_t stream) {
    return run_chunks(vae, 1, latent, n_img, h, w, image, unnormalize ? 1 : 0, workspace, workspace_bytes, stream);
}

}  // extern "C"
