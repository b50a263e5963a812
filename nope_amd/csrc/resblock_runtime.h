// Shared host-side pieces of the U-Net variants built on guided-diffusion's ResBlock (openaimodel.py:177-288 of the LDM code,
// guided_diffusion/u_net.py:141-253): the LDM cross-attention variant (ldm_runtime.hip) and the guided-diffusion variant
// (gd_runtime.hip).  Weight loading of convs, GroupNorms and ResBlocks (up / down, FiLM), the bump arena over the caller's
// workspace, and the forward pieces: conv / GroupNorm launches with the NOPE_F16X2 range tracking (x2_range.h), avg-pool 2x2,
// nearest x2 and the ResBlock itself.  A network handle derives from RtNet; its loader and forward derive from LoaderBase /
// FwdBase and add their attention blocks.
#pragma once
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "nope_common.h"
#include "x2_range.h"

namespace nope {
namespace rb {

struct LConv { void* w = nullptr; float* bias = nullptr; int Cin = 0, Cout = 0, ntaps = 1, mode = NOPE_CONV_PLAIN; void* w_x2 = nullptr; int x2_id = -1; };   // w_x2 / x2_id: NOPE_F16X2, the 3x3 convs' second pack and its slot in the range table (x2_range.h)
struct LNorm { float* gamma = nullptr; float* beta = nullptr; int C = 0; };
struct LRes { LNorm n1, n2; LConv c1, c2, skip; bool has_skip = false; float *emb_w = nullptr, *emb_b = nullptr; int Cin = 0, Cout = 0;
              int updown = 0; };      // updown: 0, RES_DOWN or RES_UP (resblock_updown, openaimodel.py:224-231)
enum { RES_DOWN = 1, RES_UP = 2 };

// What the shared code reads of a network handle
struct RtNet {
    int dt = NOPE_F32;      // compute dtype (conv kernels, weight packing)
    int sdt = NOPE_F32;     // storage dtype of the activations (every other kernel)
    bool x2 = false;        // NOPE_F16X2: dt = NOPE_BF16X3 everywhere, plus a second weight pack per 3x3 conv for the ping-pong kernels' f16 + MX-fp8 tile
    mutable X2Range x2r;    // ... and the activation-range tracking that keeps the tile inside its accurate window (x2_range.h)
    std::vector<void*> allocs;
    int emb_dim = 0;        // width of the embedding the ResBlocks' emb_layers read (4 * model_channels)
    bool film = false;      // use_scale_shift_norm: emb_layers give (scale | shift), applied by the out_layers GroupNorm
    bool emb_zero = false;  // the embedding is zeros: emb_layers(emb) is its bias, folded into in_layers' conv bias at create time (no FiLM)
};

struct LoaderBase {
    RtNet* net;
    hipStream_t s;
    std::map<std::string, const nope_tensor_desc*> tab;
    int err = NOPE_OK;
    std::string missing;
    void fail(const std::string& n) { if (err == NOPE_OK) { err = NOPE_ERR_WEIGHT; missing = n; } }
    // device-to-device copy of a state-dict tensor at create time; a refused copy (bad pointer, wrong device) fails the create call itself,
    // not just the stream synchronisation that ends it
    void copy_d2d(void* dst, const void* src, size_t bytes) {
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess && err == NOPE_OK) err = NOPE_ERR_LAUNCH;
    }
    void chk(int e) { if (e && err == NOPE_OK) err = e; }
    const nope_tensor_desc* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = tab.find(name);
        if (it == tab.end() || !it->second->data || it->second->ndim != (int)shape.size()) { fail(name); return nullptr; }
        int i = 0;
        for (int64_t v : shape) if (it->second->shape[i++] != v) { fail(name); return nullptr; }
        return it->second;
    }
    void* dmalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { if (err == NOPE_OK) err = NOPE_ERR_ALLOC; return nullptr; }
        net->allocs.push_back(p);
        return p;
    }
    std::vector<void*> temps;                  // staging buffers of create time, freed after its final synchronize
    void* tmalloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { if (err == NOPE_OK) err = NOPE_ERR_ALLOC; return nullptr; }
        temps.push_back(p);
        return p;
    }
    void free_temps() { for (void* p : temps) hipFree(p); temps.clear(); }
    float* copy_f32(const std::string& name, std::initializer_list<int64_t> shape) {
        const nope_tensor_desc* d = get(name, shape);
        if (!d) return nullptr;
        size_t n = 1;
        for (int64_t v : shape) n *= (size_t)v;
        float* p = (float*)dmalloc(n * 4);
        if (p) copy_d2d(p, d->data, n * 4);
        return p;
    }
    // conv (4-d weight) or linear (2-d weight) packed for the implicit-GEMM kernel
    // (Cin_pad > Cin: the kernel sees Cin_pad input channels, the last ones zero -- the 4-channel latent of vae_cin_ldm.yaml padded
    //  to one 16-byte vector of the 16-bit modes)
    LConv conv(const std::string& pfx, int Cin, int Cout, int ksz, int mode, bool has_bias, bool linear = false, int Cin_pad = 0) {
        LConv c;
        const int Ck = Cin_pad > Cin ? Cin_pad : Cin;
        c.Cin = Ck; c.Cout = Cout; c.mode = mode;
        c.ntaps = mode == NOPE_CONV_UP2P ? 4 : ksz * ksz;
        const nope_tensor_desc* d = linear ? get(pfx + "weight", {Cout, Cin}) : get(pfx + "weight", {Cout, Cin, ksz, ksz});
        if (d) {
            const size_t es = (size_t)dt_es(net->dt);
            c.w = dmalloc((size_t)Cout * c.ntaps * Ck * es * (mode == NOPE_CONV_UP2P ? 4 : 1));
            if (c.w) chk(launch_pack_conv_w(net->dt, d->data, c.w, Cout, Ck, c.ntaps, mode, s, nullptr, nullptr, Cin));
            if (net->x2 && !linear && ksz == 3 && (mode == NOPE_CONV_PLAIN || mode == NOPE_CONV_UP2P) && Ck == Cin && Cin % 32 == 0) {
                const size_t x2b = conv_w_x2_bytes(Cout, Cin, c.ntaps, mode);
                c.w_x2 = dmalloc(x2b);
                if (c.w_x2) { chk(launch_pack_conv_w_x2((const float*)d->data, c.w_x2, Cout, Cin, s, c.ntaps, mode)); c.x2_id = net->x2r.add_layer(c.w_x2, x2b); }
            }
        }
        if (has_bias) c.bias = copy_f32(pfx + "bias", {Cout});
        return c;
    }
    LNorm norm(const std::string& pfx, int C) {
        LNorm n;
        n.C = C;
        n.gamma = copy_f32(pfx + "weight", {C});
        n.beta = copy_f32(pfx + "bias", {C});
        return n;
    }
    LRes res(const std::string& p, int Cin, int Cout, int updown = 0) {
        LRes r;
        r.Cin = Cin; r.Cout = Cout; r.updown = updown;
        r.n1 = norm(p + "in_layers.0.", Cin);
        // (up: GroupNorm + SiLU -> nearest x2 -> conv 3x3 is the phase conv of Upsample; down: the conv reads the pooled activation)
        r.c1 = conv(p + "in_layers.2.", Cin, Cout, 3, updown == RES_UP ? NOPE_CONV_UP2P : NOPE_CONV_PLAIN, true);
        const int film = net->film ? 2 : 1;          // emb_layers.1: Linear(emb, 2 C) for FiLM, openaimodel.py:233-239
        r.emb_w = copy_f32(p + "emb_layers.1.weight", {film * Cout, net->emb_dim});
        r.emb_b = copy_f32(p + "emb_layers.1.bias", {film * Cout});
        r.n2 = norm(p + "out_layers.0.", Cout);
        r.c2 = conv(p + "out_layers.3.", Cout, Cout, 3, NOPE_CONV_PLAIN, true);
        r.has_skip = Cin != Cout;
        if (r.has_skip) r.skip = conv(p + "skip_connection.", Cin, Cout, 1, NOPE_CONV_PLAIN, true);
        if (net->emb_zero && !net->film && r.c1.bias && r.emb_b)     // emb == 0: emb_layers(emb) = its bias, folded into conv1's
            chk(launch_add_rowvec(NOPE_F32, r.c1.bias, r.c1.bias, r.emb_b, 1, 1, Cout, s));
        return r;
    }
};

struct Arena {
    unsigned char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    bool dry = false;
    void* alloc(size_t bytes) {
        const size_t o = align_up(off, 256);
        off = o + bytes;
        if (off > peak) peak = off;
        if (dry) return (void*)(uintptr_t)(0x1000 + o);
        if (off > cap) return nullptr;
        return base + o;
    }
};

struct Act { void* p = nullptr; int C = 0, H = 0, W = 0; };

struct FwdBase {
    const RtNet* net;
    hipStream_t s;
    Arena ar;
    int nhyp = 0, err = NOPE_OK;
    size_t es = 4;
    float* gn_partial = nullptr;
    const float* emb = nullptr;       // (nhyp, emb_dim) or null (zeros)
    X2Fwd x2;                         // NOPE_F16X2 range tracking of this forward (x2_range.h)
    bool tracking() const { return x2.on && err == NOPE_OK; }

    void chk(int e) { if (e != NOPE_OK && err == NOPE_OK) err = e; }
    bool live() const { return !ar.dry && err == NOPE_OK; }
    void* alloc_act(size_t elems) {
        void* p = ar.alloc(elems * es);
        if (!p && err == NOPE_OK) err = NOPE_ERR_WORKSPACE;
        return p;
    }
    float* alloc_f32(size_t n) {
        float* p = (float*)ar.alloc(n * 4);
        if (!p && err == NOPE_OK) err = NOPE_ERR_WORKSPACE;
        return p;
    }
    void conv(const LConv& c, const Act& a, void* out, int Ho, int Wo, const void* resid = nullptr, int out_nchw = 0, int out_dt = NOPE_F32,
              int rep = 1, int n = -1) {
        if (!live()) return;
        ConvArgs ca;
        ca.src1 = a.p; ca.C1 = a.C; ca.rep1 = rep; ca.Hs = a.H; ca.Ws = a.W; ca.Ho = Ho; ca.Wo = Wo;
        ca.mode = c.mode; ca.ntaps = c.ntaps; ca.w = c.w; ca.bias = c.bias; ca.resid = resid; ca.out = out; ca.Cout = c.Cout;
        ca.nhyp = n < 0 ? nhyp : n; ca.out_nchw = out_nchw; ca.out_dt = out_dt;
        if (a.C != c.Cin) { chk(NOPE_ERR_ARG); return; }
        if (c.w_x2 && !net->x2r.off) { ca.w_x2 = c.w_x2; ca.x2_t_zero = net->x2r.t_zero(c.x2_id) ? 1 : 0; }
        if (tracking()) {
            if (ca.w_x2 && conv_takes_x2(net->dt, ca)) {      // the two-pass tile: the layer's range shift follows its input's maximum
                x2.consumes(c.x2_id, x2.slot_for(a.p, (size_t)(ca.nhyp / rep) * a.H * a.W * a.C));
                chk(x2.err);
            }
            x2.overwritten(out);           // (conv epilogues record no maximum here: a two-pass consumer of `out` takes an absmax pass)
        }
        chk(launch_conv(net->dt, ca, s));
    }
    // y = [silu](GroupNorm(32, eps)(x))
    void gn(const LNorm& nm, const void* x, void* y, int HW, int act, float eps, const float* film = nullptr, int film_stride = 0) {
        if (!live()) return;
        const int nch = gn_stats_chunks(HW, nm.C, net->sdt);
        chk(launch_gn_stats(net->sdt, x, gn_partial, nhyp, HW, nm.C, 32, nch, s));
        GnApplyArgs ga;
        ga.x = x; ga.y = y; ga.partial = gn_partial; ga.nchunk = nch; ga.gamma = nm.gamma; ga.beta = nm.beta;
        ga.nhyp = nhyp; ga.HW = HW; ga.C = nm.C; ga.G = 32; ga.act = act; ga.eps = eps;
        ga.film = film; ga.film_stride = film_stride;
        ga.fast_silu = net->dt != NOPE_F32 ? 1 : 0;      // (f32 storage of the split-precision modes: hardware exp / rcp; the f32 mode keeps expf and the division)
        if (tracking()) {                                // (the FiLM instantiation records no maximum: its consumer takes an absmax pass)
            if (!film) { const int sl = x2.produce(y); if (sl >= 0) ga.amax_out = x2.slot_ptr(sl); }
            else x2.overwritten(y);
        }
        chk(launch_gn_apply(net->sdt, ga, s));
    }
    // parameter-free resampling of an activation (storage dtype); the output's range is unknown to x2_range.h: a two-pass conv that
    // reads it takes an absmax pass (the arena hands out addresses again -- a stale slot of an earlier tensor would misjudge it)
    void pool(const Act& x, void* y) {
        if (!live()) return;
        if (tracking()) x2.overwritten(y);
        chk(launch_avg_pool2(net->sdt, x.p, y, nhyp, x.H, x.W, x.C, s));
    }
    void up2(const Act& x, void* y) {
        if (!live()) return;
        if (tracking()) x2.overwritten(y);
        chk(launch_nearest2(net->sdt, x.p, y, nhyp, x.H, x.W, x.C, s));
    }
    // ResBlock._forward, openaimodel.py:262-288; out is at the input's size, half of it (RES_DOWN) or twice it (RES_UP)
    void res(const LRes& R, const Act& xin, void* out) {
        const size_t mark = ar.off;
        const bool film_on = net->film;
        const int Ho = R.updown == RES_DOWN ? xin.H / 2 : R.updown == RES_UP ? xin.H * 2 : xin.H;
        const int Wo = R.updown == RES_DOWN ? xin.W / 2 : R.updown == RES_UP ? xin.W * 2 : xin.W;
        const int HW = Ho * Wo;
        const size_t M = (size_t)nhyp * HW;
        void* t = alloc_act((size_t)nhyp * xin.H * xin.W * R.Cin);
        void* h = alloc_act(M * R.Cout);
        gn(R.n1, xin.p, t, xin.H * xin.W, 1, 1e-5f);
        Act x = xin;
        if (R.updown == RES_DOWN) {          // h = conv(avg_pool(silu(norm(x)))), x = avg_pool(x)
            void* tp = alloc_act(M * R.Cin);
            void* xp = alloc_act(M * R.Cin);
            pool(Act{t, R.Cin, xin.H, xin.W}, tp);
            pool(xin, xp);
            x = Act{xp, R.Cin, Ho, Wo};
            conv(R.c1, Act{tp, R.Cin, Ho, Wo}, h, Ho, Wo);
        } else if (R.updown == RES_UP) {     // h = conv(nearest(silu(norm(x)))) as the phase conv, x = nearest(x)
            void* xu = alloc_act(M * R.Cin);
            up2(xin, xu);
            x = Act{xu, R.Cin, Ho, Wo};
            conv(R.c1, Act{t, R.Cin, xin.H, xin.W}, h, Ho, Wo);
        } else {
            conv(R.c1, Act{t, R.Cin, x.H, x.W}, h, x.H, x.W);
        }
        const float* film = nullptr;                // FiLM rows [scale | shift]: emb == 0 -> the bias row, shared by every sample
        int film_stride = 0;
        if (film_on && !emb) film = R.emb_b;
        if (emb) {                                  // emb_layers(emb): added to h, or (FiLM) applied by the GroupNorm below
            const int ne = film_on ? 2 * R.Cout : R.Cout;
            float* e = alloc_f32((size_t)nhyp * ne);
            if (live()) {
                chk(launch_linear_naive(emb, R.emb_w, R.emb_b, e, nhyp, ne, net->emb_dim, 1, ne, s));
                if (!film_on) chk(launch_add_rowvec(net->sdt, h, h, e, (long long)M, HW, R.Cout, s));
            }
            if (film_on) { film = e; film_stride = ne; }
        }
        void* t2 = alloc_act(M * R.Cout);
        gn(R.n2, h, t2, HW, 1, 1e-5f, film, film_stride);
        const void* resid = x.p;
        if (R.has_skip) {
            void* sk = alloc_act(M * R.Cout);
            conv(R.skip, x, sk, x.H, x.W);
            resid = sk;
        }
        conv(R.c2, Act{t2, R.Cout, x.H, x.W}, out, x.H, x.W, resid);
        ar.off = mark;
    }
};

}  // namespace rb
}  // namespace nope
