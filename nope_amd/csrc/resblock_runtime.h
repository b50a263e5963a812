// Shared host-side pieces of the U-Net variants built on guided-diffusion's ResBlock (openaimodel.py:177-288 of the LDM code,
// guided_diffusion/u_net.py:141-253): the LDM cross-attention variant (ldm_runtime.hip) and the guided-diffusion variant
// (gd_runtime.hip).  Only what is ResBlock-specific lives here: the conv shape rule of these networks (3x3 PLAIN / UP2P layers take the
// NOPE_F16X2 second pack), loading a ResBlock (up / down, FiLM), and the forward pieces avg-pool 2x2, nearest x2 and the ResBlock itself.
// Everything else -- the loader core, the bump arena, conv / GroupNorm launches with the range tracking, the entry-point bodies -- is
// runtime_common.h.  A network handle derives from RtNet; its loader and forward derive from LoaderBase / FwdBase and add their
// attention blocks.
#pragma once
#include "runtime_common.h"

namespace nope {
namespace rb {

using namespace rt;

struct LRes { NormW n1, n2; PackedConv c1, c2, skip; bool has_skip = false; float *emb_w = nullptr, *emb_b = nullptr; int Cin = 0, Cout = 0;
              int updown = 0; };      // updown: 0, RES_DOWN or RES_UP (resblock_updown, openaimodel.py:224-231)
enum { RES_DOWN = 1, RES_UP = 2 };

// What the ResBlock code reads of a network handle, over rt::Net (dt / sdt / x2 / x2r / allocs)
struct RtNet : Net {
    int emb_dim = 0;        // width of the embedding the ResBlocks' emb_layers read (4 * model_channels)
    bool film = false;      // use_scale_shift_norm: emb_layers give (scale | shift), applied by the out_layers GroupNorm
    bool emb_zero = false;  // the embedding is zeros: emb_layers(emb) is its bias, folded into in_layers' conv bias at create time (no FiLM)
};

struct LoaderBase : LoaderCore {
    RtNet* net;
    LoaderBase(RtNet* n, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors) : LoaderCore(n->allocs, n->dt, s_, tensors, n_tensors, &n->x2r), net(n) {}
    // conv (4-d weight) or linear (2-d weight) packed for the implicit-GEMM kernel
    // (Cin_pad > Cin: the kernel sees Cin_pad input channels, the last ones zero -- the 4-channel latent of vae_cin_ldm.yaml padded
    //  to one 16-byte vector of the 16-bit modes)
    PackedConv conv(const std::string& pfx, int Cin, int Cout, int ksz, int mode, bool has_bias, bool linear = false, int Cin_pad = 0) {
        const int Ck = Cin_pad > Cin ? Cin_pad : Cin;
        const nope_tensor_desc* d = linear ? get(pfx + "weight", {Cout, Cin}) : get(pfx + "weight", {Cout, Cin, ksz, ksz});
        const bool second = net->x2 && !linear && ksz == 3 && (mode == NOPE_CONV_PLAIN || mode == NOPE_CONV_UP2P) && Ck == Cin && Cin % 32 == 0;
        return pack_conv(d, pfx, Cin, Ck, Cout, mode == NOPE_CONV_UP2P ? 4 : ksz * ksz, mode, has_bias, second);
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

struct FwdBase : FwdCore<RtNet> {
    const float* emb = nullptr;       // (nhyp, emb_dim) or null (zeros)
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
        gn(R.n1, 32, xin.p, t, xin.H * xin.W, 1, 1e-5f);
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
        gn(R.n2, 32, h, t2, HW, 1, 1e-5f, film, film_stride);
        const void* resid = x.p;
        if (R.has_skip) {
            void* sk = alloc_act(M * R.Cout);
            conv(R.skip, x, sk, x.H, x.W);
            resid = sk;
        }
        conv(R.c2, Act{t2, R.Cout, x.H, x.W}, out, x.H, x.W, with_resid(resid));
        ar.off = mark;
    }
};

}  // namespace rb
}  // namespace nope
