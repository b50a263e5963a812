// Host-side core of the five network runtimes (unet_runtime.hip, encoder_runtime.hip, ldm_runtime.hip, gd_runtime.hip, vae_runtime.hip):
// what each of them needs whatever its network looks like.
//   * PackedConv / NormW: a conv packed for the implicit-GEMM kernels, a norm's affine;
//   * Net: what the shared code reads of a network handle (compute / storage dtype, NOPE_F16X2 state, device allocations);
//   * LoaderCore: the state-dict table of a create call, device / staging allocations, copies, and the conv-packing skeleton every
//     network's conv() calls with its own shape rule.  Bound to the handle's `allocs` vector, not to a handle type;
//   * Arena / Act / FwdCore: the bump arena over the caller's workspace, an NHWC activation (with how many hypotheses share each of its
//     samples), and a forward's bookkeeping.  FwdCore holds the ONE copy of what every conv launch and every GroupNorm ends with under
//     the NOPE_F16X2 range tracking (x2_range.h): conv_args (sources, the second pack) and conv_tracked (conv_plan, consumes / produce /
//     overwritten), gn_apply (SiLU form, max |y| slot, launch, the fused 1x1 tail).  conv() / gn() are those and nothing more; the
//     U-Net's own conv / gn put a second source, statistics and split-K scratch, PreNorm and profile events between the same halves;
//   * ConvOpts / FwdReq: the optional inputs of a conv launch and one forward request, as structs whose fields are set by name;
//   * the bodies the extern "C" entry points share: workspace base alignment, the x2 poll / range-check / enable trio, the poll in
//     front of a forward, the tail of a create call, freeing a handle's device memory.
// ResBlock networks (LDM, guided diffusion) add resblock_runtime.h on top.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "conv_plan.h"      // (nope_common.h; ConvLaunch)
#include "x2_range.h"

namespace nope {
namespace rt {

// w_x2 / x2_id: NOPE_F16X2 only, the same weights in the f16 + MX-fp8 tile's layout and the layer's slot in the range table (x2_range.h)
struct PackedConv { void* w = nullptr; float* bias = nullptr; int Cin = 0, Cout = 0, ntaps = 1, mode = NOPE_CONV_PLAIN; void* w_x2 = nullptr; int x2_id = -1; };
struct NormW { float* gamma = nullptr; float* beta = nullptr; int C = 0; };

struct Net {
    int dt = NOPE_F32;      // compute dtype: what the conv kernels and the weight packing see
    int sdt = NOPE_F32;     // storage dtype of the activations: what every other kernel sees (NOPE_BF16X3 keeps f32 activations)
    bool x2 = false;        // NOPE_F16X2: dt = NOPE_BF16X3 everywhere, plus a second weight pack per layer the ping-pong kernels' f16 + MX-fp8 tile may run
    mutable X2Range x2r;    // ... and the activation-range tracking that keeps the tile inside its accurate window (x2_range.h)
    std::vector<void*> allocs;
};

struct LoaderCore {
    std::vector<void*>& allocs;      // the handle's device allocations (freed by its destroy)
    int dt;                          // compute dtype the weights are packed for
    hipStream_t s;
    X2Range* x2r;                    // where second packs register (null: the network never takes one)
    std::map<std::string, const nope_tensor_desc*> tab;
    int err = NOPE_OK;
    std::string missing;
    std::vector<void*> temps;        // staging buffers of create time, freed after its final synchronize

    LoaderCore(std::vector<void*>& allocs_, int dt_, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors, X2Range* x2r_ = nullptr)
        : allocs(allocs_), dt(dt_), s(s_), x2r(x2r_) {
        for (int i = 0; i < n_tensors; ++i)
            if (tensors[i].name) tab[tensors[i].name] = &tensors[i];
    }
    void fail(const std::string& n) { if (err == NOPE_OK) { err = NOPE_ERR_WEIGHT; missing = n; } }
    void chk(int e) { if (e != NOPE_OK && err == NOPE_OK) err = e; }
    const nope_tensor_desc* get(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = tab.find(name);
        if (it == tab.end() || !it->second->data || it->second->ndim != (int)shape.size()) { fail(name); return nullptr; }
        int i = 0;
        for (int64_t v : shape) if (it->second->shape[i++] != v) { fail(name); return nullptr; }
        return it->second;
    }
    void* dmalloc(size_t bytes, std::vector<void*>* owner = nullptr) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { chk(NOPE_ERR_ALLOC); return nullptr; }
        (owner ? *owner : allocs).push_back(p);
        return p;
    }
    void* tmalloc(size_t bytes) { return dmalloc(bytes, &temps); }
    void free_temps() { for (void* p : temps) hipFree(p); temps.clear(); }
    // device-to-device copy of a state-dict tensor at create time; a refused copy (bad pointer, wrong device) fails the create call itself,
    // not just the stream synchronisation that ends it
    void copy_d2d(void* dst, const void* src, size_t bytes) {
        if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) chk(NOPE_ERR_LAUNCH);
    }
    float* copy_f32(const std::string& name, std::initializer_list<int64_t> shape) {
        const nope_tensor_desc* d = get(name, shape);
        if (!d) return nullptr;
        size_t n = 1;
        for (int64_t v : shape) n *= (size_t)v;
        float* p = (float*)dmalloc(n * 4);
        if (p) copy_d2d(p, d->data, n * 4);
        return p;
    }
    NormW norm(const std::string& pfx, int C) {
        NormW n;
        n.C = C;
        n.gamma = copy_f32(pfx + "weight", {C});
        n.beta = copy_f32(pfx + "bias", {C});
        return n;
    }
    // The skeleton of every network's conv(): `d` is the weight the caller found under its own shape rule (null: reported already).
    // The kernel sees Cin input channels of which the stored weight has Csrc (the rest zero), ntaps taps in geometry `mode`.
    // pack_taps / pack_mode: what the packing kernels are told where that differs (a ConvTranspose2d source's 16 taps; a geometry
    // whose weights are laid out as another's); second_pack: the layer also gets the NOPE_F16X2 pack and a slot in the range table;
    // cin_scale / cout_scale: per-channel factors folded into the packed weights.
    PackedConv pack_conv(const nope_tensor_desc* d, const std::string& pfx, int Csrc, int Cin, int Cout, int ntaps, int mode, bool has_bias,
                         bool second_pack = false, int pack_taps = 0, int pack_mode = -1, const float* cin_scale = nullptr,
                         const float* cout_scale = nullptr) {
        PackedConv c;
        c.Cin = Cin; c.Cout = Cout; c.ntaps = ntaps; c.mode = mode;
        if (pack_taps <= 0) pack_taps = ntaps;
        if (pack_mode < 0) pack_mode = mode;
        if (d) {
            c.w = dmalloc((size_t)Cout * ntaps * Cin * (size_t)dt_es(dt) * (mode == NOPE_CONV_UP2P ? 4 : 1));
            if (c.w) chk(launch_pack_conv_w(dt, (const float*)d->data, c.w, Cout, Cin, pack_taps, pack_mode, s, cin_scale, cout_scale, Csrc));
            if (second_pack && x2r) {
                const size_t x2b = conv_w_x2_bytes(Cout, Cin, ntaps, mode);
                c.w_x2 = dmalloc(x2b);
                if (c.w_x2) { chk(launch_pack_conv_w_x2((const float*)d->data, c.w_x2, Cout, Cin, s, pack_taps, pack_mode)); c.x2_id = x2r->add_layer(c.w_x2, x2b); }
            }
        }
        if (has_bias) c.bias = copy_f32(pfx + "bias", {Cout});
        return c;
    }
    // after the last second pack: the range tracking's device / pinned buffers
    void init_x2() {
        if (err == NOPE_OK && x2r) chk(x2r->init([&](size_t bytes) { return dmalloc(bytes); }, s));
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
        if (dry) return (void*)(uintptr_t)(0x1000 + o);   // never dereferenced
        if (off > cap) return nullptr;
        return base + o;
    }
};

// rep: the tensor holds nhyp / rep samples, each shared by rep hypotheses of the forward that reads it
struct Act { void* p = nullptr; int C = 0, H = 0, W = 0, rep = 1; };

// The optional inputs of a conv launch, set by name.
struct ConvOpts {
    const void* resid = nullptr;            // added to the output (same layout)
    int out_nchw = 0, out_dt = NOPE_F32;    // the network's output conv: NCHW of type out_dt
    bool track_out = false;                 // the output goes straight into f16x2 convs: its epilogue records max |out| when it is one that can
                                            // (the wide NHWC epilogue); otherwise a later f16x2 consumer of `out` takes an absmax pass over it
    // GroupNorm tail on the residual (ConvArgs::gn_*): out = conv + SiLU(GN(resid)), the norm's affine, its groups, (mean, rstd) [nhyp][G][2] of resid
    // and, optionally, where the GroupNorm(1) partials of the output go (ConvArgs::tail_stats)
    const NormW* gn = nullptr; int gn_G = 0; const float* gn_ms = nullptr; float* tail_stats = nullptr;
    // The conv's own GroupNorm (ConvArgs::gn_self): out = SiLU(GN(conv)) [+ emb row] [+ gn_resid], the norm's affine in `gn`, its groups in gn_G
    bool gn_self = false; const float* gn_emb = nullptr; int gn_emb_stride = 0; const void* gn_resid = nullptr;
};
inline ConvOpts with_resid(const void* resid) { ConvOpts o; o.resid = resid; return o; }
inline ConvOpts to_nchw(int out_dt) { ConvOpts o; o.out_nchw = 1; o.out_dt = out_dt; return o; }

// One forward of a pose-conditioned network, as its entry point received it: out[j] = net(x[j / x_rep], pose[j]), n_hyp = n_src * x_rep.
// Filled once per entry point (a workspace-size query leaves the pointers null).
struct FwdReq {
    const float* x = nullptr; const float* pose = nullptr; void* out = nullptr;
    int out_dtype = NOPE_F32, n_src = 0, x_rep = 1, n_hyp = 0, H = 0, W = 0;
    int split = 0;      // the U-Net's NOPE_SHARED_SPLIT of this forward
};

// One forward over `nhyp` samples.  N: the handle, a Net.
template <class N> struct FwdCore {
    const N* net = nullptr;
    hipStream_t s = nullptr;
    Arena ar;
    int nhyp = 0, err = NOPE_OK;
    size_t es = 4;
    float* gn_partial = nullptr;
    X2Fwd x2;                         // NOPE_F16X2 range tracking of this forward (x2_range.h)

    void begin(const N* net_, int n, void* ws, size_t ws_bytes, hipStream_t s_, bool dry) {
        net = net_; s = s_; nhyp = n; es = (size_t)dt_es(net->dt);
        ar.base = (unsigned char*)ws; ar.cap = ws_bytes; ar.dry = dry;
        x2.r = &net->x2r; x2.s = s; x2.on = net->x2 && net->x2r.active() && !dry;
    }
    bool tracking() const { return x2.on && err == NOPE_OK; }
    void chk(int e) { if (e != NOPE_OK && err == NOPE_OK) err = e; }
    bool live() const { return !ar.dry && err == NOPE_OK; }      // false in a workspace-size query: only the arena bookkeeping matters
    void* alloc_act(size_t elems) {
        void* p = ar.alloc(elems * es);
        if (!p) chk(NOPE_ERR_WORKSPACE);
        return p;
    }
    float* alloc_f32(size_t n) {
        float* p = (float*)ar.alloc(n * 4);
        if (!p) chk(NOPE_ERR_WORKSPACE);
        return p;
    }
    // First half of every conv launch: the ConvArgs of out = conv(a [cat b]) (+bias) (+o.resid) over nhyp samples, on the layer's NOPE_F16X2
    // pack when it has one.  False (error latched, nothing else touched): the sources' channels are not the layer's.
    bool conv_args(ConvArgs& ca, const PackedConv& c, const Act& a, const Act* b, void* out, int Ho, int Wo, const ConvOpts& o) {
        if (a.C + (b ? b->C : 0) != c.Cin) { chk(NOPE_ERR_ARG); return false; }
        ca.src1 = a.p; ca.C1 = a.C; ca.rep1 = a.rep;
        if (b) { ca.src2 = b->p; ca.C2 = b->C; ca.rep2 = b->rep; }
        ca.Hs = a.H; ca.Ws = a.W; ca.Ho = Ho; ca.Wo = Wo;
        ca.mode = c.mode; ca.ntaps = c.ntaps; ca.w = c.w; ca.bias = c.bias; ca.resid = o.resid;
        ca.out = out; ca.Cout = c.Cout; ca.nhyp = nhyp; ca.out_nchw = o.out_nchw; ca.out_dt = o.out_dt;
        if (c.w_x2 && c.x2_id >= 0 && !net->x2r.off) { ca.w_x2 = c.w_x2; ca.x2_t_zero = net->x2r.t_zero(c.x2_id) ? 1 : 0; }
        if (o.gn) { ca.gn_ms = o.gn_ms; ca.gn_gamma = o.gn->gamma; ca.gn_beta = o.gn->beta; ca.gn_G = o.gn_G; ca.tail_stats = o.tail_stats; }
        if (o.gn && o.gn_self) { ca.gn_self = 1; ca.gn_emb = o.gn_emb; ca.gn_emb_stride = o.gn_emb_stride; ca.gn_resid = o.gn_resid; }
        return true;
    }
    // Second half: the plan of the filled ConvArgs (made once: the tracking, a profile and launch_conv read the same decisions), tracked -- a
    // two-pass launch makes its layer's shift follow its sources' maxima, a then b; the epilogue records max |out| (track_out, where the plan
    // can) or out's stale slot is dropped.  The caller launches what comes back.
    ConvLaunch conv_tracked(const ConvArgs& ca, const PackedConv& c, const Act& a, const Act* b, bool track_out) {
        ConvLaunch L = conv_plan(net->dt, ca);
        if (tracking()) {
            if (L.x2 && c.x2_id >= 0) {
                x2.consumes(c.x2_id, x2.slot_for(a.p, (size_t)(ca.nhyp / a.rep) * a.H * a.W * a.C));
                if (b) x2.consumes(c.x2_id, x2.slot_for(b->p, (size_t)(ca.nhyp / b->rep) * b->H * b->W * b->C));
                chk(x2.err);
            }
            if (track_out && L.records_out_amax) {
                const int sl = x2.produce(ca.out);
                if (sl >= 0) L.record_out_amax(x2.slot_ptr(sl));
            } else x2.overwritten(ca.out);
        }
        return L;
    }
    void conv(const PackedConv& c, const Act& a, void* out, int Ho, int Wo, const ConvOpts& o = ConvOpts()) {
        if (!live()) return;
        ConvArgs ca;
        if (conv_args(ca, c, a, nullptr, out, Ho, Wo, o)) chk(launch_conv(conv_tracked(ca, c, a, nullptr, o.track_out), s));
    }
    // The end of every GroupNorm: the SiLU form, y's range slot (the apply kernel records max |y|; records_max false, the FiLM instantiation: it
    // does not), the launch.  True: ga named a fused 1x1 tail (GnApplyArgs::proj_*) that qualified -- one pass, y not written, no maximum for it.
    bool gn_apply(GnApplyArgs& ga, bool records_max = true) {
        ga.fast_silu = net->dt != NOPE_F32 ? 1 : 0;      // (f32 storage of the split-precision modes: hardware exp / rcp; the f32 mode keeps expf and the division)
        const bool proj = ga.proj_out && gn_apply_proj_ok(net->sdt, ga);
        if (tracking()) {
            const int sl = records_max ? x2.produce(ga.y) : -1;
            if (sl >= 0) ga.amax_out = x2.slot_ptr(sl);
            if (!records_max || proj) x2.overwritten(ga.y);
        }
        chk(proj ? launch_gn_apply_proj(net->sdt, ga, s) : launch_gn_apply(net->sdt, ga, s));
        return proj;
    }
    // y = [silu](GroupNorm(G, eps)(x)) [FiLM]
    void gn(const NormW& nm, int G, const void* x, void* y, int HW, int act, float eps, const float* film = nullptr, int film_stride = 0) {
        if (!live()) return;
        const int nch = gn_stats_chunks(HW, nm.C, net->sdt);
        chk(launch_gn_stats(net->sdt, x, gn_partial, nhyp, HW, nm.C, G, nch, s));
        GnApplyArgs ga;
        ga.x = x; ga.y = y; ga.partial = gn_partial; ga.nchunk = nch; ga.gamma = nm.gamma; ga.beta = nm.beta;
        ga.nhyp = nhyp; ga.HW = HW; ga.C = nm.C; ga.G = G; ga.act = act; ga.eps = eps;
        ga.film = film; ga.film_stride = film_stride;
        gn_apply(ga, !film);
    }
};

// ---- bodies of the extern "C" entry points ----------------------------------------------------------------------------------------------
// The arena's base is the first 256-byte boundary inside the caller's workspace (nope_*_workspace_bytes reports the peak + 256 for it);
// false: not even that fits.
inline bool workspace_base(void* workspace, size_t bytes, unsigned char*& base, size_t& cap) {
    base = (unsigned char*)(((uintptr_t)workspace + 255) / 256 * 256);
    const size_t lost = (size_t)(base - (unsigned char*)workspace);
    if (bytes < lost) return false;
    cap = bytes - lost;
    return true;
}

// NOPE_F16X2 activation ranges (include/nope_hip.h: nope_unet_x2_poll / _x2_range_check / _x2_enable; x2_range.h).  The poll reads the
// verdicts that have arrived in mapped host memory since the previous poll -- no synchronisation -- and re-centres the shifts of the
// layers that were out of, or near the end of, their windows; the new shifts travel on `stream`, ahead of whatever is enqueued next.
template <class N> int x2_poll(N* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) {
    if (n_out_of_range) *n_out_of_range = 0;
    if (n_adjusted) *n_adjusted = 0;
    if (max_abs) *max_abs = 0.f;
    if (!net) return NOPE_ERR_ARG;
    if (!net->x2) return NOPE_OK;
    return net->x2r.poll((hipStream_t)stream, n_out_of_range, n_adjusted, max_abs);
}
// ... behind a synchronisation of `stream`: the verdicts of every forward issued on it so far.  NOPE_ERR_RANGE: at least one of them was out
// of range (its output is NaN); the shifts are re-centred -- issue it again.
template <class N> int x2_range_check(N* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) {
    if (!net) return NOPE_ERR_ARG;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return NOPE_ERR_LAUNCH;
    return x2_poll(net, stream, n_out_of_range, n_adjusted, max_abs);
}
template <class N> int x2_enable(N* net, int on) {
    if (!net) return NOPE_ERR_ARG;
    net->x2r.off = on == 0;
    return NOPE_OK;
}
// in front of a forward: verdicts that have arrived re-centre the shifts first
template <class N> void x2_poll_before_forward(const N* net, nope_stream_t stream) {
    if (net->x2 && net->x2r.active()) (void)net->x2r.poll((hipStream_t)stream, nullptr, nullptr, nullptr);
}

// The end of nope_<x>_create: wait for the packing kernels (the caller may free the sources), drop the staging buffers, hand the handle out
// or, on an error, name the tensor under the function `fn` and destroy it.
template <class N, class Destroy> int finish_create(LoaderCore& ld, const char* fn, N* net, Destroy destroy, N** out) {
    if (hipStreamSynchronize(ld.s) != hipSuccess) ld.chk(NOPE_ERR_LAUNCH);
    ld.free_temps();
    if (ld.err != NOPE_OK) {
        if (!ld.missing.empty()) fprintf(stderr, "%s: missing or mis-shaped tensor '%s'\n", fn, ld.missing.c_str());
        destroy(net);
        return ld.err;
    }
    *out = net;
    return NOPE_OK;
}

inline void free_device(std::vector<void*>& allocs, X2Range* x2r = nullptr) {
    for (void* p : allocs) hipFree(p);
    allocs.clear();
    if (x2r) x2r->destroy();
}

}  // namespace rt
}  // namespace nope
