// Host-side runtime of the pose-conditioned U-Net: weight repacking (nope_unet_create) and
// the launch schedule of one forward over a batch of pose hypotheses (nope_unet_forward).
//
// Op order follows UNet.forward, u_net.py:160-198, exactly (mid block twice with shared
// weights :177-183, final_conv.0 without the embedding :154-157,197).  What differs is the
// execution model, chosen for MI355X:
//   * NHWC activations, every conv/linear an implicit GEMM on MFMA (kernels_gemm.hip);
//     torch.cat / nn.Upsample / Rearrange are folded into that kernel's loader, so none of
//     those tensors ever exists in HBM;
//   * all N pose hypotheses of a reference image run as ONE batch (n_hyp = B*N): at the 4x4
//     bottleneck a single hypothesis has only 16 GEMM rows, the batch has 16*n_hyp;
//   * pose-independent work is done once per reference image instead of once per template:
//     init_conv, the skip `r`, and conv+GroupNorm+SiLU of downs[0][0].block1 (the embedding is
//     only added after that activation, model_utils.py:272-276) -- the reference re-runs all
//     of it, and the ResNet encoder, N times (model.py:115,219);
//   * NOPE_SHARED_SPLIT (read per forward; bit 0 | bit 1, default 3, 0 = neither; f32 activation storage, x_rep > 1, maps of >= 2 x 2):
//     two 3x3 convs further down still multiplied per-reference data once per template.  Bit 0, downs[0][0].block2: its input is
//     u + e_n 1 with u per reference and e_n the block's embedding row, so conv2 = S + E[n][border class of the pixel] with S = conv2(u) +
//     bias per reference and E a 512 x 192 x 1728 f32 GEMM against the nine border-class weights; the per-template conv launch is gone and
//     the block's last GroupNorm forms S + E itself (kernels_norm.hip, the shared addend).  Bit 1, final_res_block.block1: its input is
//     cat(cur, r) with r per reference, so conv = conv(W[:, :C], cur) + Sr, Sr = conv(W[:, C:], r) + bias per reference; the per-template
//     launch has half the K and the GroupNorm that follows forms cur' + Sr.  Summation order changes, nothing else: the shared parts run
//     in f32 / bf16x3 even under NOPE_F16X2 (Fwd::resnet);
//   * NOPE_GN_EPI (read per forward; bit 0 | bit 1, default 3, 0 = neither; f32 activation storage in bf16x3 / f16x2): at the 16 x 16, 8 x 8 and
//     4 x 4 levels a ResnetBlock's 3x3 conv on the tap-resident kernel normalises its own output -- GroupNorm + SiLU (+ embedding row, + identity
//     residual) in its epilogue, the statistics formed in LDS by the workgroup that owns the samples -- so the GroupNorm pass over the tensor is
//     not launched.  Bit 0 = block1, bit 1 = block2 of blocks without a res_conv that no attention follows.  Bit-identical to the two launches,
//     taken only where conv_plan grants it (Fwd::conv_gn_self);
//   * the 19 per-block `Linear(SiLU(c))` embeddings (model_utils.py:261-265,274-275) are one
//     f32 GEMM against the row-concatenated weights;
//   * a bump arena over caller-provided workspace: no allocation, no host sync, one stream.
//
// The loader core, the arena, the forward's bookkeeping and the bodies of the entry points are the ones every network runtime uses
// (runtime_common.h); the conv shape rule (space-to-depth, ConvTranspose2d, cin_scale, which layers take the NOPE_F16X2 pack) and the
// launch schedule (fused statistics, PreNorm, the tail fusion) are this file's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "runtime_common.h"

using namespace nope;
using rt::Act;
using rt::FwdReq;
using rt::NormW;
using rt::PackedConv;

namespace {

struct Res {
    PackedConv c1, c2, res; NormW n1, n2; bool has_res = false; int emb_off = -1;
    // NOPE_SHARED_SPLIT (see the file header), f32 activation storage only:
    float* c2_cls = nullptr;       // downs[0][0]: block2's nine border-class weights [9 * Cout][Cout] f32 (launch_pack_conv_classes)
    PackedConv c1_hyp, c1_ref;     // final_res_block: block1 split by input channels -- the up path's half (no bias) and the skip r's half (with the bias)
};
// PreNorm's GroupNorm(1) is folded into the qkv conv: gamma into the packed weights, c0 = W beta, c1 = W gamma
// (f32 [3*heads*dim_head]); mean / rstd enter in the conv epilogue.
struct LinAttn { NormW pre, post; PackedConv qkv, out; float *c0 = nullptr, *c1 = nullptr; };
struct Attn { NormW pre; PackedConv qkv, out; float *c0 = nullptr, *c1 = nullptr; };
struct Level { Res r0, r1; LinAttn attn; PackedConv resample; };

}  // namespace

// One captured launch sequence of a forward: valid for exactly this (workspace, shape, output type); x, pose and the output are
// staged through the workspace so that the caller's pointers stay out of the graph.
struct UGraph { void* ws; size_t ws_bytes; int n_hyp, n_src, H, W, out_dt; hipGraphExec_t exec; };

struct nope_unet : rt::Net {      // (dt / sdt / x2 / x2r / allocs: rt::Net, runtime_common.h)
    nope_unet_config cfg;
    int dims[9];
    int classes = 0;
    PackedConv init_conv, final_conv1;
    float* final_w_raw = nullptr;      // final_conv.1.weight as stored, [out_dim][u_net_dim] f32: the fused tail (gn_apply_proj, kernels_norm.hip)
    Level downs[8], ups[8];
    Res mid1, mid2, final_res, final_conv0;
    Attn mid_attn;
    float *pose_w0 = nullptr, *pose_b0 = nullptr, *pose_w2 = nullptr, *pose_b2 = nullptr;
    float *emb_w = nullptr, *emb_b = nullptr;
    int emb_total = 0;
    // optional per-launch timing of the implicit-GEMM kernel (bench.py roofline leg)
    struct Ev { hipEvent_t a, b; double flops, bytes; nope_conv_launch_info info; };
    mutable bool profile = false;
    mutable std::vector<Ev> evs;
    // hipGraph cache for SMALL hypothesis batches (the reference evaluates on 26 / 91 / 341 templates, shapeNet.py:252-263): there
    // a forward is ~150 dependent launches of 5-20 us each and the gaps between them are a visible share of the pass.
    // OPT-IN (nope_unet_graph_limit, or NOPE_UNET_GRAPH read once at create time; default 0 = never): measured +-0 against direct launches
    // (profiles/r03c_small_banks.txt -- a 64-hypothesis pass is GPU-bound, not launch-bound), and a cached graph freezes the launch plan
    // it was captured with (the NOPE_* tuning variables are not part of the key).  The cache is guarded by a mutex: ctypes callers
    // have released the GIL.
    mutable std::vector<UGraph> graphs;
    mutable bool graphs_ok = true;           // cleared when capture is unavailable: direct launches from then on
    mutable std::mutex graph_mu;
    mutable int graph_split = -1;            // NOPE_SHARED_SPLIT | NOPE_RES_TAIL << 2 | NOPE_GN_EPI << 4 | NOPE_HALO_PADSKIP << 6 the cached graphs were captured under
    mutable int graph_replays = 0;           // forwards served by a graph replay since create (tests assert the path really ran)
    long long graph_max = 0;                 // largest n_hyp * H * W that replays a graph; 0 = off
};

namespace {

struct Loader : rt::LoaderCore {
    nope_unet* net;
    Loader(nope_unet* n, hipStream_t s_, const nope_tensor_desc* tensors, int n_tensors) : LoaderCore(n->allocs, n->dt, s_, tensors, n_tensors, &n->x2r), net(n) {}
    // (ksz 4 with UP2P: the weight is a ConvTranspose2d(4, 2, 1)'s, [Cin][Cout][4][4], repacked into the same four phase sets)
    // (Cin_pad > Cin: the kernel sees Cin_pad input channels, the last ones zero -- a latent whose channel count is not a whole 16-byte
    //  vector, e.g. a 4-channel VAE latent, zero-padded at pack time and in the NHWC input)
    PackedConv conv(const std::string& pfx, int Cin, int Cout, int ksz, int mode, bool has_bias, const float* cin_scale = nullptr, int Cin_pad = 0) {
        const int Csrc = Cin;
        if (Cin_pad > Cin) Cin = Cin_pad;
        const bool convT = mode == NOPE_CONV_UP2P && ksz == 4;
        const nope_tensor_desc* d = mode == NOPE_CONV_DOWN2 ? get(pfx + "weight", {Cout, (int64_t)Cin * 4, 1, 1})
                                    : convT             ? get(pfx + "weight", {Cin, Cout, 4, 4})
                                                        : get(pfx + "weight", {Cout, Csrc, ksz, ksz});
        // NOPE_F16X2: every layer a ping-pong kernel may run (3x3, 1x1, space-to-depth, phase convs) carries the second pack; launch_conv
        // takes it when the launch's shape lands on one of them
        const bool second = net->x2 && (mode == NOPE_CONV_PLAIN || mode == NOPE_CONV_DOWN2 || mode == NOPE_CONV_UP2P) &&
                            (ksz == 3 || ksz == 1 || mode != NOPE_CONV_PLAIN) && !cin_scale && Csrc == Cin && Cin % 32 == 0;
        return pack_conv(d, pfx, Csrc, Cin, Cout, (mode == NOPE_CONV_DOWN2 || mode == NOPE_CONV_UP2P) ? 4 : ksz * ksz, mode, has_bias, second,
                         convT ? 16 : 0, -1, cin_scale);
    }
    // NOPE_SHARED_SPLIT, create time.  The nine border-class weights of a 3x3 conv as a 1x1 GEMM weight [9 * Cout][Cin] f32 (Res::c2_cls):
    float* conv_classes(const std::string& pfx, int Cin, int Cout) {
        const nope_tensor_desc* d = get(pfx + "weight", {Cout, Cin, 3, 3});
        float* out = (float*)dmalloc((size_t)9 * Cout * Cin * 4);
        if (d && out) chk(launch_pack_conv_classes(d->data, out, Cout, Cin, s));
        return out;
    }
    // ... and a 3x3 conv over input channels [c0, c0 + Cin) of a stored [Cout][Ctot][3][3] weight (Res::c1_hyp / c1_ref): those rows are
    // staged contiguously and packed like any conv's (`second`: with the NOPE_F16X2 pack and a layer id of its own)
    PackedConv conv_cin_range(const std::string& pfx, int Ctot, int c0, int Cin, int Cout, bool has_bias, bool second) {
        const nope_tensor_desc* d = get(pfx + "weight", {Cout, Ctot, 3, 3});
        const size_t rb = (size_t)Cin * 9 * 4;
        float* st = (float*)tmalloc((size_t)Cout * rb);
        if (!d || !st) return PackedConv();
        if (hipMemcpy2DAsync(st, rb, d->data + (size_t)c0 * 9, (size_t)Ctot * 9 * 4, rb, (size_t)Cout, hipMemcpyDeviceToDevice, s) != hipSuccess) chk(NOPE_ERR_LAUNCH);
        nope_tensor_desc sd = *d;
        sd.data = st;
        return pack_conv(&sd, pfx, Cin, Cin, Cout, 9, NOPE_CONV_PLAIN, has_bias, second && net->x2 && Cin % 32 == 0);
    }
    // qkv conv of an attention block with its PreNorm folded in (see LinAttn)
    void prenorm_qkv(const std::string& p, int C, int N, NormW& pre, PackedConv& qkv, float*& c0, float*& c1) {
        pre = norm(p + "fn.norm.", C);
        qkv = conv(p + "fn.fn.to_qkv.", C, N, 1, NOPE_CONV_PLAIN, false, pre.gamma);
        c0 = (float*)dmalloc((size_t)N * 4);
        c1 = (float*)dmalloc((size_t)N * 4);
        const nope_tensor_desc* w = get(p + "fn.fn.to_qkv.weight", {N, C, 1, 1});
        if (w && c0 && c1 && pre.beta && qkv.w) {
            int e = launch_linear_naive(pre.beta, w->data, nullptr, c0, 1, N, C, 0, N, s);
            if (!e) e = launch_rowsum(net->dt, qkv.w, c1, N, C, s);
            chk(e);
        }
    }
    Res res(const std::string& pfx, int Cin, int Cout, bool use_emb, std::vector<std::pair<std::string, int>>& embs) {
        Res r;
        r.c1 = conv(pfx + "block1.proj.", Cin, Cout, 3, NOPE_CONV_PLAIN, true);
        r.n1 = norm(pfx + "block1.norm.", Cout);
        r.c2 = conv(pfx + "block2.proj.", Cout, Cout, 3, NOPE_CONV_PLAIN, true);
        r.n2 = norm(pfx + "block2.norm.", Cout);
        r.has_res = Cin != Cout;
        if (r.has_res) r.res = conv(pfx + "res_conv.", Cin, Cout, 1, NOPE_CONV_PLAIN, true);
        if (use_emb) { r.emb_off = net->emb_total; net->emb_total += Cout; embs.push_back({pfx + "mlp.1.", Cout}); }
        return r;
    }
};

// Fused GroupNorm statistics of a conv output: [n][blocks][C][2] column sums per row block (null: the conv cannot emit them --
// the GroupNorm takes its own statistics pass)
struct Stats { float* cs = nullptr; int blocks = 0; };

// The optional inputs of Fwd::conv over rt::ConvOpts (resid, out_nchw / out_dt, track_out), set by name.
struct ConvOpts : rt::ConvOpts {
    Stats* stats = nullptr;                          // also emit the column statistics of the output when this launch can
    const float *c0 = nullptr, *c1 = nullptr;        // PreNorm folded into this (qkv) conv: see LinAttn
};
// The 1x1 conv that is the ONLY reader of a block's output (the U-Net's tail), for the block's last GroupNorm pass to take along.
struct ProjTail { const PackedConv* proj = nullptr; void* out = nullptr; int out_dt = NOPE_F32; };
// The optional inputs of Fwd::gn, set by name.
struct GnOpts {
    int x_rep = 1;                                   // x holds nhyp / x_rep samples
    int act = 1;                                     // SiLU
    int emb_off = -1;                                // + this block's row of the embedding (offset into emb_all)
    const void* resid = nullptr; int resid_rep = 1;  // + resid, each of its samples shared by resid_rep hypotheses
    Stats stats;                                     // the producing conv's column statistics: they only need folding
    float* out_stats = nullptr;                      // also emit the GroupNorm(1) partials of y (the next attention block's PreNorm)
    const GnShared* sh = nullptr;                    // the shared addend: x_eff = [x] + S [+ E]
    ProjTail tail;
};

// The shared core's bookkeeping (arena, error state) and the two halves of every conv launch and the end of every GroupNorm with their range
// tracking; conv / gn add what is this network's own: fused statistics, split-K scratch, PreNorm, profile events, the shared addend
struct Fwd : rt::FwdCore<nope_unet> {
    using Arena = rt::Arena;
    float* pn_partial = nullptr;   // (sum, sum sq) partials of the tensor that feeds the next attention block
    float* pn_ms = nullptr;        // its per-hypothesis (mean, rstd)
    const float* emb_all = nullptr;
    int pn_blocks = 0;             // entries per hypothesis of pn_partial as its last producer laid them out (gn_apply_blocks, or conv_tail_stat_blocks)
    int split = 0;                 // NOPE_SHARED_SPLIT of this forward: bit 0 = downs[0][0].block2, bit 1 = final_res_block.block1
    int gn_epi = 0;                // NOPE_GN_EPI of this forward: bit 0 = block1, bit 1 = block2 with an identity residual (conv_gn_self)

    // run `fn` as a forward over n samples (the per-reference launches: profiled, traced and range-tracked like every other)
    template <class F> void over(int n, F fn) { const int keep = nhyp; nhyp = n; fn(); nhyp = keep; }
    // ... on this view of an activation that rep hypotheses share: its samples, one each
    static Act per_ref(Act a) { a.rep = 1; return a; }
    static ConvOpts with_stats(Stats& st) { ConvOpts o; o.stats = &st; return o; }
    // a conv's packed weights without the NOPE_F16X2 pack: the per-reference launches stay on the three-pass kernels
    static PackedConv exact(PackedConv c) { c.w_x2 = nullptr; c.x2_id = -1; return c; }

    // out = conv(a [cat b]) (+bias) (+resid) over nhyp samples.  o.stats: the launch emits its output's column statistics when it can
    // (conv_stat_rows: whole 64-row blocks per sample on every kernel, 16 / 32-pixel maps on the small-tile kernel); the scratch comes
    // from the arena and lives until the caller's release.
    void conv(const PackedConv& c, const Act& a, const Act* b, void* out, int Ho, int Wo, const ConvOpts& o = ConvOpts()) {
        if (err != NOPE_OK) return;
        ConvArgs ca;
        if (!conv_args(ca, c, a, b, out, Ho, Wo, o)) return;
        if (o.c0) { ca.pn_ms = pn_ms; ca.pn_c0 = o.c0; ca.pn_c1 = o.c1; }
        if (o.stats) {
            const int sr = conv_stat_rows(net->dt, ca);
            if (sr > 0) {
                const int blocks = Ho * Wo / sr;
                ca.colstats = (float*)ar.alloc((size_t)nhyp * blocks * c.Cout * 2 * sizeof(float));
                if (!ca.colstats) { chk(NOPE_ERR_WORKSPACE); return; }
                ca.stat_rows = sr; *o.stats = Stats{ca.colstats, blocks};
            }
        }
        // few output tiles + long K (small hypothesis batches at the 4x4 level): deterministic split-K through a
        // scratch taken from the arena for the duration of the launch
        const size_t sk_mark = ar.off;
        if (!o.c0 && !o.out_nchw) {
            const int S = conv_splitk_factor(net->dt, ca);      // (1 for a conv that emits its statistics itself)
            if (S > 1) {
                ca.splitk_bytes = (size_t)S * nhyp * Ho * Wo * c.Cout * 4;
                ca.splitk_ws = ar.alloc(ca.splitk_bytes);
                if (!ca.splitk_ws) { chk(NOPE_ERR_WORKSPACE); return; }
            }
        }
        struct Release { Arena& a; size_t m; ~Release() { a.off = m; } } release{ar, sk_mark};
        if (!live()) return;               // workspace-size query: only the arena bookkeeping above matters
        const ConvLaunch L = conv_tracked(ca, c, a, b, o.track_out);
        if (!net->profile) { chk(launch_conv(L, s)); return; }
        nope_unet::Ev ev;
        hipEventCreate(&ev.a); hipEventCreate(&ev.b);
        ev.flops = L.flops;   // executed MACs (UP2P: 4 taps per output pixel; padding taps of small maps skipped)
        // algorithmic HBM bytes: every input, weight and output element exactly once (+ the residual a GroupNorm tail normalises: a pass of its own before)
        ev.bytes = ((double)(nhyp / a.rep) * a.H * a.W * a.C + (b ? (double)(nhyp / b->rep) * a.H * a.W * b->C : 0.0) +
                    (double)c.Cout * c.ntaps * c.Cin * (c.mode == NOPE_CONV_UP2P ? 4 : 1) + (double)nhyp * Ho * Wo * c.Cout * (o.gn ? 2 : 1)) * (double)es;
        ev.info = nope_conv_launch_info{0.0, ev.flops, ev.bytes, L.kind, c.mode, c.ntaps, c.Cin, c.Cout, a.H, a.W, nhyp,
                                        net->dt != NOPE_BF16X3 ? 1 : L.x2 ? 2 : 3, L.posmajor ? 1 : 0};
        hipEventRecord(ev.a, s);
        chk(launch_conv(L, s));
        hipEventRecord(ev.b, s);
        net->evs.push_back(ev);
    }
    // y = act(GN(x)) [+emb] [+resid]; x holds nhyp / o.x_rep samples.
    // o.tail: GroupNorm + SiLU + residual + that 1x1 conv in one pass (launch_gn_apply_proj: y is not written) when the arguments
    // qualify; returns whether it did -- the caller launches the conv itself otherwise
    bool gn(const NormW& nm, int G, const void* x, void* y, int HW, const GnOpts& o = GnOpts()) {
        if (!live()) return false;
        const int nx = nhyp / o.x_rep;
        int nch = 1;
        GnApplyArgs ga;
        ga.x = x; ga.nhyp = nhyp; ga.HW = HW; ga.C = nm.C; ga.G = G; ga.x_rep = o.x_rep;
        if (o.sh) {
            // the shared addend (GnApplyArgs::sh_*): x_eff = [x] + S [+ E] is formed by the statistics pass and by the apply pass, never stored
            ga.sh_s = o.sh->S; ga.sh_e = o.sh->E; ga.sh_rep = o.sh->s_rep; ga.sh_H = o.sh->H; ga.sh_W = o.sh->W;
            nch = gn_stats_chunks(HW, nm.C, net->sdt);
            chk(launch_gn_stats_shared(net->sdt, ga, gn_partial, nch, s));
        } else if (o.stats.cs) {
            // Every gn_apply workgroup folds its sample's column statistics itself (stats.blocks * C * 8 bytes out of L2 per workgroup; a
            // separate fold launch costs ~7 us + a kernel boundary).  Round 2 measured the inline fold +0.25 ms per 512-hypothesis step
            // (one thread per group then); with the wave-wide group sums of round 4 it is -0.02 .. -0.05 ms there and -0.2 ms at 64
            // hypotheses (profiles/r04o_fold_inline_ab.txt): always on.  NOPE_GN_FOLD_INLINE = most re-read bytes per launch (0 = never).
            const long long fold_inline_max = NOPE_ENV_LL("NOPE_GN_FOLD_INLINE", 1ll << 50);
            const long long refold = (long long)nhyp * gn_apply_blocks(HW, nm.C, net->sdt, nhyp) * o.stats.blocks * nm.C * 8;
            if (refold <= fold_inline_max) { ga.colstats = o.stats.cs; ga.stat_blocks = o.stats.blocks; }
            else chk(launch_gn_fold(o.stats.cs, gn_partial, nx, o.stats.blocks, nm.C, G, s));
        } else {
            nch = gn_stats_chunks(HW, nm.C, net->sdt);
            chk(launch_gn_stats(net->sdt, x, gn_partial, nx, HW, nm.C, G, nch, s));
        }
        ga.y = y; ga.partial = gn_partial; ga.nchunk = nch; ga.gamma = nm.gamma; ga.beta = nm.beta; ga.act = o.act;
        if (o.emb_off >= 0) { ga.emb = emb_all + o.emb_off; ga.emb_stride = net->emb_total; }
        ga.resid = o.resid; ga.resid_rep = o.resid_rep; ga.out_stats = o.out_stats;
        if (o.tail.proj && o.tail.out && net->final_w_raw) {
            ga.proj_w = net->final_w_raw; ga.proj_b = o.tail.proj->bias; ga.proj_cout = o.tail.proj->Cout; ga.proj_out = o.tail.out; ga.proj_out_dt = o.tail.out_dt;
        }
        return gn_apply(ga);
    }

    // The end of a ResnetBlock with a res_conv in ONE pass: res_conv reads the raw output of block2's conv (`out`) as its residual, normalises and
    // activates it on the way in (ConvArgs::gn_*: gn_apply's arithmetic, the same bits) and stores the block's output over it -- res_conv's own output
    // is never written and the apply pass never runs: 4 of 6 activation tensors moved.  Taken where conv_plan puts res_conv on the per-tap ping-pong
    // kernel with the lean epilogue (the only one that has the tail), f32 storage in a split-precision mode (the fast SiLU), whole 64-row blocks per
    // sample, groups of whole 4-channel chunks.  NOPE_RES_TAIL: bit 0 = blocks not followed by attention (bit-identical to the three passes), bit 1 =
    // blocks followed by attention (the GroupNorm(1) partials of the output come from the epilogue's wave tiles: another summation order, results
    // move at rounding level); 0 = the three passes everywhere.  Default 1: bit 1 measures another 0.2 ms per 512-template step, but a forward would
    // then depend on NOPE_EPILOGUE_LEAN in its last bits, which tests/test_conv_stream.py forbids.  False: not taken, nothing launched.
    bool res_tail(const Res& R, const Act& a, const Act* b, void* out, const Stats& st, bool next_is_attention) {
        const int HW = a.H * a.W, G = net->cfg.groups, C = R.res.Cout;
        if (!(NOPE_ENV("NOPE_RES_TAIL", 1) & (next_is_attention ? 2 : 1))) return false;
        if (net->sdt != NOPE_F32 || net->dt == NOPE_F32 || !st.cs || HW < 64 || HW % 64 || G < 1 || C % G || (C / G) % 4) return false;
        ConvOpts o;
        o.resid = out; o.track_out = true;
        o.gn = &R.n2; o.gn_G = G; o.gn_ms = gn_partial;      // (gn_partial: free between block1's GroupNorm and the next one; [nhyp][G][2] fits its [nhyp][16][G][2])
        if (next_is_attention) o.tail_stats = pn_partial;
        ConvArgs ca;
        if (err != NOPE_OK || !conv_args(ca, R.res, a, b, out, a.H, a.W, o) || conv_plan(net->dt, ca).err != NOPE_OK) return false;
        if (live()) chk(launch_gn_colstats_finalize(st.cs, gn_partial, nhyp, st.blocks, C, G, HW, 1e-5f, s));
        conv(R.res, a, b, out, a.H, a.W, o);
        if (next_is_attention) pn_blocks = conv_tail_stat_blocks(HW, C);
        return true;
    }

    // A ResnetBlock's conv with its OWN GroupNorm in ONE launch: out = SiLU(GN(conv(a [cat b]))) [+ the embedding row] [+ resid] (ConvArgs::gn_self).  At the
    // 16 x 16, 8 x 8 and 4 x 4 levels a 256-row tile of the tap-resident kernel holds whole samples and a 192-column tile whole groups, so the workgroup
    // that computes a tile forms (mean, rstd) itself and the GroupNorm pass that would read the tensor back is never launched -- with that pass's
    // fold order and arithmetic: bit-identical to the two launches.  Taken where conv_plan grants it (asked, never assumed: split-K launches, the
    // 32 x 32 level, the other kernels and NOPE_EPILOGUE_LEAN=0 say no); a workspace-size query always sizes the two launches.  False: not taken,
    // nothing launched.  NOPE_GN_EPI: bit 0 = block1 (conv -> GN -> SiLU -> + emb), bit 1 = block2 with an identity residual (no res_conv, not
    // followed by attention, no fused projection, no shared addend); 0 = the two launches everywhere.
    bool conv_gn_self(const PackedConv& c, const Act& a, const Act* b, void* out, const NormW& nm, int emb_off, const void* resid) {
        const int G = net->cfg.groups;
        if (!live() || net->sdt != NOPE_F32 || net->dt == NOPE_F32 || G < 1 || c.Cout % G) return false;
        ConvOpts o;
        o.gn = &nm; o.gn_G = G; o.gn_self = true; o.gn_resid = resid; o.track_out = true;
        if (emb_off >= 0) { o.gn_emb = emb_all + emb_off; o.gn_emb_stride = net->emb_total; }
        ConvArgs ca;
        if (!conv_args(ca, c, a, b, out, a.H, a.W, o)) return false;
        if (conv_splitk_factor(net->dt, ca) > 1 || conv_plan(net->dt, ca).err != NOPE_OK) return false;
        conv(c, a, b, out, a.H, a.W, o);
        return true;
    }

    // ResnetBlock, model_utils.py:271-279.  `a` may be shared by a.rep hypotheses (rep > 1 only for the very first block, where b == nullptr).
    // `next_is_attention`: also emit the GroupNorm(1) partials of the block's output into pn_partial.
    // tail: fused into the block's last pass where gn() can; returns whether it was (then `out` holds the un-normalised conv output and
    // must not be read)
    bool resnet(const Res& R, const Act& a, const Act* b, bool use_emb, void* out, bool next_is_attention = false, const ProjTail& tail = ProjTail()) {
        const int HW = a.H * a.W, G = net->cfg.groups;
        const size_t M = (size_t)nhyp * HW;
        const size_t mark = ar.off;
        const int emb_off = use_emb ? R.emb_off : -1;
        const bool f32_acts = net->sdt == NOPE_F32 && a.H >= 2 && a.W >= 2;      // (S and E are f32; a 1-pixel-wide map has no nine border classes)
        GnOpts g2;                     // the block's last GroupNorm: + the block's input (or res_conv of it)
        g2.resid = a.p; g2.resid_rep = a.rep; g2.out_stats = next_is_attention ? pn_partial : nullptr;
        if (next_is_attention) pn_blocks = gn_apply_blocks(HW, R.n2.C, net->sdt, nhyp);
        if (a.rep > 1 && !b && (split & 1) && !R.has_res && R.c2_cls && use_emb && f32_acts) {
            // downs[0][0] with NOPE_SHARED_SPLIT bit 0: block2 convolves u + e_n 1, u = SiLU(GN(block1(x0))) per reference and e_n this block's
            // embedding row, constant over the map.  By linearity conv2(u + e_n 1)[p] = S[p] + E[n][cls(p)]: S = conv2(u) + bias once per
            // reference, E = e_n against the nine border-class weights (one small f32 GEMM).  The per-hypothesis conv, the pass that expanded
            // u to nhyp copies and the read of the conv output by its GroupNorm are gone; x_eff is formed inside the two GroupNorm passes.
            const int ns = nhyp / a.rep, C = R.c2.Cout;
            void* t1s = alloc_act((size_t)ns * HW * C);
            void* us = alloc_act((size_t)ns * HW * C);
            float* S = (float*)alloc_act((size_t)ns * HW * C);
            float* erows = alloc_f32((size_t)nhyp * C);
            float* E = alloc_f32((size_t)nhyp * 9 * C);
            over(ns, [&] {
                GnOpts g1;
                conv(R.c1, per_ref(a), nullptr, t1s, a.H, a.W, with_stats(g1.stats));
                gn(R.n1, G, t1s, us, HW, g1);
                conv(exact(R.c2), Act{us, C, a.H, a.W}, nullptr, S, a.H, a.W);
            });
            if (live()) {
                if (hipMemcpy2DAsync(erows, (size_t)C * 4, emb_all + emb_off, (size_t)net->emb_total * 4, (size_t)C * 4, (size_t)nhyp, hipMemcpyDeviceToDevice, s) != hipSuccess)
                    chk(NOPE_ERR_LAUNCH);
                ConvArgs ea;   // E[nhyp][9 * C] = e @ Wcls^T, exact-f32 MFMA as emb_all
                ea.src1 = erows; ea.C1 = C; ea.w = R.c2_cls; ea.out = E; ea.Cout = 9 * C; ea.nhyp = nhyp;
                chk(launch_conv(NOPE_F32, ea, s));
            }
            const GnShared sh{S, E, a.rep, a.H, a.W};
            g2.sh = &sh;
            gn(R.n2, G, /*x: S + E alone*/ nullptr, out, HW, g2);
            ar.off = mark;
            return false;
        }
        void* t1 = alloc_act(M * R.c1.Cout);
        GnOpts g1;                     // block1's GroupNorm: + the embedding row, in place
        g1.emb_off = emb_off;
        if (b && b->rep > 1 && a.rep == 1 && (split & 2) && R.c1_hyp.w && R.c1_ref.w && f32_acts) {
            // final_res_block with NOPE_SHARED_SPLIT bit 1: block1 convolves cat(cur, r), r = x0 per reference.  By linearity over the input
            // channels conv(W, cat(cur, r)) = conv(W[:, :C1], cur) + Sr, Sr = conv(W[:, C1:], r) + bias once per reference: the per-hypothesis
            // launch has half the K.  The epilogue's column statistics no longer see the whole GroupNorm input: a statistics pass forms cur' + Sr.
            const int ns = nhyp / b->rep;
            float* Sr = (float*)alloc_act((size_t)ns * HW * R.c1.Cout);
            over(ns, [&] { conv(exact(R.c1_ref), per_ref(*b), nullptr, Sr, a.H, a.W); });
            conv(R.c1_hyp, a, nullptr, t1, a.H, a.W);
            const GnShared sh{Sr, nullptr, b->rep, a.H, a.W};
            g1.sh = &sh;
            gn(R.n1, G, t1, t1, HW, g1);
        } else if (a.rep > 1 && !b) {
            // pose-independent prefix: conv + GN statistics once per reference sample
            const int ns = nhyp / a.rep;
            void* t1s = alloc_act((size_t)ns * HW * R.c1.Cout);
            over(ns, [&] { conv(R.c1, per_ref(a), nullptr, t1s, a.H, a.W, with_stats(g1.stats)); });
            g1.x_rep = a.rep;
            gn(R.n1, G, t1s, t1, HW, g1);
        } else if (!((gn_epi & 1) && conv_gn_self(R.c1, a, b, t1, R.n1, emb_off, nullptr))) {
            conv(R.c1, a, b, t1, a.H, a.W, with_stats(g1.stats));
            gn(R.n1, G, t1, t1, HW, g1);
        }
        if ((gn_epi & 2) && !R.has_res && !b && !next_is_attention && !tail.proj && a.rep == 1 &&
            conv_gn_self(R.c2, Act{t1, R.c1.Cout, a.H, a.W}, nullptr, out, R.n2, -1, a.p)) { ar.off = mark; return false; }
        conv(R.c2, Act{t1, R.c1.Cout, a.H, a.W}, nullptr, out, a.H, a.W, with_stats(g2.stats));
        if (R.has_res) {
            void* t3 = alloc_act(M * R.res.Cout);      // (allocated under the one-pass form too: the workspace of a shape does not depend on NOPE_RES_TAIL)
            if (!tail.proj && res_tail(R, a, b, out, g2.stats, next_is_attention)) { ar.off = mark; return false; }
            conv(R.res, a, b, t3, a.H, a.W);
            g2.resid = t3; g2.resid_rep = 1;
        } else if (b) { chk(NOPE_ERR_ARG); }
        g2.tail = tail;
        const bool fused = gn(R.n2, G, out, out, HW, g2);
        ar.off = mark;
        return fused;
    }

    // PreNorm folded into the qkv conv: finalize (mean, rstd) of x from the producer's partials, then
    // qkv = rstd * ((W gamma) x - mean * c1) + c0 in the conv epilogue -- x is read once, never re-written.
    void qkv_prenorm(const PackedConv& qkvw, const float* c0, const float* c1, const Act& x, void* qkv) {
        if (!live()) return;
        const int HW = x.H * x.W;
        chk(launch_gn_finalize(pn_partial, pn_ms, nhyp, pn_blocks, (float)HW * (float)x.C, 1e-5f, s));
        ConvOpts o; o.c0 = c0; o.c1 = c1;
        conv(qkvw, x, nullptr, qkv, x.H, x.W, o);
    }

    // Residual(PreNorm(LinearAttention)), model_utils.py:198-204,226-234,393-418.  x must come from
    // resnet(..., next_is_attention = true).
    void linattn(const LinAttn& L, const Act& x, void* out) {
        const int HW = x.H * x.W, heads = net->cfg.heads, dh = net->cfg.dim_head;
        const size_t M = (size_t)nhyp * HW;
        const size_t mark = ar.off;
        void* y = alloc_act(M * x.C);
        void* qkv = alloc_act(M * 3 * heads * dh);
        void* a = alloc_act(M * heads * dh);
        qkv_prenorm(L.qkv, L.c0, L.c1, x, qkv);
        if (live()) { chk(launch_linattn(net->sdt, qkv, a, nhyp, HW, heads, dh, s)); x2.overwritten(a); }
        GnOpts post;                   // GroupNorm(1) without SiLU, + x
        conv(L.out, Act{a, heads * dh, x.H, x.W}, nullptr, y, x.H, x.W, with_stats(post.stats));
        post.act = 0; post.resid = x.p;
        gn(L.post, 1, y, out, HW, post);
        ar.off = mark;
    }

    // Residual(PreNorm(Attention)), model_utils.py:367-390
    void attn(const Attn& A, const Act& x, void* out) {
        const int HW = x.H * x.W, heads = net->cfg.heads, dh = net->cfg.dim_head;
        const size_t M = (size_t)nhyp * HW;
        const size_t mark = ar.off;
        void* qkv = alloc_act(M * 3 * heads * dh);
        void* a = alloc_act(M * heads * dh);
        qkv_prenorm(A.qkv, A.c0, A.c1, x, qkv);
        if (live()) { chk(launch_attn(net->sdt, qkv, a, nhyp, HW, heads, dh, s)); x2.overwritten(a); }
        ConvOpts o; o.resid = x.p; o.track_out = true;
        conv(A.out, Act{a, heads * dh, x.H, x.W}, nullptr, out, x.H, x.W, o);
        ar.off = mark;
    }
};

// dry: a workspace-size query -- all of the arena bookkeeping, none of the launches; the arena's peak goes to *peak
int run_forward(const nope_unet* net, const FwdReq& q, void* ws, size_t ws_bytes, hipStream_t s, bool dry = false, size_t* peak = nullptr) {
    const nope_unet_config& cfg = net->cfg;
    const int L = cfg.n_levels, n_src = q.n_src, n_hyp = q.n_hyp, H = q.H, W = q.W;
    Fwd f;
    f.begin(net, n_hyp, ws, ws_bytes, s, dry);
    f.split = q.split;
    f.gn_epi = NOPE_ENV("NOPE_GN_EPI", 3) & 3;
    const int HW = H * W;
    const int* dims = net->dims;

    // ---- persistent buffers ------------------------------------------------------------------
    const int cin_k = net->init_conv.Cin;         // latent channels rounded up to 8
    void* x_in = f.alloc_act((size_t)n_src * HW * cin_k);
    void* x0 = f.alloc_act((size_t)n_src * HW * dims[0]);
    float* c0 = (float*)f.ar.alloc((size_t)n_hyp * net->classes * 4);
    float* c1 = (float*)f.ar.alloc((size_t)n_hyp * net->classes * 4);
    float* emb_all = (float*)f.ar.alloc((size_t)n_hyp * net->emb_total * 4);
    f.gn_partial = (float*)f.ar.alloc((size_t)n_hyp * 16 * (cfg.groups > 1 ? cfg.groups : 1) * 2 * 4);
    f.pn_partial = (float*)f.ar.alloc((size_t)n_hyp * 64 * 2 * 4);
    f.pn_ms = (float*)f.ar.alloc((size_t)n_hyp * 2 * 4);
    f.emb_all = emb_all;
    size_t cur_elems = 0;
    for (int l = 0; l <= L; ++l) {   // every tensor handed from one stage to the next
        const int rd = l < L ? l : L - 1;                 // down-path / bottleneck outputs
        const int ru = l > 0 ? l - 1 : 0;                 // up-path outputs (dims[l] at one level finer)
        const size_t e1 = (size_t)n_hyp * (HW >> (2 * rd)) * dims[l];
        const size_t e2 = l < L ? (size_t)n_hyp * (HW >> (2 * ru)) * dims[l] : 0;
        if (e1 > cur_elems) cur_elems = e1;
        if (e2 > cur_elems) cur_elems = e2;
    }
    void* curbuf[2] = {f.alloc_act(cur_elems), f.alloc_act(cur_elems)};
    void* hbuf[16];
    for (int l = 0; l < L; ++l) {
        const size_t e = (size_t)n_hyp * (HW >> (2 * l)) * dims[l];
        hbuf[2 * l] = f.alloc_act(e);
        hbuf[2 * l + 1] = f.alloc_act(e);
    }
    if (!dry && (!c0 || !c1 || !emb_all || !f.gn_partial || !f.pn_partial || !f.pn_ms)) f.chk(NOPE_ERR_WORKSPACE);
    if (f.err) return f.err;

    // ---- input + pose embedding ----------------------------------------------------------------
    if (f.live()) {
        f.chk(launch_nchw_to_nhwc(net->sdt, q.x, x_in, n_src, cin_k, HW, s, cfg.channels));
        if (cfg.pose_mlp_layers == 0) f.chk(launch_pos_emb(q.pose, c0, n_hyp, cfg.pose_dim, net->classes, s));   // u_net.py:73-76
        else f.chk(launch_linear_naive(q.pose, net->pose_w0, net->pose_b0, c0, n_hyp, net->classes, cfg.pose_dim, 0, net->classes, s));
        const float* c = c0;
        if (cfg.pose_mlp_layers == 2) {
            f.chk(launch_linear_naive(c0, net->pose_w2, net->pose_b2, c1, n_hyp, net->classes, net->classes, 2, net->classes, s));
            c = c1;
        }
        float* sc = (c == c0) ? c1 : c0;
        f.chk(launch_silu_f32(c, sc, (size_t)n_hyp * net->classes, s));
        ConvArgs ea;   // emb_all[n_hyp][emb_total] = SiLU(c) @ W_all^T + b_all, exact-f32 MFMA
        ea.src1 = sc; ea.C1 = net->classes; ea.w = net->emb_w; ea.bias = net->emb_b; ea.out = emb_all;
        ea.Cout = net->emb_total; ea.nhyp = n_hyp;
        f.chk(launch_conv(NOPE_F32, ea, s));
    }
    f.over(n_src, [&] { f.conv(net->init_conv, Act{x_in, cin_k, H, W}, nullptr, x0, H, W); });      // once per reference sample
    Act r0{x0, dims[0], H, W, q.x_rep};
    ConvOpts tracked; tracked.track_out = true;      // the resampling convs: their outputs go straight into f16x2 convs
    Act cur = r0;
    int slot = 0;

    // ---- down path ---------------------------------------------------------------------------------
    for (int l = 0; l < L; ++l) {
        const Level& D = net->downs[l];
        Act h1{hbuf[2 * l], dims[l], cur.H, cur.W};
        Act h2{hbuf[2 * l + 1], dims[l], cur.H, cur.W};
        f.resnet(D.r0, cur, nullptr, true, h1.p);
        {
            const size_t mark = f.ar.off;
            Act t{f.alloc_act((size_t)n_hyp * cur.H * cur.W * dims[l]), dims[l], cur.H, cur.W};
            f.resnet(D.r1, h1, nullptr, true, t.p, /*next_is_attention=*/true);
            f.linattn(D.attn, t, h2.p);
            f.ar.off = mark;
        }
        Act nxt{curbuf[slot], dims[l + 1], cur.H, cur.W};
        if (l < L - 1) { nxt.H = cur.H / 2; nxt.W = cur.W / 2; }
        f.conv(D.resample, h2, nullptr, nxt.p, nxt.H, nxt.W, tracked);
        cur = nxt;
        slot ^= 1;
    }
    // ---- bottleneck, applied twice with the same weights (u_net.py:177-183) ---------------------------
    for (int it = 0; it < 2; ++it) {
        const size_t mark = f.ar.off;
        const size_t e = (size_t)n_hyp * cur.H * cur.W * cur.C;
        Act a{f.alloc_act(e), cur.C, cur.H, cur.W};
        Act b{f.alloc_act(e), cur.C, cur.H, cur.W};
        f.resnet(net->mid1, cur, nullptr, true, a.p, /*next_is_attention=*/true);
        f.attn(net->mid_attn, a, b.p);
        Act c{curbuf[slot], cur.C, cur.H, cur.W};
        f.resnet(net->mid2, b, nullptr, true, c.p);
        f.ar.off = mark;
        cur = c;
        slot ^= 1;
    }
    // ---- up path --------------------------------------------------------------------------------------
    for (int l = 0; l < L; ++l) {
        const Level& U = net->ups[l];
        const int r = L - 1 - l;
        Act h2{hbuf[2 * r + 1], dims[r], cur.H, cur.W};
        Act h1{hbuf[2 * r], dims[r], cur.H, cur.W};
        const size_t mark = f.ar.off;
        const size_t e = (size_t)n_hyp * cur.H * cur.W * dims[r + 1];
        Act a{f.alloc_act(e), dims[r + 1], cur.H, cur.W};
        Act b{f.alloc_act(e), dims[r + 1], cur.H, cur.W};
        f.resnet(U.r0, cur, &h2, true, a.p);
        f.resnet(U.r1, a, &h1, true, b.p, /*next_is_attention=*/true);
        f.linattn(U.attn, b, a.p);
        Act nxt{curbuf[slot], dims[r], cur.H, cur.W};
        if (l < L - 1) { nxt.H = cur.H * 2; nxt.W = cur.W * 2; }
        f.conv(U.resample, a, nullptr, nxt.p, nxt.H, nxt.W, tracked);
        f.ar.off = mark;
        cur = nxt;
        slot ^= 1;
    }
    // ---- head --------------------------------------------------------------------------------------------
    {
        const size_t mark = f.ar.off;
        const size_t e = (size_t)n_hyp * HW * cfg.u_net_dim;
        Act a{f.alloc_act(e), cfg.u_net_dim, H, W};
        Act b{f.alloc_act(e), cfg.u_net_dim, H, W};
        f.resnet(net->final_res, cur, &r0, true, a.p);
        // final_conv = ResnetBlock -> Conv2d(dim, out_dim, 1) (u_net.py:154-157,197): the 1x1 conv rides in the block's last GroupNorm pass in the
        // split-precision modes (NOPE_FINAL_FUSED=0: its own launch, as in the other modes)
        if (!f.resnet(net->final_conv0, a, nullptr, false, b.p, false, ProjTail{&net->final_conv1, q.out, q.out_dtype})) {
            ConvOpts o; o.out_nchw = 1; o.out_dt = q.out_dtype;
            f.conv(net->final_conv1, b, nullptr, q.out, H, W, o);
        }
        f.ar.off = mark;
    }
    if (f.tracking())      // the forward's verdict and, if a layer left its window, NaNs over its output -- device side, no synchronisation (x2_range.h)
        f.chk(f.x2.finish(q.out, (size_t)n_hyp * cfg.out_dim * HW * (size_t)(q.out_dtype == NOPE_F32 ? 4 : 2), q.out_dtype));
    if (peak) *peak = f.ar.peak;
    return f.err;
}

}  // namespace

extern "C" {

int nope_unet_create(const nope_unet_config* cfg, const nope_tensor_desc* tensors, int n_tensors, nope_stream_t stream,
                     nope_unet** out) {
    if (!cfg || !tensors || !out || n_tensors <= 0) return NOPE_ERR_ARG;
    if (cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->groups < 1 || cfg->heads < 1 || cfg->dim_head != 32) return NOPE_ERR_UNSUPPORTED;
    if (!dt_is_compute(cfg->compute_dtype)) return NOPE_ERR_UNSUPPORTED;
    if (cfg->pose_mlp_layers < 0 || cfg->pose_mlp_layers > 2) return NOPE_ERR_UNSUPPORTED;   // 0 = "posEncoding" (no parameters)
    if (cfg->pose_mlp_layers == 0 && (cfg->pose_dim < 1 || (cfg->u_net_dim * 4) % (2 * cfg->pose_dim) || cfg->u_net_dim * 4 / cfg->pose_dim < 4)) return NOPE_ERR_UNSUPPORTED;
    if (cfg->u_net_dim % 8 || cfg->channels < 1 || cfg->out_dim < 1 || cfg->u_net_dim % cfg->groups) return NOPE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    nope_unet* net = new nope_unet();
    net->cfg = *cfg;
    net->x2 = cfg->compute_dtype == NOPE_F16X2;
    net->dt = dt_base(cfg->compute_dtype);
    net->sdt = dt_storage(net->dt);
    const int L = cfg->n_levels;
    net->dims[0] = cfg->u_net_dim;
    for (int l = 0; l < L; ++l) net->dims[l + 1] = cfg->u_net_dim * cfg->dim_mults[l];
    net->classes = cfg->u_net_dim * 4;
    net->graph_max = getenv("NOPE_UNET_GRAPH") ? atoll(getenv("NOPE_UNET_GRAPH")) : 0;
    const int* dims = net->dims;
    const int HD = cfg->heads * cfg->dim_head;

    Loader ld(net, s, tensors, n_tensors);
    std::vector<std::pair<std::string, int>> embs;

    if (cfg->pose_mlp_layers >= 1) {
        net->pose_w0 = ld.copy_f32("pose_mlp.0.weight", {net->classes, cfg->pose_dim});
        net->pose_b0 = ld.copy_f32("pose_mlp.0.bias", {net->classes});
    }
    if (cfg->pose_mlp_layers == 2) {
        net->pose_w2 = ld.copy_f32("pose_mlp.2.weight", {net->classes, net->classes});
        net->pose_b2 = ld.copy_f32("pose_mlp.2.bias", {net->classes});
    }
    net->init_conv = ld.conv("init_conv.", cfg->channels, dims[0], 3, NOPE_CONV_PLAIN, true, nullptr, (cfg->channels + 7) / 8 * 8);
    auto linattn = [&](const std::string& p, int C) {
        LinAttn a;
        ld.prenorm_qkv(p, C, 3 * HD, a.pre, a.qkv, a.c0, a.c1);
        a.out = ld.conv(p + "fn.fn.to_out.0.", HD, C, 1, NOPE_CONV_PLAIN, true);
        a.post = ld.norm(p + "fn.fn.to_out.1.", C);
        return a;
    };
    for (int l = 0; l < L; ++l) {
        const std::string p = "downs." + std::to_string(l) + ".";
        Level& D = net->downs[l];
        D.r0 = ld.res(p + "0.", dims[l], dims[l], true, embs);
        if (l == 0 && net->sdt == NOPE_F32) D.r0.c2_cls = ld.conv_classes(p + "0.block2.proj.", dims[0], dims[0]);
        D.r1 = ld.res(p + "1.", dims[l], dims[l], true, embs);
        D.attn = linattn(p + "2.", dims[l]);
        if (l < L - 1 && cfg->soft_up_down) D.resample = ld.conv(p + "3.", dims[l], dims[l + 1], 4, NOPE_CONV_STRIDE2, true);   // Conv2d(4, 2, 1)
        else if (l < L - 1) D.resample = ld.conv(p + "3.1.", dims[l], dims[l + 1], 1, NOPE_CONV_DOWN2, true);
        else D.resample = ld.conv(p + "3.", dims[l], dims[l + 1], 3, NOPE_CONV_PLAIN, true);
    }
    net->mid1 = ld.res("mid_block1.", dims[L], dims[L], true, embs);
    ld.prenorm_qkv("mid_attn.", dims[L], 3 * HD, net->mid_attn.pre, net->mid_attn.qkv, net->mid_attn.c0, net->mid_attn.c1);
    net->mid_attn.out = ld.conv("mid_attn.fn.fn.to_out.", HD, dims[L], 1, NOPE_CONV_PLAIN, true);
    net->mid2 = ld.res("mid_block2.", dims[L], dims[L], true, embs);
    for (int l = 0; l < L; ++l) {
        const int r = L - 1 - l;
        const std::string p = "ups." + std::to_string(l) + ".";
        Level& U = net->ups[l];
        U.r0 = ld.res(p + "0.", dims[r + 1] + dims[r], dims[r + 1], true, embs);
        U.r1 = ld.res(p + "1.", dims[r + 1] + dims[r], dims[r + 1], true, embs);
        U.attn = linattn(p + "2.", dims[r + 1]);
        if (l < L - 1 && cfg->soft_up_down) U.resample = ld.conv(p + "3.", dims[r + 1], dims[r], 4, NOPE_CONV_UP2P, true);   // ConvTranspose2d(4, 2, 1)
        else if (l < L - 1) U.resample = ld.conv(p + "3.1.", dims[r + 1], dims[r], 3, NOPE_CONV_UP2P, true);   // 4 phase 2x2 convs
        else U.resample = ld.conv(p + "3.", dims[r + 1], dims[r], 3, NOPE_CONV_PLAIN, true);
    }
    net->final_res = ld.res("final_res_block.", cfg->u_net_dim * 2, cfg->u_net_dim, true, embs);
    if (net->sdt == NOPE_F32) {
        const int C = cfg->u_net_dim;
        net->final_res.c1_hyp = ld.conv_cin_range("final_res_block.block1.proj.", 2 * C, 0, C, C, false, true);
        net->final_res.c1_ref = ld.conv_cin_range("final_res_block.block1.proj.", 2 * C, C, C, C, true, false);
    }
    net->final_conv0 = ld.res("final_conv.0.", cfg->u_net_dim, cfg->u_net_dim, false, embs);
    net->final_conv1 = ld.conv("final_conv.1.", cfg->u_net_dim, cfg->out_dim, 1, NOPE_CONV_PLAIN, true);
    net->final_w_raw = ld.copy_f32("final_conv.1.weight", {cfg->out_dim, cfg->u_net_dim, 1, 1});
    if (dims[0] != cfg->u_net_dim) ld.fail("init_dim");

    // row-concatenated embedding linears
    net->emb_w = (float*)ld.dmalloc((size_t)net->emb_total * net->classes * 4);
    net->emb_b = (float*)ld.dmalloc((size_t)net->emb_total * 4);
    int off = 0;
    for (auto& e : embs) {
        const nope_tensor_desc* w = ld.get(e.first + "weight", {e.second, net->classes});
        const nope_tensor_desc* b = ld.get(e.first + "bias", {e.second});
        if (w && b && net->emb_w && net->emb_b) {
            ld.copy_d2d(net->emb_w + (size_t)off * net->classes, w->data, (size_t)e.second * net->classes * 4);
            ld.copy_d2d(net->emb_b + off, b->data, (size_t)e.second * 4);
        }
        off += e.second;
    }
    ld.init_x2();
    return rt::finish_create(ld, "nope_unet_create", net, nope_unet_destroy, out);
}

int nope_unet_profile(nope_unet* net, int enable) {
    if (!net) return NOPE_ERR_ARG;
    for (auto& e : net->evs) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    net->evs.clear();
    net->profile = enable != 0;
    return NOPE_OK;
}

int nope_unet_profile_read(nope_unet* net, int* n_launches, double* total_ms, double* total_flops, double* total_bytes) {
    if (!net || !n_launches || !total_ms || !total_flops || !total_bytes) return NOPE_ERR_ARG;
    double ms = 0.0, fl = 0.0, by = 0.0;
    for (auto& e : net->evs) {
        if (hipEventSynchronize(e.b) != hipSuccess) return NOPE_ERR_LAUNCH;
        float t = 0.f;
        if (hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) return NOPE_ERR_LAUNCH;
        ms += t; fl += e.flops; by += e.bytes;
    }
    *n_launches = (int)net->evs.size(); *total_ms = ms; *total_flops = fl; *total_bytes = by;
    return NOPE_OK;
}

int nope_unet_profile_launches(nope_unet* net, nope_conv_launch_info* out, int max, int* n) {
    if (!net || !n || (max > 0 && !out)) return NOPE_ERR_ARG;
    int i = 0;
    for (auto& e : net->evs) {
        if (i < max) {
            if (hipEventSynchronize(e.b) != hipSuccess) return NOPE_ERR_LAUNCH;
            float t = 0.f;
            if (hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) return NOPE_ERR_LAUNCH;
            out[i] = e.info;
            out[i].ms = t;
        }
        ++i;
    }
    *n = i;
    return NOPE_OK;
}

// ---- NOPE_F16X2 activation ranges: the poll / range check / switch every tracked network shares (runtime_common.h, x2_range.h) -------------------
// (a cached hipGraph replays the same kernels and pointers; the shifts live in device memory: a poll leaves nothing to rebuild)
int nope_unet_x2_poll(nope_unet* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return rt::x2_poll(net, stream, n_out_of_range, n_adjusted, max_abs); }
int nope_unet_x2_range_check(nope_unet* net, nope_stream_t stream, int* n_out_of_range, int* n_adjusted, float* max_abs) { return rt::x2_range_check(net, stream, n_out_of_range, n_adjusted, max_abs); }

int nope_unet_x2_enable(nope_unet* net, int on) {
    if (!net) return NOPE_ERR_ARG;
    std::lock_guard<std::mutex> lock(net->graph_mu);
    if (net->x2r.off != (on == 0)) {           // the launch plan changes: cached graphs are stale
        for (const UGraph& g : net->graphs) hipGraphExecDestroy(g.exec);
        net->graphs.clear();
    }
    return rt::x2_enable(net, on);
}

int nope_unet_x2_shifts(const nope_unet* net, int* shifts, int max, int* n) {
    if (!net || !n || (max > 0 && !shifts)) return NOPE_ERR_ARG;
    return net->x2r.shifts(shifts, max, n);
}

int nope_unet_graph_limit(nope_unet* net, long long max_hyp_pixels) {
    if (!net || max_hyp_pixels < 0) return NOPE_ERR_ARG;
    std::lock_guard<std::mutex> lock(net->graph_mu);
    net->graph_max = max_hyp_pixels;
    return NOPE_OK;
}

int nope_unet_graph_replays(const nope_unet* net) {
    if (!net) return NOPE_ERR_ARG;
    std::lock_guard<std::mutex> lock(net->graph_mu);
    return net->graph_replays;
}

void nope_unet_destroy(nope_unet* net) {
    if (!net) return;
    for (const UGraph& g : net->graphs) hipGraphExecDestroy(g.exec);
    for (auto& e : net->evs) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    rt::free_device(net->allocs, &net->x2r);
    delete net;
}

static int check_shape(const nope_unet* net, int n_hyp, int n_src, int x_rep, int H, int W) {
    if (!net || n_hyp <= 0 || n_src <= 0 || x_rep <= 0 || (long long)n_src * x_rep != n_hyp || H <= 0 || W <= 0) return NOPE_ERR_ARG;
    const int f = 1 << (net->cfg.n_levels - 1);
    if (H % f || W % f) return NOPE_ERR_UNSUPPORTED;
    if ((H / f) * (W / f) > 64) return NOPE_ERR_UNSUPPORTED;   // bottleneck attention tile
    return NOPE_OK;
}

// Workspace = [staged x | staged pose | staged output (largest element type) | activation arena]
static size_t unet_stage_bytes(const nope_unet* net, int n_hyp, int n_src, int H, int W, size_t& xb, size_t& pb, size_t& ob) {
    xb = align_up((size_t)n_src * net->cfg.channels * H * W * 4, 256);
    pb = align_up((size_t)n_hyp * net->cfg.pose_dim * 4, 256);
    ob = align_up((size_t)n_hyp * net->cfg.out_dim * H * W * 4, 256);
    return xb + pb + ob;
}

size_t nope_unet_workspace_bytes(const nope_unet* net, int n_hyp, int n_src, int H, int W) {
    if (!net || n_src <= 0 || n_hyp % n_src) return 0;
    if (check_shape(net, n_hyp, n_src, n_hyp / n_src, H, W) != NOPE_OK) return 0;
    FwdReq q; q.n_src = n_src; q.x_rep = n_hyp / n_src; q.n_hyp = n_hyp; q.H = H; q.W = W;
    size_t peak = 0;
    for (q.split = 0; q.split <= 3; q.split += 3) {      // NOPE_SHARED_SPLIT is read per forward: the workspace holds either schedule
        size_t pk = 0;
        run_forward(net, q, nullptr, 0, nullptr, true, &pk);
        if (pk > peak) peak = pk;
    }
    size_t xb, pb, ob;
    return unet_stage_bytes(net, n_hyp, n_src, H, W, xb, pb, ob) + align_up(peak, 256) + 256;
}

int nope_unet_forward(const nope_unet* net, const float* x, int n_src, int x_rep, const float* pose, int n_hyp, int H, int W,
                      void* out, int out_dtype, void* workspace, size_t workspace_bytes, nope_stream_t stream) {
    int e = check_shape(net, n_hyp, n_src, x_rep, H, W);
    if (e) return e;
    if (!x || !pose || !out || !workspace) return NOPE_ERR_ARG;
    if (out_dtype != NOPE_F32 && out_dtype != NOPE_BF16 && out_dtype != NOPE_F16) return NOPE_ERR_UNSUPPORTED;
    unsigned char* base;
    size_t avail;
    if (!rt::workspace_base(workspace, workspace_bytes, base, avail)) return NOPE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    size_t xb, pb, ob;
    const size_t sb = unet_stage_bytes(net, n_hyp, n_src, H, W, xb, pb, ob);
    // Opt-in (net->graph_max > 0): batches of at most that many hypothesis-pixels replay a captured launch sequence; everything else
    // launches directly.
    // (NOPE_F16X2 with range tracking launches directly: the per-forward table of the verdict kernel is a host-to-device copy)
    const bool want_graph = net->graph_max > 0 && net->graphs_ok && !net->profile && avail > sb && (long long)n_hyp * H * W <= net->graph_max &&
                            !(net->x2 && net->x2r.active());
    rt::x2_poll_before_forward(net, stream);
    const int split = NOPE_ENV("NOPE_SHARED_SPLIT", 3) & 3;
    FwdReq q; q.x = x; q.pose = pose; q.out = out; q.out_dtype = out_dtype;
    q.n_src = n_src; q.x_rep = x_rep; q.n_hyp = n_hyp; q.H = H; q.W = W; q.split = split;
    if (!want_graph) return run_forward(net, q, base, avail, s);
    std::lock_guard<std::mutex> lock(net->graph_mu);
    const int plan_key = split | (NOPE_ENV("NOPE_RES_TAIL", 1) & 3) << 2 | (NOPE_ENV("NOPE_GN_EPI", 3) & 3) << 4 |
                         (NOPE_ENV("NOPE_HALO_PADSKIP", 1) != 0) << 6;      // the switches read per forward that change the launch sequence, and the conv planner's NOPE_HALO_PADSKIP (another kernel form in the captured launches)
    if (net->graph_split != plan_key) {        // the launch plan changes: cached graphs are stale (as in nope_unet_x2_enable)
        for (const UGraph& g : net->graphs) hipGraphExecDestroy(g.exec);
        net->graphs.clear();
        net->graph_split = plan_key;
    }

    float* x_s = (float*)base;
    float* pose_s = (float*)(base + xb);
    void* out_s = base + xb + pb;
    unsigned char* arena = base + sb;
    const size_t arena_bytes = avail - sb;
    const UGraph* hit = nullptr;
    for (const UGraph& g : net->graphs)
        if (g.ws == workspace && g.ws_bytes == workspace_bytes && g.n_hyp == n_hyp && g.n_src == n_src && g.H == H && g.W == W && g.out_dt == out_dtype) { hit = &g; break; }
    if (!hit) {
        {   // dry pass: fail on a too-small arena BEFORE a capture is open
            size_t peak = 0;
            e = run_forward(net, q, nullptr, 0, nullptr, true, &peak);
            if (e) return e;
            if (align_up(peak, 256) > arena_bytes) return NOPE_ERR_WORKSPACE;
        }
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            net->graphs_ok = false;
            return run_forward(net, q, base, avail, s);
        }
        FwdReq staged = q;      // the graph reads and writes the staging buffers: the caller's pointers stay out of it
        staged.x = x_s; staged.pose = pose_s; staged.out = out_s;
        e = run_forward(net, staged, arena, arena_bytes, s);
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(s, &graph);
        hipGraphExec_t exec = nullptr;
        if (e != NOPE_OK || ce != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            if (graph) hipGraphDestroy(graph);
            (void)hipGetLastError();
            net->graphs_ok = false;
            return e != NOPE_OK ? e : run_forward(net, q, base, avail, s);
        }
        hipGraphDestroy(graph);
        if (net->graphs.size() >= 16) { hipGraphExecDestroy(net->graphs.front().exec); net->graphs.erase(net->graphs.begin()); }
        net->graphs.push_back(UGraph{workspace, workspace_bytes, n_hyp, n_src, H, W, out_dtype, exec});
        hit = &net->graphs.back();
    }
    const size_t out_bytes = (size_t)n_hyp * net->cfg.out_dim * H * W * (size_t)(out_dtype == NOPE_F32 ? 4 : 2);
    if (hipMemcpyAsync(x_s, x, (size_t)n_src * net->cfg.channels * H * W * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (hipMemcpyAsync(pose_s, pose, (size_t)n_hyp * net->cfg.pose_dim * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (hipGraphLaunch(hit->exec, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    ++net->graph_replays;
    if (hipMemcpyAsync(out, out_s, out_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    return NOPE_OK;
}

}  // extern "C"
