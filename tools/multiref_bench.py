"""Multi-reference retrieval micro-benchmark.
    python tools/multiref_bench.py [--runs 4] [--reps 20] [--skip-step]
a. kernel: nope_multiref_similarity at 32 queries x R = 4 x 512 templates x 8 x 32 x 32, each bank type, against nope_similarity over the
   same bytes (the bank viewed as (32, 2048, ...)), alternating in one process: bytes/s and share of the 8 TB/s peak of both, their ratio.
b. step: PoseConditional.retrieve_multi for R = 1, 2, 4 at one 256 x 256 query and 512 poses in f16x2, next to generate_and_retrieve:
   ms per step and step(R) - R step(1), what fusion costs beyond the R U-Net passes.
c. (--only xrep) c: forward_hypotheses with one source per hypothesis (x_rep = 1) over one shared source, 512 hypotheses.
d. (--only sparse) retrieve_multi_from_feat from embeddings, dense against max_refs = 1, 2 for R = 2, 4, 8 at 512 poses in f16x2, next to the
   single-reference retrieval: ms per step, alternating in one process.
e. (--only select-gather) nope_op_multiref_select and nope_op_multiref_gather alone at that size.
Device events around synchronised windows, after warm-up.  One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nope_amd import hip  # noqa: E402


def window_ms(fn, reps):
    """ms per call over one synchronised window of `reps` calls."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def spread(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def kernel_bench(runs, reps):
    B, R, N, C, h = 32, 4, 512, 8, 32
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        bank = torch.randn(B, R, N, C, h, h, device="cuda", dtype=torch.float16).to(dtype)
        flat = bank.view(B, R * N, C, h, h)
        q = torch.randn(B, C, h, h, device="cuda")
        w = torch.softmax(torch.randn(B, R, N, device="cuda"), dim=1).contiguous()
        out_f, out_s = torch.empty(B, N, device="cuda"), torch.empty(B, R * N, device="cuda")
        fused = lambda: hip.multiref_similarity(q, bank, w, out=out_f)
        single = lambda: hip.similarity(q, flat, out=out_s)
        for _ in range(10):
            fused()
            single()
        tf, ts = [], []
        for _ in range(runs):                      # alternating, in one process
            tf.append(window_ms(fused, reps))
            ts.append(window_ms(single, reps))
        bank_bytes = bank.numel() * bank.element_size()
        bf, bs = bank_bytes + w.numel() * 4 + B * N * 4, bank_bytes + B * R * N * 4
        gf, gs = [bf / t / 1e6 for t in tf], [bs / t / 1e6 for t in ts]
        print(json.dumps(dict(bench="kernel", dtype=str(dtype), B=B, R=R, N=N, C=C, H=h, W=h, runs=runs, reps=reps,
                              fused_gbs=spread(gf), single_gbs=spread(gs), fused_of_peak=spread(gf)["median"] / 8000.0,
                              single_of_peak=spread(gs)["median"] / 8000.0, ratio=spread(gf)["median"] / spread(gs)["median"])))


def step_bench(runs, reps):
    from nope_amd.harness import build_model, synthetic_batch
    model = build_model(2022, "f16x2", "f32", "cuda")
    ms = {}
    for R in (1, 2, 4):
        b = synthetic_batch(1, 512, 256, seed=2022, device="cuda", n_references=R)
        if R == 1:
            single = lambda: model.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"])
            for _ in range(3):
                single()
            ms["single"] = spread([window_ms(single, reps) for _ in range(runs)])
        for fusion in ("feature", "score"):
            multi = lambda: model.retrieve_multi(b["query"], b["references"], b["reference_poses"], b["template_poses"][:1], fusion=fusion)
            for _ in range(3):
                multi()
            ms[f"R{R}_{fusion}"] = spread([window_ms(multi, reps) for _ in range(runs)])
    beyond = {k: v["median"] - int(k[1]) * ms[f"R1_{k.split('_')[1]}"]["median"] for k, v in ms.items() if k.startswith("R")}
    print(json.dumps(dict(bench="step", mode="f16x2", size=256, poses=512, runs=runs, reps=reps, ms=ms, ms_beyond_R_single_passes=beyond)))


def xrep_bench(runs, reps):
    """c: what forward_hypotheses costs when every hypothesis brings its own source (x_rep = 1, the pose-independent work once per
    hypothesis) over one shared source (x_rep = N): 512 hypotheses on a 32 x 32 x 8 latent, f16x2, alternating."""
    from nope_amd.harness import build_model
    model = build_model(2022, "f16x2", "f32", "cuda")
    n = 512
    g = torch.Generator().manual_seed(2022)
    x = torch.randn(1, 8, 32, 32, generator=g).cuda()
    poses = torch.randn(1, n, 6, generator=g).cuda()
    x_own, poses_own = x.expand(n, -1, -1, -1).contiguous(), poses.view(n, 1, 6)
    out = torch.empty(n, 8, 32, 32, device="cuda")
    shared = lambda: model.u_net.forward_hypotheses(x, poses, out=out.view(1, n, 8, 32, 32))
    own = lambda: model.u_net.forward_hypotheses(x_own, poses_own, out=out.view(n, 1, 8, 32, 32))
    for _ in range(3):
        shared()
        own()
    ts, to = [], []
    for _ in range(runs):
        ts.append(window_ms(shared, reps))
        to.append(window_ms(own, reps))
    print(json.dumps(dict(bench="xrep", mode="f16x2", latent=[8, 32, 32], hypotheses=n, runs=runs, reps=reps, shared_ms=spread(ts), own_ms=spread(to),
                          shared_runs=ts, own_runs=to, c=spread(to)["median"] / spread(ts)["median"])))


def sparse_bench(runs, reps):
    from nope_amd.harness import build_model, synthetic_batch
    model = build_model(2022, "f16x2", "f32", "cuda")
    enc = model.u_net.encoder
    fns = {}
    for R in (2, 4, 8):
        b = synthetic_batch(1, 512, 256, seed=2022, device="cuda", n_references=R)
        q = enc.encode_image(b["query"], mode="mode")
        feats = enc.encode_image(b["references"][0], mode="mode")[None]
        P, T = b["reference_poses"], b["template_poses"][:1]
        if R == 2:
            rel = b["all_relativeR"]
            fns["single"] = lambda q=q, x=feats[:, 0].contiguous(), rel=rel: model.retrieval_from_feat(q, model.generate_templates_from_feat(x, rel))
        fns[f"R{R}_dense"] = lambda q=q, f=feats, P=P, T=T: model.retrieve_multi_from_feat(q, f, P, T)
        for M in (1, 2):
            fns[f"R{R}_M{M}"] = lambda q=q, f=feats, P=P, T=T, M=M: model.retrieve_multi_from_feat(q, f, P, T, max_refs=M)
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(runs):                          # alternating, in one process
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps))
    print(json.dumps(dict(bench="sparse", mode="f16x2", size=256, poses=512, runs=runs, reps=reps, ms={k: spread(v) for k, v in ms.items()})))


def select_gather_bench(runs, reps):
    """The two kernels' device time: back-to-back bare C calls (pointers taken once, outputs preallocated, no binding work) inside one
    window of device events.  `floor` is the same window over the gather of ONE 16-byte row: what a launch costs whatever it moves; a
    figure above the floor is the kernel's own time."""
    from nope_amd.harness import synthetic_batch
    dll = hip.lib().dll
    out = {}
    for R in (2, 8):
        b = synthetic_batch(1, 512, 32, seed=2022, device="cuda", n_references=R)
        P, T = b["reference_poses"].double().contiguous(), b["template_poses"][:1].double().contiguous()
        feats = torch.randn(1, R, 8, 32, 32, device="cuda")
        for M in (1, 2):
            sel = hip.op_multiref_select(T, P, max_refs=M)
            dst = torch.empty(1, M * 512, 8, 32, 32, device="cuda")
            sargs = (T.data_ptr(), 0, 512, P.data_ptr(), R, None, None, 512, M, 1, 0.5, 0, sel.src.data_ptr(), sel.all_relativeR.data_ptr(),
                     sel.weights.data_ptr(), None, sel.status.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
            gargs = (feats.data_ptr(), sel.src.data_ptr(), dst.data_ptr(), 1, R, M * 512, 8 * 32 * 32, torch.cuda.current_stream().cuda_stream)
            fargs = (feats.data_ptr(), sel.src.data_ptr(), dst.data_ptr(), 1, R, 1, 4, torch.cuda.current_stream().cuda_stream)
            select = lambda: dll.nope_op_multiref_select(*sargs)
            gather = lambda: dll.nope_op_multiref_gather(*gargs)
            floor = lambda: dll.nope_op_multiref_gather(*fargs)
            for _ in range(10):
                assert select() == 0 and gather() == 0 and floor() == 0
            ts, tg, tf = [], [], []
            for _ in range(runs):
                ts.append(window_ms(select, reps))
                tg.append(window_ms(gather, reps))
                tf.append(window_ms(floor, reps))
            out[f"R{R}_M{M}"] = dict(select_ms=spread(ts), gather_ms=spread(tg), floor_ms=spread(tf), gather_mib=2 * dst.numel() * 4 / 2 ** 20,
                                     gather_gbs=2 * dst.numel() * 4 / spread(tg)["median"] / 1e6)
    print(json.dumps(dict(bench="select-gather", poses=512, latent=[8, 32, 32], runs=runs, reps=reps, ms=out)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--only", default=None, choices=["xrep", "sparse", "select-gather"], help="one of the section 4.13 measurements alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiref_bench needs an MI355X")
    if a.only == "xrep":
        xrep_bench(max(a.runs, 4), a.step_reps)
        raise SystemExit(0)
    if a.only == "sparse":
        sparse_bench(max(a.runs, 4), a.step_reps)
        raise SystemExit(0)
    if a.only == "select-gather":
        select_gather_bench(max(a.runs, 4), a.reps)
        raise SystemExit(0)
    kernel_bench(max(a.runs, 4), a.reps)
    if not a.skip_step:
        step_bench(max(a.runs, 4), a.step_reps)
