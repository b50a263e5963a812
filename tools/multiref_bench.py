"""Multi-reference retrieval micro-benchmark.
    python tools/multiref_bench.py [--runs 4] [--reps 20] [--skip-step]
a. kernel: nope_multiref_similarity at 32 queries x R = 4 x 512 templates x 8 x 32 x 32, each bank type, against nope_similarity over the
   same bytes (the bank viewed as (32, 2048, ...)), alternating in one process: bytes/s and share of the 8 TB/s peak of both, their ratio.
b. step: PoseConditional.retrieve_multi for R = 1, 2, 4 at one 256 x 256 query and 512 poses in f16x2, next to generate_and_retrieve:
   ms per step and step(R) - R step(1), what fusion costs beyond the R U-Net passes.
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiref_bench needs an MI355X")
    kernel_bench(max(a.runs, 4), a.reps)
    if not a.skip_step:
        step_bench(max(a.runs, 4), a.step_reps)
