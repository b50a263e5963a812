"""Occlusion-robust scoring micro-benchmark (DESIGN.md sections 4.14 and 9).
    python tools/robust_bench.py [--runs 5] [--reps 20] [--skip-step]
a. kernel: nope_robust_similarity at 32 queries x 512 templates x 8 x 32 x 32, each bank type, trim 0 and 0.25, with and without a mask
   (a seeded random mask of ~5/9 of the pixels), against nope_similarity over the same bytes, alternating in one process: bytes/s and share of
   the 8 TB/s peak of each setting, and its ratio to nope_similarity.  nope_similarity is the yardstick: its kernels are those of the commit
   before the robust score (kernels_retrieval.hip did not change, nor did their register counts).
b. step: PoseConditional.retrieve_robust (trim 0.25, masked and not) next to generate_and_retrieve at one 256 x 256 query, 512 poses, f16x2.
Device events around synchronised windows, after warm-up; every figure is reported with its span over the runs.  One JSON line per measurement."""
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
    B, N, C, h = 32, 512, 8, 32
    g = torch.Generator().manual_seed(2022)
    mask = (torch.rand(B, h, h, generator=g) < 5.0 / 9.0).to(torch.uint8).cuda()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        bank = torch.randn(B, N, C, h, h, device="cuda", dtype=torch.float16).to(dtype)
        q = torch.randn(B, C, h, h, device="cuda")
        out = torch.empty(B, N, device="cuda")
        fns = {"similarity": lambda: hip.similarity(q, bank, out=out)}
        for trim in (0.0, 0.25):
            for m, tag in ((None, "nomask"), (mask, "mask")):
                fns[f"robust_trim{trim}_{tag}"] = lambda trim=trim, m=m: hip.robust_similarity(q, bank, m, trim, out=out)
        for fn in fns.values():
            for _ in range(10):
                fn()
        ms = {k: [] for k in fns}
        for _ in range(runs):                      # alternating, in one process
            for k, fn in fns.items():
                ms[k].append(window_ms(fn, reps))
        nbytes = bank.numel() * bank.element_size() + B * N * 4
        res = {}
        for k, v in ms.items():
            gbs = [nbytes / t / 1e6 for t in v]
            res[k] = dict(ms=spread(v), gbs=spread(gbs), of_peak=spread(gbs)["median"] / 8000.0,
                          ratio_to_similarity=spread(ms["similarity"])["median"] / spread(v)["median"])
        print(json.dumps(dict(bench="kernel", lib=os.path.basename(hip.LIB_PATH), dtype=str(dtype), B=B, N=N, C=C, H=h, W=h, runs=runs, reps=reps,
                              mask_pixels=[int(x) for x in mask.flatten(1).sum(1)[:4].tolist()], settings=res)), flush=True)


def step_bench(runs, reps):
    from nope_amd.harness import build_model, occlude_queries, synthetic_batch
    model = build_model(2022, "f16x2", "f32", "cuda")
    b, vis = occlude_queries(synthetic_batch(1, 512, 256, seed=2022, device="cuda"), 0.2, 2022)
    lat = model.u_net.encoder.encode_image(b["query"], mode="mode").shape[2:]
    mask = hip.op_pool_mask(vis, lat, 0.5)
    fns = {"generate_and_retrieve": lambda: model.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"]),
           "retrieve_robust_trim0.25": lambda: model.retrieve_robust(b["query"], b["reference"], b["all_relativeR"], trim=0.25),
           "retrieve_robust_trim0.25_mask": lambda: model.retrieve_robust(b["query"], b["reference"], b["all_relativeR"], mask=mask, trim=0.25)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(runs):                          # alternating, in one process
        for k, fn in fns.items():
            ms[k].append(window_ms(fn, reps))
    base = spread(ms["generate_and_retrieve"])["median"]
    print(json.dumps(dict(bench="step", mode="f16x2", size=256, poses=512, latent=list(lat), runs=runs, reps=reps, ms={k: spread(v) for k, v in ms.items()},
                          ms_over_plain={k: spread(v)["median"] - base for k, v in ms.items()})), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robust_bench needs an MI355X")
    kernel_bench(max(a.runs, 4), a.reps)
    if not a.skip_step:
        step_bench(max(a.runs, 4), a.step_reps)
