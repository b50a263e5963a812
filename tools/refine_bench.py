"""Sub-grid pose refinement on one MI355X: what it costs next to the grid steps it follows, and how it converges
in every compute mode.  One JSON line per record; records, no bar.

  * times, HIP-event medians, same process, the shipped U-Net (u_net_dim 192, 256 x 256 images, 32 x 32 x 8 embeddings): the 26- and
    341-template `generate_and_retrieve` steps (B = 1), and `refine_from_feat` with 1 and 3 iterations for (B, k) = (1, 5) and (32, 5); one
    iteration = (3 iterations - 1 iteration) / 2, i.e. one 7k-hypothesis pass + normal equations + step;
  * convergence of the planted problem (the query is the f32 network's output at a known pose; starts 4 / 8 / 10 degrees away; 4
    iterations) per compute mode on the reduced U-Net of smoke() (u_net_dim 32, 16 x 16 x 8): error against the planted pose after every
    iteration.  f16x2 is forced onto its two-pass kernels as smoke() does (a pass this small would not reach them).

    python tools/refine_bench.py [--dtype f16x2] [--steps 20] [--skip-times] [--skip-convergence]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nope_amd import hip
from nope_amd.harness import StubEncoder, build_model, random_rotations, synthetic_batch


def event_median_ms(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def rodrigues(axis, deg):
    axis = axis / axis.norm()
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    t = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def angle_deg(A, B):
    M = A @ B.transpose(-1, -2)
    s = 0.5 * torch.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1).norm(dim=-1)
    return torch.rad2deg(torch.atan2(s, 0.5 * (M.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0)))


def times(a):
    m = build_model(compute_dtype=a.dtype, bank_dtype="f32", device="cuda")
    for level, n in ((0, 26), (2, 341)):
        b = synthetic_batch(1, 0, 256, seed=2022, device="cuda", pose_level=level)
        ms = event_median_ms(lambda: m.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"]), a.steps)
        print(json.dumps({"record": "grid_step", "dtype": a.dtype, "B": 1, "templates": b["all_relativeR"].shape[1], "ms": round(ms, 4)}), flush=True)
    for B in (1, 32):
        b = synthetic_batch(B, 0, 256, seed=2022, device="cuda", pose_level=0)
        sim, idx, _, qf, rf = m._encode_generate_retrieve(b["query"], b["reference"], b["all_relativeR"])
        row = {"record": "refine", "dtype": a.dtype, "B": B, "k": idx.shape[1], "templates": 26}
        for iters in (1, 3):
            row[f"ms_{iters}_iters"] = round(event_median_ms(lambda: m.refine_from_feat(qf, rf, b["all_relativeR"], idx, sim, iters=iters), a.steps), 4)
        row["ms_per_iteration"] = round((row["ms_3_iters"] - row["ms_1_iters"]) / 2, 4)
        if B > 1:
            row["ms_grid_step_26"] = round(event_median_ms(lambda: m.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"]), a.steps), 4)
        r = m.refine_from_feat(qf, rf, b["all_relativeR"], idx, sim, iters=3)
        row["accepted"] = int(r.accepted.sum())
        print(json.dumps(row), flush=True)


def convergence(a):
    from nope_amd.model import PoseConditional
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    g = torch.Generator().manual_seed(31)
    B, starts, iters = 2, (4.0, 8.0, 10.0), 4
    x = torch.randn(B, 8, 16, 16, generator=g).cuda()
    true = random_rotations(B, g)
    rel = torch.stack([torch.stack([(rodrigues(torch.randn(3, generator=g, dtype=torch.float64), d) @ true[b])[:2].reshape(6) for d in starts])
                       for b in range(B)]).float().cuda()
    true6 = true[:, :2].reshape(B, 6).float().cuda()
    idx = torch.arange(len(starts)).expand(B, -1).contiguous().cuda()
    query = None
    for cdt in ("f32", "bf16x3", "f16x2", "f16", "bf16"):
        saved = os.environ.get("NOPE_CONV_PP")
        if cdt == "f16x2":
            os.environ["NOPE_CONV_PP"] = "11"
        try:
            u = UNet(u_net_dim=32, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
            synth_init_(u, 2022)
            m = PoseConditional(u, None, {"similarity_metric": "l2"}, None).cuda()
            if query is None:
                query = m.u_net(x, true6)                   # the f32 network's output: the same question for every mode
            sim = hip.similarity(query, m.u_net.forward_hypotheses(x, rel))
            r = m.refine_from_feat(query, x, rel, idx, sim, iters=iters)
            torch.cuda.synchronize()
        finally:
            if saved is None:
                os.environ.pop("NOPE_CONV_PP", None)
            else:
                os.environ["NOPE_CONV_PP"] = saved
        err = angle_deg(r.trajectory.cpu(), true[None, :, None])          # (iters + 1, B, k)
        print(json.dumps({"record": "convergence", "dtype": cdt, "starts_deg": starts, "fd_step": 1e-2,
                          "worst_error_deg_per_iteration": [float(f"{v:.3g}") for v in err.amax(dim=(1, 2)).tolist()],
                          "median_error_deg_per_iteration": [float(f"{v:.3g}") for v in err.flatten(1).median(dim=1).values.tolist()],
                          "accepted": int(r.accepted.sum()), "candidates": B * len(starts),
                          "status_last": r.status[-1].flatten().tolist()}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "bf16x3", "f16x2", "f16", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-times", action="store_true")
    ap.add_argument("--skip-convergence", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/refine_bench.py needs an MI355X")
    if not a.skip_convergence:
        convergence(a)
    if not a.skip_times:
        times(a)
