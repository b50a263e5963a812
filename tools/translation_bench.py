"""Times of the translation stages on the device (nope_op_mask_boxes, nope_op_fit_translation, nope_op_depth_shift:
csrc/kernels_posefit.hip; bop.refine_translation_depth) for a T-LESS batch of 32 queries x 5 estimates = 160 poses of a 30 k-vertex
model in 540 x 720 images: HIP-event medians per stage, stated against the bytes the stage reads.  The model is the level-6 icosphere
scaled to an ellipsoid (40 962 vertices, 81 920 faces); the fit reads its first 30 000 vertices (they hold every vertex of level 5, so they
cover the surface), the rendering of the depth stage draws the whole mesh.  The boxes are those of planted translations with every edge
moved by up to a pixel, as a detector's would be.  One JSON line per stage; measured, not promised.

    python tools/translation_bench.py [--queries 32] [--k 5] [--verts 30000] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nope_amd import bop, vsd  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--verts", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/translation_bench.py needs an MI355X")
    B, k, V, H, W = a.queries, a.k, a.verts, 540, 720
    P = B * k
    K = np.array([[1075.65, 0, 360.0], [0, 1073.90, 270.0], [0, 0, 1]])
    rng = np.random.default_rng(0)
    v, f = vsd.icosphere(6, 1.0)
    v = (v.astype(np.float64) * np.array([70.0, 45.0, 30.0])).astype(np.float32)
    V = min(V, len(v))
    bank = vsd.MeshBank({1: (v, f)}, device="cuda")
    R = rotations(rng, P).reshape(B, k, 3, 3)
    t = np.stack([rng.uniform(-60, 60, B), rng.uniform(-40, 40, B), rng.uniform(550, 800, B)], 1)
    ids = [1] * B
    # the detections: masks rendered at the first estimate's rotation and the planted translation
    gt_depth = vsd.render_depth(bank, ids, vsd.compose_poses(R[:, 0], t), K, H, W)
    mask = (gt_depth > 0).to(torch.uint8)
    box, count = bop.op_mask_boxes(mask)
    assert int(count.min()) > 0
    mask_ms = timed(lambda: bop.op_mask_boxes(mask), a.reps)
    print(json.dumps({"what": "mask_boxes", "B": B, "H": H, "W": W, "ms": mask_ms, "bytes_read": B * H * W,
                      "GB_per_s": B * H * W / (mask_ms * 1e-3) / 1e9}), flush=True)

    i32 = lambda x: torch.full((P,), x, dtype=torch.int32, device="cuda")
    vo, vc = i32(0), i32(V)
    Rp = torch.from_numpy(R.reshape(P, 3, 3)).cuda()
    Kp = torch.from_numpy(K)[None].expand(P, 3, 3).contiguous().cuda()
    bp = box.reshape(B, 1, 4).expand(B, k, 4).reshape(P, 4).contiguous()
    fit = lambda iters=32: bop.op_fit_translation(bank.verts, vo, vc, V, Rp, Kp, bp, max_iters=iters)
    out = fit()
    iters = out["iters"].cpu().numpy()
    conv = int((out["status"] == 0).sum())
    fit_ms, fit0_ms = timed(fit, a.reps), timed(lambda: fit(0), a.reps)
    passes = int((iters + 2).sum())                       # pass 0, then one pass per evaluation of the projected box (iters + 1)
    print(json.dumps({"what": "fit_translation", "P": P, "V": V, "ms": fit_ms, "ms_max_iters_0": fit0_ms, "converged": conv,
                      "iters_mean": float(iters.mean()), "iters_max": int(iters.max()), "vertex_passes": passes,
                      "bytes_read_per_pass": V * 12, "bytes_read": passes * V * 12, "GB_per_s": passes * V * 12 / (fit_ms * 1e-3) / 1e9,
                      "mesh_bytes": V * 12, "residual_px_median": float(out["residual"].nanmedian()),
                      "t_z_error_first_estimate_mm_median": float((out["t"].reshape(B, k, 3)[:, 0, 2].cpu() - torch.from_numpy(t[:, 2])).abs().median())}),
          flush=True)

    pred_t = torch.where((out["status"] != 0).reshape(B, k, 1), torch.from_numpy(t).cuda().reshape(B, 1, 3), out["t"].reshape(B, k, 3))
    poses = vsd.compose_poses(torch.from_numpy(R).cuda(), pred_t).reshape(P, 4, 4)
    est = vsd.render_depth(bank, [1] * P, poses, K, H, W).reshape(B, k, H, W)
    tau = 20.0
    for m, name in ((None, "depth_shift"), (mask, "depth_shift_masked")):
        shift, cnt = bop.op_depth_shift(gt_depth, est, tau, m)
        ms = timed(lambda: bop.op_depth_shift(gt_depth, est, tau, m), a.reps)
        nbytes = B * k * H * W * (8 + (1 if m is not None else 0))
        print(json.dumps({"what": name, "B": B, "k": k, "H": H, "W": W, "tau": tau, "ms": ms, "bytes_read": nbytes,
                          "GB_per_s": nbytes / (ms * 1e-3) / 1e9, "inliers_mean": float(cnt.double().mean()),
                          "abs_shift_mm_median": float(shift.abs().nanmedian())}), flush=True)
    rnd = lambda: bop.refine_translation_depth(bank, ids, R, pred_t, K, gt_depth, tau, mask=mask, rounds=1)
    o = rnd()
    print(json.dumps({"what": "refine_translation_depth, one round (rendering + shift + update)", "P": P, "faces": len(f), "ms": timed(rnd, a.reps),
                      "flagged": int((o["status"] != 0).sum())}), flush=True)


if __name__ == "__main__":
    main()
