"""Times of the T-LESS evaluation on the device: rendering the B (1 + k) depth maps of a batch (nope_op_render_depth) and the VSD pass
over them (nope_op_vsd), at 720x540 with k = 5 and a synthetic ~20 k-face mesh (an icosphere at level 5, 20 480 faces).  The VSD pass
reads (2 + k) f32 images per query; its bytes / time is reported against the device copy of this run (read + write bytes / s, measured
as tools/copy_ceiling.py does).  One JSON line per shape.

    python tools/vsd_bench.py [--batches 16,64] [--reps 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nope_amd import vsd  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def copy_tb_s(mb=805, reps=10):
    n = mb * 1024 * 1024 // 4
    x = torch.randn(n, device="cuda")
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x), reps)
    return 2 * n * 4 / ms / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--level", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vsd_bench.py needs an MI355X")
    H, W, k = 540, 720, a.k
    K = np.array([[1075.65, 0, 360.0], [0, 1073.90, 270.0], [0, 0, 1]])      # T-LESS primesense-like intrinsics
    v, f = vsd.icosphere(a.level, 60.0)
    bank = vsd.MeshBank({1: (v, f)})
    copy = copy_tb_s()
    rng = np.random.default_rng(0)
    for B in (int(x) for x in a.batches.split(",")):
        q = torch.from_numpy(rng.normal(size=(B * (1 + k), 4))).double()
        q = q / q.norm(dim=1, keepdim=True)
        w, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        t = torch.from_numpy(np.stack([rng.uniform(-80, 80, B), rng.uniform(-60, 60, B), rng.uniform(500, 800, B)], 1))
        t = t.repeat_interleave(1 + k, 0)
        poses = vsd.compose_poses(R, t).cuda()
        Ks = torch.from_numpy(K)[None].expand(B * (1 + k), 3, 3).contiguous().cuda()
        ids = [1] * (B * (1 + k))
        depth = vsd.render_depth(bank, ids, poses, Ks, H, W)
        render_ms = timed(lambda: vsd.render_depth(bank, ids, poses, Ks, H, W), a.reps)
        d = depth.reshape(B, 1 + k, H, W)
        d_gt, d_est = d[:, 0].contiguous(), d[:, 1:].contiguous()
        d_test = (d_gt + 2.0 * torch.randn_like(d_gt)) * (d_gt > 0) + 900.0 * (d_gt == 0)
        Kb = Ks[: B]
        err = vsd.vsd_from_depth(d_test, d_gt, d_est, Kb)
        vsd_ms = timed(lambda: vsd.vsd_from_depth(d_test, d_gt, d_est, Kb), a.reps)
        nbytes = B * (2 + k) * H * W * 4
        print(json.dumps({"what": "vsd", "B": B, "k": k, "H": H, "W": W, "faces": int(f.shape[0]), "images": B * (1 + k),
                          "covered_fraction": float((depth > 0).float().mean()), "render_ms": render_ms, "vsd_ms": vsd_ms,
                          "vsd_gb_read": nbytes / 1e9, "vsd_tb_s": nbytes / vsd_ms / 1e9, "copy_tb_s": copy,
                          "vsd_fraction_of_copy": nbytes / vsd_ms / 1e9 / copy, "mean_err_top1": float(err[:, 0].mean())}))


if __name__ == "__main__":
    main()
