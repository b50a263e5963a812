"""Times of the BOP pose errors on the device (nope_op_pose_errors, nope_op_mesh_diameter: csrc/kernels_poseerr.hip) on a synthetic vertex
cloud: HIP-event medians of the ADI pass, the ADD pass, the MSSD + MSPD walk and the diameter, at (P poses, V vertices, S symmetries) =
(5, 2 k, 1), (160, 30 k, 1) and (160, 30 k, 320) -- a T-LESS batch of 32 queries x 5 estimates, its largest models, its largest
symmetry sets.  The ADI pass's pair rate (P V^2 / time) is reported against the f64 vector peak: a pair is 3 subtractions, 3
multiplications, 2 additions and a minimum, nine f64 instructions none of which is an FMA (no contraction), so the peak pair rate is
(78.6e12 / 2) / 9 per second.  One JSON line per shape.

    python tools/pose_error_bench.py [--shapes 5x2000x1,160x30000x1,160x30000x320] [--reps 7]
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

from nope_amd import bop  # noqa: E402

F64_VECTOR_PEAK = 78.6e12        # FLOP/s with every instruction an FMA (2 FLOP); half the f32 vector peak
PAIR_INSTRUCTIONS = 9


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


def poses(rng, n):
    T = np.zeros((n, 4, 4))
    T[:, :3, :3] = rotations(rng, n)
    T[:, :3, 3] = np.stack([rng.uniform(-80, 80, n), rng.uniform(-60, 60, n), rng.uniform(500, 800, n)], 1)
    T[:, 3, 3] = 1.0
    return T


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="5x2000x1,160x30000x1,160x30000x320")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_error_bench.py needs an MI355X")
    K = np.array([[1075.65, 0, 360.0], [0, 1073.90, 270.0], [0, 0, 1]])
    rng = np.random.default_rng(0)
    for shape in a.shapes.split(","):
        P, V, S = (int(x) for x in shape.split("x"))
        verts = torch.from_numpy(rng.uniform(-60, 60, size=(V, 3)).astype(np.float32)).cuda()
        syms = np.zeros((S, 4, 4))
        syms[:, :3, :3] = rotations(rng, S)
        syms[:, 3, 3] = 1.0
        syms[0] = np.eye(4)
        syms = torch.from_numpy(syms).cuda()
        gt = poses(rng, P)
        est = gt.copy()
        est[:, :3, :3] = rotations(rng, P)
        est, gt = torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda()
        Ks = torch.from_numpy(K)[None].expand(P, 3, 3).contiguous().cuda()
        i32 = lambda v: torch.full((P,), v, dtype=torch.int32, device="cuda")
        vo, vc, so, sc = i32(0), i32(V), i32(0), i32(S)
        run = lambda want: bop.op_pose_errors(verts, vo, vc, V, syms, so, sc, S, est, gt, Ks, want)
        out = run(bop.METRICS)
        assert int(out["status"].abs().sum()) == 0
        adi_ms = timed(lambda: run(("adi",)), a.reps)
        add_ms = timed(lambda: run(("add",)), a.reps)
        sym_ms = timed(lambda: run(("mssd", "mspd")), a.reps)
        all_ms = timed(lambda: run(bop.METRICS), a.reps)
        diam_ms = timed(lambda: bop.op_mesh_diameter(verts, vo[:1], vc[:1], V), a.reps)
        pairs = P * V * V
        rate = pairs / (adi_ms * 1e-3)
        print(json.dumps({"what": "pose_errors", "P": P, "V": V, "S": S, "adi_ms": adi_ms, "add_ms": add_ms, "mssd_mspd_ms": sym_ms,
                          "all_four_ms": all_ms, "diameter_one_object_ms": diam_ms, "adi_pairs": pairs, "adi_pairs_per_s": rate,
                          "adi_fraction_of_f64_vector_peak": rate * PAIR_INSTRUCTIONS / (F64_VECTOR_PEAK / 2),
                          "sym_points_per_s": P * V * S / (sym_ms * 1e-3), "mean_adi_mm": float(out["adi"].mean()),
                          "mean_mssd_mm": float(out["mssd"].mean())}), flush=True)


if __name__ == "__main__":
    main()
