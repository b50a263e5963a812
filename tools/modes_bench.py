"""The pose-distribution / distinct-modes op on one MI355X: what `nope_op_pose_modes` costs at three sizes, next to
`nope_topk` (k = 5) on the same scores in the same process.  One JSON line per size; records, no bar: the op has no predecessor, the top-k is
there only to place it.

Scores at the real scale (mean -2000, spread 300), Haar-random template poses, symmetry classes 0 / 1 / 2 cycling over the batch, max_modes = 5,
radius = the median nearest-neighbour distance of the grid x 1.5 (so a mode holds a handful of templates, as on the icosphere grids).  Times are
HIP-event medians over single calls (the launch and the status memset included: what a caller pays), alternating the two ops.

    python tools/modes_bench.py [--steps 200] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nope_amd import hip
from nope_amd.harness import random_rotations

SIZES = ((1, 341), (32, 2048), (32, 8192))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--temperature", type=float, default=100.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/modes_bench.py needs an MI355X (no CPU fallback)")
    g = torch.Generator().manual_seed(2022)
    for B, N in SIZES:
        s = (torch.randn(B, N, generator=g) * 300.0 - 2000.0).float().cuda()
        P = random_rotations(N, g)
        rel = torch.einsum("aij,bij->ab", P[:256], P)                       # nearest-neighbour angle of the first 256 templates
        cos = ((rel - 1.0) / 2.0).clamp(-1.0, 1.0)
        cos[torch.arange(min(256, N)), torch.arange(min(256, N))] = -1.0
        radius_deg = 1.5 * float(torch.rad2deg(torch.acos(cos.max(dim=1).values)).median())
        P = P[None].cuda()
        sym = (torch.arange(B) % 3).to(torch.int32).cuda()
        modes = lambda: hip.op_pose_modes(s, P, sym, temperature=a.temperature, radius_deg=radius_deg, max_modes=5, want_prob=True)
        topk = lambda: hip.topk(s, 5)
        for _ in range(a.warmup):
            modes()
            topk()
        torch.cuda.synchronize()
        ev = [(event_ms(modes), event_ms(topk)) for _ in range(a.steps)]
        torch.cuda.synchronize()
        r = modes()
        row = {"record": "pose_modes", "B": B, "N": N, "max_modes": 5, "radius_deg": round(radius_deg, 3), "temperature": a.temperature,
               "ms_pose_modes": round(float(np.median([m[0].elapsed_time(m[1]) for m, _ in ev])), 4),
               "ms_topk5": round(float(np.median([t[0].elapsed_time(t[1]) for _, t in ev])), 4),
               "mean_count_mode0": float(r.count[:, 0].float().mean()), "mean_entropy": round(float(r.entropy.mean()), 4), "steps": a.steps}
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
