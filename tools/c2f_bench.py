"""Coarse-to-fine retrieval next to the exhaustive step on one MI355X: the shipped U-Net (u_net_dim 192, 256 x 256
images, 32 x 32 x 8 embeddings), the level-2 (341) and level-3 (1321) upper grids, B = 1 and 8, compute modes f16x2 and f16.  One JSON line
per (mode, grid, B) cell; records, no bar.

Both paths run in one process on one box, alternating, `--runs` (4) runs each; a run is the HIP-event time of `--steps` consecutive calls
divided by their number.  Exhaustive = `generate_and_retrieve`; search = `retrieve_coarse_to_fine` (seeds = 3, the default radii and
capacities), both from the images.  A cell reports both medians, both spans (min, max over the runs), the share of the grid the search
evaluated and `top1_agree`, the share of queries whose top-1 is the exhaustive one -- with synthetic weights the score landscape is not
smooth, so that share says nothing about real data.  `faster` is true only where EVERY run of the search is below EVERY exhaustive run.

    python tools/c2f_bench.py [--dtypes f16x2,f16] [--levels 2,3] [--batches 1,8] [--runs 4] [--steps 3] [--seeds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nope_amd.harness import build_model, synthetic_batch
from nope_amd.poses import grid_stages


def run_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dtypes", default="f16x2,f16")
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/c2f_bench.py needs an MI355X (no CPU fallback)")
    for dtype in a.dtypes.split(","):
        model = build_model(compute_dtype=dtype, bank_dtype="f32", device="cuda")
        for level in (int(v) for v in a.levels.split(",")):
            stage_of = grid_stages(level, "upper")
            for B in (int(v) for v in a.batches.split(",")):
                b = synthetic_batch(B, 0, a.size, seed=2022, device="cuda", pose_level=level)
                exhaustive = lambda: model.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"])
                search = lambda: model.retrieve_coarse_to_fine(b["query"], b["reference"], b["all_relativeR"], b["template_poses"][:1], stage_of, seeds=a.seeds)
                _, idx, _ = exhaustive()           # (warm-up as well: the first call of a shape plans its launches)
                r = search()
                torch.cuda.synchronize()
                t_ex, t_c2f = [], []
                for _ in range(a.runs):
                    t_ex.append(run_ms(exhaustive, a.steps))
                    t_c2f.append(run_ms(search, a.steps))
                N = b["all_relativeR"].shape[1]
                row = {"record": "c2f", "dtype": dtype, "level": level, "templates": N, "B": B, "seeds": a.seeds, "runs": a.runs, "steps": a.steps,
                       "ms_exhaustive": round(float(np.median(t_ex)), 3), "span_exhaustive": [round(min(t_ex), 3), round(max(t_ex), 3)],
                       "ms_c2f": round(float(np.median(t_c2f)), 3), "span_c2f": [round(min(t_c2f), 3), round(max(t_c2f), 3)],
                       "faster": bool(max(t_c2f) < min(t_ex)), "ratio_of_medians": round(float(np.median(t_ex) / np.median(t_c2f)), 2),
                       "evaluated_frac": round(float(r.n_evaluated.float().mean()) / N, 4), "n_dropped": int(r.n_dropped.sum()),
                       "top1_agree": float((r.nearest_idx[:, 0] == idx[:, 0]).float().mean())}
                line = json.dumps(row)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
