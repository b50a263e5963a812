"""Times of the visualisation pass on the device (nope_amd/vis.py, csrc/kernels_vis.hip), one JSON line per measurement:

  sheet      one nope_op_vis_sheet call for the pictures of a 341-template bank: B = 4, F = 341, 256 x 256 images, three columns (the
             reference image shared by every frame, ground-truth and predicted templates per frame), tile 64, nrow 16, padding 2 -- and
             the share of the 8 TB/s HBM peak (the figure bench.py uses) that its time implies for the bytes the pass has to move: the source
             rows its taps touch, once, plus the sheet.
  torch_ops  the op sequence the reference runs for the same pictures (cast, index-assign into a zero f16 grid, F.interpolate, make_grid
             restated, the f16 quantisation), as torch-ROCm ops on the same GPU, batched over the frames: the yardstick.
  eval       wall time of PoseConditional.eval_geodesic at --encoder vae with and without visualize (PNG / video encoding included).

HIP events, a warm-up call, the median of --reps runs.

    python tools/vis_bench.py [--reps 7] [--frames 341] [--batch 4] [--size 256] [--no-eval]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nope_amd import hip, vis  # noqa: E402

HBM_PEAK = 8.0e12


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
    return statistics.median(ms), min(ms), max(ms)


def touched_rows(S, tile):
    """Source rows the bilinear taps of a tile-high output read (nope_hip.h: nope_op_vis_sheet)."""
    rows = set()
    scale = S / tile
    for o in range(tile):
        src = max(scale * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(src), S - 1)
        rows.update((i0, min(i0 + 1, S - 1)))
    return len(rows)


def unnormalize_to_zero_to_one(t):          # src/model/utils.py:12-15
    img = t.clone()
    img = (img + 1) * 0.5
    return img.clamp(0, 1)


def torch_sequence(ref, gt, pred, tile, nrow, padding):
    """The reference's ops for F pictures at once: (F, Hs, Ws, 3) u8."""
    B, Fr, _, S, _ = gt.shape
    n_img = B * 4
    grid = torch.zeros((Fr, n_img, 3, S, S), device=ref.device).to(torch.float16)      # put_image_to_grid
    idx = torch.arange(0, n_img, 4, device=ref.device).to(torch.int64)
    grid[:, idx] = unnormalize_to_zero_to_one(ref).to(torch.float16)[None]
    grid[:, idx + 1] = unnormalize_to_zero_to_one(gt).to(torch.float16).transpose(0, 1)
    grid[:, idx + 2] = pred.clamp(0, 1).to(torch.float16).transpose(0, 1)
    small = F.interpolate(grid.reshape(Fr * n_img, 3, S, S).clone(), (tile, tile), mode="bilinear", align_corners=False)
    small = small.reshape(Fr, n_img, 3, tile, tile)
    xmaps = min(nrow, n_img)
    ymaps = -(-n_img // xmaps)
    cell = tile + padding
    sheet = small.new_full((Fr, 3, cell * ymaps + padding, cell * xmaps + padding), 0.0)          # make_grid
    for k in range(n_img):
        y, x = (k // xmaps) * cell + padding, (k % xmaps) * cell + padding
        sheet[:, :, y:y + tile, x:x + tile] = small[:, k]
    return sheet.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()      # save_image


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=341)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--eval-dtype", default="bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vis_bench.py needs an MI355X")
    B, Fr, S, tile, nrow, padding = a.batch, a.frames, a.size, 64, 16, 2
    g = torch.Generator().manual_seed(0)
    ref = (torch.rand(B, 3, S, S, generator=g) * 2.8 - 1.4).cuda()
    gt = (torch.rand(B, Fr, 3, S, S, generator=g) * 2.8 - 1.4).cuda()
    pred = (torch.rand(B, Fr, 3, S, S, generator=g) * 1.4 - 0.2).cuda()
    cols = [vis.Column(ref, True, True), vis.Column(gt, True, True), vis.Column(pred, False, True)]
    Hs, Ws = hip.vis_sheet_shape(3, B, tile, nrow, padding)
    out = torch.empty((Fr, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    med, lo, hi = timed(lambda: hip.op_vis_sheet(cols, tile, nrow, padding, out=out), a.reps)
    rows = touched_rows(S, tile)
    src_bytes = (B + 2 * B * Fr) * 3 * rows * S * 4              # the shared column once, the two framed columns per frame
    nbytes = src_bytes + out.numel()
    print(json.dumps(dict(what="sheet", B=B, F=Fr, S=S, tile=tile, sheet_shape=list(out.shape), ms_median=med, ms_min=lo, ms_max=hi, reps=a.reps,
                          source_rows_touched=rows, gb_moved=nbytes / 1e9, tb_s=nbytes / med / 1e9, hbm_fraction_of_8tb_s=nbytes / (med * 1e-3) / HBM_PEAK)), flush=True)
    want = torch_sequence(ref, gt, pred, tile, nrow, padding)
    d = (out.int() - want.int()).abs()
    tmed, tlo, thi = timed(lambda: torch_sequence(ref, gt, pred, tile, nrow, padding), a.reps)
    print(json.dumps(dict(what="torch_ops", ms_median=tmed, ms_min=tlo, ms_max=thi, reps=a.reps, kernel_over_torch=med / tmed,
                          bytes_that_differ=int((d > 0).sum()), worst_level_difference=int(d.max()))), flush=True)
    del want, d, gt, pred, cols, out
    torch.cuda.empty_cache()
    if a.no_eval:
        return
    from nope_amd.harness import build_model, synthetic_batch
    with tempfile.TemporaryDirectory() as tmp:
        model = build_model(2022, a.eval_dtype, "f32", "cuda", save_dir=tmp, encoder="vae")
        batch = synthetic_batch(1, Fr, S, 2022, "cuda", gt_templates=True)
        res = {}
        for visualize in (False, True, False, True):          # (alternating; the first pair warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.eval_geodesic(batch, "synthetic", visualize=visualize, save_prediction=True)
            torch.cuda.synchronize()
            res[visualize] = time.perf_counter() - t0
        files = os.listdir(os.path.join(tmp, "media"))
        print(json.dumps(dict(what="eval", encoder="vae", dtype=a.eval_dtype, B=1, templates=Fr, S=S, seconds_plain=res[False], seconds_visualize=res[True],
                              files=len(files), video=[f for f in files if f.startswith("video_")])), flush=True)


if __name__ == "__main__":
    main()
