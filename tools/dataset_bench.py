"""Times of the ShapeNet test loader for ONE sample with the full level-2 bank (nope_amd/dataset.py, csrc/kernels_misc.hip): 2 + 341 RGBA frames of
512 x 512 -> 256 x 256 crops, one JSON line per measurement:

  decode     PNG decode of the 343 files on the host (PIL, `decode_frame`), wall time.
  upload     the one staging buffer [frames | maps]: filling it on the host (wall time) and its one host-to-device copy (HIP events).
  launch     the one nope_op_crop_frames launch over the 343 frames (HIP events) and the bytes it writes / the source bytes under its boxes.
  batched    `crop_frames` end to end from decoded frames: maps solved on the host, staging, upload, launch (wall time, synchronised).
  parent     the same 343 frames through the path of the parent commit: PIL paste on black per frame on the host (wall time), then
             process_test_sample's per-frame loop -- one host-to-device copy, one host map and one nope_op_warp_perspective launch per frame
             (wall time, synchronised) -- and whether the two results are the same bits.

The frames are synthetic renders (a shaded, textured blob on a transparent background), written as PNGs to a temporary directory.  A warm-up
call, the median of --reps runs.

    python tools/dataset_bench.py [--reps 7] [--templates 341] [--source 512] [--size 256]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nope_amd import hip  # noqa: E402
from nope_amd.dataset import SHAPENET_INTRINSIC, crop_frame, crop_frames, crop_transform, decode_frame  # noqa: E402
from nope_amd.poses import get_obj_poses_from_template_level  # noqa: E402


def synthetic_render(rng, S):
    """(S, S, 4) uint8: a shaded blob with a soft edge and some texture over a transparent background."""
    y, x = np.mgrid[0:S, 0:S].astype(np.float32) / S - 0.5
    cx, cy, r = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0.22, 0.34)
    d = np.sqrt((x - cx) ** 2 + ((y - cy) * rng.uniform(0.8, 1.25)) ** 2)
    alpha = np.clip((r - d) * S / 3, 0, 1)
    shade = np.clip(1.0 - d / r, 0, 1)[..., None] * rng.uniform(0.4, 1.0, size=3)
    tex = 0.12 * np.sin(x * rng.uniform(40, 90) + y * rng.uniform(40, 90))[..., None] + rng.normal(size=(S, S, 3)) * 0.02
    rgb = np.clip(shade + tex, 0, 1) * (alpha[..., None] > 0)
    return np.ascontiguousarray(np.concatenate([rgb * 255, alpha[..., None] * 255], -1).astype(np.uint8))


def wall(fn, reps, sync=True):
    fn()
    if sync:
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def events(fn, reps):
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


def main():
    from PIL import Image
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--templates", type=int, default=341)
    ap.add_argument("--source", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dataset_bench.py needs an MI355X")
    F, Hs, S = 2 + a.templates, a.source, a.size
    rng = np.random.default_rng(0)
    grid = get_obj_poses_from_template_level(2, "upper")
    poses = np.stack([grid[i % len(grid)] for i in range(F)]).copy()
    poses[:, :3, 3] = np.array([0.0, 0.0, 1.1]) + rng.normal(size=(F, 3)) * 0.02      # the unit box covers ~480 of the 512 pixels
    K = np.diag([Hs / 512, Hs / 512, 1.0]) @ SHAPENET_INTRINSIC
    say = lambda **kw: print(json.dumps(kw), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for f in range(F):
            paths.append(os.path.join(tmp, f"frame_{f:06d}.png"))
            Image.fromarray(synthetic_render(rng, Hs), "RGBA").save(paths[-1])
        png_bytes = sum(os.path.getsize(p) for p in paths)
        med, lo, hi = wall(lambda: [decode_frame(p) for p in paths], max(1, a.reps // 2), sync=False)
        say(what="decode", frames=F, source=Hs, png_mb=png_bytes / 1e6, ms_median=med, ms_min=lo, ms_max=hi, ms_per_frame=med / F)
        frames = [decode_frame(p) for p in paths]
    # ---- the batched path, piece by piece
    minv = np.stack([np.linalg.inv(crop_transform(K, poses[f], S, False, 1.0)) for f in range(F)]).reshape(F, 9).astype(np.float32)
    per = Hs * Hs * 4
    host = torch.empty(F * per + F * 36, dtype=torch.uint8, pin_memory=True)

    def stage():
        hv = host.numpy()
        fv = hv[:F * per].reshape(F, Hs, Hs, 4)
        for f in range(F):
            fv[f] = frames[f]
        hv[F * per:].view(np.float32).reshape(F, 9)[:] = minv
    med, lo, hi = wall(stage, a.reps, sync=False)
    say(what="upload_staging", mb=host.numel() / 1e6, ms_median=med, ms_min=lo, ms_max=hi)
    dev_buf = torch.empty_like(host, device="cuda")
    med, lo, hi = events(lambda: dev_buf.copy_(host, non_blocking=True), a.reps)
    say(what="upload_copy", mb=host.numel() / 1e6, ms_median=med, ms_min=lo, ms_max=hi, gb_s=host.numel() / med / 1e6)
    d_frames, d_minv = dev_buf[:F * per].view(F, Hs, Hs, 4), dev_buf[F * per:].view(torch.float32).view(F, 9)
    med, lo, hi = events(lambda: hip.op_crop_frames(d_frames, d_minv, S, 2.0 / 255.0, -1.0, True), a.reps)
    out_bytes = F * 3 * S * S * 4
    say(what="launch", kernel="nope_op_crop_frames", frames=F, source=Hs, size=S, ms_median=med, ms_min=lo, ms_max=hi, reps=a.reps, out_mb=out_bytes / 1e6,
        source_mb=F * per / 1e6, tb_s_out_plus_source=(out_bytes + F * per) / med / 1e9)
    bmed, blo, bhi = wall(lambda: crop_frames(frames, poses, K, S, 1.0), a.reps)
    say(what="batched", ms_median=bmed, ms_min=blo, ms_max=bhi, note="maps + staging + upload + launch, from decoded frames")
    got = crop_frames(frames, poses, K, S, 1.0)
    # ---- the parent commit's path on the same frames
    def paste(fr):
        img = Image.fromarray(fr, "RGBA")
        black = Image.new("RGB", img.size, (0, 0, 0))
        black.paste(img, mask=img.getchannel("A"))
        return np.array(black)
    med, lo, hi = wall(lambda: [paste(fr) for fr in frames], max(1, a.reps // 2), sync=False)
    say(what="parent_paste", ms_median=med, ms_min=lo, ms_max=hi, ms_per_frame=med / F)
    pasted = [paste(fr) for fr in frames]
    loop = lambda: [crop_frame(pasted[f], None, K, poses[f], S, virtual_bbox_size=1.0, normalize=True, round_u8=True) for f in range(F)]
    pmed, plo, phi = wall(loop, a.reps)
    want = torch.stack(loop())
    say(what="parent_loop", ms_median=pmed, ms_min=plo, ms_max=phi, launches=F, same_bits=bool(torch.equal(got, want)),
        batched_over_parent=bmed / pmed, black_fraction=float((want == -1.0).float().mean()))


if __name__ == "__main__":
    main()
