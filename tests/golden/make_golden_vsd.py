"""Fixture of the VSD error (nope_amd.vsd, nope_op_vsd), recorded from THE REFERENCE'S `vsd_obj` (src/poses/vsd.py:57-132 with
src/poses/vsd_utils.py):

    python tests/golden/make_golden_vsd.py        # build container only (needs the reference sources)

vsd_obj renders with pyrender and reads the test depth with cv2; neither exists here, so `pyrenderer` is replaced by a function that
returns the case's ground-truth / estimated depth maps and `cv2.imread` by one that returns 10 x the case's test depth (vsd.py:74 divides
by 10: the f32 test depth comes back exactly).  vsd_obj fixes visib_mode="bop19"; the bop18 cases replace its estimate_visib_mask_gt / _est
by the same vsd_utils functions called with visib_mode="bop18".  Everything else is the reference's own code.

Inputs are regenerated from a seed (`case_inputs()`, pinned by their digest); only the errors are stored.  They contain: missing test
depth (d_test == 0), an occluder in front of the object, an estimate that does not overlap the ground truth, an empty union (error 1.0),
and pixels at exactly f32 d_diff == delta and dists == tau (the principal-point pixel, where the distance is the depth itself, plus
pixels searched to land on d_diff == delta in f32).
"""
from __future__ import annotations

import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 2024
B, K, H, W = 4, 4, 96, 128
DELTA, TAU = 15, 20
CASES = (("step", "bop19"), ("tlinear", "bop19"), ("step", "bop18"), ("tlinear", "bop18"))


def _dist(d, prex, prey):
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt(np.multiply(prex, d) ** 2 + np.multiply(prey, d) ** 2 + d ** 2)


def case_inputs():
    """(depth_test (B,H,W) f32, depth_gt (B,H,W) f32, depth_est (B,K,H,W) f32, K (B,3,3) f64), deterministic."""
    rng = np.random.default_rng(SEED)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dtest = np.zeros((B, H, W), np.float32)
    dgt = np.zeros((B, H, W), np.float32)
    dest = np.zeros((B, K, H, W), np.float32)
    Ks = np.zeros((B, 3, 3))
    for b in range(B):
        fx, fy = 520.0 + 13 * b, 515.0 - 7 * b
        cx, cy = float(60 + 3 * b), float(44 + 2 * b)            # integer principal point: pre_X = pre_Y = 0 at (cx, cy)
        Ks[b] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
        prex, prey = (xs - cx) / fx, (ys - cy) / fy
        # object: a tilted ellipsoidal cap around (cx + ox, cy + oy)
        ox, oy = rng.integers(-6, 7, size=2)
        r2 = ((xs - cx - ox) / 30.0) ** 2 + ((ys - cy - oy) / 24.0) ** 2
        obj = r2 < 1.0
        z = 600.0 + 40 * b + 0.8 * (xs - cx) - 0.5 * (ys - cy) - 30.0 * np.sqrt(np.clip(1 - r2, 0, 1))
        z = z + rng.normal(0, 0.3, size=z.shape)
        if b < 3:
            dgt[b] = np.where(obj, z, 0).astype(np.float32)
        # scene: background wall, the object with sensor noise, an occluder, missing depth
        scene = 900.0 + 0.3 * xs + rng.normal(0, 1.0, size=(H, W))
        scene = np.where(dgt[b] > 0, dgt[b] + rng.normal(0, 4.0, size=(H, W)), scene)
        occ = (xs > cx + 8) & (xs < cx + 22) & (ys > cy - 30) & (ys < cy + 30)
        scene = np.where(occ, 420.0 + rng.normal(0, 1.0, size=(H, W)), scene)
        hole = ((xs - cx + 15) ** 2 + (ys - cy - 10) ** 2) < 36
        scene = np.where(hole | (rng.random((H, W)) < 0.03), 0.0, scene)
        dtest[b] = scene.astype(np.float32)
        # estimates: near the truth, shifted by a few pixels and deeper, not overlapping at all, empty
        dest[b, 0] = np.where(dgt[b] > 0, dgt[b] + rng.normal(0, 6.0, size=(H, W)).astype(np.float32), 0)
        dest[b, 1] = np.roll(dgt[b], (3, 5), axis=(0, 1)) * np.float32(1.02)
        dest[b, 2] = np.roll(np.where(obj, z, 0).astype(np.float32), 60, axis=1) * (np.roll(xs, 60, axis=1) < 20)
        dest[b, 3] = 0.0 if b == 3 else np.roll(dgt[b], -2, axis=0)
        # exact boundaries at the principal point: dist = depth there
        iy, ix = int(cy), int(cx)
        if b < 3:
            dtest[b, iy, ix], dgt[b, iy, ix] = 500.0, 515.0           # d_diff == delta
            dest[b, 0, iy, ix] = 495.0                                 # |dist_gt - dist_est| == tau
            dest[b, 1, iy, ix] = 515.0 + 15.0                          # est: d_diff == delta against the test depth, dists == 15 < tau
        # more pixels at f32 d_diff == delta exactly: step d_gt by f32 ulps until f32(dist_gt) - f32(dist_test) == 15
        for (yy, xx) in [(cy + dy, cx + dx) for dy, dx in ((-5, -7), (4, -3), (9, 2), (-2, 11), (6, -12))]:
            yy, xx = int(yy), int(xx)
            if dgt[b, yy, xx] <= 0 or dtest[b, yy, xx] <= 0:
                continue
            px, py = prex[yy, xx], prey[yy, xx]
            t32 = np.float32(_dist(dtest[b, yy, xx], px, py))
            g = np.float32(dtest[b, yy, xx] + 15.0)
            for _ in range(4000):
                diff = np.float32(_dist(g, px, py)) - t32
                if diff == np.float32(15.0):
                    dgt[b, yy, xx] = g
                    break
                g = np.nextafter(g, np.float32(np.inf) if diff < 15 else np.float32(-np.inf))
    return dtest, dgt, dest, Ks


def digest(arrs) -> str:
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def reference_errors(dtest, dgt, dest, Ks, cost_type, visib):
    """(B, K) errors of the reference's vsd_obj, frame by frame."""
    sys.path.insert(0, HERE)
    import _ref_import
    _ref_import.install()
    import src.poses.vsd as V
    import src.poses.vsd_utils as U
    out = np.zeros((dtest.shape[0], dest.shape[1]))
    # vsd_obj passes visib_mode="bop19" itself: route both mask functions to the case's mode
    V.estimate_visib_mask_gt = lambda a, c, d, visib_mode=None: U.estimate_visib_mask_gt(a, c, d, visib_mode=visib)
    V.estimate_visib_mask_est = lambda a, c, g, d, visib_mode=None: U.estimate_visib_mask_est(a, c, g, d, visib_mode=visib)
    for b in range(dtest.shape[0]):
        calls = []

        def fake_renderer(obj_poses, BOP_cad_trimesh, intrinsic, img_size, b=b):
            calls.append(1)
            n = obj_poses.shape[0] if obj_poses.ndim == 3 else 1
            if len(calls) == 1:                       # gt_depths = renderer(gt_poses)
                return [dgt[b].copy() for _ in range(n)]
            return [dest[b, j].copy() for j in range(n)]

        V.pyrenderer = fake_renderer
        V.cv2 = types.SimpleNamespace(imread=lambda p, flag, b=b: dtest[b].astype(np.float64) * 10.0)
        frame = {"mesh": None, "intrinsic": Ks[b], "depth_path": f"frame{b}.png",
                 "pred_poses": np.tile(np.eye(4), (dest.shape[1], 1, 1)), "query_pose": np.eye(4)}
        out[b] = V.vsd_obj(0, [frame], delta_vsd=DELTA, tau_vsd=TAU, cost_type=cost_type, use_gt_translation=True)
    return out


def main():
    sys.path.insert(0, HERE)
    import _ref_import
    if not _ref_import.available():
        print("reference tree not present: nothing to record")
        return
    ins = case_inputs()
    rec = {"inputs_sha256": np.array(digest(ins))}
    for cost, vis in CASES:
        rec[f"{cost}_{vis}"] = reference_errors(*ins, cost, vis)
        print(cost, vis, rec[f"{cost}_{vis}"].round(6).tolist())
    np.savez_compressed(os.path.join(HERE, "vsd_ref.npz"), **rec)


if __name__ == "__main__":
    main()
