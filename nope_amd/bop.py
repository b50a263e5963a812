"""The BOP pose errors besides VSD on the device: MSSD, MSPD, ADD, ADI (ADD-S), mesh diameters, and the recalls the BOP benchmark averages
into AR.  No reference counterpart: the reference reads models_info.json (dataloader/baseBOP.py:284) and evaluates one VSD threshold
(src/model/model.py:530-537).  The definitions are those of the BOP toolkit (pose_error.py, misc.get_symmetry_transformations,
eval_calc_scores), restated in include/nope_hip.h and DESIGN.md section 4.15 because the toolkit is not a dependency.

The errors are HIP kernels (nope_op_pose_errors, nope_op_mesh_diameter: csrc/kernels_poseerr.hip); symmetry sets and score tables are
small host arithmetic in numpy.

A translation of the library's own (estimate_translation, refine_translation_depth): from the retrieved rotation, the mesh and the detected 2D
box, corrected along the viewing ray from a depth image (nope_op_fit_translation, nope_op_mask_boxes, nope_op_depth_shift:
csrc/kernels_posefit.hip).  It is what pose_errors(pred_t=...) and vsd.vsd_error(pred_t=...) are given.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import hip
from .vsd import MeshBank, _as_f64, compose_poses

# NOPE_POSE_ERR_* (include/nope_hip.h)
ST_NONFINITE, ST_BEHIND, ST_VERT_RANGE, ST_SYM_RANGE = 1, 2, 4, 8
POINT_BLOCK, TILE, SYM_CHUNK = 512, 1024, 8
# NOPE_FIT_* (include/nope_hip.h): status bits of op_fit_translation, and the lanes of one pose's workgroup
FIT_NONFINITE, FIT_BAD_BOX, FIT_VERT_RANGE, FIT_BEHIND, FIT_NOT_CONVERGED = 1, 2, 4, 8, 16
FIT_THREADS = 256
# status bits of refine_translation_depth (host arithmetic; above the NOPE_FIT_* bits, so that one status word can carry both stages)
ST_DEPTH_FEW, ST_DEPTH_POSE = 256, 512
METRICS = ("mssd", "mspd", "add", "adi")
THRESHOLDS = tuple(round(0.05 * i, 2) for i in range(1, 11))           # 0.05 ... 0.50: the BOP19 sweep of theta and of tau / diameter
MSPD_THRESHOLDS = tuple(5.0 * i for i in range(1, 11))                 # px at an image width of 640


# ---- models_info.json, symmetry sets -----------------------------------------------------------------------------------------------
def load_models_info(path: str) -> Dict[int, dict]:
    """models_info.json of a BOP models directory (or the file itself): {obj_id: {"diameter": mm, "symmetries_discrete": [...16 numbers],
    "symmetries_continuous": [{"axis", "offset"}], ...}} with integer keys."""
    if os.path.isdir(path):
        path = os.path.join(path, "models_info.json")
    with open(path) as f:
        raw = json.load(f)
    return {int(k): v for k, v in raw.items()}


def _rodrigues(axis, angle: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    n = np.linalg.norm(a)
    if not n > 0:
        raise ValueError(f"symmetries_continuous: axis {axis!r}")
    a = a / n
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def symmetry_transforms(info: Optional[dict], max_sym_disc_step: float = 0.01) -> np.ndarray:
    """The symmetry set (S, 4, 4) f64 of one models_info entry: the toolkit's misc.get_symmetry_transformations.
    Discrete part: the identity, then every `symmetries_discrete` entry (16 numbers, a row-major 4x4).  Continuous part, per
    `symmetries_continuous` entry {axis, offset}: n = ceil(pi / max_sym_disc_step) rotations by i 2 pi / n about `axis` (Rodrigues),
    i = 0 ... n - 1, each with t = offset - R offset.  The set is every (continuous o discrete) pair, R = R_c R_d, t = R_c t_d + t_c,
    the continuous index outermost; without a continuous part it is the discrete part.
    The toolkit starts i at 1 and so drops the identity whenever a continuous symmetry exists; here i starts at 0, so the identity is always
    entry 0.  The difference can only lower an error, by less than one step of the discretisation."""
    info = info or {}
    disc = [np.eye(4)]
    for m in info.get("symmetries_discrete", []):
        m = np.asarray(m, dtype=np.float64)
        if m.size != 16:
            raise ValueError(f"symmetries_discrete: an entry of {m.size} numbers (16 expected)")
        disc.append(m.reshape(4, 4))
    cont = []
    for sym in info.get("symmetries_continuous", []):
        if not max_sym_disc_step > 0:
            raise ValueError(f"max_sym_disc_step {max_sym_disc_step}")
        n = int(math.ceil(math.pi / max_sym_disc_step))
        off = np.asarray(sym.get("offset", [0, 0, 0]), dtype=np.float64).reshape(3)
        for i in range(n):
            R = _rodrigues(sym["axis"], i * 2.0 * math.pi / n)
            T = np.eye(4)
            T[:3, :3] = R
            T[:3, 3] = off - R @ off
            cont.append(T)
    if not cont:
        return np.stack(disc)
    out = []
    for c in cont:
        for d in disc:
            T = np.eye(4)
            T[:3, :3] = c[:3, :3] @ d[:3, :3]
            T[:3, 3] = c[:3, :3] @ d[:3, 3] + c[:3, 3]
            out.append(T)
    return np.stack(out)


class SymmetryBank:
    """Symmetry sets concatenated into one device buffer (S_total, 4, 4) f64 with each object's range.  Entry 0 is the identity: the range
    of every object that is not listed."""

    def __init__(self, transforms: Optional[Dict[int, np.ndarray]] = None, device="cuda"):
        parts, self.sym_off, self.sym_cnt = [np.eye(4).reshape(1, 4, 4)], {}, {}
        n = 1
        for oid in sorted(transforms or {}):
            t = np.asarray(transforms[oid], dtype=np.float64).reshape(-1, 4, 4)
            if len(t) == 0:
                raise ValueError(f"SymmetryBank: object {oid} has an empty symmetry set (the identity is a member of every set)")
            parts.append(t)
            self.sym_off[int(oid)], self.sym_cnt[int(oid)] = n, len(t)
            n += len(t)
        self.syms = torch.from_numpy(np.concatenate(parts)).to(device).contiguous()
        self.device = self.syms.device

    @classmethod
    def from_models_info(cls, models_info: Dict[int, dict], device="cuda", max_sym_disc_step: float = 0.01) -> "SymmetryBank":
        return cls({oid: symmetry_transforms(info, max_sym_disc_step) for oid, info in models_info.items()}, device=device)

    def ranges(self, obj_ids: Iterable[int]):
        return [(self.sym_off.get(int(o), 0), self.sym_cnt.get(int(o), 1)) for o in obj_ids]


# ---- the two operators ----------------------------------------------------------------------------------------------------------------
def _i32(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.tensor(list(x), dtype=torch.int32)
    return t.to(device=device, dtype=torch.int32).contiguous()


def op_pose_errors(verts: torch.Tensor, vert_off, vert_cnt, max_verts: int, syms: torch.Tensor, sym_off, sym_cnt, max_syms: int,
                   pose_est, pose_gt, K, want: Sequence[str] = METRICS) -> Dict[str, torch.Tensor]:
    """nope_op_pose_errors as it is declared: verts (V, 3) f32 and syms (S_total, 4, 4) f64 on the device, ranges per pose (P,), poses
    (P, 4, 4), K (P, 3, 3).  Returns {metric: (P,) f64 for each of `want`, "status": (P,) int32 of ST_* bits}.  Nothing is checked here
    that the entry checks: bad ranges come back as NaN rows with their status bit."""
    for w in want:
        if w not in METRICS:
            raise ValueError(f"pose_errors: unknown metric {w!r} (known: {METRICS})")
    hip.require_device(verts)
    dev = verts.device
    pe, pg, Kt = _as_f64(pose_est, dev).reshape(-1, 4, 4), _as_f64(pose_gt, dev).reshape(-1, 4, 4), _as_f64(K, dev).reshape(-1, 3, 3)
    P = pe.shape[0]
    vo, vc, so, sc = (_i32(x, dev) for x in (vert_off, vert_cnt, sym_off, sym_cnt))
    if verts.dtype != torch.float32 or syms.dtype != torch.float64 or not verts.is_contiguous() or not syms.is_contiguous():
        raise hip.NopeError(f"pose_errors: verts {verts.dtype}, syms {syms.dtype}: contiguous f32 (V, 3) and f64 (S, 4, 4) expected")
    if pg.shape[0] != P or Kt.shape[0] != P or any(t.numel() != P for t in (vo, vc, so, sc)):
        raise hip.NopeError(f"pose_errors: {P} estimates, {pg.shape[0]} ground truths, K {tuple(Kt.shape)}, ranges "
                            f"{[t.numel() for t in (vo, vc, so, sc)]}")
    out = {w: torch.empty(P, dtype=torch.float64, device=dev) for w in want}
    status = torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        l = hip.lib()
        ws = torch.empty(int(l.dll.nope_op_pose_errors_workspace_bytes(P, int(max_verts), int(max_syms))), dtype=torch.uint8, device=dev)
        l.check(l.dll.nope_op_pose_errors(verts.data_ptr(), verts.shape[0], vo.data_ptr(), vc.data_ptr(), int(max_verts), syms.data_ptr(),
                                          syms.shape[0], so.data_ptr(), sc.data_ptr(), int(max_syms), pe.data_ptr(), pg.data_ptr(),
                                          Kt.data_ptr(), P, *(hip._ptr(out.get(m)) for m in METRICS), status.data_ptr(), ws.data_ptr(),
                                          ws.numel(), hip._stream(verts)), "nope_op_pose_errors")
    out["status"] = status
    return out


def op_mesh_diameter(verts: torch.Tensor, vert_off, vert_cnt, max_verts: int) -> torch.Tensor:
    """nope_op_mesh_diameter: (n_obj,) f64 diameters max_ij |x_i - x_j| of the vertex ranges; NaN for an empty or bad range."""
    hip.require_device(verts)
    dev = verts.device
    vo, vc = _i32(vert_off, dev), _i32(vert_cnt, dev)
    if verts.dtype != torch.float32 or not verts.is_contiguous() or vo.numel() != vc.numel():
        raise hip.NopeError(f"mesh_diameter: verts {verts.dtype}, {vo.numel()} offsets, {vc.numel()} counts")
    n = vo.numel()
    out = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        l = hip.lib()
        ws = torch.empty(int(l.dll.nope_op_mesh_diameter_workspace_bytes(n, int(max_verts))), dtype=torch.uint8, device=dev)
        l.check(l.dll.nope_op_mesh_diameter(verts.data_ptr(), verts.shape[0], vo.data_ptr(), vc.data_ptr(), n, int(max_verts), out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), hip._stream(verts)), "nope_op_mesh_diameter")
    return out


def mesh_diameters(bank: MeshBank) -> Dict[int, float]:
    """{obj_id: diameter in mm} of every mesh of the bank (the `diameter` of models_info.json, from the vertices)."""
    ids = bank.obj_ids
    rng = bank.vert_ranges(ids)
    d = op_mesh_diameter(bank.verts, [r[0] for r in rng], [r[1] for r in rng], max(r[1] for r in rng)).cpu().numpy()
    return {o: float(x) for o, x in zip(ids, d)}


def pose_errors(meshes: MeshBank, symmetries: Optional[SymmetryBank], obj_ids, pred_R, gt_R, gt_t, K, pred_t=None,
                want: Sequence[str] = METRICS) -> Dict[str, torch.Tensor]:
    """{metric: (B, k) f64} of k predicted rotations per query, plus "status" (B, k) int32 of ST_* bits.  Shapes as vsd.vsd_error's:
    obj_ids (B,); pred_R (B, k, 3, 3); gt_R (B, 3, 3); gt_t (B, 3, 1) or (B, 3) in mm; K (B, 3, 3) or (3, 3); pred_t (B, k, 3) or None:
    the predictions take the ground-truth translation, as vsd_error's do (the method predicts none).  symmetries None: the identity.
    mssd, add, adi are in mm, mspd in pixels.  A pose with a NaN or inf gives NaN in every metric; a vertex behind the camera gives
    NaN in mspd alone (status says which)."""
    dev = meshes.device
    pred_R, gt_R, gt_t = _as_f64(pred_R, dev), _as_f64(gt_R, dev), _as_f64(gt_t, dev)
    if pred_R.dim() != 4 or tuple(pred_R.shape[2:]) != (3, 3):
        raise hip.NopeError(f"pose_errors: pred_R {tuple(pred_R.shape)}: expected (B, k, 3, 3)")
    B, k = pred_R.shape[:2]
    ids = [int(o) for o in (obj_ids.tolist() if hasattr(obj_ids, "tolist") else obj_ids)]
    Kt = _as_f64(K, dev)
    if Kt.dim() == 2:
        Kt = Kt.reshape(1, 3, 3).expand(B, 3, 3).contiguous()
    if len(ids) != B or gt_R.shape != (B, 3, 3) or gt_t.numel() != 3 * B or tuple(Kt.shape) != (B, 3, 3):
        raise hip.NopeError(f"pose_errors: {len(ids)} obj_ids, pred_R {tuple(pred_R.shape)}, gt_R {tuple(gt_R.shape)}, gt_t {tuple(gt_t.shape)}, "
                            f"K {tuple(Kt.shape)}")
    gt_t = gt_t.reshape(B, 3)
    if pred_t is None:
        pt = gt_t.reshape(B, 1, 3).expand(B, k, 3)
    else:
        pt = _as_f64(pred_t, dev)
        if pt.numel() != 3 * B * k:
            raise hip.NopeError(f"pose_errors: pred_t {tuple(pt.shape)} for pred_R {tuple(pred_R.shape)}")
        pt = pt.reshape(B, k, 3)
    if B * k == 0:
        out = {w: torch.empty((B, k), dtype=torch.float64, device=dev) for w in want}
        out["status"] = torch.empty((B, k), dtype=torch.int32, device=dev)
        return out
    if symmetries is None:
        symmetries = SymmetryBank(None, device=dev)
    est = compose_poses(pred_R, pt).reshape(B * k, 4, 4)
    gt = compose_poses(gt_R, gt_t).reshape(B, 1, 4, 4).expand(B, k, 4, 4).reshape(B * k, 4, 4)
    Kp = Kt.reshape(B, 1, 3, 3).expand(B, k, 3, 3).reshape(B * k, 3, 3)
    vr = [r for r in meshes.vert_ranges(ids) for _ in range(k)]
    sr = [r for r in symmetries.ranges(ids) for _ in range(k)]
    out = op_pose_errors(meshes.verts, [r[0] for r in vr], [r[1] for r in vr], max(r[1] for r in vr), symmetries.syms,
                         [r[0] for r in sr], [r[1] for r in sr], max(r[1] for r in sr), est, gt, Kp, want)
    return {name: t.reshape(B, k) for name, t in out.items()}


# ---- translation from a 2D box, and its correction from depth ------------------------------------------------------------------------
def op_fit_translation(verts: torch.Tensor, vert_off, vert_cnt, max_verts: int, R, K, box, max_iters: int = 32, tol_scale: float = 1e-9,
                       tol_px: float = 1e-6) -> Dict[str, torch.Tensor]:
    """nope_op_fit_translation as it is declared: verts (V, 3) f32 on the device, ranges per pose (P,), R (P, 3, 3), K (P, 3, 3), box (P, 4)
    (u0, v0, u1, v1).  Returns {"t": (P, 3) f64, "residual": (P,) f64 pixels, "iters": (P,) int32, "status": (P,) int32 of FIT_* bits}.
    Nothing is checked here that the entry checks."""
    hip.require_device(verts)
    dev = verts.device
    Rt, Kt, bx = _as_f64(R, dev).reshape(-1, 3, 3), _as_f64(K, dev).reshape(-1, 3, 3), _as_f64(box, dev).reshape(-1, 4)
    P = Rt.shape[0]
    vo, vc = _i32(vert_off, dev), _i32(vert_cnt, dev)
    if verts.dtype != torch.float32 or not verts.is_contiguous():
        raise hip.NopeError(f"fit_translation: verts {verts.dtype}: contiguous f32 (V, 3) expected")
    if Kt.shape[0] != P or bx.shape[0] != P or vo.numel() != P or vc.numel() != P:
        raise hip.NopeError(f"fit_translation: {P} rotations, K {tuple(Kt.shape)}, box {tuple(bx.shape)}, ranges {[vo.numel(), vc.numel()]}")
    out = {"t": torch.empty((P, 3), dtype=torch.float64, device=dev), "residual": torch.empty(P, dtype=torch.float64, device=dev),
           "iters": torch.empty(P, dtype=torch.int32, device=dev), "status": torch.empty(P, dtype=torch.int32, device=dev)}
    if P:
        l = hip.lib()
        l.check(l.dll.nope_op_fit_translation(verts.data_ptr(), verts.shape[0], vo.data_ptr(), vc.data_ptr(), int(max_verts), Rt.data_ptr(),
                                              Kt.data_ptr(), bx.data_ptr(), P, int(max_iters), float(tol_scale), float(tol_px),
                                              out["t"].data_ptr(), out["residual"].data_ptr(), out["iters"].data_ptr(),
                                              out["status"].data_ptr(), hip._stream(verts)), "nope_op_fit_translation")
    return out


def _u8(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    t = t.to(device)
    return (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8)).contiguous()


def op_mask_boxes(mask: torch.Tensor):
    """nope_op_mask_boxes: mask (B, H, W) (uint8, or anything whose non-zero pixels count) -> (box (B, 4) f64 = (xmin, ymin, xmax + 1,
    ymax + 1), NaN for an empty mask; count (B,) int32)."""
    hip.require_device(mask)
    if mask.dim() != 3:
        raise hip.NopeError(f"mask_boxes: mask {tuple(mask.shape)}: expected (B, H, W)")
    m = _u8(mask, mask.device)
    B, H, W = m.shape
    box = torch.empty((B, 4), dtype=torch.float64, device=m.device)
    count = torch.empty(B, dtype=torch.int32, device=m.device)
    if B:
        l = hip.lib()
        l.check(l.dll.nope_op_mask_boxes(m.data_ptr(), B, H, W, box.data_ptr(), count.data_ptr(), hip._stream(m)), "nope_op_mask_boxes")
    return box, count


def op_depth_shift(depth_test: torch.Tensor, depth_est: torch.Tensor, tau: float, mask: Optional[torch.Tensor] = None):
    """nope_op_depth_shift: depth_test (B, H, W), depth_est (B, k, H, W) f32 mm, mask (B, H, W) or None -> (shift (B, k) f64: the mean of
    test - est over the pixels where both are > 0, the mask is set and |test - est| <= tau, NaN without such a pixel; count (B, k) int32)."""
    hip.require_device(depth_est)
    dev = depth_est.device
    f32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(device=dev, dtype=torch.float32).contiguous()
    dt, de = f32(depth_test), f32(depth_est)
    if de.dim() != 4 or dt.shape != de.shape[:1] + de.shape[2:]:
        raise hip.NopeError(f"depth_shift: depth_test {tuple(dt.shape)}, depth_est {tuple(de.shape)}: expected (B,H,W), (B,k,H,W)")
    B, k, H, W = de.shape
    if not 1 <= k <= 16:
        raise hip.NopeError(f"depth_shift: k = {k} estimates per query (1..16)")
    m = None
    if mask is not None:
        m = _u8(mask, dev)
        if tuple(m.shape) != (B, H, W):
            raise hip.NopeError(f"depth_shift: mask {tuple(m.shape)} for depth_test {tuple(dt.shape)}")
    shift = torch.empty((B, k), dtype=torch.float64, device=dev)
    count = torch.empty((B, k), dtype=torch.int32, device=dev)
    if B:
        l = hip.lib()
        ws = torch.empty(int(l.dll.nope_op_depth_shift_workspace_bytes(B, k, H, W)), dtype=torch.uint8, device=dev)
        l.check(l.dll.nope_op_depth_shift(dt.data_ptr(), de.data_ptr(), hip._ptr(m), B, k, H, W, float(tau), shift.data_ptr(), count.data_ptr(),
                                          ws.data_ptr(), ws.numel(), hip._stream(de)), "nope_op_depth_shift")
    return shift, count


def _batch_K(K, B: int, dev) -> torch.Tensor:
    Kt = _as_f64(K, dev)
    if Kt.dim() == 2:
        Kt = Kt.reshape(1, 3, 3).expand(B, 3, 3).contiguous()
    return Kt


def estimate_translation(meshes: MeshBank, obj_ids, pred_R, K, box=None, mask=None, max_iters: int = 32, tol_scale: float = 1e-9,
                         tol_px: float = 1e-6) -> Dict[str, torch.Tensor]:
    """The translation under which the projected box of mesh obj_ids[b] at rotation pred_R[b, j] is the detected box of query b
    (op_fit_translation).  obj_ids (B,); pred_R (B, k, 3, 3); K (B, 3, 3) or (3, 3); exactly one of box (B, 4) =
    (u0, v0, u1, v1) in the rasteriser's image coordinates and mask (B, H, W), whose box op_mask_boxes takes.  Returns {"t": (B, k, 3) f64
    mm, "residual": (B, k) f64 pixels (how well the rotation explains the box's aspect), "iters", "status": (B, k) int32 of FIT_* bits}.
    A candidate whose status is not 0 has no usable t (NaN, or not converged).  No host synchronisation."""
    if (box is None) == (mask is None):
        raise ValueError("estimate_translation: exactly one of box (B, 4) and mask (B, H, W) must be given")
    dev = meshes.device
    pred_R = _as_f64(pred_R, dev)
    if pred_R.dim() != 4 or tuple(pred_R.shape[2:]) != (3, 3):
        raise hip.NopeError(f"estimate_translation: pred_R {tuple(pred_R.shape)}: expected (B, k, 3, 3)")
    B, k = pred_R.shape[:2]
    ids = [int(o) for o in (obj_ids.tolist() if hasattr(obj_ids, "tolist") else obj_ids)]
    Kt = _batch_K(K, B, dev)
    if mask is not None:
        box = op_mask_boxes(mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.asarray(mask)).to(dev))[0]
    bx = _as_f64(box, dev)
    if len(ids) != B or tuple(Kt.shape) != (B, 3, 3) or tuple(bx.shape) != (B, 4):
        raise hip.NopeError(f"estimate_translation: {len(ids)} obj_ids, pred_R {tuple(pred_R.shape)}, K {tuple(Kt.shape)}, box {tuple(bx.shape)}")
    vr = [r for r in meshes.vert_ranges(ids) for _ in range(k)]
    if B * k == 0:
        return {"t": torch.empty((B, k, 3), dtype=torch.float64, device=dev), "residual": torch.empty((B, k), dtype=torch.float64, device=dev),
                "iters": torch.empty((B, k), dtype=torch.int32, device=dev), "status": torch.empty((B, k), dtype=torch.int32, device=dev)}
    out = op_fit_translation(meshes.verts, [r[0] for r in vr], [r[1] for r in vr], max(r[1] for r in vr), pred_R.reshape(B * k, 3, 3),
                             Kt.reshape(B, 1, 3, 3).expand(B, k, 3, 3).reshape(B * k, 3, 3), bx.reshape(B, 1, 4).expand(B, k, 4).reshape(B * k, 4),
                             max_iters, tol_scale, tol_px)
    return {name: t.reshape((B, k) + tuple(t.shape[1:])) for name, t in out.items()}


def refine_translation_depth(meshes: MeshBank, obj_ids, pred_R, t, K, depth_test, tau: float, mask=None, rounds: int = 2,
                             min_count: int = 1) -> Dict[str, torch.Tensor]:
    """The distance of k estimates per query corrected from a depth image.  Per round: the estimates are rendered at (pred_R, t)
    (vsd.render_depth), op_depth_shift gives the mean of test - rendered over the inliers within tau (mm; no default: nothing here is
    tuned), and t <- t (t_z + shift) / t_z: a move along the viewing ray, which keeps the box centre.  t (B, k, 3); depth_test (B, H, W)
    mm; mask (B, H, W) or None restricts the inliers to the detection.  Where a round finds fewer than min_count inliers (or none: a NaN
    shift) t is kept and ST_DEPTH_FEW is set; where t cannot be rendered (a NaN, t_z <= 0, a triangle at Z <= znear) or the corrected
    t_z would not be positive, t is kept and ST_DEPTH_POSE is set.  Returns {"t": (B, k, 3) f64, "shift": (B, k) f64 of the last round,
    "count": (B, k) int32 of the last round, "status": (B, k) int32}.  No host synchronisation."""
    from . import vsd
    dev = meshes.device
    pred_R, tt = _as_f64(pred_R, dev), _as_f64(t, dev)
    if pred_R.dim() != 4 or tuple(pred_R.shape[2:]) != (3, 3) or tt.numel() != 3 * pred_R.shape[0] * pred_R.shape[1]:
        raise hip.NopeError(f"refine_translation_depth: pred_R {tuple(pred_R.shape)}, t {tuple(tt.shape)}: expected (B, k, 3, 3), (B, k, 3)")
    B, k = pred_R.shape[:2]
    tt = tt.reshape(B, k, 3).clone()
    ids = [int(o) for o in (obj_ids.tolist() if hasattr(obj_ids, "tolist") else obj_ids)]
    dtest = (depth_test if isinstance(depth_test, torch.Tensor) else torch.from_numpy(np.asarray(depth_test))).to(device=dev, dtype=torch.float32)
    if len(ids) != B or dtest.dim() != 3 or dtest.shape[0] != B:
        raise hip.NopeError(f"refine_translation_depth: {len(ids)} obj_ids, pred_R {tuple(pred_R.shape)}, depth_test {tuple(dtest.shape)}")
    H, W = dtest.shape[-2:]
    Kp = _batch_K(K, B, dev).reshape(B, 1, 3, 3).expand(B, k, 3, 3).reshape(B * k, 3, 3)
    status = torch.zeros((B, k), dtype=torch.int32, device=dev)
    shift = torch.full((B, k), float("nan"), dtype=torch.float64, device=dev)
    count = torch.zeros((B, k), dtype=torch.int32, device=dev)
    if B * k == 0:
        return {"t": tt, "shift": shift, "count": count, "status": status}
    rep = [o for o in ids for _ in range(k)]
    for _ in range(int(rounds)):
        depth, skipped = vsd.render_depth(meshes, rep, compose_poses(pred_R, tt).reshape(B * k, 4, 4), Kp, H, W, return_skipped=True)
        shift, count = op_depth_shift(dtest, depth.reshape(B, k, H, W), tau, mask)
        tz = tt[..., 2]
        new_z = tz + shift
        bad_pose = (skipped.reshape(B, k) != 0) | ~torch.isfinite(tt).all(dim=-1) | ~(tz > 0)
        few = ~bad_pose & ((count < int(min_count)) | torch.isnan(shift))
        bad_pose = bad_pose | (~few & ~(new_z > 0))
        keep = bad_pose | few
        status = status | torch.where(few, ST_DEPTH_FEW, 0).to(torch.int32) | torch.where(bad_pose, ST_DEPTH_POSE, 0).to(torch.int32)
        tt = torch.where(keep[..., None], tt, tt * (new_z / tz)[..., None])
    return {"t": tt, "shift": shift, "count": count, "status": status}


# ---- recalls --------------------------------------------------------------------------------------------------------------------------
def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _best(err: np.ndarray, k: int) -> np.ndarray:
    """The best of the first k estimates per query, along the last axis; a NaN estimate never wins (and never passes a threshold)."""
    e = err[..., :k]
    return np.min(np.where(np.isnan(e), np.inf, e), axis=-1)


def bop_scores(errors: Dict[str, object], diameters, image_width: float, vsd_errors=None) -> Dict[str, float]:
    """Recalls of the BOP benchmark from (B, k) error tables (pose_errors): the share, in [0, 1], of queries whose error is < threshold,
    strict as in the toolkit's eval_calc_scores.  diameters: (B,) mm, of each query's object.  Per k in 1, 3, 5 (those <= the table's k):
    the best of the first k estimates, named after vsd_scores' pattern:
      "top {k}, AR_MSSD"      mean over theta in 0.05 ... 0.50 of recall(mssd < theta diameter)
      "top {k}, AR_MSPD"      mean over theta in 5 ... 50 of recall(mspd < theta image_width / 640) px
      "top {k}, ADD 0.1d", "top {k}, ADD-S 0.1d"    recall(add < 0.1 diameter), recall(adi < 0.1 diameter)
      "top {k}, AR_ADD", "top {k}, AR_ADD-S"        their means over theta in 0.05 ... 0.50
    and with vsd_errors, a (10, B, k) stack over tau in 0.05 ... 0.50 times the diameter:
      "top {k}, AR_VSD"       mean over tau and theta in 0.05 ... 0.50 of recall(vsd < theta)
      "top {k}, AR"           (AR_VSD + AR_MSSD + AR_MSPD) / 3, when all three are there
    Only the metrics present in `errors` are reported."""
    diam = _np(diameters).astype(np.float64).reshape(-1)
    tabs = {m: _np(errors[m]).astype(np.float64) for m in METRICS if m in errors}
    vs = None if vsd_errors is None else _np(vsd_errors).astype(np.float64)
    shapes = {t.shape for t in tabs.values()} | ({vs.shape[1:]} if vs is not None else set())
    if len(shapes) != 1:
        raise ValueError(f"bop_scores: error tables of shapes {sorted(shapes)}")
    B, kmax = next(iter(shapes))
    if diam.shape[0] != B or (vs is not None and vs.shape[0] != len(THRESHOLDS)):
        raise ValueError(f"bop_scores: {diam.shape[0]} diameters for {B} queries" + ("" if vs is None else f", vsd_errors {vs.shape}"))
    th = np.asarray(THRESHOLDS)
    scores: Dict[str, float] = {}
    for k in [k for k in (1, 3, 5) if k <= kmax]:
        sweep = {}
        for m in ("mssd", "add", "adi"):
            if m in tabs:
                sweep[m] = (_best(tabs[m], k)[None, :] < th[:, None] * diam[None, :]).mean(axis=1) if B else np.zeros(len(th))
        if "mssd" in sweep:
            scores[f"top {k}, AR_MSSD"] = float(sweep["mssd"].mean())
        if "mspd" in tabs:
            px = np.asarray(MSPD_THRESHOLDS) * (float(image_width) / 640.0)
            r = (_best(tabs["mspd"], k)[None, :] < px[:, None]).mean(axis=1) if B else np.zeros(len(px))
            scores[f"top {k}, AR_MSPD"] = float(r.mean())
        for m, name in (("add", "ADD"), ("adi", "ADD-S")):
            if m in sweep:
                scores[f"top {k}, {name} 0.1d"] = float(sweep[m][THRESHOLDS.index(0.1)])
                scores[f"top {k}, AR_{name}"] = float(sweep[m].mean())
        if vs is not None:
            best = _best(vs, k)                                                      # (10 tau, B)
            r = (best[:, None, :] < th[None, :, None]).mean(axis=2) if B else np.zeros((len(th), len(th)))
            scores[f"top {k}, AR_VSD"] = float(r.mean())
            if "mssd" in sweep and "mspd" in tabs:
                scores[f"top {k}, AR"] = (scores[f"top {k}, AR_VSD"] + scores[f"top {k}, AR_MSSD"] + scores[f"top {k}, AR_MSPD"]) / 3.0
    return scores
