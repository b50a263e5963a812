"""VSD (Visible Surface Discrepancy, the BOP pose error) on the device -- the T-LESS evaluation of the reference:
src/poses/vsd.py:25-132 (`pyrenderer`, `vsd_obj`), src/poses/vsd_utils.py (distance images and visibility masks from bop_toolkit)
and the aggregation of PoseConditional.eval_vsd, src/model/model.py:530-537.

Depth maps are rendered by a HIP rasteriser (nope_op_render_depth) instead of pyrender's OpenGL renderer, and the per-pose VSD
arithmetic runs in one HIP pass (nope_op_vsd).  Meshes are read with plain numpy (`load_ply`, no trimesh) and depth PNGs with PIL
(`load_depth`, no cv2).  The reference's glue (model.py:470-541 calling vsd.py:57) does not run as written; what is followed is its
per-frame arithmetic (vsd_obj) and its `final_scores`.
"""
from __future__ import annotations

import os
import struct
from typing import Dict, Iterable, Sequence

import numpy as np
import torch

from . import hip

VSD_STEP, VSD_TLINEAR = 0, 1          # NOPE_VSD_* (include/nope_hip.h)
VISIB_BOP19, VISIB_BOP18 = 0, 1       # NOPE_VISIB_*
_COST = {"step": VSD_STEP, "tlinear": VSD_TLINEAR}
_VISIB = {"bop19": VISIB_BOP19, "bop18": VISIB_BOP18}

# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def load_ply(path: str):
    """(vertices (V,3) float32, faces (F,3) int32) of an ascii or binary_little_endian PLY: vertex x / y / z as float or double (other
    vertex properties are read and dropped), face lists with any integer count type, polygons fan-triangulated (0, i, i + 1)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data[data.index(b"\n", end) + 1:]
    fmt, elements = None, []
    for line in data[:end].decode("ascii").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info", "ply"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], "list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None, None))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} (ascii and binary_little_endian are read)")
    verts, faces = None, None
    if fmt == "ascii":
        words = body.split()
        pos = 0
        for name, n, props in elements:
            rows = []
            for _ in range(n):
                row = {}
                for pname, kind, ctype, itype in props:
                    if kind == "list":
                        c = int(words[pos]); pos += 1
                        row[pname] = [int(w) for w in words[pos:pos + c]]; pos += c
                    else:
                        row[pname] = float(words[pos]); pos += 1
                rows.append(row)
            if name == "vertex":
                verts = np.array([[r["x"], r["y"], r["z"]] for r in rows], dtype=np.float64).reshape(n, 3)
            elif name == "face":
                key = "vertex_indices" if props and any(p[0] == "vertex_indices" for p in props) else props[0][0]
                faces = [r[key] for r in rows]
    else:
        pos = 0
        for name, n, props in elements:
            if all(p[1] != "list" for p in props):
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                arr = np.frombuffer(body, dtype=dt, count=n, offset=pos)
                pos += n * dt.itemsize
                if name == "vertex":
                    verts = np.stack([arr["x"], arr["y"], arr["z"]], axis=1).astype(np.float64)
                continue
            rows = []
            for _ in range(n):
                row = {}
                for pname, kind, ctype, itype in props:
                    if kind == "list":
                        c = int(np.frombuffer(body, "<" + ctype, 1, pos)[0]); pos += np.dtype(ctype).itemsize
                        row[pname] = np.frombuffer(body, "<" + itype, c, pos).astype(np.int64).tolist(); pos += c * np.dtype(itype).itemsize
                    else:
                        pos += np.dtype(kind).itemsize
                rows.append(row)
            if name == "face":
                key = "vertex_indices" if any(p[0] == "vertex_indices" for p in props) else props[0][0]
                faces = [r[key] for r in rows]
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    tris = []
    for poly in faces or []:
        for i in range(1, len(poly) - 1):
            tris.append((poly[0], poly[i], poly[i + 1]))
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError(f"{path}: a face indexes a vertex outside [0, {len(verts)})")
    return verts.astype(np.float32), tris.astype(np.int32)


def save_ply(path: str, verts, faces, binary: bool = True):
    """Write a PLY (float x / y / z, uchar-counted int face lists); polygons of any size may be given as a list of index lists."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = [list(map(int, f)) for f in faces]
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {len(verts)}", "property float x",
            "property float y", "property float z", f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(verts.astype("<f4").tobytes())
            for poly in faces:
                f.write(struct.pack("<B", len(poly)) + np.asarray(poly, dtype="<i4").tobytes())
        else:
            for v in verts:
                f.write(("%r %r %r\n" % tuple(float(x) for x in v)).encode("ascii"))
            for poly in faces:
                f.write((" ".join(str(x) for x in [len(poly)] + poly) + "\n").encode("ascii"))


def load_depth(path: str, scale: float = 0.1) -> np.ndarray:
    """A 16-bit depth PNG in mm, f64: `cv2.imread(path, -1) / 10.0` (vsd.py:74) for the default scale 0.1 (BOP's depth_scale)."""
    from PIL import Image
    with Image.open(path) as im:
        raw = np.array(im)
    if raw.dtype not in (np.uint16, np.int32, np.uint8, np.int16, np.uint32):
        raise ValueError(f"{path}: expected an integer depth image, got {raw.dtype}")
    return raw / 10.0 if scale == 0.1 else raw * float(scale)


# ---- meshes on the device -------------------------------------------------------------------------------------------------------------
class MeshBank:
    """Meshes concatenated into one device vertex buffer (V,3) f32 and one face buffer (F,3) int32 (global vertex indices), with each
    object's face range and vertex range: one rasteriser launch (or one pose-error launch, nope_amd/bop.py) serves a batch of mixed
    objects."""

    def __init__(self, meshes: Dict[int, tuple], device="cuda"):
        if not meshes:
            raise ValueError("MeshBank needs at least one mesh")
        vs, fs, self.face_off, self.face_cnt = [], [], {}, {}
        self.vert_off, self.vert_cnt = {}, {}
        nv = nf = 0
        for oid in sorted(meshes):
            v, f = meshes[oid]
            v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
            f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
            if f.size and (f.min() < 0 or f.max() >= len(v)):
                raise ValueError(f"mesh {oid}: a face indexes a vertex outside [0, {len(v)})")
            vs.append(v)
            fs.append(f + nv)
            self.face_off[int(oid)], self.face_cnt[int(oid)] = nf, len(f)
            self.vert_off[int(oid)], self.vert_cnt[int(oid)] = nv, len(v)
            nv += len(v)
            nf += len(f)
        if nv == 0 or nf == 0 or nv >= 2 ** 31 or nf >= 2 ** 31:
            raise ValueError(f"MeshBank: {nv} vertices / {nf} faces")
        self.verts = torch.from_numpy(np.concatenate(vs)).to(device).contiguous()
        self.faces = torch.from_numpy(np.concatenate(fs).astype(np.int32)).to(device).contiguous()
        self.device = self.verts.device

    @property
    def obj_ids(self):
        return sorted(self.face_off)

    def ranges(self, obj_ids: Iterable[int]):
        try:
            return [(self.face_off[int(o)], self.face_cnt[int(o)]) for o in obj_ids]
        except KeyError as e:
            raise KeyError(f"obj_id {e.args[0]} is not in the mesh bank (loaded: {self.obj_ids})") from None

    def vert_ranges(self, obj_ids: Iterable[int]):
        try:
            return [(self.vert_off[int(o)], self.vert_cnt[int(o)]) for o in obj_ids]
        except KeyError as e:
            raise KeyError(f"obj_id {e.args[0]} is not in the mesh bank (loaded: {self.obj_ids})") from None


def _as_f64(x, device) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return t.to(device=device, dtype=torch.float64).contiguous()


def render_depth(bank: MeshBank, obj_ids: Sequence[int], poses, K, height: int, width: int, return_skipped: bool = False):
    """Depth maps (P, H, W) f32 in mm of mesh obj_ids[p] under poses[p] (4x4 object-to-camera, OpenCV axes) with intrinsics K[p] (3x3;
    one (3, 3) K serves every pose): pyrenderer(..., DEPTH_ONLY) of vsd.py:25-54 on the device.  Pixel (x, y) samples the image point
    (x + 0.5, y + 0.5).  A pose that puts a vertex at Z <= 0.05 (pyrender's znear) raises: the renderer skips such triangles.
    return_skipped: nothing is raised and nothing waits for the device; (depth, skipped (P,) int32: the triangles each pose skipped) is
    returned and the caller decides (a NaN pose skips every triangle)."""
    dev = bank.device
    hip.require_device(bank.verts)
    obj_ids = [int(o) for o in (obj_ids.tolist() if hasattr(obj_ids, "tolist") else obj_ids)]
    P = len(obj_ids)
    poses = _as_f64(poses, dev).reshape(-1, 4, 4)
    K = _as_f64(K, dev)
    if K.dim() == 2:
        K = K.reshape(1, 3, 3).expand(P, 3, 3).contiguous()
    if poses.shape[0] != P or tuple(K.shape) != (P, 3, 3):
        raise hip.NopeError(f"render_depth: {P} obj_ids, poses {tuple(poses.shape)}, K {tuple(K.shape)}")
    depth = torch.empty((P, height, width), dtype=torch.float32, device=dev)
    if P == 0:
        return (depth, torch.empty(0, dtype=torch.int32, device=dev)) if return_skipped else depth
    rng = bank.ranges(obj_ids)
    off = torch.tensor([r[0] for r in rng], dtype=torch.int32).to(dev)
    cnt = torch.tensor([r[1] for r in rng], dtype=torch.int32).to(dev)
    max_faces = max(r[1] for r in rng)
    skipped = torch.empty(P, dtype=torch.int32, device=dev)
    l = hip.lib()
    ws = torch.empty(int(l.dll.nope_op_render_depth_workspace_bytes(P, max_faces)), dtype=torch.uint8, device=dev)
    l.check(l.dll.nope_op_render_depth(bank.verts.data_ptr(), bank.verts.shape[0], bank.faces.data_ptr(), bank.faces.shape[0], off.data_ptr(),
                                       cnt.data_ptr(), max_faces, poses.data_ptr(), K.data_ptr(), P, height, width, depth.data_ptr(),
                                       skipped.data_ptr(), ws.data_ptr(), ws.numel(), hip._stream(depth)), "nope_op_render_depth")
    if return_skipped:
        return depth, skipped
    sk = skipped.cpu()
    if bool((sk != 0).any()):
        bad = [(p, int(sk[p])) for p in range(P) if sk[p] != 0]
        raise hip.NopeError("render_depth: triangles with a vertex at Z <= znear (0.05 mm) were skipped: "
                            + ", ".join(f"pose {p} (obj_id {obj_ids[p]}): {n} triangles" for p, n in bad[:8]))
    return depth


def vsd_from_depth(depth_test, depth_gt, depth_est, K, delta=15, tau=20, cost_type="step", visib_mode="bop19") -> torch.Tensor:
    """VSD errors (B, k) f64 from depth maps in mm: depth_test / depth_gt (B, H, W), depth_est (B, k, H, W), K (B, 3, 3) or (3, 3).
    The per-pose loop of vsd_obj (vsd.py:91-131) in one device pass (nope_op_vsd)."""
    if cost_type not in _COST:
        raise ValueError("Unknown pixel matching cost.")        # vsd.py:124
    if visib_mode not in _VISIB:
        raise ValueError("Unknown visibility mode.")            # vsd_utils.py:109
    dev = depth_est.device if isinstance(depth_est, torch.Tensor) else torch.device("cuda")
    f32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(device=dev, dtype=torch.float32).contiguous()
    dt, dg, de = f32(depth_test), f32(depth_gt), f32(depth_est)
    hip.require_device(de)
    if de.dim() != 4 or dt.shape != de.shape[:1] + de.shape[2:] or dg.shape != dt.shape:
        raise hip.NopeError(f"vsd: depth_test {tuple(dt.shape)}, depth_gt {tuple(dg.shape)}, depth_est {tuple(de.shape)}: expected (B,H,W), (B,H,W), (B,k,H,W)")
    B, k, H, W = de.shape
    if not 1 <= k <= 16:
        raise hip.NopeError(f"vsd: k = {k} estimates per query (1..16)")
    Kt = _as_f64(K, dev)
    if Kt.dim() == 2:
        Kt = Kt.reshape(1, 3, 3).expand(B, 3, 3).contiguous()
    if tuple(Kt.shape) != (B, 3, 3):
        raise hip.NopeError(f"vsd: K {tuple(Kt.shape)} for {B} queries")
    err = torch.empty((B, k), dtype=torch.float64, device=dev)
    if B == 0:
        return err
    l = hip.lib()
    ws = torch.empty(int(l.dll.nope_op_vsd_workspace_bytes(B, k, H, W)), dtype=torch.uint8, device=dev)
    l.check(l.dll.nope_op_vsd(dt.data_ptr(), dg.data_ptr(), de.data_ptr(), Kt.data_ptr(), B, k, H, W, float(delta), float(tau), _COST[cost_type],
                              _VISIB[visib_mode], err.data_ptr(), ws.data_ptr(), ws.numel(), hip._stream(de)), "nope_op_vsd")
    return err


def compose_poses(R, t) -> torch.Tensor:
    """[R | t; 0 0 0 1] (..., 4, 4) f64 from R (..., 3, 3) and t (..., 3, 1) or (..., 3)."""
    R = R if isinstance(R, torch.Tensor) else torch.from_numpy(np.asarray(R))
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
    R, t = R.double(), t.double().to(R.device)
    out = torch.zeros(R.shape[:-2] + (4, 4), dtype=torch.float64, device=R.device)
    out[..., :3, :3] = R
    out[..., :3, 3] = t.reshape(R.shape[:-2] + (3,))
    out[..., 3, 3] = 1.0
    return out


def vsd_error(depth_test, meshes: MeshBank, obj_ids, pred_R, gt_R, gt_t, K, delta=15, tau=20, cost_type="step",
              use_gt_translation=True, visib_mode="bop19", return_depth=False, pred_t=None):
    """VSD errors (B, k) f64 of k predicted rotations per query -- vsd_obj (vsd.py:57-132), batched over B queries.
    depth_test (B, H, W) in mm (load_depth); obj_ids (B,); pred_R (B, k, 3, 3); gt_R (B, 3, 3); gt_t (B, 3, 1) or (B, 3) in mm;
    K (B, 3, 3).  The predictions take the ground-truth translation (use_gt_translation=True, vsd.py:84-87; False raises
    NotImplementedError as the reference does) unless pred_t (B, k, 3) is given (nope_amd.bop.estimate_translation): then the
    estimates are rendered at it, and it has to be renderable (finite, every vertex beyond znear).  The B (1 + k) depth maps are rendered
    in one launch.  return_depth: also return (depth_gt (B,H,W), depth_est (B,k,H,W))."""
    if pred_t is None and not use_gt_translation:
        raise NotImplementedError
    if cost_type not in _COST:
        raise ValueError("Unknown pixel matching cost.")
    dev = meshes.device
    pred_R = _as_f64(pred_R, dev)
    gt_R = _as_f64(gt_R, dev)
    gt_t = _as_f64(gt_t, dev)
    B, k = pred_R.shape[:2]
    dtest = depth_test if isinstance(depth_test, torch.Tensor) else torch.from_numpy(np.asarray(depth_test))
    H, W = dtest.shape[-2:]
    Kt = _as_f64(K, dev)
    if Kt.dim() == 2:
        Kt = Kt.reshape(1, 3, 3).expand(B, 3, 3).contiguous()
    gt_pose = compose_poses(gt_R, gt_t)                                              # (B, 4, 4)
    if pred_t is None:
        pt = gt_t.reshape(B, 1, 3).expand(B, k, 3)                                   # translation of the ground truth
    else:
        pt = _as_f64(pred_t, dev)
        if pt.numel() != 3 * B * k:
            raise hip.NopeError(f"vsd_error: pred_t {tuple(pt.shape)} for pred_R {tuple(pred_R.shape)}")
        pt = pt.reshape(B, k, 3)
    pred_pose = compose_poses(pred_R, pt)                                            # (B, k, 4, 4)
    ids = [int(o) for o in (obj_ids.tolist() if hasattr(obj_ids, "tolist") else obj_ids)]
    all_pose = torch.cat([gt_pose.reshape(B, 1, 4, 4), pred_pose], dim=1).reshape(B * (1 + k), 4, 4)
    all_K = Kt.reshape(B, 1, 3, 3).expand(B, 1 + k, 3, 3).reshape(B * (1 + k), 3, 3)
    depth = render_depth(meshes, [o for o in ids for _ in range(1 + k)], all_pose, all_K, H, W).reshape(B, 1 + k, H, W)
    d_gt, d_est = depth[:, 0], depth[:, 1:]
    err = vsd_from_depth(dtest, d_gt.contiguous(), d_est.contiguous(), Kt, delta, tau, cost_type, visib_mode)
    return (err, d_gt, d_est) if return_depth else err


def vsd_scores(err) -> Dict[str, float]:
    """`final_scores` of eval_vsd (model.py:530-537) from the (B, k >= 5) errors: per k in 1, 3, 5 the median of the best of the first k
    and the percentage of queries whose best error is <= 0.3."""
    err = err.detach().cpu().numpy() if isinstance(err, torch.Tensor) else np.asarray(err)
    final_scores = {}
    for k in [1, 3, 5]:
        best_vsd = np.min(err[:, :k], 1)
        final_scores[f"top {k}, vsd_median"] = float(np.median(best_vsd))
        for threshold in [0.3]:
            vsd_acc = (best_vsd <= threshold) * 100.0
            final_scores[f"top {k}, vsd_scores {threshold}"] = float(np.mean(vsd_acc))
    return final_scores


def load_mesh_bank(cad_dir: str, obj_ids: Iterable[int] = range(1, 31), device="cuda") -> MeshBank:
    """obj_000001.ply ... obj_000030.ply of a BOP models directory (model.py:378-389) as one MeshBank."""
    meshes = {}
    for oid in obj_ids:
        meshes[int(oid)] = load_ply(os.path.join(cad_dir, f"obj_{int(oid):06d}.ply"))
    return MeshBank(meshes, device=device)


# ---- synthetic meshes (tests, tools/vsd_bench.py) -------------------------------------------------------------------------------------
def icosphere(level: int, radius: float = 1.0):
    """(verts (V,3) f32, faces (20 * 4^level, 3) int32): the icosahedron subdivided `level` times, vertices on the sphere, faces
    wound outwards."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nf
    return (np.asarray(verts) * radius).astype(np.float32), np.asarray(faces, dtype=np.int32)


def box(sx: float, sy: float, sz: float):
    """(verts (8,3) f32, faces (12,3) int32): a closed axis-aligned box centred at the origin."""
    verts = np.array([[x, y, z] for x in (-sx / 2, sx / 2) for y in (-sy / 2, sy / 2) for z in (-sz / 2, sz / 2)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return verts, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
