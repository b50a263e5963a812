"""Dataset-side producer of the hot path's inputs: the virtual-bounding-box crop of a rendered
frame (`crop_frame`, src/poses/utils.py:204-272), the loader's image transform (src/dataloader/shapeNet.py:64-69) and the
assembly of a test-split sample as `ShapeNet.process` / `__getitem__` build it (shapeNet.py:265-357).

The reference does the crop with OpenCV on the host (`cv2.getPerspectiveTransform` + `cv2.warpPerspective`, one image at a
time); here the 3x3 map is solved on the host in float64 (same four-point system) and the warp runs on the GPU
(`nope_op_warp_perspective`, csrc/kernels_misc.hip), fused with `/255, *2-1, HWC->CHW`, so a frame never leaves the
device between decode and encoder.  cv2 is not installed in this environment and the reference ships no image fixtures:
the crop is **parity-unpinned** against OpenCV's fixed-point bilinear interpolation (it differs by interpolation-weight
quantisation, ~1/32 pixel); geometry (corner correspondences) and interpolation are checked against closed forms and
`torch.nn.functional.grid_sample` in tests/.

The test split itself (`class ShapeNet`, shapeNet.py:38-357 for a category split): the object list, the query / reference / template files,
their poses and the sample dict, with the loader's whole image chain -- paste on black, crop, ToTensor, * 2 - 1 -- for all frames of a
batch in ONE launch (`crop_frames` -> `nope_op_crop_frames`): PNGs are decoded on the host (PIL) and uploaded as they are, RGBA.  The
training splits and the zip repair of `open_image` stay out; the synset-id -> category table is data of the reference and is passed in.
"""
from __future__ import annotations

import glob
import json
import logging
import os
import os.path as osp
import random
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import hip
from .poses import compute_relative_pose, get_obj_poses_from_template_level, load_index_level0_in_level2

SHAPENET_INTRINSIC = np.array([[525.0, 0, 256], [0, 525.0, 256], [0, 0, 1]])      # shapeNet.py:175


def get_perspective_transform(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """3x3 M with M (src_i, 1) ~ (dst_i, 1) for four point pairs -- the system cv2.getPerspectiveTransform solves."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y, u, v = src[i, 0], src[i, 1], dst[i, 0], dst[i, 1]
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    h = np.linalg.solve(A, b)
    return np.append(h, 1.0).reshape(3, 3)


def perspective(K: np.ndarray, obj_pose: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """utils.py:50-57: project 3-D points, truncating to int32 as the reference does."""
    R, T = obj_pose[:3, :3], obj_pose[:3, 3]
    out = np.zeros((len(pts), 2))
    for i, p in enumerate(pts):
        rep = K @ (R @ p.reshape(3, 1) + T.reshape(3, 1))
        out[i, 0] = np.int32(rep[0, 0] / rep[2, 0])
        out[i, 1] = np.int32(rep[1, 0] / rep[2, 0])
    return out


def crop_transform(intrinsic: np.ndarray, openCV_pose: np.ndarray, image_size: int, keep_inplane: bool = False,
                   virtual_bbox_size: float = 0.3) -> np.ndarray:
    """The 3x3 map of `crop_frame` (utils.py:204-266): a square of side `virtual_bbox_size` facing the camera around the object
    origin, projected and mapped onto the (image_size x image_size) output."""
    origin = (openCV_pose @ np.array([0, 0, 0, 1.0]))[:3]
    if keep_inplane:
        upper = np.array([0.0, -origin[2], origin[1]])
        right = np.array([origin[1] ** 2 + origin[2] ** 2, -origin[0] * origin[1], -origin[0] * origin[2]])
    else:
        upV = np.array([0, 0, 6.0]) - origin
        upV = (openCV_pose @ np.array([upV[0], upV[1], upV[2], 1.0]))[:3]
        right = np.cross(origin, upV)
        upper = np.cross(right, origin)
    if np.linalg.norm(upper) == 0 and np.linalg.norm(right) == 0:
        upper, right = np.array([0.0, -1, 0]), np.array([1.0, 0, 0])
    upper = upper * (virtual_bbox_size / 2) / np.linalg.norm(upper)
    right = right * (virtual_bbox_size / 2) / np.linalg.norm(right)
    corners = np.stack([origin + upper - right, origin - upper - right, origin + upper + right, origin - upper + right])
    bbox2d = perspective(intrinsic, np.eye(4), corners).astype(np.int32).astype(np.float32)
    target = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.float32) * image_size
    return get_perspective_transform(bbox2d, target)


def crop_frame(img, mask, intrinsic, openCV_pose, image_size, keep_inplane=False, virtual_bbox_size=0.3,
               normalize: bool = False, round_u8: bool = False):
    """utils.py:204-272 with the warp on the device.  img (H,W,C) uint8 / f32 tensor (or array) -> (C,S,S) f32 tensor; raw values,
    or the loader's `/255 * 2 - 1` when `normalize`.  `round_u8` (uint8 frames): the warped value is rounded and clamped to
    [0, 255] before the transform, as the reference's uint8 `cv2.warpPerspective` output is before `ToTensor` -- the sample then
    lies on the same k/255 grid as the reference loader's (within one grey level where OpenCV's 1/32-pixel fixed-point weights
    round the other way: unpinned, cv2 is not installed).  Returns (img, mask) when a mask is given."""
    M = crop_transform(np.asarray(intrinsic, np.float64), np.asarray(openCV_pose, np.float64), image_size, keep_inplane, virtual_bbox_size)
    Minv = np.linalg.inv(M)
    def warp(a, norm):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        if t.dim() == 2:
            t = t[..., None]
        if not t.is_cuda and hip.compute_device().type == "cuda" and torch.cuda.is_available():
            t = t.cuda()
        sc, sh = ((2.0 / 255.0, -1.0) if t.dtype == torch.uint8 else (2.0, -1.0)) if norm else (1.0, 0.0)
        return hip.op_warp_perspective(t, Minv, image_size, sc, sh, round_u8=round_u8 and t.dtype == torch.uint8)
    out = warp(img, normalize)
    return (out, warp(mask, False)) if mask is not None else out


def process_test_sample(query_img, reference_img, template_imgs: Sequence, query_pose: np.ndarray, ref_pose: np.ndarray,
                        template_img_poses: Sequence[np.ndarray], testing_template_poses: np.ndarray, img_size: int = 256,
                        symmetry: int = 0) -> Dict[str, torch.Tensor]:
    """`ShapeNet.process` + `__getitem__` on the test split (shapeNet.py:265-357) for already decoded frames: crops (virtual bbox
    of size 1, shapeNet.py:171-184), image transform, relative poses; keys and shapes as the reference's sample dict."""
    crop = lambda im, pose: crop_frame(im, None, SHAPENET_INTRINSIC, pose, img_size, virtual_bbox_size=1, normalize=True, round_u8=True)
    rel, _ = compute_relative_pose(query_pose, ref_pose)
    all_rel = torch.stack([compute_relative_pose(testing_template_poses[i], ref_pose)[0] for i in range(len(template_imgs))])
    return {
        "query": crop(query_img, query_pose), "reference": crop(reference_img, ref_pose),
        "gt_relativeR": rel, "all_relativeR": all_rel,
        "gt_templates": torch.stack([crop(im, p) for im, p in zip(template_imgs, template_img_poses)]),
        "symmetry": torch.tensor([float(symmetry)]),
        "query_pose": torch.from_numpy(np.asarray(query_pose))[:3, :3],
        "template_poses": torch.from_numpy(np.asarray(testing_template_poses))[:, :3, :3],
    }


def decode_frame(path: str, mask_path: Optional[str] = None) -> np.ndarray:
    """`Image.open` of the loaders (shapeNet.py:184-186, bop.py:212-220) -> (H, W, 4) uint8 RGBA, NOT composited: the paste on black happens
    on the device, tap by tap (`crop_frames`).  A file without alpha gets alpha 255; `mask_path` (BOP's separate mask image) fills the alpha
    channel instead, with the first channel of a 3-channel mask.  A file PIL cannot read raises with its path (no zip repair)."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            rgba = np.array(im if im.mode == "RGBA" else im.convert("RGBA"), dtype=np.uint8)
        if mask_path is not None:
            with Image.open(mask_path) as mk:
                m = np.array(mk)
            if m.ndim == 3:
                m = m[:, :, 0]
            if m.shape != rgba.shape[:2]:
                raise ValueError(f"mask {mask_path} is {m.shape}, image is {rgba.shape[:2]}")
            rgba[:, :, 3] = m.astype(np.uint8)
    except Exception as e:
        raise OSError(f"{path}: cannot decode ({type(e).__name__}: {e})") from e
    return rgba


def _per_frame(v, F: int, shape: tuple) -> np.ndarray:
    """One value for every frame, or one per frame -> (F, *shape) float64."""
    a = np.asarray(v, np.float64)
    if a.shape == shape:
        return np.broadcast_to(a, (F,) + shape)
    if a.shape != (F,) + shape:
        raise ValueError(f"expected shape {shape} or {(F,) + shape}, got {a.shape}")
    return a


def crop_frames(frames, poses, intrinsics, image_size: int, virtual_bbox_sizes, keep_inplane: bool = False, normalize: bool = True,
                round_u8: bool = True) -> torch.Tensor:
    """`crop_frame` + image transform for a stack of frames: F uint8 frames (H, W, 3 | 4) -- one array / tensor (F, H, W, C) or a sequence of
    frames -- with their F openCV poses -> (F, 3, S, S) f32 on the device.  RGBA frames are pasted on black through their alpha on the way
    (shapeNet.py:206-208).  The F maps are solved on the host (`crop_transform`); frames and maps go up in ONE copy and are cropped by ONE
    `nope_op_crop_frames` launch (frames of different source sizes: one copy and one launch per size).  `intrinsics` (3, 3) and
    `virtual_bbox_sizes` (a number) may be given once or per frame; BOP's crop (bop.py:193-199) is `diameter * 1.2 / 1000` with the pose's
    translation in metres."""
    poses = np.asarray(poses, np.float64)
    F = len(poses)
    if F == 0 or len(frames) != F:
        raise ValueError(f"crop_frames: {len(frames)} frames, {F} poses")
    Ks, vbs = _per_frame(intrinsics, F, (3, 3)), _per_frame(virtual_bbox_sizes, F, ())
    minv = np.stack([np.linalg.inv(crop_transform(Ks[f], poses[f], image_size, keep_inplane, float(vbs[f]))) for f in range(F)])
    minv = np.ascontiguousarray(minv.reshape(F, 9), np.float32)
    scale, shift = (2.0 / 255.0, -1.0) if normalize else (1.0, 0.0)
    if isinstance(frames, torch.Tensor):            # already one stack, possibly on the device: only the maps travel
        dev = frames.device if frames.is_cuda else hip.compute_device()
        return hip.op_crop_frames(frames.to(dev), torch.from_numpy(minv).to(dev), image_size, scale, shift, round_u8)
    dev = hip.compute_device()
    groups: Dict[tuple, List[int]] = {}
    for f in range(F):
        fr = frames[f]
        if fr.dtype != np.uint8 or fr.ndim != 3:
            raise ValueError(f"crop_frames: frame {f} must be (H, W, C) uint8, got {fr.shape} {fr.dtype}")
        groups.setdefault(tuple(fr.shape), []).append(f)
    out = None
    for shape, idx in groups.items():
        n, per = len(idx), int(np.prod(shape))
        # one staging buffer = one upload: [n maps | n frames] (the maps first: 36 n bytes keep the RGBA taps' 32-bit loads aligned)
        host = torch.empty(n * 36 + n * per, dtype=torch.uint8, pin_memory=dev.type == "cuda")
        hv = host.numpy()
        hv[:n * 36].view(np.float32).reshape(n, 9)[:] = minv[idx]
        fv = hv[n * 36:].reshape((n,) + shape)
        for k, f in enumerate(idx):
            fv[k] = frames[f]
        buf = host.to(dev, non_blocking=True)
        res = hip.op_crop_frames(buf[n * 36:].view((n,) + shape), buf[:n * 36].view(torch.float32).view(n, 9), image_size, scale, shift, round_u8)
        if len(groups) == 1:
            return res
        if out is None:
            out = torch.empty((F, 3, image_size, image_size), dtype=torch.float32, device=res.device)
        out[torch.as_tensor(idx, device=res.device)] = res
    return out


def process_test_batch(query_frames: Sequence, reference_frames: Sequence, template_frames: Optional[Sequence], query_poses, ref_poses,
                       template_img_poses, testing_template_poses: np.ndarray, img_size: int = 256, symmetries: Optional[Sequence] = None,
                       with_templates: bool = True) -> Dict[str, torch.Tensor]:
    """`process_test_sample` for B samples from undecorated RGBA (or RGB) frames: the same keys, shapes and dtypes with a leading batch axis, all
    B * (2 [+ N]) frames through ONE `crop_frames` call.  query_frames / reference_frames: B frames; template_frames: B sequences of N frames
    with their poses template_img_poses (B, N, 4, 4); testing_template_poses (N, 4, 4): the grid, shared by the samples.  with_templates
    False (or no template frames): no "gt_templates" key -- they only feed the pictures (model.py:214-249)."""
    B = len(query_frames)
    grid = np.asarray(testing_template_poses)
    with_templates = bool(with_templates) and template_frames is not None
    frames, poses = list(query_frames) + list(reference_frames), list(query_poses) + list(ref_poses)
    N = 0
    if with_templates:
        N = len(template_frames[0])
        for b in range(B):
            if len(template_frames[b]) != N or len(template_img_poses[b]) != N:
                raise ValueError(f"process_test_batch: sample {b} has {len(template_frames[b])} template frames, sample 0 has {N}")
            frames += list(template_frames[b])
            poses += list(template_img_poses[b])
    crops = crop_frames(frames, np.stack([np.asarray(p, np.float64) for p in poses]), SHAPENET_INTRINSIC, img_size, 1, normalize=True, round_u8=True)
    n_rel = N if with_templates else len(grid)
    out = {
        "query": crops[:B], "reference": crops[B:2 * B],
        "gt_relativeR": torch.stack([compute_relative_pose(query_poses[b], ref_poses[b])[0] for b in range(B)]),
        "all_relativeR": torch.stack([torch.stack([compute_relative_pose(grid[i], ref_poses[b])[0] for i in range(n_rel)]) for b in range(B)]),
        "symmetry": torch.tensor([[float(symmetries[b]) if symmetries is not None else 0.0] for b in range(B)]),
        "query_pose": torch.stack([torch.from_numpy(np.asarray(query_poses[b]))[:3, :3] for b in range(B)]),
        "template_poses": torch.from_numpy(grid)[:, :3, :3].unsqueeze(0).repeat(B, 1, 1, 1),
    }
    out = {k: v.to(crops.device) for k, v in out.items()}          # the batch goes to the model as it is
    if with_templates:
        out["gt_templates"] = crops[2 * B:].view(B, N, 3, img_size, img_size)
    return out


class ShapeNet:
    """The reference's `ShapeNet` dataset (dataloader/shapeNet.py:38-357) for a TESTING split: `split` is a category name.  Same constructor
    arguments; `id2cat` = the synset-id -> category table (a dict, or the path of the reference's src/utils/shapeNet_id2cat_v2.json: data of
    the reference, not shipped here), `pose_root` = the reference's predefined_poses directory (None: the synthesised grids of
    nope_amd.poses, whose template numbering is this package's own), `seed` = the dataset's own random.Random (object shuffle, query order,
    reference choice: the reference draws from the global generator), `with_templates` = decode and crop the ground-truth templates too.
    `glob` results are sorted before they are shuffled, so the order does not depend on the file system.  Template frame i is cropped with row i
    of the object's template poses, as the reference does (`template_frame_poses`).  `__getitem__` returns the reference's
    sample dict with the images on the device; `load_batch(indices)` the collated batch from one `process_test_batch` call."""

    def __init__(self, root_dir, split, pose_distribution="upper", rot_representation="rotation6d", fast_evaluation=False, img_size=256, level=2,
                 id2cat: Union[dict, str, None] = None, seed: int = 2023, with_templates: bool = True, pose_root: Optional[str] = None):
        if split in ("training", "unseen_training"):
            raise NotImplementedError(f"ShapeNet(split={split!r}): only the testing splits (a category name) are built")
        if rot_representation != "rotation6d":
            raise NotImplementedError(f"ShapeNet(rot_representation={rot_representation!r}): only 'rotation6d' (configs/model: the U-Net's pose input)")
        if id2cat is None:
            raise ValueError("ShapeNet needs id2cat: the synset-id -> category table (dict, or path of the reference's shapeNet_id2cat_v2.json)")
        if not isinstance(id2cat, dict):
            with open(id2cat) as f:
                id2cat = json.load(f)
        self.id2cat = dict(id2cat)
        self.root_dir = str(root_dir)
        self.split, self.rot_representation, self.pose_distribution = split, rot_representation, pose_distribution
        self.fast_evaluation, self.level, self.img_size = fast_evaluation, level, img_size
        self.with_templates, self.pose_root = with_templates, pose_root
        self.rng = random.Random(seed)
        self.is_testing_split = True
        self.load_testing_template_poses()
        self.load_symmetry_mapping()
        self.load_metaData()
        logging.info(f"Length of dataset: query={len(self.query_paths)}")

    def __len__(self):
        return len(self.query_paths)

    def load_testing_template_poses(self):
        """shapeNet.py:252-263."""
        level = 0 if self.fast_evaluation else 2
        self.testing_indexes, self.testing_templates_poses = get_obj_poses_from_template_level(level, self.pose_distribution, return_index=True,
                                                                                               root=self.pose_root)
        if self.fast_evaluation and self.level == 2:
            self.testing_indexes = load_index_level0_in_level2(self.pose_distribution, root=self.pose_root)

    def _cad_names(self) -> List[str]:
        with open(osp.join(self.root_dir, "cad_names.txt")) as f:
            return [line.strip() for line in f.readlines()]

    def load_symmetry_mapping(self):
        """shapeNet.py:156-165."""
        self.all_cad_names = self._cad_names()
        self.obj_name2symmetry = {f"obj_{i:06d}": 2 if self.id2cat[name.split("_")[0]] in ["bottle"] else 0
                                  for i, name in enumerate(self.all_cad_names)}

    def get_img_from_paths(self, paths: Sequence[str]) -> List[str]:
        """shapeNet.py:88-106 on a testing split: every query_*.png under the object folders, sorted, then shuffled."""
        all_images: List[str] = []
        for path in paths:
            all_images += sorted(glob.glob(osp.join(path, "query_*.png")))
        self.rng.shuffle(all_images)
        return all_images

    def load_metaData(self):
        """shapeNet.py:108-154 on a testing split: the category's objects in cad_names.txt order, shuffled, the first 100; objects without a
        folder are skipped with a warning."""
        ids = [i for i, name in enumerate(self.all_cad_names) if self.id2cat[name.split("_")[0]] == self.split]
        self.rng.shuffle(ids)
        self.obj_ids = ids[:100]
        obj_paths, self.query_to_references = [], {}
        for obj_id in self.obj_ids:
            obj_path = f"{self.root_dir}/images/obj_{obj_id:06d}"
            if not os.path.exists(obj_path):
                logging.warning(f"Path {obj_path} does not exist")
                continue
            obj_paths.append(obj_path)
            self.query_to_references[f"obj_{obj_id:06d}"] = self.get_img_from_paths([obj_path])
        self.query_paths = self.get_img_from_paths(obj_paths)

    def sample_reference(self, query_path: str) -> str:
        """shapeNet.py:222-229."""
        ref_paths = sorted(glob.glob(osp.join(osp.dirname(query_path), "reference*.png")))
        if not ref_paths:
            raise FileNotFoundError(f"no reference*.png next to {query_path}")
        return self.rng.choice(ref_paths)

    def get_pose(self, path: str) -> np.ndarray:
        """shapeNet.py:231-241."""
        obj_name, filename = osp.basename(osp.dirname(path)), osp.basename(path)
        kind = filename.split("_")[0]
        if kind == "templates":
            kind = "template"
        idx = int(filename.split("_")[1].split(".")[0])
        return np.load(osp.join(self.root_dir, f"object_{kind}_poses", obj_name + ".npy"))[idx]

    def get_symmetry(self, query_path: str) -> torch.Tensor:
        return torch.Tensor([self.obj_name2symmetry[osp.basename(osp.dirname(query_path))]])

    def template_paths(self, query_path: str) -> List[str]:
        """shapeNet.py:287-291: the template frames of the query's object, in the order of the testing grid."""
        return [f"{osp.dirname(query_path)}/templates_{idx:06d}.png" for idx in self.testing_indexes]

    def template_frame_poses(self, query_path: str) -> List[np.ndarray]:
        """shapeNet.py:292-299: the pose template frame i is CROPPED with.  The reference opens `templates_{testing_indexes[i]}.png` but asks
        `get_pose` for `templates_{i}.png`, i = 0 .. N - 1: row i of the object's template-pose file, not row testing_indexes[i].  That is
        followed here (the rendered data decides whether the file is indexed by grid position or by template number; with fast_evaluation the two
        differ in the reference as well).  These crops only feed the pictures."""
        obj_path = osp.dirname(query_path)
        return [self.get_pose(f"{obj_path}/templates_{i:06d}.png") for i in range(len(self.testing_indexes))]

    def load_batch(self, indices: Sequence[int], reference_paths: Optional[Sequence[str]] = None, with_templates: Optional[bool] = None):
        """The collated batch of samples `indices` (what a DataLoader over the reference's dataset hands to `PoseConditional.test_step` under
        the key f"shapeNet_{split}"): decode on the host, then one `process_test_batch` call.  reference_paths: the reference frame of each
        sample instead of a random one."""
        with_templates = self.with_templates if with_templates is None else with_templates
        q_paths = [self.query_paths[i] for i in indices]
        r_paths = list(reference_paths) if reference_paths is not None else [self.sample_reference(q) for q in q_paths]
        t_frames = t_poses = None
        if with_templates:
            t_paths = [self.template_paths(q) for q in q_paths]
            t_frames = [[decode_frame(p) for p in ps] for ps in t_paths]
            t_poses = [self.template_frame_poses(q) for q in q_paths]
        return process_test_batch([decode_frame(p) for p in q_paths], [decode_frame(p) for p in r_paths], t_frames,
                                  [self.get_pose(p) for p in q_paths], [self.get_pose(p) for p in r_paths], t_poses, self.testing_templates_poses,
                                  self.img_size, [float(self.get_symmetry(q)) for q in q_paths], with_templates)

    def __getitem__(self, index: int, reference_path: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """shapeNet.py:325-357 on a testing split."""
        batch = self.load_batch([index], None if reference_path is None else [reference_path])
        return {k: v[0] for k, v in batch.items()}
