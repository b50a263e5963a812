"""A synthetic rendered-ShapeNet root in the reference's layout (dataloader/shapeNet.py: cad_names.txt, images/obj_*/{query,reference,templates}_*.png,
object_{query,reference,template}_poses/obj_*.npy), built from a seed: tests/golden/make_golden_shapenet.py runs the reference's `ShapeNet` over it and
tests/test_shapenet_dataset.py rebuilds the same root for nope_amd.dataset.ShapeNet.  Three made-up synset ids (tests/golden/shapenet_id2cat_synthetic.json):
bottle (6 objects), mug (104 objects, so the [:100] cut bites; one of them has no folder) and chair, a training category (5 objects)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ID2CAT_PATH = os.path.join(HERE, "golden", "shapenet_id2cat_synthetic.json")
SEED = 20231
N_QUERY, N_REFERENCE, N_TEMPLATE_POSES = 2, 2, 642
COUNTS = {"bottle": 6, "mug": 104, "chair": 5}
MISSING_MUG = 17                  # the 18th mug of cad_names.txt has no folder


def id2cat():
    with open(ID2CAT_PATH) as f:
        return json.load(f)


def cad_categories():
    """The category of every line of cad_names.txt: the three categories interleaved."""
    left, cats = dict(COUNTS), []
    while any(left.values()):
        for c in ("mug", "bottle", "chair", "mug"):
            if left[c]:
                cats.append(c)
                left[c] -= 1
    return cats


# An object here has its unit crop box (dataset.SHAPENET_INTRINSIC: focal 525, centre 256) over a 64 x 64 frame: 525 / 8.2 = 64 pixels around (32, 32)
OVER_64_FRAME = (-3.5, -3.5, 8.2)


def _poses(rng, n, translation=(0.0, 0.0, 1.0)):
    """n object poses: Haar rotations (QR of a Gaussian), the object at `translation` (by default about one unit in front of the camera), slightly off it."""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=-2, axis2=-1))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = q
    T[:, :3, 3] = np.array(translation, np.float64) + rng.normal(size=(n, 3)) * 0.03
    return T


def build_root(root, template_indexes=(), image_hw=(4, 4), translation=(0.0, 0.0, 1.0)):
    """Write the root.  template_indexes: the templates_{idx:06d}.png written for the BOTTLE objects (the only ones samples are drawn from).
    translation: where the poses put the objects.  Returns the object ids of each category."""
    from PIL import Image
    rng = np.random.default_rng(SEED)
    cat2id = {c: s for s, c in id2cat().items()}
    cats = cad_categories()
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "cad_names.txt"), "w") as f:
        for i, c in enumerate(cats):
            f.write(f"{cat2id[c]}_{i * 7919 % 100003:08x}\n")
    for kind in ("query", "reference", "template"):
        os.makedirs(os.path.join(root, f"object_{kind}_poses"), exist_ok=True)
    by_cat, mugs = {c: [] for c in COUNTS}, 0
    for i, c in enumerate(cats):
        by_cat[c].append(i)
        name = f"obj_{i:06d}"
        frames = rng.integers(0, 256, size=(N_QUERY + N_REFERENCE,) + tuple(image_hw) + (4,), dtype=np.uint8)
        poses = {"query": _poses(rng, N_QUERY, translation), "reference": _poses(rng, N_REFERENCE, translation),
                 "template": _poses(rng, N_TEMPLATE_POSES if c == "bottle" else 1, translation)}
        for kind, p in poses.items():
            np.save(os.path.join(root, f"object_{kind}_poses", name + ".npy"), p)
        if c == "mug":
            mugs += 1
            if mugs - 1 == MISSING_MUG:
                continue
        d = os.path.join(root, "images", name)
        os.makedirs(d, exist_ok=True)
        for k in range(N_QUERY):
            Image.fromarray(frames[k], "RGBA").save(os.path.join(d, f"query_{k:06d}.png"))
        for k in range(N_REFERENCE):
            Image.fromarray(frames[N_QUERY + k], "RGBA").save(os.path.join(d, f"reference_{k:06d}.png"))
        if c == "bottle":
            for idx in template_indexes:
                t = np.random.default_rng([SEED, i, int(idx)]).integers(0, 256, size=tuple(image_hw) + (4,), dtype=np.uint8)
                Image.fromarray(t, "RGBA").save(os.path.join(d, f"templates_{int(idx):06d}.png"))
    return by_cat


def write_pose_root(path, fixture):
    """The reference's predefined_poses files the loader reads ("upper", levels 0 and 2), from the arrays recorded in shapenet_ref.npz."""
    os.makedirs(path, exist_ok=True)
    for name in ("obj_poses_level0", "sphere_poses_level0", "obj_poses_level2", "sphere_poses_level2", "idx_upper_level0_in_level2"):
        np.save(os.path.join(path, name + ".npy"), np.asarray(fixture["grid/" + name]))
    return path


def relative(root, paths):
    return sorted(os.path.relpath(p, root) for p in paths)
