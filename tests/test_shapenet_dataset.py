"""nope_amd.dataset.ShapeNet against the reference's own `ShapeNet` (src/dataloader/shapeNet.py) run over the same synthetic root
(tests/shapenet_fixture.py; recorded by tests/golden/make_golden_shapenet.py into shapenet_ref.npz), and one pass of a loaded batch through
PoseConditional.test_step and the harness.

The reference shuffles with Python's global generator and in directory order, so ORDER parity is not defined: sets of paths are compared, and
tensors for the (query, reference) pairs the record names."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import shapenet_fixture as SF

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
MODES = [("full", False), ("fast", True)]


@pytest.fixture(scope="module")
def ref(golden):
    return golden("shapenet_ref.npz")


@pytest.fixture(scope="module")
def host_root(tmp_path_factory, ref):
    """The root the record was made from (no template frames: the host part opens none) and the reference's pose grids next to it."""
    root = str(tmp_path_factory.mktemp("shapenet_host"))
    by_cat = SF.build_root(os.path.join(root, "data"))
    assert np.array_equal(by_cat["bottle"], ref["objects/bottle"]) and np.array_equal(by_cat["mug"], ref["objects/mug"])
    return os.path.join(root, "data"), SF.write_pose_root(os.path.join(root, "predefined_poses"), ref)


def _dataset(host_root, split, fast, **kw):
    from nope_amd.dataset import ShapeNet
    data, pose_root = host_root
    return ShapeNet(data, split, "upper", "rotation6d", fast_evaluation=fast, img_size=kw.pop("img_size", 256), level=2, id2cat=SF.ID2CAT_PATH,
                    pose_root=pose_root, **kw)


@pytest.mark.parametrize("tag,fast", MODES)
def test_splits_indexes_and_symmetries(host_root, ref, tag, fast, caplog):
    data = host_root[0]
    ds = _dataset(host_root, "bottle", fast)
    # a category of at most 100 objects: the same objects, the same queries
    assert SF.relative(data, ds.query_paths) == list(ref[f"{tag}/bottle/queries"]) and len(ds) == 12
    assert sorted(ds.obj_ids) == list(ref["objects/bottle"].numpy()) and int(ref[f"{tag}/bottle/n_objects"]) == 6
    assert np.array_equal(ds.testing_indexes, ref[f"{tag}/testing_indexes"].numpy())
    assert len(ds.testing_templates_poses) == len(ds.testing_indexes) == (26 if fast else 341)
    assert [ds.obj_name2symmetry[f"obj_{i:06d}"] for i in range(len(ds.all_cad_names))] == list(ref["symmetry"].numpy())
    assert set(ref["symmetry"].numpy()) == {0, 2}
    # 104 objects: 100 are kept -- WHICH depends on the generator (the reference's is Python's global one), so only the cut and the rule are compared:
    # every query of the kept objects that have a folder, and a warning for the one that has none
    with caplog.at_level(logging.WARNING):
        mug = _dataset(host_root, "mug", fast, seed=7)
    all_mugs = list(ref["objects/mug"].numpy())
    missing = all_mugs[SF.MISSING_MUG]
    assert len(mug.obj_ids) == 100 and len(set(mug.obj_ids)) == 100 and set(mug.obj_ids) <= set(all_mugs)
    kept = [i for i in mug.obj_ids if i != missing]
    want = sorted(f"images/obj_{i:06d}/query_{k:06d}.png" for i in kept for k in range(SF.N_QUERY))
    assert SF.relative(data, mug.query_paths) == want
    assert (missing in mug.obj_ids) == any(f"obj_{missing:06d} does not exist" in r.getMessage() for r in caplog.records)
    # the reference on the same root: 100 kept too (99 folders when the missing one is among them), two queries each, all of them mugs
    n_ref = int(ref[f"{tag}/mug/n_objects"])
    assert n_ref in (99, 100) and len(ref[f"{tag}/mug/queries"]) == SF.N_QUERY * n_ref
    assert {int(p.split("/")[1][4:]) for p in ref[f"{tag}/mug/queries"]} <= set(all_mugs) - {missing}
    # another seed: another cut and another order, the same rule
    other = _dataset(host_root, "mug", fast, seed=8)
    assert set(other.obj_ids) != set(mug.obj_ids) and len(other.obj_ids) == 100
    assert _dataset(host_root, "mug", fast, seed=7).query_paths == mug.query_paths


def test_constructor_refusals(host_root):
    from nope_amd.dataset import ShapeNet
    data, pose_root = host_root
    for split in ("training", "unseen_training"):
        with pytest.raises(NotImplementedError):
            ShapeNet(data, split, id2cat=SF.ID2CAT_PATH)
    for rot in ("quaternion", "euler_angles"):
        with pytest.raises(NotImplementedError):
            ShapeNet(data, "bottle", rot_representation=rot, id2cat=SF.ID2CAT_PATH)
    ds = ShapeNet(data, "bottle", "upper", "rotation6d", id2cat=SF.id2cat(), fast_evaluation=True)        # a dict; the synthesised grids
    assert len(ds) == 12 and list(ds.testing_indexes) == list(range(26))
    bad = os.path.join(os.path.dirname(data), "corrupt.png")
    with open(bad, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\nnot a png")
    from nope_amd.dataset import decode_frame
    with pytest.raises(OSError, match="corrupt.png"):
        decode_frame(bad)


def test_decode_frame(tmp_path):
    """RGBA as stored (nothing composited on the host), RGB with alpha 255, a mask image as the alpha channel (first channel of a 3-channel mask)."""
    from PIL import Image
    from nope_amd.dataset import decode_frame
    rng = np.random.default_rng(1)
    rgba = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    Image.fromarray(rgba, "RGBA").save(tmp_path / "a.png")
    Image.fromarray(rgba[:, :, :3].copy(), "RGB").save(tmp_path / "b.png")
    mask3 = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    Image.fromarray(mask3, "RGB").save(tmp_path / "m3.png")
    Image.fromarray(mask3[:, :, 1].copy(), "L").save(tmp_path / "m1.png")
    a = decode_frame(str(tmp_path / "a.png"))
    assert a.dtype == np.uint8 and a.shape == (5, 7, 4) and np.array_equal(a, rgba)
    b = decode_frame(str(tmp_path / "b.png"))
    assert np.array_equal(b[:, :, :3], rgba[:, :, :3]) and bool((b[:, :, 3] == 255).all())
    assert np.array_equal(decode_frame(str(tmp_path / "b.png"), str(tmp_path / "m3.png"))[:, :, 3], mask3[:, :, 0])
    assert np.array_equal(decode_frame(str(tmp_path / "b.png"), str(tmp_path / "m1.png"))[:, :, 3], mask3[:, :, 1])


@pytest.mark.parametrize("tag,fast", MODES)
def test_crop_transform_maps_the_recorded_points(host_root, ref, tag, fast):
    """The four source points the reference's crop_frame hands to cv2 for the query and the reference frame of each recorded pair: the map of
    crop_transform for that frame's pose takes them onto the corners of the output."""
    from nope_amd.dataset import SHAPENET_INTRINSIC, crop_transform
    ds = _dataset(host_root, "bottle", fast)
    data = host_root[0]
    for p, (q_rel, r_rel) in enumerate(ref[f"{tag}/pairs"]):
        for j, rel_path in enumerate((q_rel, r_rel)):
            M = crop_transform(SHAPENET_INTRINSIC, ds.get_pose(os.path.join(data, rel_path)), 256, virtual_bbox_size=1)
            src, dst = ref[f"{tag}/crop_src"][p, j].numpy(), ref[f"{tag}/crop_dst"][p, j].numpy()
            assert np.array_equal(dst, np.array([[0, 0], [0, 1], [1, 0], [1, 1]]) * 256.0)
            h = M @ np.concatenate([src, np.ones((4, 1))], 1).T
            assert np.allclose((h[:2] / h[2]).T, dst, rtol=0, atol=1e-6), (p, j)


@pytest.mark.parametrize("tag,fast", MODES)
def test_template_frames_and_their_crop_poses(host_root, ref, tag, fast):
    """The reference opens templates_{testing_indexes[i]}.png and crops it with row i of the object's template poses (shapeNet.py:292-299 asks
    get_pose for templates_{i}.png): the source points it hands to cv2 for EVERY template of the recorded pairs are those of `template_frame_poses`,
    and -- the rows differing -- not those of row testing_indexes[i]."""
    from nope_amd.dataset import SHAPENET_INTRINSIC, crop_transform
    ds = _dataset(host_root, "bottle", fast)
    data = host_root[0]
    N = len(ds.testing_indexes)
    corners = np.concatenate([np.array([[0, 0], [0, 1], [1, 0], [1, 1]]) * 256.0, np.ones((4, 1))], 1)
    other_rows_differ = 0
    for p, (q_rel, _) in enumerate(ref[f"{tag}/pairs"]):
        q_path = os.path.join(data, q_rel)
        paths, poses = ds.template_paths(q_path), ds.template_frame_poses(q_path)
        assert [os.path.basename(x) for x in paths] == [f"templates_{int(i):06d}.png" for i in ref[f"{tag}/testing_indexes"]] and len(poses) == N
        all_rows = np.load(os.path.join(data, "object_template_poses", os.path.basename(os.path.dirname(q_path)) + ".npy"))
        src = ref[f"{tag}/template_crop_src"][p].numpy().astype(np.float64)
        assert src.shape == (N, 4, 2)
        for i in range(N):
            assert np.array_equal(poses[i], all_rows[i])
            h = np.linalg.inv(crop_transform(SHAPENET_INTRINSIC, poses[i], 256, virtual_bbox_size=1)) @ corners.T      # output corners -> source points
            assert np.allclose((h[:2] / h[2]).T, src[i], rtol=0, atol=1e-6), (p, i)
            h = np.linalg.inv(crop_transform(SHAPENET_INTRINSIC, all_rows[ds.testing_indexes[i]], 256, virtual_bbox_size=1)) @ corners.T
            other_rows_differ += not np.allclose((h[:2] / h[2]).T, src[i], rtol=0, atol=0.5)
    assert other_rows_differ > 5 * N          # (the record tells the two row choices apart)


@pytest.mark.parametrize("tag,fast", MODES)
def test_pose_tensors_of_the_recorded_pairs(emu, host_root, ref, tag, fast):
    """__getitem__ steered to the recorded reference frame: the reference's pose tensors (the images go through the interpreter build of the
    kernel at a small size and are not compared here)."""
    data = host_root[0]
    ds = _dataset(host_root, "bottle", fast, img_size=8, with_templates=False)
    for p, (q_rel, r_rel) in enumerate(ref[f"{tag}/pairs"]):
        s = ds.__getitem__(ds.query_paths.index(os.path.join(data, q_rel)), reference_path=os.path.join(data, r_rel))
        assert sorted(s) == ["all_relativeR", "gt_relativeR", "query", "query_pose", "reference", "symmetry", "template_poses"]
        want = {"gt_relativeR": ref[f"{tag}/gt_relativeR"][p], "all_relativeR": ref[f"{tag}/all_relativeR"][p], "query_pose": ref[f"{tag}/query_pose"][p],
                "template_poses": ref[f"{tag}/template_poses"], "symmetry": ref[f"{tag}/symmetry"][p]}
        for k, w in want.items():
            assert s[k].dtype == w.dtype and s[k].shape == w.shape, (k, s[k].dtype, s[k].shape)
            assert torch.allclose(s[k].cpu(), w, rtol=1e-6, atol=0), (p, k)
        assert s["query"].shape == s["reference"].shape == (3, 8, 8) and s["query"].dtype == torch.float32


@pytest.fixture(scope="module")
def lib_root(tmp_path_factory):
    """The same root with the 26 template frames of the fast grid (the synthesised one: templates 0..25), 64 x 64 frames and poses that put the
    objects' crop boxes over those frames (the loader's intrinsics are those of a 512-pixel render)."""
    root = str(tmp_path_factory.mktemp("shapenet_lib"))
    SF.build_root(root, range(26), image_hw=(64, 64), translation=SF.OVER_64_FRAME)
    return root


def _paste(rgba):
    from PIL import Image
    img = Image.fromarray(rgba, "RGBA")
    black = Image.new("RGB", img.size, (0, 0, 0))
    black.paste(img, mask=img.getchannel("A"))
    return np.asarray(black).copy()


@pytest.mark.parametrize("backend", BACKENDS)
def test_load_batch_pixels_and_aggregation(request, backend, lib_root):
    """load_batch against the per-frame path of the parent (PIL paste, crop_frame) on the files and pose rows it has to pair -- the frames carry
    pixels here, so a swapped frame or pose shows -- and run_split's pooling over batches of 2 + 2 + 1 samples against a direct computation."""
    hip = request.getfixturevalue(backend)
    dev = "cuda" if backend == "gpu" else "cpu"
    from nope_amd import harness
    from nope_amd.dataset import SHAPENET_INTRINSIC, ShapeNet, crop_frame, decode_frame
    S, N = 16, 26
    ds = ShapeNet(lib_root, "bottle", "upper", "rotation6d", fast_evaluation=True, img_size=S, level=2, id2cat=SF.ID2CAT_PATH, seed=3)
    refs = [sorted(p for p in os.listdir(os.path.dirname(q)) if p.startswith("reference"))[k] for k, q in zip((1, 0), ds.query_paths[:2])]
    refs = [os.path.join(os.path.dirname(q), r) for q, r in zip(ds.query_paths[:2], refs)]
    batch = ds.load_batch([0, 1], reference_paths=refs)
    crop = lambda path, pose: crop_frame(torch.from_numpy(_paste(decode_frame(path))).to(dev), None, SHAPENET_INTRINSIC, pose, S, virtual_bbox_size=1,
                                         normalize=True, round_u8=True)
    for b in range(2):
        q = ds.query_paths[b]
        obj = os.path.basename(os.path.dirname(q))
        rows = {k: np.load(os.path.join(lib_root, f"object_{k}_poses", obj + ".npy")) for k in ("query", "reference", "template")}
        qi, ri = int(os.path.basename(q)[6:12]), int(os.path.basename(refs[b])[10:16])
        assert torch.equal(batch["query"][b], crop(q, rows["query"][qi])), b
        assert torch.equal(batch["reference"][b], crop(refs[b], rows["reference"][ri])), b
        for i in (0, 7, N - 1):
            want = crop(os.path.join(os.path.dirname(q), f"templates_{int(ds.testing_indexes[i]):06d}.png"), rows["template"][i])
            assert torch.equal(batch["gt_templates"][b, i], want), (b, i)
        assert torch.equal(batch["query_pose"][b].cpu(), torch.from_numpy(rows["query"][qi][:3, :3]))
    for k in ("query", "reference", "gt_templates"):         # mostly object, not border; all different pictures
        assert float((batch[k] != -1.0).float().mean()) > 0.5, k
    assert not torch.equal(batch["query"][0], batch["query"][1]) and not torch.equal(batch["query"], batch["reference"])
    assert not torch.equal(batch["gt_templates"][0, 0], batch["gt_templates"][0, 1])
    # ---- run_split: a model whose retrieval is a fixed function of the batch, so that the pooled figures can be computed directly
    mugs = ShapeNet(lib_root, "mug", "upper", "rotation6d", fast_evaluation=True, img_size=S, level=2, id2cat=SF.ID2CAT_PATH, seed=5)

    class FixedRetrieval:
        save_dir, global_rank, global_step = None, 0, 0

        def _decoder(self):
            return None

        def forward(self, query, reference, gt):
            return torch.zeros(())

        def generate_and_retrieve(self, query, reference, all_rel):
            first = (query.flatten(1).abs().sum(1) * 1000).long() % N                # (a function of the sample alone, not of its batch)
            idx = (first[:, None] + torch.arange(5, device=query.device)[None]) % N
            return torch.zeros(query.shape[0], N, device=query.device), idx, None

    model = FixedRetrieval()
    n = 5
    res = harness.run_split(model, mugs, batch_size=2, limit=n)
    errs = []
    for i in range(n):
        b = mugs.load_batch([i], with_templates=False)
        idx = model.generate_and_retrieve(b["query"], None, None)[1]
        errs.append(float(harness.geodesic_deg(b["template_poses"][0, idx[0, 0]], b["query_pose"][0])))
    errs = torch.tensor(errs, dtype=torch.float64)
    assert res["samples"] == n
    assert res["median"] == pytest.approx(float(errs.median()), rel=1e-5)
    for t in (15, 30):
        assert res[f"accuracy_{t}"] == pytest.approx(float((errs <= t).double().mean() * 100), abs=1e-9)
    per_batch = [errs[0:2].median(), errs[2:4].median(), errs[4:5].median()]
    assert abs(float(torch.stack(per_batch).mean()) - float(errs.median())) > 1e-3        # (a mean of per-batch medians would be another number)
    assert harness.run_split(model, mugs, batch_size=1, limit=n) == res


@pytest.mark.parametrize("backend", BACKENDS)
def test_batch_through_test_step_and_harness(request, backend, lib_root, tmp_path, capsys):
    hip = request.getfixturevalue(backend)
    dev = "cuda" if backend == "gpu" else "cpu"
    from nope_amd import harness
    from nope_amd.dataset import ShapeNet
    from nope_amd.model import PoseConditional
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    S, N = 8, 26
    ds = ShapeNet(lib_root, "bottle", "upper", "rotation6d", fast_evaluation=True, img_size=S, level=2, id2cat=SF.ID2CAT_PATH, seed=3)
    batch = ds.load_batch([0, 1])
    shapes = {"query": (2, 3, S, S), "reference": (2, 3, S, S), "gt_relativeR": (2, 6), "all_relativeR": (2, N, 6), "gt_templates": (2, N, 3, S, S),
              "symmetry": (2, 1), "query_pose": (2, 3, 3), "template_poses": (2, N, 3, 3)}
    assert sorted(batch) == sorted(shapes)
    for k, shp in shapes.items():
        assert tuple(batch[k].shape) == shp and batch[k].device.type == dev, k
        assert batch[k].dtype == (torch.float64 if k in ("query_pose", "template_poses") else torch.float32), k
    assert bool((batch["symmetry"] == 2).all())
    one = ds.__getitem__(0)
    assert {k: tuple(v.shape) for k, v in one.items()} == {k: s[1:] for k, s in shapes.items()}
    assert torch.equal(one["query"], batch["query"][0]) and torch.equal(one["query_pose"], batch["query_pose"][0])
    assert float((batch["query"] != -1.0).float().mean()) > 0.5
    assert "gt_templates" not in ds.load_batch([0, 1], with_templates=False)
    u = UNet(u_net_dim=8, rot_representation_dim=6, encoder=harness.StubEncoder(3), pose_mlp_name="single_layer", dim_mults=(1, 2), compute_dtype="f32")
    synth_init_(u, 2022)
    pc = PoseConditional(u, None, {"similarity_metric": "l2"}, None).to(dev).eval()
    res = pc.test_step({"shapeNet_bottle": batch}, 0)
    assert list(res) == ["shapeNet_bottle"]
    scores = res["shapeNet_bottle"]
    assert {"loss", "top1, accuracy_15", "top1, accuracy_30", "top1, median"} <= set(scores) and all(np.isfinite(v) for v in scores.values())
    capsys.readouterr()
    out = harness.main(["--data-root", lib_root, "--split", "bottle", "--id2cat", SF.ID2CAT_PATH, "--fast", "--limit", "2", "--batch", "2", "--size", "8",
                        "--u-net-dim", "8", "--encoder", "stub"])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert {"accuracy_15", "accuracy_30", "median"} <= set(rec) and rec["samples"] == 2 and rec["dataloader"] == "shapeNet_bottle" and rec["templates"] == N
    assert 0.0 <= rec["accuracy_15"] <= rec["accuracy_30"] <= 100.0 and 0.0 <= rec["median"] <= 180.0
    assert out["median"] == rec["median"]
