"""VSD evaluation (nope_amd/vsd.py, nope_op_render_depth / nope_op_vsd, PoseConditional.eval_vsd / load_mesh / test_step).

The VSD arithmetic is pinned to the reference's own vsd_obj (tests/golden/make_golden_vsd.py -> vsd_ref.npz); the rasteriser, which has
no runnable counterpart here (pyrender is not installed), to analytic depths and to a numpy restatement with the same sampling rule.

This file runs one shape family: k = 4 or 5 (vsd_kernel<5, 4>, 16-byte aligned images with H W % 4 == 0), images at most 96 rows high,
meshes whose listed triangles fit one trip of raster_big_kernel's loops.  tests/test_vsd_paths.py, which imports the helpers below,
reaches the rest on the interpreter and on the device: vsd_kernel<1, .>, <5, .> with the `j >= k` skip, <16, .>; vsd_kernel<., 1> for
H W % 4 != 0 and for a depth pointer at 4 mod 16; fewer pixels than one workgroup has threads; empty inputs, one K, B = 1;
raster_big_kernel's second trips of `yb += 16 * gridDim.y` (a box more than 128 rows high) and `e += gridDim.x` (more than 256 listed
triangles) and its list at the capacity P * max_faces; the kSmallArea boundary (64 / 65 pixels); `fl >= cnt` with cnt < max_faces over
several blockIdx.x; the pixel box clamped at each border alone, triangles outside, sub-pixel, degenerate and beyond zfar; the exact
skipped count; the launchers' argument checks and (interpreter only) their index and range guards; vsd_error at k = 1 and k = 7."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_vsd import CASES, DELTA, TAU, case_inputs, digest

REF_KEYS = {"top 1, vsd_median", "top 1, vsd_scores 0.3", "top 3, vsd_median", "top 3, vsd_scores 0.3", "top 5, vsd_median",
            "top 5, vsd_scores 0.3"}


# ---- numpy restatements -------------------------------------------------------------------------------------------------------------
def np_vsd(dtest, dgt, dest, Ks, delta=DELTA, tau=TAU, cost_type="step", visib_mode="bop19"):
    """vsd_utils.py + vsd.py:91-131 in numpy, batched: (B, k) f64."""
    B, k, H, W = dest.shape
    out = np.zeros((B, k))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

    def dist(d, K):
        px, py = (xs - K[0, 2]) / np.float64(K[0, 0]), (ys - K[1, 2]) / np.float64(K[1, 1])
        return np.sqrt(np.multiply(px, d) ** 2 + np.multiply(py, d) ** 2 + d.astype(np.float64) ** 2)

    def visib(d_test, d_model):
        d_diff = d_model.astype(np.float32) - d_test.astype(np.float32)
        if visib_mode == "bop18":
            return np.logical_and(d_diff <= delta, np.logical_and(d_test > 0, d_model > 0))
        return np.logical_and(np.logical_or(d_diff <= delta, d_test == 0), d_model > 0)

    for b in range(B):
        dt, dg = dist(dtest[b].astype(np.float64), Ks[b]), dist(dgt[b], Ks[b])
        vg = visib(dt, dg)
        for j in range(k):
            de = dist(dest[b, j], Ks[b])
            ve = np.logical_or(visib(dt, de), np.logical_and(vg, de > 0))
            inter, union = np.logical_and(vg, ve), np.logical_or(vg, ve)
            n_union = union.sum()
            d = np.abs(dg[inter] - de[inter])
            if n_union == 0:
                out[b, j] = 1.0
                continue
            costs = d >= tau if cost_type == "step" else np.minimum(d / tau, 1.0)
            out[b, j] = (np.sum(costs) + (n_union - inter.sum())) / float(n_union)
    return out


def np_render(verts, faces, pose, K, H, W):
    """The rasteriser's rule in numpy: sample (x + 0.5, y + 0.5), f64 set-up, inclusive edges, 1/Z interpolated, nearest wins.
    Returns (depth (H,W) f64, projected vertices (V,2))."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    cam = verts.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    u, v, Z = fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy, cam[:, 2]
    zb = np.full((H, W), np.inf)
    for a, b, c in faces:
        x, y, iz = u[[a, b, c]], v[[a, b, c]], 1.0 / Z[[a, b, c]]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        if area == 0:
            continue
        x0, x1 = max(int(np.ceil(x.min() - 0.5)), 0), min(int(np.floor(x.max() - 0.5)), W - 1)
        y0, y1 = max(int(np.ceil(y.min() - 0.5)), 0), min(int(np.floor(y.max() - 0.5)), H - 1)
        if x0 > x1 or y0 > y1:
            continue
        sy, sx = np.mgrid[y0:y1 + 1, x0:x1 + 1] + 0.5
        w0 = (x[2] - x[1]) * (sy - y[1]) - (y[2] - y[1]) * (sx - x[1])
        w1 = (x[0] - x[2]) * (sy - y[2]) - (y[0] - y[2]) * (sx - x[2])
        w2 = (x[1] - x[0]) * (sy - y[0]) - (y[1] - y[0]) * (sx - x[0])
        s = 1.0 if area > 0 else -1.0
        inside = (s * w0 >= 0) & (s * w1 >= 0) & (s * w2 >= 0)
        z = 1.0 / ((w0 * iz[0] + w1 * iz[1] + w2 * iz[2]) / area)
        blk = zb[y0:y1 + 1, x0:x1 + 1]
        blk[inside] = np.minimum(blk[inside], z[inside])
    zb[np.isinf(zb)] = 0.0
    return zb, np.stack([u, v], 1)


def edge_distance(px, py, uv, faces):
    """Distance of the point (px, py) to the nearest projected triangle edge."""
    best = np.inf
    for tri in faces:
        for i in range(3):
            a, b = uv[tri[i]], uv[tri[(i + 1) % 3]]
            ab = b - a
            t = np.clip(np.dot([px, py] - a, ab) / max(np.dot(ab, ab), 1e-300), 0, 1)
            best = min(best, float(np.linalg.norm([px, py] - (a + t * ab))))
    return best


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_of(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def plate(half, z=0.0):
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def concat(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


K0 = np.array([[500.0, 0, 64.3], [0, 505.0, 47.7], [0, 0, 1]])


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_fixture_inputs_are_the_recorded_ones(golden):
    g = golden("vsd_ref.npz")
    assert str(g["inputs_sha256"]) == digest(case_inputs())


def test_numpy_vsd_restatement_matches_reference_fixture(golden):
    """The numpy VSD used by the end-to-end test is the reference's arithmetic (vsd_ref.npz from vsd_obj)."""
    g = golden("vsd_ref.npz")
    ins = case_inputs()
    for cost, vis in CASES:
        want = g[f"{cost}_{vis}"].numpy()
        got = np_vsd(*ins, cost_type=cost, visib_mode=vis)
        if cost == "step":
            assert np.array_equal(got, want), (cost, vis)
        else:
            assert np.allclose(got, want, rtol=1e-12, atol=0), (cost, vis)
    assert np.all(g["step_bop19"].numpy()[3] == 1.0)      # empty ground truth, and an empty union


def test_load_ply_ascii_binary_quads(tmp_path):
    from nope_amd import vsd
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]], dtype=np.float32)
    polys = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]]
    want_f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])
    for binary in (False, True):
        p = str(tmp_path / f"m{int(binary)}.ply")
        vsd.save_ply(p, verts, polys, binary=binary)
        v, f = vsd.load_ply(p)
        assert v.dtype == np.float32 and f.dtype == np.int32
        assert np.array_equal(v, verts) and np.array_equal(f, want_f)
    # double coordinates, extra vertex properties, int face counts (BOP models carry normals / colours)
    p = str(tmp_path / "d.ply")
    head = ("ply\nformat binary_little_endian 1.0\ncomment x\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\n"
            "property float nx\nproperty uchar red\nelement face 1\nproperty list int int vertex_indices\nend_header\n")
    vt = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("red", "u1")])
    rows = np.array([(1.5, 2.0, -3.0, 0.1, 7), (4.0, 5.0, 6.0, 0.2, 8), (7.0, 8.25, 9.0, 0.3, 9)], dtype=vt)
    with open(p, "wb") as fh:
        fh.write(head.encode() + rows.tobytes() + np.array([3, 2, 1, 0], "<i4").tobytes())
    v, f = vsd.load_ply(p)
    assert np.array_equal(v, np.array([[1.5, 2, -3], [4, 5, 6], [7, 8.25, 9]], np.float32)) and np.array_equal(f, [[2, 1, 0]])
    p = str(tmp_path / "a.ply")
    with open(p, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty float s\n"
                 "element face 1\nproperty list uchar uint vertex_indices\nend_header\n0 0 0 9\n2 0 0 9\n2 2 0 9\n0 2 0 9\n4 0 1 2 3\n")
    v, f = vsd.load_ply(p)
    assert np.array_equal(f, [[0, 1, 2], [0, 2, 3]]) and v[2].tolist() == [2, 2, 0]


def test_load_depth_is_png_over_10(tmp_path):
    from PIL import Image
    from nope_amd import vsd
    raw = (np.arange(48, dtype=np.uint16).reshape(6, 8) * 1237 + 3).astype(np.uint16)
    p = str(tmp_path / "d.png")
    Image.fromarray(raw).save(p)
    d = vsd.load_depth(p)
    assert d.dtype == np.float64 and np.array_equal(d, raw / 10.0)


def test_vsd_scores_formula():
    from nope_amd import vsd
    rng = np.random.default_rng(5)
    err = rng.random((7, 5))
    err[2, :] = 0.3
    s = vsd.vsd_scores(err)
    assert set(s) == REF_KEYS
    for k in (1, 3, 5):     # model.py:530-537
        best = np.min(err[:, :k], 1)
        assert s[f"top {k}, vsd_median"] == np.median(best)
        assert s[f"top {k}, vsd_scores 0.3"] == np.mean((best <= 0.3) * 100.0)


def test_use_gt_translation_false_raises():
    from nope_amd import vsd
    with pytest.raises(NotImplementedError):
        vsd.vsd_error(np.zeros((1, 4, 4)), None, [1], np.eye(3)[None, None], np.eye(3)[None], np.zeros((1, 3, 1)), K0,
                      use_gt_translation=False)


def test_vsd_kernel_on_emu_matches_reference(emu, golden):
    """nope_op_vsd's source on the CPU interpreter build: the step cost equals the reference bit for bit."""
    from nope_amd import vsd
    g = golden("vsd_ref.npz")
    dtest, dgt, dest, Ks = case_inputs()
    for cost, vis in (("step", "bop19"), ("tlinear", "bop18")):
        err = vsd.vsd_from_depth(torch.from_numpy(dtest), torch.from_numpy(dgt), torch.from_numpy(dest), Ks, DELTA, TAU, cost, vis).numpy()
        want = g[f"{cost}_{vis}"].numpy()
        assert np.array_equal(err, want) if cost == "step" else np.allclose(err, want, rtol=1e-12, atol=0)


def test_rasteriser_on_emu_matches_numpy(emu):
    from nope_amd import vsd
    sph = vsd.icosphere(1, 30.0)
    bank = vsd.MeshBank({1: plate(25.0), 2: sph}, device="cpu")
    H, W = 24, 32
    K = np.array([[60.0, 0, 15.3], [0, 61.0, 11.6], [0, 0, 1]])
    poses = np.stack([pose_of(rot(0.2, -0.3, 0.1), [1, 2, 300]), pose_of(rot(0.5, 0.1, 0.0), [-3, 1, 250]), pose_of(np.eye(3), [0, 0, 20])])
    ids = [1, 2, 1]       # the last plate covers the image (the workgroup path)
    d = vsd.render_depth(bank, ids, poses, K, H, W).numpy()
    meshes = {1: plate(25.0), 2: sph}
    for p, o in enumerate(ids):
        want, _ = np_render(*meshes[o], poses[p], K, H, W)
        both = (want > 0) & (d[p] > 0)
        assert np.array_equal(want > 0, d[p] > 0), p
        assert np.abs(d[p][both] - want[both]).max() <= 1e-5 * want[both].max()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vsd_matches_reference_fixture(gpu, golden):
    from nope_amd import vsd
    g = golden("vsd_ref.npz")
    dtest, dgt, dest, Ks = (torch.from_numpy(a) for a in case_inputs())
    for cost, vis in CASES:
        err = vsd.vsd_from_depth(dtest.cuda(), dgt.cuda(), dest.cuda(), Ks, DELTA, TAU, cost, vis).cpu().numpy()
        want = g[f"{cost}_{vis}"].numpy()
        if cost == "step":
            assert np.array_equal(err, want), (vis, err, want)
        else:
            assert np.allclose(err, want, rtol=1e-12, atol=0), (vis, np.abs(err - want).max())
        again = vsd.vsd_from_depth(dtest.cuda(), dgt.cuda(), dest.cuda(), Ks, DELTA, TAU, cost, vis).cpu().numpy()
        assert np.array_equal(err, again)


@pytest.mark.gpu
def test_vsd_rejects_bad_arguments(gpu):
    from nope_amd import hip, vsd
    d = torch.zeros(2, 8, 8, device="cuda")
    with pytest.raises(hip.NopeError):
        vsd.vsd_from_depth(d, d, torch.zeros(2, 17, 8, 8, device="cuda"), K0)
    with pytest.raises(hip.NopeError):
        vsd.vsd_from_depth(d, d[:1], torch.zeros(2, 3, 8, 8, device="cuda"), K0)
    with pytest.raises(ValueError):
        vsd.vsd_from_depth(d, d, torch.zeros(2, 3, 8, 8, device="cuda"), K0, cost_type="linear")
    l = hip.lib()
    assert l.dll.nope_op_vsd(None, None, None, None, 1, 1, 8, 8, 15.0, 20.0, 0, 0, None, None, 0, None) == -1
    assert l.dll.nope_op_render_depth(None, 1, None, 1, None, None, 1, None, None, 1, 8, 8, None, None, None, 0, None) == -1


@pytest.mark.gpu
def test_render_fronto_parallel_plate(gpu):
    from nope_amd import vsd
    H, W, half = 96, 128, 40.0
    bank = vsd.MeshBank({1: plate(half)})
    d = vsd.render_depth(bank, [1], pose_of(np.eye(3), [0, 0, 500])[None], K0, H, W)[0].cpu().numpy()
    fx, fy, cx, cy = K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2]
    u0, u1 = fx * -half / 500 + cx, fx * half / 500 + cx
    v0, v1 = fy * -half / 500 + cy, fy * half / 500 + cy
    sy, sx = np.mgrid[0:H, 0:W] + 0.5
    inside = (sx > u0 + 1e-3) & (sx < u1 - 1e-3) & (sy > v0 + 1e-3) & (sy < v1 - 1e-3)
    outside = (sx < u0) | (sx > u1) | (sy < v0) | (sy > v1)
    assert inside.sum() > 5000
    ulp = np.spacing(np.float32(500))
    assert np.abs(d[inside] - 500).max() <= ulp
    assert np.all(d[outside] == 0)


@pytest.mark.gpu
def test_render_tilted_plane_and_plate_larger_than_image(gpu):
    from nope_amd import vsd
    H, W = 96, 128
    R, t = rot(0.35, -0.5, 0.2), np.array([5.0, -3.0, 600.0])
    bank = vsd.MeshBank({1: plate(60.0), 2: plate(2000.0)})
    poses = np.stack([pose_of(R, t), pose_of(np.eye(3), [0, 0, 100])])
    d = vsd.render_depth(bank, [1, 2], poses, K0, H, W).cpu().numpy()
    sy, sx = np.mgrid[0:H, 0:W] + 0.5
    dirs = np.stack([(sx - K0[0, 2]) / K0[0, 0], (sy - K0[1, 2]) / K0[1, 1], np.ones_like(sx)], -1)
    n = R[:, 2]
    zray = (n @ t) / (dirs @ n)
    cov = d[0] > 0
    assert cov.sum() > 1000
    assert np.abs(d[0][cov] - zray[cov]).max() <= 1e-5 * zray[cov].max()
    assert np.all(np.abs(d[1] - 100.0) <= np.spacing(np.float32(100)))


@pytest.mark.gpu
def test_render_occlusion_mixed_objects_and_numpy(gpu):
    """Two objects in one face range (either order): the nearer wins; a box and an icosphere in the same launch against np_render."""
    from nope_amd import vsd
    H, W = 72, 96
    K = np.array([[300.0, 0, 47.6], [0, 310.0, 35.2], [0, 0, 1]])
    far, near = plate(80.0), plate(20.0, z=-200.0)      # the near plate sits 200 mm in front of the far one
    bx, sph = vsd.box(60.0, 40.0, 50.0), vsd.icosphere(2, 35.0)
    meshes = {1: concat(far, near), 2: concat(near, far), 3: bx, 4: sph}
    bank = vsd.MeshBank(meshes)
    poses = np.stack([pose_of(np.eye(3), [0, 0, 500]), pose_of(np.eye(3), [0, 0, 500]), pose_of(rot(0.4, 0.7, 0.2), [4, -6, 400]),
                      pose_of(rot(-0.3, 0.2, 1.1), [-5, 3, 350])])
    ids = [1, 2, 3, 4]
    d = vsd.render_depth(bank, ids, poses, K, H, W).cpu().numpy()
    assert np.array_equal(d[0], d[1])
    assert np.isclose(d[0][int(K[1, 2]), int(K[0, 2])], 300.0) and np.isclose(d[0][2, 2], 500.0)
    for p in range(4):
        want, uv = np_render(*meshes[ids[p]], poses[p], K, H, W)
        both = (want > 0) & (d[p] > 0)
        assert both.sum() > 200
        assert np.abs(d[p][both] - want[both]).max() <= 1e-5 * want[both].max(), p
        for y, x in zip(*np.nonzero((want > 0) != (d[p] > 0))):
            assert edge_distance(x + 0.5, y + 0.5, uv, meshes[ids[p]][1]) <= 1e-3, (p, y, x)
    again = vsd.render_depth(bank, ids, poses, K, H, W).cpu().numpy()
    assert np.array_equal(d.view(np.uint32), again.view(np.uint32))


@pytest.mark.gpu
def test_render_reports_vertices_behind_znear(gpu):
    from nope_amd import hip, vsd
    bank = vsd.MeshBank({1: vsd.box(50.0, 50.0, 50.0)})
    poses = np.stack([pose_of(np.eye(3), [0, 0, 400]), pose_of(np.eye(3), [0, 0, 10])])
    with pytest.raises(hip.NopeError, match="pose 1"):
        vsd.render_depth(bank, [1, 1], poses, K0, 32, 32)
    d = vsd.render_depth(bank, [1], poses[:1], K0, 32, 32)
    assert float(d.max()) > 0


def _tless_batch(B, H, W, bank, seed=7):
    from nope_amd import vsd
    from nope_amd.harness import synthetic_batch
    b = synthetic_batch(B, 16, 128, seed=seed, device="cuda")
    K = torch.tensor([[250.0, 0, W / 2 - 0.3], [0, 252.0, H / 2 + 0.2], [0, 0, 1]], dtype=torch.float64)
    t = torch.tensor([[3.0], [-2.0], [450.0]], dtype=torch.float64)
    b["query_translation"] = t[None].expand(B, 3, 1).contiguous().cuda()
    b["intrinsic"] = K[None].expand(B, 3, 3).contiguous().cuda()
    b["obj_id"] = torch.tensor([1, 2, 1, 2][:B])
    gt = vsd.render_depth(bank, b["obj_id"], vsd.compose_poses(b["query_pose"], b["query_translation"]), b["intrinsic"], H, W)
    g = torch.Generator().manual_seed(seed)
    scene = gt.cpu() + torch.randn(gt.shape, generator=g) * 3
    scene[gt.cpu() == 0] = 700.0
    scene[:, :, W // 2: W // 2 + 6] = 380.0          # an occluder
    scene[:, H // 3, :] = 0.0                        # missing depth
    b["depth"] = scene.float()
    return b


@pytest.mark.gpu
def test_eval_vsd_end_to_end(gpu, tmp_path):
    from nope_amd import vsd
    from nope_amd.harness import build_model
    cad = tmp_path / "models"
    cad.mkdir()
    for oid in range(1, 31):
        v, f = vsd.icosphere(2, 40.0) if oid % 2 == 0 else vsd.box(70.0, 50.0, 40.0 + oid)
        vsd.save_ply(str(cad / f"obj_{oid:06d}.ply"), v, f, binary=oid % 2 == 0)
    m = build_model(device="cuda", save_dir=str(tmp_path / "run"))
    m.load_mesh(str(cad))
    B, H, W = 4, 60, 80
    batch = _tless_batch(B, H, W, m.tless_cad)
    out = m.eval_vsd(batch, "tless", save_path=str(tmp_path / "e.npy"))
    assert set(out) == REF_KEYS | {"loss/val_tless"}
    # host composition of the same retrieval, the device depth maps and the numpy VSD pinned to the reference above
    bank, _, _ = m.generate_templates(batch["reference"], batch["all_relativeR"])
    _, idx = m.retrieval(batch["query"], bank)
    idx = idx.cpu()
    tp = batch["template_poses"].cpu()
    predR = torch.stack([tp[b, idx[b]] for b in range(B)])
    t = batch["query_translation"].cpu()
    ids = batch["obj_id"].tolist()
    d_gt = vsd.render_depth(m.tless_cad, ids, vsd.compose_poses(batch["query_pose"].cpu(), t), batch["intrinsic"].cpu(), H, W).cpu().numpy()
    d_est = vsd.render_depth(m.tless_cad, [o for o in ids for _ in range(5)], vsd.compose_poses(predR, t[:, None].expand(B, 5, 3, 1)).reshape(-1, 4, 4),
                             batch["intrinsic"].cpu().repeat_interleave(5, 0), H, W).cpu().numpy().reshape(B, 5, H, W)
    err = np_vsd(batch["depth"].numpy(), d_gt, d_est, batch["intrinsic"].cpu().numpy())
    assert not np.all(err == 1.0)
    want = vsd.vsd_scores(err)
    for k in REF_KEYS:
        assert out[k] == want[k], (k, out[k], want[k])
    assert out["loss/val_tless"] == float(m.forward(batch["query"], batch["reference"], batch["gt_relativeR"]))
    assert np.array_equal(np.load(str(tmp_path / "e.npy")), err[:, 0])
    # test_step routes "tless_<category>" to eval_vsd and saves under predictions/ (model.py:550-557)
    res = m.test_step({"tless_primesense": batch}, 3)
    assert set(res["tless_primesense"]) == REF_KEYS | {"loss/val_primesense"}
    assert all(res["tless_primesense"][k] == out[k] for k in REF_KEYS)
    saved = os.path.join(str(tmp_path / "run"), "predictions", "vsd_primesense_batch3_rank_0.npy")
    assert np.array_equal(np.load(saved), err[:, 0])
    # depth_path instead of depth
    from PIL import Image
    paths = []
    for b in range(B):
        p = str(tmp_path / f"depth{b}.png")
        Image.fromarray(np.round(batch["depth"][b].numpy() * 10).astype(np.uint16)).save(p)
        paths.append(p)
    b2 = {k: v for k, v in batch.items() if k != "depth"}
    b2["depth_path"] = paths
    out2 = m.eval_vsd(b2, "tless")
    assert set(out2) == set(out)
