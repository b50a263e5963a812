"""The paths of nope_op_vsd and nope_op_render_depth (csrc/kernels_vsd.hip) that tests/test_vsd.py's one shape family does not reach,
each on the interpreter (tests/hipemu) and on the device.

  vsd_kernel          KC = 1 (k = 1), KC = 5 with the `j >= k` skip (k = 2) and full (k = 5), KC = 16 (k = 6, 7, 16); VW = 1 because
                      H W % 4 != 0 (95x127 over several blocks, 7x9 with fewer pixels than one workgroup has threads) and because a
                      depth pointer is not 16-byte aligned (the grid sized for 4-pixel groups walks four times as many); empty
                      estimates / ground truth / test depth; one K for all queries; B = 1
  raster_big_kernel   a second trip of `yb += 16 * gridDim.y` (a box more than 128 rows high), a second trip of `e += gridDim.x` (more
                      than 256 listed triangles), the list filled to P * max_faces
  raster_tri_kernel   a 64-pixel box (drawn by one lane) next to a 65-pixel one (listed); `fl >= cnt` with cnt < max_faces over several
                      blockIdx.x; the box clamped at each image border alone; triangles outside the image, smaller than a pixel,
                      degenerate, farther than zfar; the exact skipped count; on the interpreter alone the vertex-index and face-range
                      guards that MeshBank makes unreachable
  vsd.vsd_error       the (B, 1 + k) launch and its slicing at k = 1 and k = 7

References: np_vsd (pinned to the reference's vsd_obj by test_vsd.py) and np_render / the analytic planes.  Depth bound: both sides
evaluate Z in f64 and the kernel rounds once to f32, so |d - want| <= one f32 ulp of want.  Coverage may differ from np_render only where
the sample point lies within 1e-3 px of a projected edge, at no more than 0.1 % of the covered pixels."""
import functools
import re

import numpy as np
import pytest
import torch

from tests.golden.make_golden_vsd import CASES, DELTA, TAU, case_inputs
from tests.test_vsd import concat, edge_distance, np_render, np_vsd, plate, pose_of, rot

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
ERR_ARG, ERR_WORKSPACE = -1, -3


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def _np(t):
    return t.cpu().numpy()


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ---- A. nope_op_vsd -----------------------------------------------------------------------------------------------------------------
SIZES = {"96x128": (96, 128), "95x127": (95, 127), "7x9": (7, 9)}


@functools.lru_cache(maxsize=None)
def vsd_inputs(size):
    """case_inputs() with sixteen estimates per query, cropped to `size` (K unchanged)."""
    dtest, dgt, dest, Ks = case_inputs()
    dest = np.concatenate([dest, np.roll(dest, 3, axis=3), np.roll(dest, -5, axis=2), np.roll(dest, 7, axis=3)], 1)
    H, W = SIZES[size]
    return tuple(np.ascontiguousarray(a) for a in (dtest[:, :H, :W], dgt[:, :H, :W], dest[:, :, :H, :W])) + (Ks,)


@functools.lru_cache(maxsize=None)
def vsd_want(size, cost, vis):
    """np_vsd of all sixteen estimates: an estimate's error does not depend on the others, so [:, :k] is the reference for k."""
    return np_vsd(*vsd_inputs(size), cost_type=cost, visib_mode=vis)


def assert_vsd(got, want, cost, what):
    if cost == "step":
        assert np.array_equal(got, want), (what, got, want)
    else:
        assert np.allclose(got, want, rtol=1e-12, atol=0), (what, np.abs(got - want).max())


@pytest.mark.parametrize("k", [1, 2, 5, 6, 7, 16])
@pytest.mark.parametrize("size", list(SIZES))
def test_vsd_every_instantiation(be, size, k):
    """KC in {1, 5, 16} x VW in {4, 1}, several blocks per image and fewer pixels than one workgroup's threads."""
    from nope_amd import vsd
    _, dev, name = be
    dtest, dgt, dest, Ks = vsd_inputs(size)
    t, g, e = (torch.from_numpy(a).to(dev) for a in (dtest, dgt, np.ascontiguousarray(dest[:, :k])))
    for cost, vis in CASES:
        err = _np(vsd.vsd_from_depth(t, g, e, Ks, DELTA, TAU, cost, vis))
        assert err.shape == (4, k)
        assert_vsd(err, vsd_want(size, cost, vis)[:, :k], cost, (size, k, cost, vis))
        if name == "gpu":
            again = _np(vsd.vsd_from_depth(t, g, e, Ks, DELTA, TAU, cost, vis))
            assert np.array_equal(err.view(np.uint64), again.view(np.uint64)), (size, k, cost, vis)


def _offset_by_4_bytes(a, dev):
    buf = torch.empty(1 + a.size, dtype=torch.float32, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


@pytest.mark.parametrize("which", ["test", "gt", "est", "all"])
def test_vsd_misaligned_buffers(be, which):
    """H W % 4 == 0 but a depth pointer at 4 mod 16: the scalar form on the grid sized for 4-pixel groups."""
    from nope_amd import vsd
    _, dev, _ = be
    k = 5
    dtest, dgt, dest, Ks = vsd_inputs("96x128")
    dest = np.ascontiguousarray(dest[:, :k])
    aligned = [torch.from_numpy(a).to(dev) for a in (dtest, dgt, dest)]
    args = list(aligned)
    for i, n in enumerate(("test", "gt", "est")):
        assert aligned[i].data_ptr() % 16 == 0
        if which in (n, "all"):
            args[i] = _offset_by_4_bytes((dtest, dgt, dest)[i], dev)
            assert args[i].is_contiguous() and args[i].data_ptr() % 16 == 4
    for cost, vis in CASES:
        err = _np(vsd.vsd_from_depth(*args, Ks, DELTA, TAU, cost, vis))
        assert_vsd(err, vsd_want("96x128", cost, vis)[:, :k], cost, (which, cost, vis))
        if cost == "step":
            assert np.array_equal(err, _np(vsd.vsd_from_depth(*aligned, Ks, DELTA, TAU, cost, vis))), (which, vis)


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("hw", [(8, 12), (7, 9)])
def test_vsd_degenerate_contents(be, hw, k):
    from nope_amd import vsd
    _, dev, _ = be
    B, (H, W) = 2, hw
    rng = np.random.default_rng(100 * H + k)
    Ks = np.array([[[40.0, 0, 4.0], [0, 41.0, 3.0], [0, 0, 1]], [[38.0, 0, 5.5], [0, 36.0, 2.5], [0, 0, 1]]])
    gt = (500.0 + rng.normal(0, 30.0, (B, H, W))).astype(np.float32)
    gt[:, :2, :] = 0.0                                              # the object does not fill the image
    test = (gt + rng.normal(0, 8.0, gt.shape)).astype(np.float32)
    test[gt == 0] = 800.0
    est = (gt[:, None] + rng.normal(0, 12.0, (B, k, H, W))).astype(np.float32)
    est[:, :, :, :3] = 0.0
    zero3, zero4 = np.zeros_like(gt), np.zeros_like(est)
    same = np.repeat(gt[:, None], k, 1)
    #        test   gt     est    closed form per (cost, vis), None: np_vsd alone
    plain = np_vsd(test, gt, est, Ks)
    assert np.all((plain > 0) & (plain < 1))           # the shapes carry a real answer before anything is emptied
    cases = {"nothing empty": (test, gt, est, lambda cost, vis: None),
             "estimates all zero": (test, gt, zero4, lambda cost, vis: 1.0),
             "ground truth all zero": (test, zero3, est, lambda cost, vis: None),
             "test depth all zero": (zero3, gt, est, lambda cost, vis: 1.0 if vis == "bop18" else None),      # bop18: nothing visible
             "estimate == ground truth == test": (gt, gt, same, lambda cost, vis: 0.0)}
    for what, (t, g, e, closed) in cases.items():
        for cost, vis in CASES:
            err = _np(vsd.vsd_from_depth(*(torch.from_numpy(a).to(dev) for a in (t, g, e)), Ks, DELTA, TAU, cost, vis))
            assert_vsd(err, np_vsd(t, g, e, Ks, cost_type=cost, visib_mode=vis), cost, (what, hw, k, cost, vis))
            if closed(cost, vis) is not None:
                assert np.all(err == closed(cost, vis)), (what, hw, k, cost, vis, err)


def test_vsd_one_K_for_all_queries_and_one_query(be):
    from nope_amd import vsd
    _, dev, _ = be
    k = 5
    dtest, dgt, dest, Ks = vsd_inputs("96x128")
    t, g, e = (torch.from_numpy(a).to(dev) for a in (dtest, dgt, np.ascontiguousarray(dest[:, :k])))
    K1 = Ks[1]
    for cost, vis in CASES:
        one = _np(vsd.vsd_from_depth(t, g, e, K1, DELTA, TAU, cost, vis))
        rep = _np(vsd.vsd_from_depth(t, g, e, np.repeat(K1[None], 4, 0), DELTA, TAU, cost, vis))
        assert np.array_equal(one, rep), (cost, vis)
        assert_vsd(one, np_vsd(dtest, dgt, dest[:, :k], np.repeat(K1[None], 4, 0), cost_type=cost, visib_mode=vis), cost, (cost, vis))
        b1 = _np(vsd.vsd_from_depth(t[2:3], g[2:3], e[2:3], Ks[2], DELTA, TAU, cost, vis))
        assert b1.shape == (1, k)
        assert np.array_equal(b1, _np(vsd.vsd_from_depth(t[2:3], g[2:3], e[2:3], Ks[2:3], DELTA, TAU, cost, vis))), (cost, vis)
        assert_vsd(b1, vsd_want("96x128", cost, vis)[2:3, :k], cost, ("B = 1", cost, vis))


# ---- B. nope_op_render_depth --------------------------------------------------------------------------------------------------------
def np_boxes(verts, faces, pose, K, H, W):
    """Pixels in each face's clamped box, as raster_tri_kernel counts them (0: no box): <= 64 is drawn by one lane, more is listed."""
    cam = verts.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    u, v = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
    out = []
    for tri in faces:
        x, y = u[tri], v[tri]
        x0, x1 = max(int(np.ceil(x.min() - 0.5)), 0), min(int(np.floor(x.max() - 0.5)), W - 1)
        y0, y1 = max(int(np.ceil(y.min() - 0.5)), 0), min(int(np.floor(y.max() - 0.5)), H - 1)
        out.append((x1 - x0 + 1, y1 - y0 + 1) if x0 <= x1 and y0 <= y1 else (0, 0))
    return np.array(out)


def assert_depth(d, want, uv=None, faces=None, what=None):
    """One f32 ulp on the pixels both cover; coverage by the edge rule (a use of that allowance is printed)."""
    got_m, want_m = d > 0, want > 0
    both = got_m & want_m
    assert both.any() or not want_m.any(), what
    over = np.abs(d[both].astype(np.float64) - want[both]) - np.spacing(want[both].astype(np.float32))
    assert np.all(over <= 0), (what, "depth off by more than one f32 ulp at", int((over > 0).sum()), "pixels, largest excess", over.max())
    ys, xs = np.nonzero(got_m != want_m)
    if uv is None:
        assert len(ys) == 0, (what, list(zip(ys, xs))[:8])
        return
    assert len(ys) <= 1e-3 * want_m.sum(), (what, len(ys), int(want_m.sum()))
    for y, x in zip(ys, xs):
        assert edge_distance(x + 0.5, y + 0.5, uv, faces) <= 1e-3, (what, y, x)
    if len(ys):
        print(f"{what}: {len(ys)} of {int(want_m.sum())} covered pixels differ in coverage, all within 1e-3 px of an edge")


def test_render_triangle_more_than_128_rows_high(be):
    """raster_big_kernel's second trip over the row bands: 8 bands of 16 rows per trip."""
    from nope_amd import vsd
    _, dev, _ = be
    H, W = 160, 40
    K = np.array([[60.0, 0, 19.3], [0, 61.0, 80.6], [0, 0, 1]])
    pose = pose_of(np.eye(3), [0, 0, 100])
    assert np.all(np_boxes(*plate(2000.0), pose, K, H, W) == (W, H))
    d = _np(vsd.render_depth(vsd.MeshBank({1: plate(2000.0)}, device=dev), [1], pose[None], K, H, W))[0]
    assert np.all(d > 0) and np.all(np.abs(d - 100.0) <= np.spacing(np.float32(100)))
    # tilted: the ray-plane depth, and np_render
    H, W = 176, 48
    K = np.array([[60.0, 0, 23.3], [0, 75.0, 88.6], [0, 0, 1]])
    R, t = rot(0.35, -0.5, 0.2), np.array([5.0, -3.0, 600.0])
    mesh, pose = plate(600.0), pose_of(R, t)
    assert np_boxes(*mesh, pose, K, H, W)[:, 1].min() > 128
    d = _np(vsd.render_depth(vsd.MeshBank({1: mesh}, device=dev), [1], pose[None], K, H, W))[0]
    sy, sx = np.mgrid[0:H, 0:W] + 0.5
    dirs = np.stack([(sx - K[0, 2]) / K[0, 0], (sy - K[1, 2]) / K[1, 1], np.ones_like(sx)], -1)
    n = R[:, 2]
    zray = (n @ t) / (dirs @ n)
    cov = d > 0
    assert np.ptp(np.nonzero(cov.any(1))[0]) >= 128
    assert np.all(np.abs(d[cov] - zray[cov]) <= np.spacing(zray[cov].astype(np.float32)))
    want, uv = np_render(*mesh, pose, K, H, W)
    assert_depth(d, want, uv, mesh[1], "tilted plate")


def grid_mesh():
    """15 x 15 vertices over [-140, 140]^2 mm, z = 5 sin(x / 40) + 3 cos(y / 30), two triangles per cell: 392 faces."""
    c = np.linspace(-140.0, 140.0, 15)
    y, x = np.meshgrid(c, c, indexing="ij")
    verts = np.stack([x, y, 5 * np.sin(x / 40) + 3 * np.cos(y / 30)], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(14):
        for j in range(14):
            a = 15 * i + j
            faces += [(a, a + 1, a + 16), (a, a + 16, a + 15)]
    return verts, np.array(faces, dtype=np.int32)


GRID_K = np.array([[300.0, 0, 70.4], [0, 305.0, 90.7], [0, 0, 1]])
GRID_HW = (176, 150)
GRID_POSES = np.stack([pose_of(rot(0.3, -0.2, 0.4), [10, -5, 400]), pose_of(rot(-0.3, 0.25, 1.0), [-8, 6, 380]), pose_of(np.eye(3), [0, 0, 420])])
# the same rotations with the whole mesh inside a 240 x 240 image: every face of every pose is listed
INSIDE_K = np.array([[300.0, 0, 120.4], [0, 305.0, 119.7], [0, 0, 1]])
INSIDE_HW = (240, 240)
INSIDE_POSES = np.stack([pose_of(P[:3, :3], [0, 0, 550]) for P in GRID_POSES])


@functools.lru_cache(maxsize=None)
def grid_want(p, inside=False):
    return np_render(*grid_mesh(), *((INSIDE_POSES[p], INSIDE_K) + INSIDE_HW if inside else (GRID_POSES[p], GRID_K) + GRID_HW))


def listed(mesh, pose, K, H, W):
    return int((np.prod(np_boxes(*mesh, pose, K, H, W), 1) > 64).sum())


def test_render_more_than_256_listed_triangles(be):
    """392 triangles of 15 x 15 px cells, part of the mesh outside the image: 263 are listed, so some of raster_big_kernel's 256
    blockIdx.x take a second one."""
    from nope_amd import vsd
    _, dev, _ = be
    mesh = grid_mesh()
    H, W = GRID_HW
    assert len(mesh[1]) == 392 and listed(mesh, GRID_POSES[0], GRID_K, H, W) == 263
    d = _np(vsd.render_depth(vsd.MeshBank({1: mesh}, device=dev), [1], GRID_POSES[:1], GRID_K, H, W))[0]
    want, uv = grid_want(0)
    assert (want[:, 0] > 0).any() and (want[0, :] > 0).any() and not (want > 0).all()       # the mesh leaves the image on two sides
    assert_depth(d, want, uv, mesh[1], "grid mesh")


def _raw_render(hip, dev, verts, V, faces, F, off, cnt, max_faces, poses, Ks, H, W):
    """nope_op_render_depth through ctypes, its workspace inside a larger buffer of 0xAB: (code, depth, skipped, the bytes around it)."""
    dll = hip.lib().dll
    P = len(off)
    tv = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).to(dev)
    to, tc = (torch.tensor(a, dtype=torch.int32).to(dev) for a in (off, cnt))
    tp = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).to(dev)
    tk = torch.from_numpy(np.broadcast_to(np.asarray(Ks, dtype=np.float64), (P, 3, 3)).copy()).to(dev)
    depth = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    skipped = torch.full((P,), -1, dtype=torch.int32, device=dev)
    need = int(dll.nope_op_render_depth_workspace_bytes(P, max_faces))
    buf = torch.full((256 + need + 256 + 4096,), 0xAB, dtype=torch.uint8, device=dev)
    a = 256 + -buf.data_ptr() % 256
    code = dll.nope_op_render_depth(tv.data_ptr(), V, tf.data_ptr(), F, to.data_ptr(), tc.data_ptr(), max_faces, tp.data_ptr(), tk.data_ptr(), P,
                                    H, W, depth.data_ptr(), skipped.data_ptr(), buf.data_ptr() + a, need, hip._stream(depth))
    _sync(dev)
    return code, _np(depth), _np(skipped), (buf[:a], buf[a + need:])


def test_render_list_filled_to_its_capacity(be):
    """Three poses of the grid mesh in one launch through ctypes, the workspace inside a larger buffer: as above (769 of the 1176 entries:
    faces outside the image are not listed), then with the whole mesh inside the image, all 3 x 392 = P * max_faces listed -- the whole
    workspace and not a byte more."""
    hip, dev, _ = be
    mesh = verts, faces = grid_mesh()
    for inside, (poses, K, (H, W)) in enumerate(((GRID_POSES, GRID_K, GRID_HW), (INSIDE_POSES, INSIDE_K, INSIDE_HW))):
        assert sum(listed(mesh, poses[p], K, H, W) for p in range(3)) == (3 * 392 if inside else 769)
        code, d, skipped, (before, after) = _raw_render(hip, dev, verts, len(verts), faces, 392, [0, 0, 0], [392, 392, 392], 392, poses, K, H, W)
        assert code == 0 and np.all(skipped == 0)
        assert bool((before == 0xAB).all()) and bool((after == 0xAB).all()), "write outside the workspace"
        for p in range(3):
            want, uv = grid_want(p, bool(inside))
            assert_depth(d[p], want, uv, faces, ("grid mesh, inside" if inside else "grid mesh", "pose", p))


# fronto-parallel at Z = 100 with fx = fy = 100 and cx = cy = 0.5: the projected vertex is (x mm + 0.5, y mm + 0.5), so pixel (px, py)
# samples the mesh point (px, py) mm and a triangle's pixel box is [ceil(min), floor(max)] of its mm coordinates
UNIT_K = np.array([[100.0, 0, 0.5], [0, 100.0, 0.5], [0, 0, 1]])
UNIT_POSE = pose_of(np.eye(3), [0, 0, 100])


def tri(*pts):
    return np.array([[x, y, 0.0] for x, y in pts], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def _render_unit(vsd, dev, mesh, H, W):
    return _np(vsd.render_depth(vsd.MeshBank({1: mesh}, device=dev), [1], UNIT_POSE[None], UNIT_K, H, W))[0]


def test_render_64_and_65_pixel_boxes(be):
    """The kSmallArea boundary.  Right triangles, no lattice point on any edge:
      (1.75, 1.75) (9.5, 1.75) (1.75, 9.5)      pixel box x 2..9, y 2..9: 8 x 8 = 64, drawn by one lane (hypotenuse x + y = 11.25)
      (10.75, 1.75) (23.5, 1.75) (10.75, 6.5)   pixel box x 11..23, y 2..6: 13 x 5 = 65, listed (hypotenuse 76 x + 204 y = 2143, odd)
      (1.75, 10.75) (10.5, 10.75) (1.75, 17.5)  pixel box x 2..10, y 11..17: 9 x 7 = 63, one lane, its last row holds pixel (2, 17)
                                                (hypotenuse 108 x + 140 y = 2639, odd)"""
    from nope_amd import vsd
    _, dev, _ = be
    H = W = 24
    small, big = tri((1.75, 1.75), (9.5, 1.75), (1.75, 9.5)), tri((10.75, 1.75), (23.5, 1.75), (10.75, 6.5))
    less = tri((1.75, 10.75), (10.5, 10.75), (1.75, 17.5))
    assert [np_boxes(*m, UNIT_POSE, UNIT_K, H, W).tolist() for m in (small, big, less)] == [[[8, 8]], [[13, 5]], [[9, 7]]]
    ys, xs = np.mgrid[0:H, 0:W]
    in_small = (xs >= 2) & (ys >= 2) & (xs + ys <= 11)
    in_big = (xs >= 11) & (ys >= 2) & (76 * xs + 204 * ys < 2143)
    in_less = (xs >= 2) & (ys >= 11) & (108 * xs + 140 * ys < 2639)
    assert in_small.sum() == 36 and in_small[9, 2] and in_small[2, 9] and in_big[2, 22] and in_big[6, 11] and in_big.sum() > 30
    assert in_less[17, 2] and in_less[11, 10] and in_less[17].sum() == 1
    for what, mesh, mask in (("64", small, in_small), ("65", big, in_big), ("63", less, in_less),
                             ("all", concat(small, big, less), in_small | in_big | in_less)):
        d = _render_unit(vsd, dev, mesh, H, W)
        want, _ = np_render(*mesh, UNIT_POSE, UNIT_K, H, W)
        assert np.array_equal(want > 0, mask), what
        assert_depth(d, want, what=what)
        assert np.all(np.abs(d[mask] - 100.0) <= np.spacing(np.float32(100))), what


def test_render_each_border_alone_and_nothing_to_draw(be):
    """The pixel box clamped at one border at a time (the outside vertex 1e6 px away), triangles wholly outside, and sub-pixel ones."""
    from nope_amd import vsd
    _, dev, _ = be
    H, W = 40, 56
    far = 1.0e6
    crossing = {"left": tri((-far, 20.25), (30.25, 10.25), (30.25, 30.75)), "right": tri((far, 20.25), (25.75, 10.25), (25.75, 30.75)),
                "top": tri((28.25, -far), (18.25, 25.5), (38.75, 25.5)), "bottom": tri((28.25, far), (18.25, 14.5), (38.75, 14.5))}
    for what, mesh in crossing.items():
        want, uv = np_render(*mesh, UNIT_POSE, UNIT_K, H, W)
        cov = want > 0
        edge = {"left": cov[:, 0], "right": cov[:, -1], "top": cov[0], "bottom": cov[-1]}
        assert all(edge[s].any() == (s == what) for s in edge), what          # crosses this border and no other
        d = _render_unit(vsd, dev, mesh, H, W)
        assert_depth(d, want, uv, mesh[1], what)
        assert np.all(np.abs(d[d > 0] - 100.0) <= np.spacing(np.float32(100))), what
    outside = {"left": tri((-30.5, 5.5), (-2.25, 10.5), (-20.5, 30.5)), "right": tri((58.25, 5.5), (90.5, 10.5), (70.5, 30.5)),
               "top": tri((5.5, -30.5), (40.5, -2.25), (20.5, -20.5)), "bottom": tri((5.5, 42.25), (40.5, 60.5), (20.5, 80.5)),
               "no sample point in its box": tri((5.1, 5.1), (5.4, 5.1), (5.1, 5.4)),
               "its box holds a sample point outside it": tri((4.75, 4.75), (5.2, 4.75), (4.75, 5.2))}
    for what, mesh in outside.items():
        assert not np_render(*mesh, UNIT_POSE, UNIT_K, H, W)[0].any()
        assert not _render_unit(vsd, dev, mesh, H, W).any(), what
    d = _render_unit(vsd, dev, tri((4.75, 4.75), (5.5, 4.75), (4.75, 5.5)), H, W)      # holds the sample point of pixel (5, 5) alone
    assert list(zip(*np.nonzero(d))) == [(5, 5)] and abs(d[5, 5] - 100.0) <= np.spacing(np.float32(100))


def test_render_degenerate_and_far_faces_among_good_ones(be):
    from nope_amd import vsd
    _, dev, _ = be
    H, W = 72, 96
    K = np.array([[300.0, 0, 47.6], [0, 310.0, 35.2], [0, 0, 1]])
    pose = pose_of(rot(0.4, 0.7, 0.2), [4, -6, 400])
    bx = vsd.box(60.0, 40.0, 50.0)
    line = (np.array([[-10, 0, 0], [0, 0, 0], [10, 0, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32))   # collinear, inside the box
    bv, bf = plate(1.0e5, z=2.0e5)                    # fronto-parallel at Z = 200000 in the camera frame, taken back to the object's
    behind = (((bv.astype(np.float64) - pose[:3, 3]) @ pose[:3, :3]).astype(np.float32), bf)
    verts, faces = concat(bx, line, behind)
    mesh = (verts, np.concatenate([faces, np.array([[0, 0, 1], [3, 5, 5]], dtype=np.int32)]))      # and two faces with a vertex twice
    cam = verts.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    assert cam[-4:, 2].min() > 100000.0 and len(mesh[1]) == 12 + 1 + 2 + 2
    assert np.all(np.prod(np_boxes(*behind, pose, K, H, W), 1) == H * W)           # the far plate covers every pixel: all rejected by z > zfar
    alone = _np(vsd.render_depth(vsd.MeshBank({1: bx}, device=dev), [1], pose[None], K, H, W))[0]
    d = _np(vsd.render_depth(vsd.MeshBank({1: mesh}, device=dev), [1], pose[None], K, H, W))[0]
    assert (alone > 0).sum() > 500 and not (alone > 0).all()
    assert np.array_equal(d.view(np.uint32), alone.view(np.uint32))


MIXED_IDS = [2, 1, 2, 3, 1]         # box, sphere3, box, sphere2, sphere3: face counts 12, 1280, 12, 320, 1280 (max_faces 1280: 5 blockIdx.x)
MIXED_HW = (72, 96)
MIXED_POSES = np.stack([pose_of(rot(0.4, 0.7, 0.2), [4, -6, 400]), pose_of(rot(-0.3, 0.2, 1.1), [-5, 3, 350]), pose_of(rot(1.0, -0.4, 0.3), [-10, 8, 330]),
                        pose_of(rot(0.2, 0.9, -0.5), [6, 2, 300]), pose_of(rot(0.7, 0.1, 2.0), [9, -7, 280])])
MIXED_K = np.stack([np.array([[300.0 + 9 * p, 0, 47.6 - p], [0, 310.0 - 6 * p, 35.2 + 0.7 * p], [0, 0, 1]]) for p in range(5)])


@functools.lru_cache(maxsize=None)
def mixed_meshes():
    from nope_amd import vsd
    return {1: vsd.icosphere(3, 30.0), 2: vsd.box(60.0, 40.0, 50.0), 3: vsd.icosphere(2, 35.0)}


@functools.lru_cache(maxsize=None)
def mixed_want(p):
    return np_render(*mixed_meshes()[MIXED_IDS[p]], MIXED_POSES[p], MIXED_K[p], *MIXED_HW)


def test_render_mixed_face_counts_across_blocks(be):
    """`fl >= cnt` with cnt < max_faces: 12- and 320-face objects in a launch whose grid is sized for 1280 faces."""
    from nope_amd import vsd
    _, dev, _ = be
    H, W = MIXED_HW
    meshes = mixed_meshes()
    assert [len(meshes[o][1]) for o in MIXED_IDS] == [12, 1280, 12, 320, 1280]
    bank = vsd.MeshBank(meshes, device=dev)
    d = _np(vsd.render_depth(bank, MIXED_IDS, MIXED_POSES, MIXED_K, H, W))
    for p, o in enumerate(MIXED_IDS):
        want, uv = mixed_want(p)
        assert (want > 0).sum() > 300
        assert_depth(d[p], want, uv, meshes[o][1], ("pose", p))
        single = _np(vsd.render_depth(bank, [o], MIXED_POSES[p:p + 1], MIXED_K[p:p + 1], H, W))[0]
        assert np.array_equal(d[p].view(np.uint32), single.view(np.uint32)), p
    sm = np.prod(np_boxes(*meshes[1], MIXED_POSES[1], MIXED_K[1], H, W), 1)
    assert ((sm > 0) & (sm <= 64)).sum() > 500          # the one-lane path carries the spheres


def test_render_order_independence_and_repeatability(be):
    """The z-buffer's atomic maximum: the same bits whatever order the faces and the poses arrive in, and on a second call."""
    from nope_amd import vsd
    _, dev, _ = be
    H, W = MIXED_HW
    meshes = mixed_meshes()
    bank = vsd.MeshBank(meshes, device=dev)
    d = _np(vsd.render_depth(bank, MIXED_IDS, MIXED_POSES, MIXED_K, H, W)).view(np.uint32)
    again = _np(vsd.render_depth(bank, MIXED_IDS, MIXED_POSES, MIXED_K, H, W)).view(np.uint32)
    assert np.array_equal(d, again)
    flipped = vsd.MeshBank({o: (v, f[::-1].copy()) for o, (v, f) in meshes.items()}, device=dev)
    assert np.array_equal(d, _np(vsd.render_depth(flipped, MIXED_IDS, MIXED_POSES, MIXED_K, H, W)).view(np.uint32))
    back = _np(vsd.render_depth(bank, MIXED_IDS[::-1], MIXED_POSES[::-1].copy(), MIXED_K[::-1].copy(), H, W)).view(np.uint32)
    assert np.array_equal(d, back[::-1])


def test_render_skipped_count_is_exact(be):
    from nope_amd import vsd
    hip, dev, _ = be
    verts, faces = vsd.box(50.0, 50.0, 50.0)
    poses = np.stack([pose_of(np.eye(3), [0, 0, 400]), pose_of(np.eye(3), [0, 0, 10])])
    Z = verts.astype(np.float64) @ poses[1][:3, :3].T[:, 2] + poses[1][2, 3]
    n = int((Z[faces] <= 0.05).any(1).sum())
    assert 0 < n < 12          # the two triangles of the far side stay in front of znear
    bank = vsd.MeshBank({1: (verts, faces)}, device=dev)
    with pytest.raises(hip.NopeError) as ei:
        vsd.render_depth(bank, [1, 1], poses, np.array([[500.0, 0, 16.3], [0, 505.0, 15.7], [0, 0, 1]]), 32, 32)
    assert re.search(rf"pose 1 \(obj_id 1\): {n} triangles", str(ei.value)) and "pose 0" not in str(ei.value), str(ei.value)


def test_render_index_and_range_guards_on_emu(emu):
    """Guards that MeshBank makes unreachable from Python, through ctypes and on the interpreter only: a vertex index outside [0, V)
    drops that face alone, and a face range running past F is cut at F."""
    H = W = 24
    a, b, c = tri((1.75, 1.75), (9.5, 1.75), (1.75, 9.5)), tri((10.75, 1.75), (23.5, 1.75), (10.75, 6.5)), tri((2.25, 12.25), (20.5, 12.25), (2.25, 20.5))
    verts, faces = concat(a, b, c)
    want_ab = np_render(*concat(a, b), UNIT_POSE, UNIT_K, H, W)[0]
    want_ac = np_render(*concat(a, c), UNIT_POSE, UNIT_K, H, W)[0]
    assert (want_ab > 0).sum() > 60 and (want_ac > 0).sum() > 100
    # V = 6 of the 9 vertices in the buffer: the third face indexes 6, 7, 8; then a negative index in the second face
    code, d, skipped, _ = _raw_render(emu, "cpu", verts, 6, faces, 3, [0], [3], 3, UNIT_POSE[None], UNIT_K, H, W)
    assert code == 0 and skipped[0] == 0
    assert_depth(d[0], want_ab, what="vertex index >= V")
    bad = faces.copy()
    bad[1, 2] = -1
    code, d, skipped, _ = _raw_render(emu, "cpu", verts, 9, bad, 3, [0], [3], 3, UNIT_POSE[None], UNIT_K, H, W)
    assert code == 0 and skipped[0] == 0
    assert_depth(d[0], want_ac, what="negative vertex index")
    # F = 2 of the 3 faces in the buffer, a range of 3 from 0 and a range of 2 from 1
    code, d, skipped, _ = _raw_render(emu, "cpu", verts, 9, faces, 2, [0, 1], [3, 2], 3, np.stack([UNIT_POSE, UNIT_POSE]), UNIT_K, H, W)
    assert code == 0 and np.all(skipped == 0)
    assert_depth(d[0], want_ab, what="face range past F")
    assert_depth(d[1], np_render(*b, UNIT_POSE, UNIT_K, H, W)[0], what="face range past F, from 1")


def test_launchers_refuse_bad_arguments_before_any_launch(be):
    hip, dev, _ = be
    dll = hip.lib().dll
    f = torch.zeros(4 * 8 * 8, dtype=torch.float32, device=dev)
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    out = torch.full((64,), 777.0, dtype=torch.float32, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()

    def render(P=1, H=8, W=8, max_faces=1, ws_bytes=4096):
        return dll.nope_op_render_depth(p(f), 3, p(i), 1, p(i), p(i), max_faces, p(d), p(d), P, H, W, p(out), p(i), p(ws), ws_bytes, None)

    need = int(dll.nope_op_render_depth_workspace_bytes(1, 1))
    assert need == 256 + 8 and render(ws_bytes=need - 1) == ERR_WORKSPACE
    assert render(P=65536) == ERR_ARG
    assert render(H=32769, W=32768) == ERR_ARG          # H W = 2^30 + 2^15
    err = torch.full((8,), 777.0, dtype=torch.float64, device=dev)

    def vsd_op(k=1, H=8, W=8, tau=20.0, ws_bytes=4096):
        return dll.nope_op_vsd(p(f), p(f), p(f), p(d), 1, k, H, W, 15.0, tau, 0, 0, p(err), p(ws), ws_bytes, None)

    need = int(dll.nope_op_vsd_workspace_bytes(1, 1, 8, 8))
    assert need == 24 and vsd_op(ws_bytes=need - 1) == ERR_WORKSPACE
    assert vsd_op(tau=0.0) == ERR_ARG and vsd_op(k=0) == ERR_ARG and vsd_op(k=17) == ERR_ARG
    assert vsd_op(H=32769, W=32768) == ERR_ARG
    _sync(dev)
    assert bool((out == 777.0).all()) and bool((err == 777.0).all()) and not bool(ws.any()), "a refused call wrote"


# ---- C. vsd.vsd_error ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("hw", [(40, 52), (41, 53)])
def test_vsd_error_launch_layout(be, hw, k):
    """The (B, 1 + k) rasteriser launch and its slicing into ground truth and estimates, at KC = 1 and KC = 16, VW = 4 and VW = 1."""
    from nope_amd import vsd
    _, dev, _ = be
    H, W = hw
    B, ids = 2, [1, 2]
    bank = vsd.MeshBank({1: vsd.box(70.0, 50.0, 45.0), 2: vsd.icosphere(2, 40.0)}, device=dev)
    K = np.stack([np.array([[250.0 + 5 * b, 0, W / 2 - 0.3 + b], [0, 252.0 - 3 * b, H / 2 + 0.2 - b], [0, 0, 1]]) for b in range(B)])
    gt_R = np.stack([rot(0.4, 0.7, 0.2), rot(-0.3, 0.2, 1.1)])
    gt_t = np.array([[3.0, -2.0, 450.0], [-4.0, 5.0, 430.0]])
    pred_R = np.stack([np.stack([rot(0.05 * j, -0.03 * j, 0.1 * j) @ gt_R[b] for j in range(1, k + 1)]) for b in range(B)])
    gt = vsd.render_depth(bank, ids, vsd.compose_poses(gt_R, gt_t), K, H, W).cpu()
    g = torch.Generator().manual_seed(11)
    scene = gt + torch.randn(gt.shape, generator=g) * 3
    scene[gt == 0] = 700.0
    scene[:, :, W // 2: W // 2 + 6] = 380.0          # an occluder
    scene[:, H // 3, :] = 0.0                        # missing depth
    dtest = scene.float()
    for cost, vis in CASES:
        err, d_gt, d_est = vsd.vsd_error(dtest.to(dev), bank, ids, pred_R, gt_R, gt_t, K, DELTA, TAU, cost, visib_mode=vis, return_depth=True)
        err, d_gt, d_est = _np(err), _np(d_gt), _np(d_est)
        assert err.shape == (B, k) and d_gt.shape == (B, H, W) and d_est.shape == (B, k, H, W)
        want = np_vsd(dtest.numpy(), d_gt, d_est, K, cost_type=cost, visib_mode=vis)
        assert np.all(want < 1.0) and (cost == "step" or np.all(want > 0.0))
        assert_vsd(err, want, cost, (hw, k, cost, vis))
    assert np.array_equal(d_gt.view(np.uint32), gt.numpy().view(np.uint32))
    for b in range(B):
        for j in range(k):
            one = _np(vsd.render_depth(bank, [ids[b]], pose_of(pred_R[b, j], gt_t[b])[None], K[b], H, W))[0]
            assert np.array_equal(d_est[b, j].view(np.uint32), one.view(np.uint32)), (b, j)
