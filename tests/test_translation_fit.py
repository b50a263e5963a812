"""nope_op_fit_translation, nope_op_mask_boxes and nope_op_depth_shift (csrc/kernels_posefit.hip) and their host side
(nope_amd/bop.py: estimate_translation, refine_translation_depth; vsd.vsd_error(pred_t=...); PoseConditional.eval_bop(translation=...)),
each kernel test on the interpreter (tests/hipemu) and on the device.

The yardstick is the f64 NumPy restatement of include/nope_hip.h below: the same sequence of operations, every 3-term product written
out left to right, numpy's own min / max (which keep a NaN) and numpy's own sum.

Bounds:
  fit          nothing is summed over the vertices and min / max are exact in any order: t, residual, iters and status are bit-equal.
  mask boxes   integers: equal.
  depth shift  count is equal; the two means differ in summation order alone: each sum of n terms is within (n - 1) 2^-53 sum|term| of the
               exact one and each division rounds once, so |shift - numpy's| <= n 2^-52 sum|term| / n.
  recovery     the box is the restatement's own projected box of a planted t: max |t^ - t| / t_z <= 1e-8 (2000 such cases on the
               restatement converged within 23 iterations with a largest error of 1.2e-9; the bound is 8 x that).
  rasteriser   a rendered mask's box is the vertex box quantised to pixels: e = 1 px per edge (0.5 px of quantisation, the ellipsoid has
               no slivers).  With m = min(bw, bh), first order: |dt_z| <= 2 e t_z / m, |dt_x| <= e t_z / fx + |t_x| 2 e / m; the
               asserted bound is 1.5 x that for the second order (edges perturbed by +-1 px on the restatement reached 0.87 of it).
  depth stage  one round from the same t: the renderings are the same bits, the shifts differ by the summation bound D, so
               |dt_c| <= |t_c| D / t_z + 8 2^-53 |t_c|.
Shapes are named from the kernel's constant (NOPE_FIT_THREADS)."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
ERR_ARG, ERR_WORKSPACE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K0 = np.array([[1075.0, 0, 360.0], [0, 1073.0, 270.0], [0, 0, 1.0]])
NONFINITE, BAD_BOX, VERT_RANGE, BEHIND, NOT_CONVERGED = 1, 2, 4, 8, 16
RADII = (40.0, 25.0, 15.0)
DIAM = 2 * RADII[0]


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def test_constants_mirror_the_header():
    from nope_amd import bop, hip
    src = open(os.path.join(ROOT, "include", "nope_hip.h")).read()
    for name, val in (("NOPE_FIT_NONFINITE", bop.FIT_NONFINITE), ("NOPE_FIT_BAD_BOX", bop.FIT_BAD_BOX), ("NOPE_FIT_VERT_RANGE", bop.FIT_VERT_RANGE),
                      ("NOPE_FIT_BEHIND", bop.FIT_BEHIND), ("NOPE_FIT_NOT_CONVERGED", bop.FIT_NOT_CONVERGED), ("NOPE_FIT_THREADS", bop.FIT_THREADS)):
        assert re.search(rf"\b{name} = {val}\b", src), name
    assert (bop.FIT_NONFINITE, bop.FIT_BAD_BOX, bop.FIT_VERT_RANGE, bop.FIT_BEHIND, bop.FIT_NOT_CONVERGED) == (NONFINITE, BAD_BOX, VERT_RANGE, BEHIND,
                                                                                                             NOT_CONVERGED)
    assert not (bop.ST_DEPTH_FEW | bop.ST_DEPTH_POSE) & 31 and bop.ST_DEPTH_FEW != bop.ST_DEPTH_POSE
    assert int(re.search(r"#define NOPE_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == 25
    assert v_shapes() == [1, 2, 63, 64, 65, 255, 257, 513, 5000]


def v_shapes():
    from nope_amd import bop
    T = bop.FIT_THREADS
    return [1, 2, 63, 64, 65, T - 1, T + 1, 2 * T + 1, 5000]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def rot(R, x):
    """y = R x for the points x (V, 3): (R0 x + R1 y) + R2 z per row, each operation rounded once."""
    return [R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1] + R[r, 2] * x[:, 2] for r in range(3)]


def nmax(a, b):
    return a if a != a else (b if (b > a or b != b) else a)


def np_project_box(verts, R, K, t):
    """(pu0, pv0, pu1, pv1, min Z) of the vertices at (R, t): the loop's own projection."""
    with np.errstate(all="ignore"):
        yx, yy, yz = rot(R, verts.astype(np.float64))
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        Z = yz + t[2]
        u = fx * ((yx + t[0]) / Z) + cx
        v = fy * ((yy + t[1]) / Z) + cy
        return u.min(), v.min(), u.max(), v.max(), Z.min()


def np_fit(verts, R, K, box, max_iters=32, tol_scale=1e-9, tol_px=1e-6):
    """include/nope_hip.h, nope_op_fit_translation, for one pose with a good vertex range: (t (3,), residual, iters, status)."""
    nan3 = np.full(3, np.nan)
    R, K, box = np.asarray(R, np.float64), np.asarray(K, np.float64), np.asarray(box, np.float64)
    with np.errstate(all="ignore"):
        u0, v0, u1, v1 = box
        bw, bh, cu, cv = u1 - u0, v1 - v0, 0.5 * (u0 + u1), 0.5 * (v0 + v1)
        st = 0
        if not (np.isfinite(R).all() and np.isfinite(K).all() and np.isfinite(box).all()):
            st |= NONFINITE
        if np.isfinite(box).all() and (not bw > 0 or not bh > 0):
            st |= BAD_BOX
        if st:
            return nan3, np.nan, 0, st
        fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
        yx, yy, yz = rot(R, verts.astype(np.float64))
        ax0, ax1, ay0, ay1 = yx.min(), yx.max(), yy.min(), yy.max()
        z = 0.5 * ((fx * (ax1 - ax0)) / bw + (fy * (ay1 - ay0)) / bh)
        tx, ty, tz = ((cu - cx) / fx) * z - 0.5 * (ax0 + ax1), ((cv - cy) / fy) * z - 0.5 * (ay0 + ay1), z
        n = 0
        while True:
            Z = yz + tz
            if not Z.min() > 0:
                return nan3, np.nan, n, BEHIND
            u = fx * ((yx + tx) / Z) + cx
            v = fy * ((yy + ty) / Z) + cy
            pu0, pu1, pv0, pv1 = u.min(), u.max(), v.min(), v.max()
            s = 0.5 * ((pu1 - pu0) / bw + (pv1 - pv0) / bh)
            du, dv = cu - 0.5 * (pu0 + pu1), cv - 0.5 * (pv0 + pv1)
            res = nmax(nmax(nmax(abs(pu0 - u0), abs(pu1 - u1)), abs(pv0 - v0)), abs(pv1 - v1))
            if abs(s - 1.0) <= tol_scale and abs(du) <= tol_px and abs(dv) <= tol_px:
                return np.array([tx, ty, tz]), res, n, 0
            if n == max_iters:
                return np.array([tx, ty, tz]), res, n, NOT_CONVERGED
            zn = tz * s
            tx, ty, tz = tx * s + (du * zn) / fx, ty * s + (dv * zn) / fy, zn
            n += 1


def np_mask_boxes(mask):
    box, cnt = np.full((len(mask), 4), np.nan), np.zeros(len(mask), np.int32)
    for b, m in enumerate(mask):
        ys, xs = np.nonzero(m)
        cnt[b] = len(xs)
        if len(xs):
            box[b] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
    return box, cnt


def np_depth_shift(dtest, dest, tau, mask=None):
    """(shift (B, k), count (B, k), sum|term| (B, k)) with numpy's own sum."""
    B, k = dest.shape[:2]
    shift, cnt, mag = np.full((B, k), np.nan), np.zeros((B, k), np.int32), np.zeros((B, k))
    with np.errstate(all="ignore"):
        for b in range(B):
            for j in range(k):
                t, e = dtest[b].astype(np.float64), dest[b, j].astype(np.float64)
                d = t - e
                ok = (dtest[b] > 0) & (dest[b, j] > 0) & (np.abs(d) <= tau)
                if mask is not None:
                    ok &= mask[b] != 0
                cnt[b, j], mag[b, j] = ok.sum(), np.abs(d[ok]).sum()
                if cnt[b, j]:
                    shift[b, j] = d[ok].sum() / cnt[b, j]
    return shift, cnt, mag


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def haar(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def ellipsoid(level):
    """vsd.icosphere scaled per axis, so that the rotation matters: (verts f32, faces)."""
    from nope_amd import vsd
    v, f = vsd.icosphere(level, 1.0)
    return (v.astype(np.float64) * np.array(RADII)).astype(np.float32), f


def planted_t(rng, lo, hi, off_axis):
    tz = rng.uniform(lo, hi) * DIAM
    r, a = off_axis * math.sqrt(rng.uniform(0, 1)), rng.uniform(0, 2 * math.pi)
    return np.array([r * math.cos(a) * tz, r * math.sin(a) * tz, tz])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """bit-equal, a NaN matching any NaN (the sign of an invalid operation's NaN is the machine's)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


class FitCase:
    """P poses over two objects, the first V vertices of the level-5 ellipsoid and vsd.box: the flat arrays the entry takes.  The box of a
    pose is the projected box of a planted t, each edge moved outwards by 1 .. 5 px: positive sizes whatever V is, and an aspect that no
    t reproduces."""

    def __init__(self, V, P, seed):
        from nope_amd import vsd
        rng = np.random.default_rng(seed)
        self.objs = [ellipsoid(5)[0][:V], vsd.box(70.0, 50.0, 42.0)[0]]
        self.verts = np.concatenate(self.objs)
        offs = [0, V]
        self.obj = [p % 2 for p in range(P)]
        self.vert_off, self.vert_cnt = [offs[o] for o in self.obj], [len(self.objs[o]) for o in self.obj]
        self.R = np.stack([haar(rng) for _ in range(P)])
        self.K = np.repeat(K0[None], P, 0)
        self.t = np.stack([planted_t(rng, 2, 8, 0.3) for _ in range(P)])
        self.box = np.zeros((P, 4))
        for p in range(P):
            b = np_project_box(self.objs[self.obj[p]], self.R[p], K0, self.t[p])
            self.box[p] = np.array(b[:4]) + rng.uniform(1, 5, size=4) * [-1, -1, 1, 1]
        self.P = P

    def want(self, **kw):
        rows = [np_fit(self.objs[self.obj[p]], self.R[p], self.K[p], self.box[p], **kw) for p in range(self.P)]
        return {"t": np.stack([r[0] for r in rows]), "residual": np.array([r[1] for r in rows]), "iters": np.array([r[2] for r in rows]),
                "status": np.array([r[3] for r in rows])}

    def run(self, dev, verts=None, vert_off=None, vert_cnt=None, max_verts=None, R=None, K=None, box=None, **kw):
        from nope_amd import bop
        vc = self.vert_cnt if vert_cnt is None else vert_cnt
        out = bop.op_fit_translation(torch.from_numpy(self.verts if verts is None else verts).to(dev), self.vert_off if vert_off is None else vert_off,
                                     vc, max(self.vert_cnt) if max_verts is None else max_verts, self.R if R is None else R,
                                     self.K if K is None else K, self.box if box is None else box, **kw)
        return {k: t.cpu().numpy() for k, t in out.items()}


@functools.lru_cache(maxsize=None)
def fit_case(V, P, seed=0):
    return FitCase(V, P, 100 * seed + 7 * V + P)


def check_fit(got, want, what):
    assert np.array_equal(got["status"], want["status"]), (what, got["status"], want["status"])
    assert np.array_equal(got["iters"], want["iters"]), (what, got["iters"], want["iters"])
    assert same_bits(got["t"], want["t"]), (what, got["t"], want["t"])
    assert same_bits(got["residual"], want["residual"]), (what, got["residual"], want["residual"])
    assert got["t"].dtype == np.float64 and got["iters"].dtype == np.int32 and got["status"].dtype == np.int32


# ---- A. the fit against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iters", [0, 1, 32])
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 257, 513, 5000])
def test_fit_bit_equal(be, V, max_iters):
    """Two objects in one call (the V-vertex ellipsoid and the 8-vertex box).  V around the wave, around the workgroup, a lane with three
    vertices, and ~5000 (20 trips)."""
    assert V in v_shapes()
    _, dev, _ = be
    c = fit_case(V, 2)
    want = c.want(max_iters=max_iters)
    got = c.run(dev, max_iters=max_iters)
    check_fit(got, want, (V, max_iters))
    if V <= 2:
        return                                                   # (one or two vertices: the initial z is 0 or arbitrary; the bits agree all the same)
    if max_iters < 32:
        assert np.all(want["iters"] == max_iters) and np.all(want["status"] == NOT_CONVERGED) and np.all(np.isfinite(want["t"]))
    else:
        assert np.all(want["status"] == 0) and np.all(want["iters"] > 1), want      # (the widened boxes take real iterations)


@pytest.mark.parametrize("P", [1, 2, 17])
def test_fit_pose_counts_and_run_to_run_bits(be, P):
    _, dev, _ = be
    c = fit_case(65, P, seed=1)
    got = c.run(dev)
    check_fit(got, c.want(), ("P", P))
    again = c.run(dev, max_verts=1000)          # (a larger max_verts than any range: the same bits)
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)


def test_fit_status_bits(be):
    """Every status bit, each in one row of a batch whose other rows keep their bits."""
    _, dev, _ = be
    c = fit_case(65, 8, seed=2)
    base = c.run(dev)
    assert np.all(base["status"] == 0)
    R, K, box, verts = c.R.copy(), c.K.copy(), c.box.copy(), c.verts.copy()
    vo, vc = list(c.vert_off), list(c.vert_cnt)
    R[0, 1, 2] = np.nan
    K[1, 2, 0] = np.inf                                     # (no arithmetic reads it: the rule is about K, not about what is used)
    box[2, 3] = np.nan
    box[3, 2] = box[3, 0]                                   # zero width
    vo[5], vc[5] = len(verts) - 4, 8                        # past the end
    box[6] = [-1e7, -1e7, 1e7, 1e7]                         # the initial z is a fraction of a millimetre: half the vertices at Z <= 0
    got = c.run(dev, R=R, K=K, box=box, vert_off=vo, vert_cnt=vc)
    assert got["status"].tolist() == [NONFINITE, NONFINITE, NONFINITE, BAD_BOX, 0, VERT_RANGE, BEHIND, 0]
    for p in (0, 1, 2, 3, 5, 6):
        assert np.all(np.isnan(got["t"][p])) and np.isnan(got["residual"][p]) and got["iters"][p] == 0, p
    for p in (4, 7):
        assert all(same_bits(got[k][p], base[k][p]) for k in ("t", "residual")) and got["iters"][p] == base["iters"][p]
    want6 = np_fit(c.objs[0], R[6], K[6], box[6])
    assert want6[3] == BEHIND and want6[2] == 0
    # negative height, an empty range, a negative offset, a count above max_verts
    box2 = c.box.copy()
    box2[1, 1], box2[1, 3] = c.box[1, 3], c.box[1, 1]
    got = c.run(dev, box=box2, vert_off=[0, 65, 0, -1, 0, 65, 0, 65], vert_cnt=[65, 8, 0, 8, 66, 8, 65, 8])
    assert got["status"].tolist() == [0, BAD_BOX, VERT_RANGE, VERT_RANGE, VERT_RANGE, 0, 0, 0]
    # not converged: t and residual are written
    got = c.run(dev, max_iters=1)
    assert np.all(got["status"] == NOT_CONVERGED) and np.all(got["iters"] == 1) and np.all(np.isfinite(got["t"])) and np.all(got["residual"] > 0)
    # a NaN vertex at a middle index: the poses of that object are NaN (the restatement says the same), the others keep their bits
    verts[33, 1] = np.nan
    got = c.run(dev, verts=verts)
    for p in range(c.P):
        if c.obj[p] == 0:
            w = np_fit(verts[:65], c.R[p], c.K[p], c.box[p])
            assert np.all(np.isnan(w[0])) and np.all(np.isnan(got["t"][p])) and np.isnan(got["residual"][p]) and got["status"][p] == w[3] == BEHIND
        else:
            assert same_bits(got["t"][p], base["t"][p]) and got["status"][p] == 0


def test_fit_argument_errors_write_nothing(be):
    hip, dev, _ = be
    c = fit_case(65, 3, seed=3)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    a = dict(verts=t(c.verts, torch.float32), V=len(c.verts), vert_off=t(np.array(c.vert_off), torch.int32), vert_cnt=t(np.array(c.vert_cnt), torch.int32),
             max_verts=65, R=t(c.R, torch.float64), K=t(c.K, torch.float64), box=t(c.box, torch.float64), P=c.P, max_iters=32, tol_scale=1e-9,
             tol_px=1e-6, t=torch.full((c.P, 3), -7.0, dtype=torch.float64, device=dev), residual=torch.full((c.P,), -7.0, dtype=torch.float64, device=dev),
             iters=torch.full((c.P,), -7, dtype=torch.int32, device=dev), status=torch.full((c.P,), -7, dtype=torch.int32, device=dev))
    order = ("verts", "V", "vert_off", "vert_cnt", "max_verts", "R", "K", "box", "P", "max_iters", "tol_scale", "tol_px", "t", "residual", "iters", "status")
    p = lambda x: x.data_ptr() if isinstance(x, torch.Tensor) else x

    def call(**over):
        b = dict(a, **over)
        return hip.lib().dll.nope_op_fit_translation(*(p(b[k]) for k in order), None)

    def untouched():
        if dev != "cpu":
            torch.cuda.synchronize()
        return all(bool((a[o] == -7).all()) for o in ("t", "residual", "iters", "status"))

    for key in ("verts", "vert_off", "vert_cnt", "R", "K", "box", "t", "residual", "iters", "status"):
        assert call(**{key: None}) == ERR_ARG, key
    for key in ("V", "P", "max_verts"):
        for bad in (0, -1):
            assert call(**{key: bad}) == ERR_ARG, (key, bad)
    assert call(max_iters=-1) == ERR_ARG
    for key in ("tol_scale", "tol_px"):
        for bad in (-1e-30, float("nan")):
            assert call(**{key: bad}) == ERR_ARG, (key, bad)
    assert untouched()
    assert call() == 0 and not untouched()
    assert same_bits(a["t"].cpu().numpy(), c.want()["t"])
    assert call(tol_scale=0.0, tol_px=0.0, max_iters=0) == 0          # zero tolerances and no iteration are legal


# ---- B. mask boxes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_mask_boxes(be, B):
    """H x W = 37 x 50 (W no multiple of 64, 1850 pixels: no multiple of the workgroup): a pixel in each corner, the full image, the
    empty one, a blob, values other than 1, and the batch in two orders."""
    from nope_amd import bop
    _, dev, _ = be
    H, W = 37, 50
    rng = np.random.default_rng(3)
    imgs = []
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        imgs.append(m)
    imgs.append(np.full((H, W), 255, np.uint8))
    imgs.append(np.zeros((H, W), np.uint8))
    blob = np.zeros((H, W), np.uint8)
    blob[5:30, 7:41] = rng.integers(0, 2, size=(25, 34)) * rng.integers(1, 256, size=(25, 34))
    imgs.append(blob)
    two = np.zeros((H, W), np.uint8)
    two[36, 3], two[2, 48] = 7, 128
    imgs.append(two)
    imgs.append(np.zeros((H, W), np.uint8))
    for i0 in range(0, len(imgs) - B + 1, B):
        mask = np.stack(imgs[i0: i0 + B])
        box, cnt = bop.op_mask_boxes(torch.from_numpy(mask).to(dev))
        wb, wc = np_mask_boxes(mask)
        assert same_bits(box.cpu().numpy(), wb) and np.array_equal(cnt.cpu().numpy(), wc), (i0, box, wb, cnt, wc)
        box2, cnt2 = bop.op_mask_boxes(torch.from_numpy(mask).to(dev))
        assert same_bits(box2.cpu().numpy(), box.cpu().numpy()) and torch.equal(cnt, cnt2), "run-to-run"
    wb, _ = np_mask_boxes(np.stack(imgs[:6]))
    assert wb[3].tolist() == [W - 1, H - 1, W, H] and wb[4].tolist() == [0, 0, W, H] and np.all(np.isnan(wb[5]))
    # a bool mask counts its True pixels
    box, cnt = bop.op_mask_boxes(torch.from_numpy(blob > 0)[None].to(dev))
    assert same_bits(box.cpu().numpy(), np_mask_boxes(blob[None])[0]) and int(cnt[0]) == int((blob > 0).sum())


def test_mask_boxes_argument_errors(be):
    hip, dev, _ = be
    m = torch.ones((2, 5, 6), dtype=torch.uint8, device=dev)
    box = torch.full((2, 4), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((2,), -7, dtype=torch.int32, device=dev)
    f = hip.lib().dll.nope_op_mask_boxes
    assert [f(None, 2, 5, 6, box.data_ptr(), cnt.data_ptr(), None), f(m.data_ptr(), 2, 5, 6, None, cnt.data_ptr(), None),
            f(m.data_ptr(), 2, 5, 6, box.data_ptr(), None, None)] == [ERR_ARG] * 3
    assert [f(m.data_ptr(), 0, 5, 6, box.data_ptr(), cnt.data_ptr(), None), f(m.data_ptr(), 2, 0, 6, box.data_ptr(), cnt.data_ptr(), None),
            f(m.data_ptr(), 2, 5, -1, box.data_ptr(), cnt.data_ptr(), None), f(m.data_ptr(), 2, 1 << 16, 1 << 15, box.data_ptr(), cnt.data_ptr(), None)] \
        == [ERR_ARG] * 4
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((box == -7).all()) and bool((cnt == -7).all())
    assert f(m.data_ptr(), 2, 5, 6, box.data_ptr(), cnt.data_ptr(), None) == 0
    assert box.cpu().tolist() == [[0.0, 0.0, 6.0, 5.0]] * 2 and cnt.cpu().tolist() == [30, 30]


# ---- C. depth shift -------------------------------------------------------------------------------------------------------------------
TAU = 20.0


@functools.lru_cache(maxsize=None)
def depth_case(k):
    """48 x 40 images (1920 pixels: two workgroups per image, the second one partly idle).  test and the k estimates = one surface near
    500 mm + noise of a few mm, each estimate off by up to 8 mm; planted per image: differences of exactly +-tau (inliers) and one f32 step beyond (outliers), zero and NaN depths in the
    middle of a row on either side, an inf, a far outlier, a column where the estimate is empty."""
    rng = np.random.default_rng(11 + k)
    B, H, W = 2, 40, 48
    plane = 500.0 + rng.uniform(-30, 30, size=(B, 1, H, W))
    est = (plane + rng.uniform(-8, 8, size=(B, k, 1, 1)) + rng.normal(0, 1.0, size=(B, k, H, W))).astype(np.float32)
    test = (plane[:, 0] + rng.normal(0, 3.0, size=(B, H, W))).astype(np.float32)
    est[:, :, :, 40:] = 0.0
    f32 = np.float32
    for b in range(B):
        for j in range(k):
            e = est[b, j]
            test_row = 3 + b
            e[test_row, 10] = test[b, test_row, 10] - f32(TAU)                               # test - est = +tau exactly (f32 values chosen so)
            e[test_row, 11] = np.nextafter(test[b, test_row, 11] - f32(TAU), f32(-np.inf))   # one step beyond
            e[test_row, 12] = test[b, test_row, 12] + f32(TAU)
            e[test_row, 13] = np.nextafter(test[b, test_row, 13] + f32(TAU), f32(np.inf))
            e[20, 17 + (j % 3)] = 0.0
            e[21, 19] = np.nan
            e[22, 5] = np.inf
        test[b, 20, 25] = 0.0
        test[b, 21, 26] = np.nan
        test[b, 22, 30] = 5000.0
        test[b, 23, 7] = -3.0
    mask = np.zeros((B, H, W), np.uint8)
    mask[:, 2:30, 4:44] = 1
    mask[1, 20:24, :] = 9
    return test, est, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [1, 16])
def test_depth_shift(be, k, masked):
    from nope_amd import bop
    _, dev, _ = be
    test, est, mask = depth_case(k)
    m = mask if masked else None
    want, wcnt, mag = np_depth_shift(test, est, TAU, m)
    # the planted pixels are what they are meant to be
    for b in range(2):
        d = test[b].astype(np.float64) - est[b, 0].astype(np.float64)
        r = 3 + b
        assert d[r, 10] == TAU and d[r, 11] > TAU and d[r, 11] - TAU < 1e-4 and d[r, 12] == -TAU and d[r, 13] < -TAU and d[r, 13] + TAU > -1e-4
    shift, cnt = bop.op_depth_shift(torch.from_numpy(test).to(dev), torch.from_numpy(est).to(dev), TAU,
                                    None if m is None else torch.from_numpy(m).to(dev))
    shift, cnt = shift.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt, wcnt) and cnt.dtype == np.int32, (cnt, wcnt)
    assert wcnt.min() > 900 and (masked or wcnt.min() > 1500) and (not masked or wcnt.max() < 28 * 40 + 4 * 48)
    bound = wcnt * 2.0 ** -52 * mag / wcnt
    diff = np.abs(shift - want)
    print("depth shift k", k, "masked", masked, "observed %.3g, bound %.3g" % (diff.max(), bound.min()))
    assert np.all(diff <= bound), (diff, bound)
    again, cnt2 = bop.op_depth_shift(torch.from_numpy(test).to(dev), torch.from_numpy(est).to(dev), TAU,
                                     None if m is None else torch.from_numpy(m).to(dev))
    assert same_bits(again.cpu().numpy(), shift) and np.array_equal(cnt2.cpu().numpy(), cnt), "run-to-run bits"
    # no inlier: a NaN shift and count 0 (tau = 0 keeps exact matches alone; an empty mask keeps nothing)
    s0, c0 = bop.op_depth_shift(torch.from_numpy(test).to(dev), torch.from_numpy(est).to(dev), TAU, torch.zeros(mask.shape, dtype=torch.uint8, device=dev))
    assert bool(torch.isnan(s0).all()) and int(c0.abs().sum()) == 0
    twin = np.repeat(test[:, None], k, 1)
    sz, cz = bop.op_depth_shift(torch.from_numpy(test).to(dev), torch.from_numpy(twin).to(dev), 0.0)
    assert np.array_equal(cz.cpu().numpy(), np_depth_shift(test, twin, 0.0)[1]) and int(cz.min()) > 1900 and np.all(sz.cpu().numpy() == 0.0)


def test_depth_shift_argument_errors(be):
    hip, dev, _ = be
    test, est, mask = depth_case(1)
    t, e = torch.from_numpy(test).to(dev), torch.from_numpy(est).to(dev)
    B, k, H, W = est.shape
    l = hip.lib()
    need = int(l.dll.nope_op_depth_shift_workspace_bytes(B, k, H, W))
    assert need > 0 and l.dll.nope_op_depth_shift_workspace_bytes(0, k, H, W) == 0 and l.dll.nope_op_depth_shift_workspace_bytes(B, k, 0, W) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    shift = torch.full((B, k), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((B, k), -7, dtype=torch.int32, device=dev)
    a = dict(t=t.data_ptr(), e=e.data_ptr(), m=None, B=B, k=k, H=H, W=W, tau=TAU, s=shift.data_ptr(), c=cnt.data_ptr(), ws=ws.data_ptr(), wb=need)
    call = lambda **o: l.dll.nope_op_depth_shift(*(dict(a, **o)[x] for x in ("t", "e", "m", "B", "k", "H", "W", "tau", "s", "c", "ws", "wb")), None)
    assert [call(t=None), call(e=None), call(s=None), call(c=None), call(ws=None)] == [ERR_ARG] * 5
    assert [call(B=0), call(B=65536), call(k=0), call(k=17), call(H=0), call(W=-2), call(H=1 << 16, W=1 << 15)] == [ERR_ARG] * 7
    assert [call(tau=-1.0), call(tau=float("nan"))] == [ERR_ARG] * 2
    assert call(wb=need - 1) == ERR_WORKSPACE and call(wb=0) == ERR_WORKSPACE
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((shift == -7).all()) and bool((cnt == -7).all()) and bool((ws == 0x5A).all())
    assert call() == 0 and np.array_equal(cnt.cpu().numpy(), np_depth_shift(test, est, TAU)[1])


# ---- D. recovery ----------------------------------------------------------------------------------------------------------------------
def test_planted_recovery(be):
    """24 planted translations at 2 .. 8 diameters, off-axis by up to 0.3 of the distance; the box is the restatement's own projected box."""
    from nope_amd import bop
    _, dev, _ = be
    rng = np.random.default_rng(2024)
    verts = ellipsoid(3)[0]
    P = 24
    R = np.stack([haar(rng) for _ in range(P)])
    t = np.stack([planted_t(rng, 2, 8, 0.3) for _ in range(P)])
    box = np.stack([np_project_box(verts, R[p], K0, t[p])[:4] for p in range(P)])
    want = [np_fit(verts, R[p], K0, box[p]) for p in range(P)]
    err = max(np.abs(w[0] - t[p]).max() / t[p, 2] for p, w in enumerate(want))
    print("planted recovery: restatement's largest error %.3g, most iterations %d" % (err, max(w[2] for w in want)))
    assert all(w[3] == 0 for w in want) and err <= 1e-8
    got = bop.op_fit_translation(torch.from_numpy(verts).to(dev), [0] * P, [len(verts)] * P, len(verts), R, np.repeat(K0[None], P, 0), box)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.all(got["status"] == 0) and np.all(got["iters"] <= 32)
    assert (np.abs(got["t"] - t).max(axis=1) / t[:, 2]).max() <= 1e-8
    assert same_bits(got["t"], np.stack([w[0] for w in want])) and np.all(got["residual"] < 1e-4)


@functools.lru_cache(maxsize=None)
def raster_case():
    """4 planted poses of the level-3 ellipsoid at 3 .. 6 diameters in a 720 x 540 image, every one with a box of at least 60 px on its short
    side and inside the image."""
    rng = np.random.default_rng(77)
    verts, faces = ellipsoid(3)
    R, t = [], []
    while len(R) < 4:
        Rp, tp = haar(rng), planted_t(rng, 3, 6, 0.12)
        b = np_project_box(verts, Rp, K0, tp)
        if min(b[2] - b[0], b[3] - b[1]) >= 60 and b[0] > 2 and b[1] > 2 and b[2] < 718 and b[3] < 538:
            R.append(Rp)
            t.append(tp)
    return verts, faces, np.stack(R), np.stack(t)


def test_rasteriser_loop(be):
    """render_depth at a planted pose -> mask = depth > 0 -> op_mask_boxes -> estimate_translation: the planted t within the first-order
    sensitivity to 1 px per edge."""
    from nope_amd import bop, vsd
    _, dev, _ = be
    verts, faces, R, t = raster_case()
    P, H, W = len(R), 540, 720
    bank = vsd.MeshBank({4: (verts, faces)}, device=dev)
    depth = vsd.render_depth(bank, [4] * P, vsd.compose_poses(R, t), K0, H, W)
    mask = depth > 0
    box, cnt = bop.op_mask_boxes(mask)
    box = box.cpu().numpy()
    exact = np.stack([np_project_box(verts, R[p], K0, t[p])[:4] for p in range(P)])
    print("rasteriser loop: box edges off by at most %.3f px" % np.abs(box - exact).max())
    assert np.all(np.abs(box - exact) <= 1.0), (box, exact)                       # (i) a condition on the inputs
    assert np.array_equal(cnt.cpu().numpy(), mask.sum(dim=(1, 2)).cpu().numpy())
    out = bop.estimate_translation(bank, [4] * P, R[:, None], K0, mask=mask)
    assert tuple(out["t"].shape) == (P, 1, 3) and int(out["status"].abs().sum()) == 0
    that = out["t"].cpu().numpy()[:, 0]
    same = bop.estimate_translation(bank, torch.tensor([4] * P), torch.from_numpy(R[:, None]), np.repeat(K0[None], P, 0), box=box)
    assert same_bits(same["t"].cpu().numpy()[:, 0], that)
    e = 1.0
    for p in range(P):
        m = min(exact[p, 2] - exact[p, 0], exact[p, 3] - exact[p, 1])
        tz = t[p, 2]
        dz = abs(that[p, 2] - tz)
        assert dz <= 1.5 * 2 * e * tz / m, (p, dz, 1.5 * 2 * e * tz / m)
        for c, f in ((0, K0[0, 0]), (1, K0[1, 1])):
            bound = 1.5 * (e * tz / f + abs(t[p, c]) * 2 * e / m)
            assert abs(that[p, c] - t[p, c]) <= bound, (p, c, abs(that[p, c] - t[p, c]), bound)
    with pytest.raises(ValueError):
        bop.estimate_translation(bank, [4] * P, R[:, None], K0)
    with pytest.raises(ValueError):
        bop.estimate_translation(bank, [4] * P, R[:, None], K0, box=box, mask=mask)


def test_estimate_translation_composes_the_batch(be):
    """(B, k) candidates over two objects against op_fit_translation composed by hand; a NaN box is that query's status, not its neighbour's."""
    from nope_amd import bop, vsd
    hip, dev, _ = be
    bank = vsd.MeshBank({1: vsd.box(70.0, 50.0, 42.0), 2: ellipsoid(2)}, device=dev)
    rng = np.random.default_rng(5)
    B, k = 3, 5
    ids = [2, 1, 2]
    R = np.stack([[haar(rng) for _ in range(k)] for _ in range(B)])
    verts = bank.verts.cpu().numpy()
    box = np.zeros((B, 4))
    for b in range(B):
        off, cnt = bank.vert_ranges([ids[b]])[0]
        box[b] = np_project_box(verts[off: off + cnt], R[b, 0], K0, planted_t(rng, 3, 6, 0.2))[:4]
    box[1] = np.nan
    out = bop.estimate_translation(bank, ids, R, K0, box=box)
    assert tuple(out["t"].shape) == (B, k, 3) and tuple(out["residual"].shape) == (B, k) and out["status"].dtype == torch.int32
    assert out["status"].cpu().tolist() == [[0] * k, [NONFINITE] * k, [0] * k] and bool(torch.isnan(out["t"][1]).all())
    for b in (0, 2):
        off, cnt = bank.vert_ranges([ids[b]])[0]
        for j in range(k):
            w = np_fit(verts[off: off + cnt], R[b, j], K0, box[b])
            assert same_bits(out["t"][b, j].cpu().numpy(), w[0]) and int(out["iters"][b, j]) == w[2]
    assert float(out["residual"][0, 0]) < 1e-4 and float(out["residual"][0, 1:].min()) > float(out["residual"][0, 0])
    with pytest.raises(hip.NopeError):
        bop.estimate_translation(bank, ids[:2], R, K0, box=box)
    with pytest.raises(KeyError):
        bop.estimate_translation(bank, [1, 2, 9], R, K0, box=box)
    assert tuple(bop.estimate_translation(bank, [], R[:0], K0, box=box[:0])["t"].shape) == (0, k, 3)


# ---- E. the depth stage ----------------------------------------------------------------------------------------------------------------
def np_depth_round(bank, ids, R, t, K, dtest, tau, H, W):
    """One round of the restatement: vsd.render_depth at (R, t), numpy's inlier mean, t (t_z + shift) / t_z.  (new t, D = the bound on the
    two shifts' difference, count)."""
    from nope_amd import vsd
    B, k = t.shape[:2]
    rep = [o for o in ids for _ in range(k)]
    d = vsd.render_depth(bank, rep, vsd.compose_poses(R, t).reshape(B * k, 4, 4), np.repeat(K[None], B * k, 0), H, W).cpu().numpy().reshape(B, k, H, W)
    shift, cnt, mag = np_depth_shift(dtest, d, tau)
    tz = t[..., 2]
    return t * ((tz + shift) / tz)[..., None], 2.0 ** -52 * mag, cnt


def test_depth_stage(be):
    """The test depth is rendered at the planted t, the start is 1.05 t: three rounds bring t at least ten times closer (asserted of the
    restatement first), and every round of the library agrees with the restatement's round from the same t within the summation bound."""
    from nope_amd import bop, vsd
    _, dev, _ = be
    verts, faces, R, t = raster_case()
    R, t = R[:2, None], t[:2, None]                         # (B, k) = (2, 1)
    B, H, W = 2, 540, 720
    bank = vsd.MeshBank({4: (verts, faces)}, device=dev)
    ids = [4] * B
    dtest = vsd.render_depth(bank, ids, vsd.compose_poses(R[:, 0], t[:, 0]), K0, H, W).cpu().numpy()
    tau = 0.5 * DIAM
    start = 1.05 * t
    cur = start
    for _ in range(3):
        cur, _, cnt = np_depth_round(bank, ids, R, cur, K0, dtest, tau, H, W)
        assert cnt.min() > 1000
    e0, e3 = np.abs(start - t).max(axis=-1), np.abs(cur - t).max(axis=-1)
    print("depth stage: |t - planted| from", e0.ravel(), "to", e3.ravel())
    assert np.all(e3 <= e0 / 10), (e0, e3)
    lib = start
    status = 0
    for _ in range(3):
        out = bop.refine_translation_depth(bank, ids, R, lib, K0, dtest, tau, rounds=1)
        want, D, _ = np_depth_round(bank, ids, R, lib, K0, dtest, tau, H, W)
        new = out["t"].cpu().numpy()
        bound = np.abs(lib) * (D / lib[..., 2])[..., None] + 8 * 2.0 ** -53 * np.abs(want)
        assert np.all(np.abs(new - want) <= bound), (np.abs(new - want), bound)
        status |= int(out["status"].abs().sum())
        first = new if lib is start else first
        lib = new
    assert status == 0 and np.all(np.abs(lib - t).max(axis=-1) <= e0 / 10)
    all3 = bop.refine_translation_depth(bank, torch.tensor(ids), torch.from_numpy(R), torch.from_numpy(start), K0, torch.from_numpy(dtest), tau, rounds=3)
    assert same_bits(all3["t"].cpu().numpy(), lib) and tuple(all3["shift"].shape) == (B, 1) and all3["count"].dtype == torch.int32
    # the move is along the viewing ray: t / t_z is kept
    assert np.abs(lib[..., :2] / lib[..., 2:] - start[..., :2] / start[..., 2:]).max() <= 1e-14
    # min_count above the overlap: t is kept, the bit says why; a mask that leaves nothing: the same
    few = bop.refine_translation_depth(bank, ids, R, start, K0, dtest, tau, rounds=1, min_count=H * W)
    assert same_bits(few["t"].cpu().numpy(), start) and few["status"].cpu().tolist() == [[bop.ST_DEPTH_FEW]] * B
    none = bop.refine_translation_depth(bank, ids, R, start, K0, dtest, tau, mask=np.zeros((B, H, W), np.uint8), rounds=1)
    assert same_bits(none["t"].cpu().numpy(), start) and none["status"].cpu().tolist() == [[bop.ST_DEPTH_FEW]] * B and int(none["count"].sum()) == 0
    # a t that cannot be rendered is kept and flagged, its neighbour is refined as before
    bad = start.copy()
    bad[1, 0, 2] = np.nan
    o = bop.refine_translation_depth(bank, ids, R, bad, K0, dtest, tau, rounds=1)
    assert o["status"].cpu().tolist() == [[0], [bop.ST_DEPTH_POSE]] and same_bits(o["t"][0].cpu().numpy(), first[0])
    assert same_bits(o["t"][1].cpu().numpy(), bad[1])
    behind = start.copy()
    behind[0, 0, 2] = 10.0                                   # half the ellipsoid behind the camera
    o = bop.refine_translation_depth(bank, ids, R, behind, K0, dtest, tau, rounds=1)
    assert o["status"].cpu().tolist() == [[bop.ST_DEPTH_POSE], [0]] and same_bits(o["t"][0].cpu().numpy(), behind[0])


# ---- F. vsd_error(pred_t), eval_bop ----------------------------------------------------------------------------------------------------
def test_vsd_error_pred_t(be):
    from nope_amd import vsd
    hip, dev, _ = be
    bank = vsd.MeshBank({1: vsd.box(70.0, 50.0, 42.0), 2: ellipsoid(2)}, device=dev)
    rng = np.random.default_rng(9)
    B, k, H, W = 2, 3, 60, 80
    K = np.array([[250.0, 0, W / 2 - 0.3], [0, 252.0, H / 2 + 0.2], [0, 0, 1]])
    ids = [1, 2]
    gtR = np.stack([haar(rng) for _ in range(B)])
    gt_t = np.array([[3.0, -2.0, 450.0], [-4.0, 1.0, 430.0]])
    predR = np.stack([[haar(rng) for _ in range(k)] for _ in range(B)])
    predR[:, 0] = gtR
    dtest = vsd.render_depth(bank, ids, vsd.compose_poses(gtR, gt_t), K, H, W).cpu().numpy()
    dtest[dtest == 0] = 700.0
    base = vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K).cpu().numpy()
    same = vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K, pred_t=np.repeat(gt_t[:, None], k, 1)).cpu().numpy()
    assert same_bits(same, base) and np.all(base[:, 0] == 0.0)
    also = vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K, pred_t=torch.from_numpy(np.repeat(gt_t[:, None], k, 1)), use_gt_translation=False)
    assert same_bits(also.cpu().numpy(), base)
    shifted = vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K, pred_t=np.repeat(gt_t[:, None], k, 1) + np.array([0.0, 0.0, 30.0])).cpu().numpy()
    assert np.all(shifted[:, 0] > 0.5), shifted                                  # 30 mm beyond tau = 20: the true rotation no longer matches
    with pytest.raises(NotImplementedError):
        vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K, use_gt_translation=False)
    with pytest.raises(hip.NopeError):
        vsd.vsd_error(dtest, bank, ids, predR, gtR, gt_t, K, pred_t=gt_t)


@pytest.mark.gpu
def test_eval_bop_translation_modes(gpu, tmp_path):
    from nope_amd import bop, vsd
    from nope_amd.harness import build_model
    from tests.test_vsd import _tless_batch
    cad = tmp_path / "models"
    cad.mkdir()
    meshes = {oid: (vsd.icosphere(2, 40.0) if oid % 2 == 0 else vsd.box(70.0, 50.0, 40.0 + oid)) for oid in range(1, 31)}
    for oid, (v, f) in meshes.items():
        vsd.save_ply(str(cad / f"obj_{oid:06d}.ply"), v, f, binary=oid % 2 == 0)
    m = build_model(device="cuda", save_dir=str(tmp_path / "run"))
    m.load_mesh(str(cad))
    B, H, W = 2, 60, 80
    batch = _tless_batch(B, H, W, m.tless_cad)
    ids = batch["obj_id"].tolist()
    Kn, Rn, tn = batch["intrinsic"].cpu().numpy(), batch["query_pose"].cpu().numpy(), batch["query_translation"].cpu().numpy().reshape(B, 3)
    batch["box"] = torch.from_numpy(np.stack([np_project_box(meshes[ids[b]][0], Rn[b], Kn[b], tn[b])[:4] for b in range(B)]))
    plain = m.eval_bop(batch, "tless", save_path=str(tmp_path / "plain.npz"))
    gt = m.eval_bop(batch, "tless", save_path=str(tmp_path / "gt.npz"), translation="gt")
    assert gt == plain
    a, b = np.load(str(tmp_path / "plain.npz")), np.load(str(tmp_path / "gt.npz"))
    assert sorted(a.files) == sorted(b.files) and all(same_bits(a[n], b[n]) for n in a.files)
    recalls = [key for key in plain if key != "loss/val_tless"]
    for mode, kw in (("box", {}), ("box+depth", {"depth_tau": 20.0})):
        out = m.eval_bop(batch, "tless", save_path=str(tmp_path / "m.npz"), translation=mode, **kw)
        assert set(out) == set(plain) and all(math.isfinite(out[key]) and 0.0 <= out[key] <= 1.0 for key in recalls), (mode, out)
        saved = np.load(str(tmp_path / "m.npz"))
        k = saved["mssd"].shape[1]
        assert saved["t"].shape == (B, k, 3) and saved["residual"].shape == (B, k) and saved["status"].shape == (B, k)
        ok = saved["status"] == 0
        assert np.all(np.isfinite(saved["t"][ok])) and all(np.all(np.isinf(saved[n][~ok])) and np.all(np.isfinite(saved[n][ok])) for n in bop.METRICS)
        assert np.all(np.isinf(saved["vsd"][:, ~ok]))
    # a query without a usable detection is a miss, never a NaN in a recall
    nan_box = dict(batch, box=batch["box"].clone())
    nan_box["box"][1] = float("nan")
    out = m.eval_bop(nan_box, "tless", save_path=str(tmp_path / "n.npz"), translation="box")
    saved = np.load(str(tmp_path / "n.npz"))
    assert np.all(saved["status"][1] == NONFINITE) and all(np.all(np.isinf(saved[n][1])) for n in bop.METRICS) and np.all(np.isinf(saved["vsd"][:, 1]))
    assert all(math.isfinite(out[key]) and out[key] <= 0.5 for key in recalls)
    # the mask in place of the box
    no_box = {key: v for key, v in batch.items() if key != "box"}
    gt_depth = vsd.render_depth(m.tless_cad, ids, vsd.compose_poses(batch["query_pose"], batch["query_translation"]), batch["intrinsic"], H, W)
    out = m.eval_bop(dict(no_box, mask=gt_depth > 0), "tless", translation="box+depth", depth_tau=20.0)
    assert set(out) == set(plain) and all(math.isfinite(out[key]) for key in recalls)
    with pytest.raises(ValueError):
        m.eval_bop(no_box, "tless", translation="box")
    with pytest.raises(ValueError):
        m.eval_bop(batch, "tless", translation="box+depth")
    with pytest.raises(ValueError):
        m.eval_bop(batch, "tless", translation="depth")
    assert m.eval_bop(batch, "tless") == plain
