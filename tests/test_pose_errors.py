"""nope_op_pose_errors and nope_op_mesh_diameter (csrc/kernels_poseerr.hip) and their host side (nope_amd/bop.py, MeshBank.vert_ranges,
PoseConditional.eval_bop), each kernel test on the interpreter (tests/hipemu) and on the device.

The yardstick is the f64 NumPy restatement of include/nope_hip.h below: a plain V x V distance matrix for ADI and the diameter, a plain
loop over the symmetries for MSSD and MSPD, every 3-term dot product written out left to right (as the header fixes it), numpy's own
max / min (which keep a NaN) and numpy's own sum.

Bounds (derived in DESIGN.md section 4.15, u = 2^-53, M = max |x_i| + max |t| >= every transformed-point norm):
  exact data  integer coordinates below 2^10, signed-permutation rotations, integer translations: every product, sum and squared
              distance is an integer below 2^53, sqrt and the division are correctly rounded on both sides -- MSSD, MSPD, ADI's
              per-point minima and the diameter are bit-equal; the ADD / ADI means differ in summation order alone: V 2^-52 relative.
  random data MSSD, ADD, ADI: 64 u M + V 2^-52 |value| (the second term for the means);  MSPD: 160 u rho U with rho = M / min Z and
              U the largest of |pixel coordinate|, fx, fy.  Both sides evaluate the same expressions, so the observed difference is far
              below the bound (printed beside it); ADI is the one metric the kernel evaluates in another frame than the restatement.
Shapes are named from the kernel's constants (NOPE_POSE_ERR_POINT_BLOCK, _TILE, _SYM_CHUNK)."""
import functools
import itertools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
ERR_ARG, ERR_WORKSPACE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
METRICS = ("mssd", "mspd", "add", "adi")


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def _consts():
    from nope_amd import bop
    return bop.POINT_BLOCK, bop.TILE, bop.SYM_CHUNK


def test_constants_mirror_the_header():
    from nope_amd import bop
    src = open(os.path.join(ROOT, "include", "nope_hip.h")).read()
    for name, val in (("NOPE_POSE_ERR_POINT_BLOCK", bop.POINT_BLOCK), ("NOPE_POSE_ERR_TILE", bop.TILE), ("NOPE_POSE_ERR_SYM_CHUNK", bop.SYM_CHUNK),
                      ("NOPE_POSE_ERR_NONFINITE", bop.ST_NONFINITE), ("NOPE_POSE_ERR_BEHIND", bop.ST_BEHIND),
                      ("NOPE_POSE_ERR_VERT_RANGE", bop.ST_VERT_RANGE), ("NOPE_POSE_ERR_SYM_RANGE", bop.ST_SYM_RANGE)):
        assert re.search(rf"\b{name} = {val}\b", src), name
    assert bop.POINT_BLOCK != bop.TILE          # (the shape list below would test one size twice)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def xf(T, x):
    """rows 0..2 of T applied to the points x (V, 3): ((T0 x + T1 y) + T2 z) + T3, each operation rounded once."""
    return np.stack([T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1] + T[r, 2] * x[:, 2] + T[r, 3] for r in range(3)], axis=1)


def norm3(d):
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def proj(K, X):
    w = K[2, 0] * X[:, 0] + K[2, 1] * X[:, 1] + K[2, 2] * X[:, 2]
    u = (K[0, 0] * X[:, 0] + K[0, 1] * X[:, 1] + K[0, 2] * X[:, 2]) / w
    v = (K[1, 0] * X[:, 0] + K[1, 1] * X[:, 1] + K[1, 2] * X[:, 2]) / w
    return u, v, w


def np_pose_errors(verts, syms, Te, Tg, K):
    """One pose pair: verts (V, 3) f32, syms (S, 4, 4).  Returns the four errors, ADI's per-point minima and whether a vertex lies at
    (K X)_2 <= 0 (then MSPD is NaN by the edge rule)."""
    with np.errstate(all="ignore"):
        x = verts.astype(np.float64)
        Xe, Xg = xf(Te, x), xf(Tg, x)
        add = norm3(Xe - Xg)
        D = norm3(Xe[:, None, :] - Xg[None, :, :])                     # the plain V x V matrix
        adi = D.min(axis=1)
        ue, ve, we = proj(K, Xe)
        behind = bool(np.any(~(we > 0)))
        m3, m2 = [], []
        for S in syms:
            Xs = xf(Tg, xf(S, x))
            m3.append(norm3(Xe - Xs).max())
            us, vs, ws = proj(K, Xs)
            behind = behind or bool(np.any(~(ws > 0)))
            du, dv = ue - us, ve - vs
            m2.append(np.sqrt(du * du + dv * dv).max())
        return {"mssd": np.min(m3), "mspd": np.nan if behind else np.min(m2), "add": add.sum() / len(x), "adi": adi.sum() / len(x),
                "adi_min": adi, "behind": behind}


def np_diameter(verts):
    x = verts.astype(np.float64)
    return norm3(x[:, None, :] - x[None, :, :]).max()


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def signed_perms():
    """The 24 signed-permutation rotations."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = signs[r]
            if np.linalg.det(R) > 0:
                out.append(R)
    return out


def haar(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def T4(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


class Case:
    """P pose pairs over n_obj objects: the flat arrays the entry takes, and per pose the slices the restatement takes."""

    def __init__(self, Vs, Ss, P, exact, seed):
        rng = np.random.default_rng(seed)
        sp = signed_perms()
        verts, syms = [], []
        self.voff, self.soff, self.Vs, self.Ss = [], [], list(Vs), list(Ss)
        for V, S in zip(Vs, Ss):
            self.voff.append(sum(len(v) for v in verts))
            self.soff.append(sum(len(s) for s in syms))
            if exact:
                verts.append(rng.integers(-1023, 1024, size=(V, 3)).astype(np.float32))
                syms.append(np.stack([np.eye(4)] + [T4(sp[rng.integers(24)], rng.integers(-8, 9, size=3).astype(np.float64)) for _ in range(S - 1)]))
            else:
                verts.append(rng.uniform(-200.0, 200.0, size=(V, 3)).astype(np.float32))
                syms.append(np.stack([np.eye(4)] + [T4(haar(rng), rng.uniform(-5, 5, size=3)) for _ in range(S - 1)]))
        self.verts, self.syms = np.concatenate(verts), np.concatenate(syms)
        self.obj = [p % len(Vs) for p in range(P)]
        self.est, self.gt, self.K = np.zeros((P, 4, 4)), np.zeros((P, 4, 4)), np.zeros((P, 3, 3))
        for p in range(P):
            if exact:
                # depths are powers of two times small integers far beyond the object: Z > 0 everywhere
                tg = np.array([rng.integers(-64, 65), rng.integers(-64, 65), 4096.0])
                te = tg + np.array([rng.integers(-16, 17), rng.integers(-16, 17), rng.integers(-16, 17)])
                self.gt[p], self.est[p] = T4(sp[rng.integers(24)], tg), T4(sp[rng.integers(24)], te)
                self.K[p] = [[512.0, 0, 256.0], [0, 1024.0, 128.0], [0, 0, 1]]
            else:
                tg = np.array([rng.uniform(-100, 100), rng.uniform(-100, 100), rng.uniform(600, 1000)])
                te = tg + rng.uniform(-20, 20, size=3)
                self.gt[p], self.est[p] = T4(haar(rng), tg), T4(haar(rng), te)
                self.K[p] = [[rng.uniform(500, 1100), 0, rng.uniform(300, 340)], [0, rng.uniform(500, 1100), rng.uniform(220, 260)], [0, 0, 1]]
        self.vert_off = [self.voff[o] for o in self.obj]
        self.vert_cnt = [self.Vs[o] for o in self.obj]
        self.sym_off = [self.soff[o] for o in self.obj]
        self.sym_cnt = [self.Ss[o] for o in self.obj]
        self.P = P

    def v(self, p):
        return self.verts[self.vert_off[p]: self.vert_off[p] + self.vert_cnt[p]]

    def s(self, p):
        return self.syms[self.sym_off[p]: self.sym_off[p] + self.sym_cnt[p]]

    @functools.cached_property
    def want(self):
        return [np_pose_errors(self.v(p), self.s(p), self.est[p], self.gt[p], self.K[p]) for p in range(self.P)]

    def run(self, dev, want=METRICS, **over):
        from nope_amd import bop
        a = dict(verts=self.verts, vert_off=self.vert_off, vert_cnt=self.vert_cnt, max_verts=max(self.vert_cnt), syms=self.syms,
                 sym_off=self.sym_off, sym_cnt=self.sym_cnt, max_syms=max(self.sym_cnt), est=self.est, gt=self.gt, K=self.K)
        a.update(over)
        out = bop.op_pose_errors(torch.from_numpy(a["verts"]).to(dev), a["vert_off"], a["vert_cnt"], a["max_verts"],
                                 torch.from_numpy(a["syms"]).to(dev), a["sym_off"], a["sym_cnt"], a["max_syms"], a["est"], a["gt"], a["K"], want)
        return {k: t.cpu().numpy() for k, t in out.items()}

    def scale(self, p):
        """M, rho, U of the bounds for pose p."""
        x = self.v(p).astype(np.float64)
        tmax = max(np.linalg.norm(self.est[p][:3, 3]), np.linalg.norm(self.gt[p][:3, 3])) + max(np.linalg.norm(S[:3, 3]) for S in self.s(p))
        M = np.linalg.norm(x, axis=1).max() + tmax
        zmin, upix = np.inf, max(self.K[p][0, 0], self.K[p][1, 1])
        for T in [self.est[p]] + [self.gt[p] @ S for S in self.s(p)]:
            u, v, w = proj(self.K[p], xf(T, x))
            zmin, upix = min(zmin, w.min()), max(upix, np.abs(u).max(), np.abs(v).max())
        return M, M / zmin, upix


@functools.lru_cache(maxsize=None)
def case(Vs, Ss, P, exact, seed=0):
    return Case(Vs, Ss, P, exact, 1000 * seed + 7 * sum(Vs) + 3 * sum(Ss) + P + (1 if exact else 0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def check_exact(c, got, what):
    assert np.all(got["status"] == 0), (what, got["status"])
    for p in range(c.P):
        w = c.want[p]
        assert same_bits(got["mssd"][p], w["mssd"]), (what, p, "mssd", got["mssd"][p], w["mssd"])
        assert same_bits(got["mspd"][p], w["mspd"]), (what, p, "mspd", got["mspd"][p], w["mspd"])
        V = c.vert_cnt[p]
        for m in ("add", "adi"):
            assert abs(got[m][p] - w[m]) <= V * 2.0 ** -52 * abs(w[m]), (what, p, m, got[m][p], w[m])
        if V == 1:
            assert same_bits(got["adi"][p], w["adi_min"][0]) and same_bits(got["add"][p], w["add"]), (what, p)


def check_random(c, got, what):
    assert np.all(got["status"] == 0), (what, got["status"])
    worst = {m: (0.0, 0.0) for m in METRICS}
    for p in range(c.P):
        w, (M, rho, upix) = c.want[p], c.scale(p)
        V = c.vert_cnt[p]
        for m in METRICS:
            bound = 160 * U * rho * upix if m == "mspd" else 64 * U * M + (V * 2.0 ** -52 * abs(w[m]) if m in ("add", "adi") else 0.0)
            diff = abs(got[m][p] - w[m])
            if diff >= worst[m][0]:
                worst[m] = (diff, bound)
            assert diff <= bound, (what, p, m, got[m][p], w[m], diff, bound)
    print(what, {m: "observed %.3g, bound %.3g" % worst[m] for m in METRICS})


# ---- A. values ------------------------------------------------------------------------------------------------------------------------
def v_shapes():
    blk, tile, _ = _consts()
    return [1, 3, 64, 65, blk - 1, blk, blk + 1, tile - 1, tile, tile + 1, 2 * tile + 1]


@pytest.mark.parametrize("V", [1, 3, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_vertex_counts_exact(be, V):
    """V around the workgroup's point block, the LDS tile, and one above two tiles (a third trip, its tile holding one vertex)."""
    assert V in v_shapes()
    _, dev, name = be
    c = case((V,), (2,), 3 if V > 1100 else 5, True)
    got = c.run(dev)
    check_exact(c, got, ("V", V))
    if name == "gpu" or V <= 65:
        assert all(same_bits(got[m], v) for m, v in c.run(dev).items() if m in METRICS), "run-to-run bits"


def test_shape_list_follows_the_constants():
    assert v_shapes() == [1, 3, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049] and _consts()[2] + 1 == 9


@pytest.mark.parametrize("V", [3, 65, 513, 1025])
def test_vertex_counts_random(be, V):
    _, dev, _ = be
    c = case((V,), (2,), 5, False)
    check_random(c, c.run(dev), ("random V", V))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("S", [1, 2, 7, 9])
def test_symmetry_counts(be, S, exact):
    """S = 9: one above the symmetry chunk (a second workgroup whose chunk holds one symmetry)."""
    _, dev, _ = be
    c = case((65,), (S,), 5, exact)
    (check_exact if exact else check_random)(c, c.run(dev), ("S", S))


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("P", [1, 5, 33])
def test_pose_counts(be, P, exact):
    _, dev, _ = be
    c = case((64, 3), (2, 1), P, exact)
    (check_exact if exact else check_random)(c, c.run(dev), ("P", P))


@pytest.mark.parametrize("exact", [True, False])
def test_mixed_objects(be, exact):
    """Three objects of different V and S in one batch: the ranges differ per pose, max_verts and max_syms exceed most of them."""
    _, dev, _ = be
    blk, tile, chunk = _consts()
    c = case((blk + 1, 3, 65), (1, chunk + 1, 2), 7, exact)
    got = c.run(dev)
    (check_exact if exact else check_random)(c, got, "mixed")
    # larger max_* than any range: more workgroups that find nothing to do, the same bits
    again = c.run(dev, max_verts=tile + 5, max_syms=3 * chunk)
    assert all(same_bits(got[m], again[m]) for m in METRICS) and np.all(again["status"] == 0)


@pytest.mark.parametrize("V", [1, 3, 65, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_diameter_exact(be, V):
    from nope_amd import bop
    _, dev, name = be
    c = case((V, 3, 64), (1, 1, 1), 3, True, seed=1)
    offs, cnts = c.voff, c.Vs
    d = bop.op_mesh_diameter(torch.from_numpy(c.verts).to(dev), offs, cnts, max(cnts)).cpu().numpy()
    want = [np_diameter(c.verts[o: o + n]) for o, n in zip(offs, cnts)]
    assert same_bits(d, want), (V, d, want)
    if V == 1:
        assert d[0] == 0.0
    assert same_bits(d, bop.op_mesh_diameter(torch.from_numpy(c.verts).to(dev), offs, cnts, max(cnts) + 700).cpu().numpy())


def test_diameter_edges(be):
    from nope_amd import bop
    _, dev, _ = be
    c = case((65, 3), (1, 1), 2, True, seed=2)
    v = torch.from_numpy(c.verts).to(dev)
    V = len(c.verts)
    d = bop.op_mesh_diameter(v, [0, 65, 0, -1, V - 2, 0], [65, 3, 0, 3, 3, 66], 65).cpu().numpy()
    assert same_bits(d[:2], [np_diameter(c.verts[:65]), np_diameter(c.verts[65:])])
    assert np.all(np.isnan(d[2:])), d                       # empty, negative offset, past the end, longer than max_verts
    bad = c.verts.copy()
    bad[40, 1] = np.nan                                     # a NaN vertex that is neither the first nor the last operand of a max
    d = bop.op_mesh_diameter(torch.from_numpy(bad).to(dev), [0, 65], [65, 3], 65).cpu().numpy()
    assert np.isnan(d[0]) and same_bits(d[1], np_diameter(c.verts[65:]))


# ---- B. what distinguishes the metrics ----------------------------------------------------------------------------------------------
def test_box_with_a_half_turn_symmetry(be):
    """estimate = ground truth o (180 degrees about z): MSSD, MSPD and ADI are exactly 0 with the symmetry set, ADD is not, and without
    the set MSSD and MSPD are the restatement's positive values."""
    from nope_amd import bop, vsd
    _, dev, _ = be
    verts, _ = vsd.box(6.0, 4.0, 2.0)
    assert np.array_equal(verts, np.round(verts))
    Rz = np.diag([-1.0, -1.0, 1.0])
    sym = np.stack([np.eye(4), T4(Rz, np.zeros(3))])
    gt = T4(signed_perms()[5], np.array([3.0, -2.0, 64.0]))
    est = gt @ sym[1]
    K = np.array([[256.0, 0, 128.0], [0, 256.0, 64.0], [0, 0, 1]])
    v, s = torch.from_numpy(verts).to(dev), torch.from_numpy(sym).to(dev)
    with_sym = {k: t.cpu().numpy() for k, t in bop.op_pose_errors(v, [0], [8], 8, s, [0], [2], 2, est[None], gt[None], K[None]).items()}
    without = {k: t.cpu().numpy() for k, t in bop.op_pose_errors(v, [0], [8], 8, s, [0], [1], 1, est[None], gt[None], K[None]).items()}
    assert with_sym["mssd"][0] == 0.0 and with_sym["mspd"][0] == 0.0 and with_sym["adi"][0] == 0.0 and with_sym["add"][0] > 0.0
    w = np_pose_errors(verts, sym[:1], est, gt, K)
    assert w["mssd"] > 0 and w["mspd"] > 0
    assert same_bits(without["mssd"][0], w["mssd"]) and same_bits(without["mspd"][0], w["mspd"]) and without["adi"][0] == 0.0
    assert same_bits(without["add"][0], with_sym["add"][0]) and abs(without["add"][0] - w["add"]) <= 8 * 2.0 ** -52 * w["add"]


def test_prism_with_a_continuous_symmetry_off_the_origin(be):
    """An n-gon prism about an axis through `offset`, the continuous rule at a coarse step: estimate = ground truth o (two steps about the
    axis) is no error under the generated set (t = offset - R offset), and a clear one without it."""
    from nope_amd import bop
    _, dev, _ = be
    step = math.pi / 6
    n = int(math.ceil(math.pi / step))
    off = np.array([10.0, 5.0, 0.0])
    ring = np.array([[30.0 * math.cos(2 * math.pi * i / n), 30.0 * math.sin(2 * math.pi * i / n)] for i in range(n)])
    verts = np.array([[x + off[0], y + off[1], z] for z in (-20.0, 25.0) for x, y in ring], dtype=np.float32)
    info = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": off.tolist()}]}
    syms = bop.symmetry_transforms(info, max_sym_disc_step=step)
    assert syms.shape == (n, 4, 4) and np.array_equal(syms[0], np.eye(4))
    rng = np.random.default_rng(5)
    gt = T4(haar(rng), np.array([20.0, -30.0, 700.0]))
    est = gt @ syms[2]
    K = np.array([[600.0, 0, 320.0], [0, 610.0, 240.0], [0, 0, 1]])
    v = torch.from_numpy(verts).to(dev)
    got = {k: t.cpu().numpy()[0] for k, t in bop.op_pose_errors(v, [0], [2 * n], 2 * n, torch.from_numpy(syms).to(dev), [0], [n], n, est[None],
                                                                gt[None], K[None]).items()}
    w = np_pose_errors(verts, syms, est, gt, K)
    M = np.linalg.norm(verts.astype(np.float64), axis=1).max() + np.linalg.norm(gt[:3, 3]) + np.linalg.norm(syms[:, :3, 3], axis=1).max()
    # the f32 vertices are not exactly symmetric: the residual is the restatement's, far below a millimetre
    assert abs(got["mssd"] - w["mssd"]) <= 64 * U * M and got["mssd"] < 1e-3 and got["mspd"] < 1e-3, (got, w)
    assert abs(got["mspd"] - w["mspd"]) <= 160 * U * (M / 600.0) * 1000.0
    alone = bop.op_pose_errors(v, [0], [2 * n], 2 * n, torch.from_numpy(syms).to(dev), [0], [1], 1, est[None], gt[None], K[None])
    w1 = np_pose_errors(verts, syms[:1], est, gt, K)
    assert w1["mssd"] > 30.0 and abs(float(alone["mssd"][0]) - w1["mssd"]) <= 64 * U * M
    assert got["add"] > 30.0 and got["adi"] < 1e-3


# ---- C. edge rules --------------------------------------------------------------------------------------------------------------------
def _neighbours_unchanged(base, got, row):
    for m in METRICS:
        keep = [p for p in range(len(base[m])) if p != row]
        assert same_bits(base[m][keep], got[m][keep]), m
    assert np.all(np.delete(got["status"], row) == 0)


@pytest.mark.parametrize("where", ["est", "gt", "K", "est_inf_times_zero", "gt_bottom_row"])
def test_nonfinite_pose(be, where):
    """A NaN or inf in one pose of a batch: that row is NaN in all four outputs, its neighbours keep their bits.  `est_inf_times_zero`:
    an inf rotation entry against vertices of which only the middle ones have x = 0 -- inf * 0 = NaN there and inf elsewhere, so the
    NaN is neither the first nor the last operand of the maxima."""
    from nope_amd import bop
    _, dev, _ = be
    c = case((65, 3), (2, 1), 5, True, seed=3)
    base = c.run(dev)
    est, gt, K, verts = c.est.copy(), c.gt.copy(), c.K.copy(), c.verts.copy()
    row = 2                                       # (object 0: 65 vertices, two symmetries)
    if where == "est":
        est[row, 1, 2] = np.nan
    elif where == "gt":
        gt[row, 0, 3] = -np.inf
    elif where == "K":
        K[row, 1, 1] = np.nan
    elif where == "gt_bottom_row":
        gt[row, 3, 0] = np.nan                    # (no arithmetic reads it: the rule is about the pose, not about what is used)
    else:
        est[row, 0, 0] = np.inf
        verts[20:40, 0] = 0.0
        base = c.run(dev, verts=verts)
    got = c.run(dev, est=est, gt=gt, K=K, verts=verts)
    for m in METRICS:
        assert np.isnan(got[m][row]), (where, m, got[m][row])
    assert got["status"][row] & bop.ST_NONFINITE
    _neighbours_unchanged(base, got, row)


def test_nan_vertex_in_the_middle(be):
    """A NaN vertex coordinate at a middle index of one object: every pose of that object is NaN in all four outputs (numpy's max, min
    and sum say the same), the other object's poses keep their bits."""
    _, dev, _ = be
    c = case((65, 3), (2, 1), 5, True, seed=3)
    base = c.run(dev)
    verts = c.verts.copy()
    verts[33, 2] = np.nan
    got = c.run(dev, verts=verts)
    for p in range(c.P):
        w = np_pose_errors(verts[c.vert_off[p]: c.vert_off[p] + c.vert_cnt[p]], c.s(p), c.est[p], c.gt[p], c.K[p])
        for m in METRICS:
            if c.obj[p] == 0:
                assert np.isnan(w[m]) and np.isnan(got[m][p]), (p, m, got[m][p])
            else:
                assert same_bits(got[m][p], base[m][p]), (p, m)


@pytest.mark.parametrize("which", ["est", "gt"])
def test_vertex_behind_the_camera(be, which):
    from nope_amd import bop
    _, dev, _ = be
    c = case((65, 3), (2, 1), 5, True, seed=4)
    base = c.run(dev)
    est, gt = c.est.copy(), c.gt.copy()
    row = 2
    (est if which == "est" else gt)[row, 2, 3] = 512.0           # coordinates reach 1023: some vertices at Z < 0, some at Z > 0
    got = c.run(dev, est=est, gt=gt)
    w = np_pose_errors(c.v(row), c.s(row), est[row], gt[row], c.K[row])
    assert w["behind"] and np.isnan(got["mspd"][row]) and got["status"][row] == bop.ST_BEHIND
    assert same_bits(got["mssd"][row], w["mssd"])
    for m in ("add", "adi"):
        assert abs(got[m][row] - w[m]) <= 65 * 2.0 ** -52 * w[m]
    _neighbours_unchanged(base, got, row)
    # a vertex exactly at Z = 0
    verts = np.array([[0, 0, 0], [1, 2, 3]], dtype=np.float32)
    T0, T1 = T4(np.eye(3), np.zeros(3)), T4(np.eye(3), np.array([0, 0, 5.0]))
    o = bop.op_pose_errors(torch.from_numpy(verts).to(dev), [0], [2], 2, torch.from_numpy(np.eye(4)[None]).to(dev), [0], [1], 1,
                           (T0 if which == "est" else T1)[None], (T1 if which == "est" else T0)[None], c.K[:1])
    assert np.isnan(float(o["mspd"][0])) and int(o["status"][0]) == bop.ST_BEHIND and float(o["mssd"][0]) == 5.0 and float(o["add"][0]) == 5.0


def test_bad_ranges(be):
    from nope_amd import bop
    _, dev, _ = be
    c = case((65, 3), (2, 1), 6, True, seed=5)
    base = c.run(dev)
    V, S = len(c.verts), len(c.syms)
    vo, vc, so, sc = list(c.vert_off), list(c.vert_cnt), list(c.sym_off), list(c.sym_cnt)
    edits = {0: ("v", 0, 0), 1: ("v", -1, 3), 2: ("v", V - 2, 3), 3: ("s", 0, 0), 4: ("s", S - 1, 2), 5: ("v", 0, 66)}
    for p, (kind, off, cnt) in edits.items():
        if kind == "v":
            vo[p], vc[p] = off, cnt
        else:
            so[p], sc[p] = off, cnt
    got = c.run(dev, vert_off=vo, vert_cnt=vc, sym_off=so, sym_cnt=sc)           # (max_verts stays 65: the count 66 exceeds it)
    for p, (kind, _, _) in edits.items():
        assert got["status"][p] == (bop.ST_VERT_RANGE if kind == "v" else bop.ST_SYM_RANGE), (p, got["status"])
        assert all(np.isnan(got[m][p]) for m in METRICS), p
    # one bad pose among good ones, and a negative symmetry offset
    vo, so = list(c.vert_off), list(c.sym_off)
    vo[3], so[1] = 2 ** 31 - 2, -3
    got = c.run(dev, vert_off=vo, sym_off=so)
    assert got["status"].tolist() == [0, bop.ST_SYM_RANGE, 0, bop.ST_VERT_RANGE, 0, 0]
    for p in (0, 2, 4, 5):
        assert all(same_bits(got[m][p], base[m][p]) for m in METRICS)


def test_null_outputs_in_every_combination(be):
    _, dev, _ = be
    c = case((513, 3), (9, 1), 4, False, seed=6)
    full = c.run(dev)
    for r in range(1, 4):
        for want in itertools.combinations(METRICS, r):
            got = c.run(dev, want=want)
            assert set(got) == set(want) | {"status"}
            assert all(same_bits(got[m], full[m]) for m in want), want
            assert np.all(got["status"] == 0)


def test_run_to_run_bits(be):
    _, dev, _ = be
    c = case((1025, 65), (9, 2), 6, False, seed=7)
    a, b = c.run(dev), c.run(dev)
    assert all(same_bits(a[m], b[m]) for m in METRICS)


def _raw_args(dev, c):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    P = c.P
    return dict(verts=t(c.verts, torch.float32), V=len(c.verts), vert_off=t(np.array(c.vert_off), torch.int32), vert_cnt=t(np.array(c.vert_cnt), torch.int32),
                max_verts=max(c.vert_cnt), syms=t(c.syms, torch.float64), S_total=len(c.syms), sym_off=t(np.array(c.sym_off), torch.int32),
                sym_cnt=t(np.array(c.sym_cnt), torch.int32), max_syms=max(c.sym_cnt), est=t(c.est, torch.float64), gt=t(c.gt, torch.float64),
                K=t(c.K, torch.float64), P=P, mssd=torch.full((P,), -7.0, dtype=torch.float64, device=dev),
                mspd=torch.full((P,), -7.0, dtype=torch.float64, device=dev), add=torch.full((P,), -7.0, dtype=torch.float64, device=dev),
                adi=torch.full((P,), -7.0, dtype=torch.float64, device=dev), status=torch.full((P,), -7, dtype=torch.int32, device=dev))


def _raw_call(hip, a, ws, ws_bytes):
    p = lambda x: None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else x)
    l = hip.lib()
    return l.dll.nope_op_pose_errors(p(a["verts"]), a["V"], p(a["vert_off"]), p(a["vert_cnt"]), a["max_verts"], p(a["syms"]), a["S_total"],
                                     p(a["sym_off"]), p(a["sym_cnt"]), a["max_syms"], p(a["est"]), p(a["gt"]), p(a["K"]), a["P"], p(a["mssd"]),
                                     p(a["mspd"]), p(a["add"]), p(a["adi"]), p(a["status"]), p(ws), ws_bytes, None)


def test_argument_errors_write_nothing(be):
    hip, dev, _ = be
    c = case((65, 3), (2, 1), 3, True, seed=8)
    a = _raw_args(dev, c)
    l = hip.lib()
    need = int(l.dll.nope_op_pose_errors_workspace_bytes(c.P, a["max_verts"], a["max_syms"]))
    assert need > 0 and l.dll.nope_op_pose_errors_workspace_bytes(0, 5, 5) == 0 and l.dll.nope_op_pose_errors_workspace_bytes(5, 0, 5) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    outs = ("mssd", "mspd", "add", "adi", "status")

    def untouched():
        if dev != "cpu":
            torch.cuda.synchronize()
        return all(bool((a[o] == -7).all()) for o in outs) and bool((ws == 0x5A).all())

    for key in ("V", "S_total", "P", "max_verts", "max_syms"):
        for bad in (0, -1):
            assert _raw_call(hip, dict(a, **{key: bad}), ws, need) == ERR_ARG, (key, bad)
    assert _raw_call(hip, dict(a, P=65536), ws, need) == ERR_ARG
    for key in ("verts", "vert_off", "vert_cnt", "syms", "sym_off", "sym_cnt", "est", "gt", "K", "status"):
        assert _raw_call(hip, dict(a, **{key: None}), ws, need) == ERR_ARG, key
    assert _raw_call(hip, dict(a, mssd=None, mspd=None, add=None, adi=None), ws, need) == ERR_ARG
    assert _raw_call(hip, a, None, need) == ERR_ARG
    assert _raw_call(hip, a, ws, need - 1) == ERR_WORKSPACE and _raw_call(hip, a, ws, 0) == ERR_WORKSPACE
    assert untouched()
    assert _raw_call(hip, a, ws, need) == 0 and not untouched()
    # nope_op_mesh_diameter
    d = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    off, cnt = a["vert_off"][:2].contiguous(), a["vert_cnt"][:2].contiguous()
    dneed = int(l.dll.nope_op_mesh_diameter_workspace_bytes(2, 65))
    dws = torch.empty(dneed, dtype=torch.uint8, device=dev)
    call = lambda v=a["verts"].data_ptr(), V=a["V"], o=off.data_ptr(), n=cnt.data_ptr(), k=2, mv=65, out=d.data_ptr(), w=dws.data_ptr(), wb=dneed: \
        l.dll.nope_op_mesh_diameter(v, V, o, n, k, mv, out, w, wb, None)
    assert dneed > 0 and l.dll.nope_op_mesh_diameter_workspace_bytes(0, 65) == 0 and l.dll.nope_op_mesh_diameter_workspace_bytes(2, 0) == 0
    assert [call(v=None), call(o=None), call(n=None), call(out=None), call(w=None)] == [ERR_ARG] * 5
    assert [call(V=0), call(k=0), call(mv=0), call(k=65536)] == [ERR_ARG] * 4
    assert call(wb=dneed - 1) == ERR_WORKSPACE
    assert bool((d == -7).all())
    assert call() == 0 and same_bits(d.cpu().numpy(), [np_diameter(c.v(0)), np_diameter(c.v(1))])


# ---- D. host --------------------------------------------------------------------------------------------------------------------------
def np_symmetries(info, step):
    """The restatement of the issue's rule, written independently: R = cos I + sin [a]x + (1 - cos) a a^T."""
    disc = [np.eye(4)] + [np.array(m, dtype=np.float64).reshape(4, 4) for m in info.get("symmetries_discrete", [])]
    cont = []
    for sym in info.get("symmetries_continuous", []):
        a = np.array(sym["axis"], dtype=np.float64)
        a = a / np.linalg.norm(a)
        o = np.array(sym["offset"], dtype=np.float64)
        n = int(np.ceil(np.pi / step))
        for i in range(n):
            th = i * 2 * np.pi / n
            ax = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R = np.cos(th) * np.eye(3) + np.sin(th) * ax + (1 - np.cos(th)) * np.outer(a, a)
            cont.append(T4(R, o - R @ o))
    if not cont:
        return np.stack(disc)
    return np.stack([c @ d for c in cont for d in disc])


def test_symmetry_transforms():
    from nope_amd import bop
    d1 = T4(np.diag([-1.0, -1.0, 1.0]), np.array([0.0, 0.0, 0.0]))
    d2 = T4(np.diag([1.0, -1.0, -1.0]), np.array([0.0, 4.0, 2.0]))
    discrete = {"diameter": 100.0, "symmetries_discrete": [d1.reshape(-1).tolist(), d2.reshape(-1).tolist()]}
    cont = {"symmetries_continuous": [{"axis": [1, 2, -2], "offset": [3.0, -1.0, 7.0]}]}
    both = dict(discrete, **cont)
    for info, step in ((discrete, 0.01), (cont, 0.5), (both, 0.4), (cont, 0.01), ({}, 0.01), (None, 0.01)):
        got = bop.symmetry_transforms(info, max_sym_disc_step=step)
        want = np_symmetries(info or {}, step)
        assert got.shape == want.shape and got.dtype == np.float64
        assert np.array_equal(got[0], np.eye(4)), "the identity is entry 0"
        assert np.abs(got - want).max() <= 64 * U * 10.0, np.abs(got - want).max()
        assert np.array_equal(got[:, 3], np.tile([0.0, 0, 0, 1], (len(got), 1)))
    assert bop.symmetry_transforms(discrete).shape == (3, 4, 4) and np.array_equal(bop.symmetry_transforms(discrete)[2], d2)
    assert bop.symmetry_transforms(cont).shape == (315, 4, 4)                       # ceil(pi / 0.01), the default step
    assert bop.symmetry_transforms(both, 0.4).shape == (8 * 3, 4, 4)
    with pytest.raises(ValueError):
        bop.symmetry_transforms({"symmetries_discrete": [[1.0] * 12]})
    # an axis off the origin keeps the points of the axis fixed
    S = bop.symmetry_transforms(cont, 0.5)
    on_axis = np.array([3.0, -1.0, 7.0]) + 2.5 * np.array([1, 2, -2]) / 3.0
    assert np.abs(S[:, :3, :3] @ on_axis + S[:, :3, 3] - on_axis).max() < 1e-13


def test_load_models_info_and_symmetry_bank(tmp_path):
    from nope_amd import bop
    d1 = T4(np.diag([-1.0, -1.0, 1.0]), np.zeros(3))
    info = {"1": {"diameter": 63.5, "min_x": -1.0}, "4": {"diameter": 80.0, "symmetries_discrete": [d1.reshape(-1).tolist()]},
            "27": {"diameter": 120.25, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    (tmp_path / "models_info.json").write_text(json.dumps(info))
    for path in (str(tmp_path), str(tmp_path / "models_info.json")):
        got = bop.load_models_info(path)
        assert sorted(got) == [1, 4, 27] and got[27]["diameter"] == 120.25 and got[4]["symmetries_discrete"] == info["4"]["symmetries_discrete"]
    bank = bop.SymmetryBank.from_models_info(got, device="cpu", max_sym_disc_step=0.5)
    assert bank.syms.dtype == torch.float64 and tuple(bank.syms.shape) == (1 + 1 + 2 + 7, 4, 4)
    assert bank.ranges([1, 4, 27, 9, 4]) == [(1, 1), (2, 2), (4, 7), (0, 1), (2, 2)]           # 9 is not listed: the identity at entry 0
    s = bank.syms.numpy()
    assert np.array_equal(s[0], np.eye(4)) and np.array_equal(s[2], np.eye(4)) and np.array_equal(s[3], d1) and np.array_equal(s[4], np.eye(4))
    assert bop.SymmetryBank(None, device="cpu").ranges([3]) == [(0, 1)]
    with pytest.raises(ValueError):
        bop.SymmetryBank({1: np.zeros((0, 4, 4))}, device="cpu")


def test_bop_scores_on_hand_made_tables():
    from nope_amd import bop
    diam = np.array([100.0, 200.0, 100.0, 50.0])
    mssd = np.array([[4.0, 60.0, 60.0, 60.0, 60.0],             # top 1 passes every theta (4 < 5)
                     [120.0, 31.0, 120.0, 120.0, 120.0],        # top 1 passes none (120 >= 100); top 3: 31 passes 0.2 ... 0.5 of 200 (7 of 10)
                     [np.nan, np.nan, np.nan, np.nan, 12.0],    # NaN never passes; top 5: 12 passes 0.15 ... (8 of 10)
                     [26.0, 26.0, 26.0, 26.0, 26.0]])           # 26 >= 25: none
    mspd = np.array([[7.0, 1.0, 1.0, 1.0, 1.0], [52.0, 52.0, 52.0, 52.0, 18.0], [33.0, 33.0, 33.0, 33.0, 33.0], [101.0] * 5])
    add = np.array([[9.0, 9, 9, 9, 9], [21.0, 19.0, 21, 21, 21], [10.5, 10.5, 10.5, 10.5, 10.5], [4.0, 4, 4, 4, 4]])
    adi = add / 2
    th = np.array(bop.THRESHOLDS)
    assert len(th) == 10 and abs(th[0] - 0.05) < 1e-15 and abs(th[-1] - 0.5) < 1e-15 and bop.MSPD_THRESHOLDS == tuple(5.0 * i for i in range(1, 11))
    width = 1280
    # no planted error lies within 1e-9 relative of a threshold: the strict `<` cannot hinge on a rounding
    for tab, scale in ((mssd, diam), (add, diam), (adi, diam)):
        for b in range(4):
            for t in th * scale[b]:
                assert np.all(~(np.abs(tab[b] - t) <= 1e-9 * t)), (tab[b], t)
    for t in np.array(bop.MSPD_THRESHOLDS) * 2.0:
        assert np.all(~(np.abs(mspd - t) <= 1e-9 * t))
    s = bop.bop_scores({"mssd": mssd, "mspd": torch.from_numpy(mspd), "add": add, "adi": adi}, diam, width)
    assert s["top 1, AR_MSSD"] == pytest.approx((10 + 0 + 0 + 0) / 40)
    assert s["top 3, AR_MSSD"] == pytest.approx((10 + 7 + 0 + 0) / 40)
    assert s["top 5, AR_MSSD"] == pytest.approx((10 + 7 + 8 + 0) / 40)
    # thresholds 10, 20, ..., 100 px at width 1280: 7 passes all 10; 52 passes 60 ... 100 (5); 33 passes 40 ... (7); 101 none; 18 passes 9; 1 all
    assert s["top 1, AR_MSPD"] == pytest.approx((10 + 5 + 7 + 0) / 40)
    assert s["top 3, AR_MSPD"] == pytest.approx((10 + 5 + 7 + 0) / 40)
    assert s["top 5, AR_MSPD"] == pytest.approx((10 + 9 + 7 + 0) / 40)
    # ADD < 0.1 d: 9 < 10 yes; 21 < 20 no (19 yes from top 3); 10.5 < 10 no; 4 < 5 yes
    assert s["top 1, ADD 0.1d"] == 0.5 and s["top 3, ADD 0.1d"] == 0.75 and s["top 5, ADD 0.1d"] == 0.75
    # ADD-S = ADD / 2: 4.5, 10.5 (9.5), 5.25, 2: all pass
    assert s["top 1, ADD-S 0.1d"] == 1.0
    assert "top 1, AR" not in s and "top 1, AR_VSD" not in s
    # VSD: (10 tau, B, k); query 0 passes every theta at every tau, query 1 at half the taus passes theta >= 0.3 (5 of 10), the rest never
    vs = np.ones((10, 4, 5))
    vs[:, 0, 0] = 0.01
    vs[::2, 1, 2] = 0.27
    s = bop.bop_scores({"mssd": mssd, "mspd": mspd}, diam, width, vsd_errors=vs)
    assert s["top 1, AR_VSD"] == pytest.approx(100 / 400) and s["top 3, AR_VSD"] == pytest.approx((100 + 5 * 5) / 400)
    for k in (1, 3, 5):
        assert s[f"top {k}, AR"] == pytest.approx((s[f"top {k}, AR_VSD"] + s[f"top {k}, AR_MSSD"] + s[f"top {k}, AR_MSPD"]) / 3)
    assert set(bop.bop_scores({"add": add[:, :2]}, diam, width)) == {"top 1, ADD 0.1d", "top 1, AR_ADD"}
    with pytest.raises(ValueError):
        bop.bop_scores({"mssd": mssd, "mspd": mspd[:, :3]}, diam, width)
    with pytest.raises(ValueError):
        bop.bop_scores({"mssd": mssd}, diam[:3], width)


def test_mesh_bank_vert_ranges():
    from nope_amd import vsd
    meshes = {7: vsd.box(2, 3, 4), 2: vsd.icosphere(1, 5.0), 30: vsd.icosphere(0, 1.0)}
    bank = vsd.MeshBank(meshes, device="cpu")
    assert bank.vert_ranges([2, 7, 30, 7]) == [(0, 42), (42, 8), (50, 12), (42, 8)]
    assert bank.vert_off == {2: 0, 7: 42, 30: 50} and bank.vert_cnt == {2: 42, 7: 8, 30: 12}
    for oid, (off, cnt) in zip([2, 7, 30], bank.vert_ranges([2, 7, 30])):
        assert np.array_equal(bank.verts[off: off + cnt].numpy(), meshes[oid][0])
        f0, fc = bank.ranges([oid])[0]
        assert int(bank.faces[f0: f0 + fc].min()) >= off and int(bank.faces[f0: f0 + fc].max()) < off + cnt
    with pytest.raises(KeyError, match="obj_id 5 is not in the mesh bank"):
        bank.vert_ranges([5])


def test_mesh_diameters_closed_forms(be):
    from nope_amd import bop, vsd
    _, dev, _ = be
    bank = vsd.MeshBank({1: vsd.icosphere(2, 40.0), 2: vsd.box(70.0, 50.0, 42.0), 3: vsd.icosphere(3, 7.5), 4: vsd.box(1.0, 2.0, 0.5)}, device=dev)
    d = bop.mesh_diameters(bank)
    assert sorted(d) == [1, 2, 3, 4]
    # the icosphere keeps the icosahedron's antipodal vertex pairs: 2 r, up to the f32 rounding of the stored vertices
    assert abs(d[1] - 80.0) <= 80.0 * 2.0 ** -22 and abs(d[3] - 15.0) <= 15.0 * 2.0 ** -22
    assert d[2] == math.sqrt(70.0 ** 2 + 50.0 ** 2 + 42.0 ** 2) and d[4] == math.sqrt(1.0 + 4.0 + 0.25)      # (halves exact in f32)


def test_pose_errors_composes_the_batch(be):
    """bop.pose_errors (B, k) against op_pose_errors composed by hand and against the restatement; pred_t; shape errors."""
    from nope_amd import bop, vsd
    hip, dev, _ = be
    bank = vsd.MeshBank({1: vsd.box(70.0, 50.0, 42.0), 2: vsd.icosphere(1, 40.0)}, device=dev)
    syms = bop.SymmetryBank({1: bop.symmetry_transforms({"symmetries_discrete": [T4(np.diag([-1.0, -1.0, 1.0]), np.zeros(3)).reshape(-1).tolist()]})},
                            device=dev)
    rng = np.random.default_rng(11)
    B, k = 3, 5
    ids = [1, 2, 1]
    predR = np.stack([[haar(rng) for _ in range(k)] for _ in range(B)])
    gtR = np.stack([haar(rng) for _ in range(B)])
    gt_t = np.stack([[rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(500, 800)] for _ in range(B)])[:, :, None]
    K = np.array([[600.0, 0, 320.0], [0, 610.0, 240.0], [0, 0, 1]])
    out = bop.pose_errors(bank, syms, torch.tensor(ids), predR, gtR, gt_t, K)
    assert set(out) == set(METRICS) | {"status"} and all(tuple(out[m].shape) == (B, k) and out[m].dtype == torch.float64 for m in METRICS)
    assert int(out["status"].abs().sum()) == 0
    verts = bank.verts.cpu().numpy()
    for b in range(B):
        off, cnt = bank.vert_ranges([ids[b]])[0]
        so, sc = syms.ranges([ids[b]])[0]
        assert (so, sc) == ((1, 2) if ids[b] == 1 else (0, 1))
        for j in range(k):
            w = np_pose_errors(verts[off: off + cnt], syms.syms.cpu().numpy()[so: so + sc], T4(predR[b, j], gt_t[b, :, 0]), T4(gtR[b], gt_t[b, :, 0]), K)
            for m in METRICS:
                assert abs(float(out[m][b, j]) - w[m]) <= 1e-9 * max(1.0, abs(w[m])), (b, j, m)
    only = bop.pose_errors(bank, syms, ids, predR, gtR, gt_t[:, :, 0], np.repeat(K[None], B, 0), want=("mssd", "add"))
    assert set(only) == {"mssd", "add", "status"} and same_bits(only["mssd"].cpu().numpy(), out["mssd"].cpu().numpy())
    none = bop.pose_errors(bank, None, ids, predR, gtR, gt_t, K)                     # no symmetries: the box's MSSD can only grow
    assert bool((none["mssd"] >= out["mssd"]).all()) and bool((none["mssd"][0] > out["mssd"][0]).any())
    assert same_bits(none["add"].cpu().numpy(), out["add"].cpu().numpy()) and same_bits(none["adi"].cpu().numpy(), out["adi"].cpu().numpy())
    shifted = bop.pose_errors(bank, syms, ids, predR, gtR, gt_t, K, pred_t=np.repeat(gt_t[:, None, :, 0], k, 1) + np.array([0.0, 0.0, 10.0]))
    assert bool((shifted["add"] != out["add"]).all())
    same_t = bop.pose_errors(bank, syms, ids, predR, gtR, gt_t, K, pred_t=np.repeat(gt_t[:, None, :, 0], k, 1))
    assert all(same_bits(same_t[m].cpu().numpy(), out[m].cpu().numpy()) for m in METRICS)
    with pytest.raises(hip.NopeError):
        bop.pose_errors(bank, syms, ids[:2], predR, gtR, gt_t, K)
    with pytest.raises(hip.NopeError):
        bop.pose_errors(bank, syms, ids, predR[:, 0], gtR, gt_t, K)
    with pytest.raises(KeyError):
        bop.pose_errors(bank, syms, [1, 2, 9], predR, gtR, gt_t, K)
    with pytest.raises(ValueError):
        bop.pose_errors(bank, syms, ids, predR, gtR, gt_t, K, want=("vsd",))
    empty = bop.pose_errors(bank, syms, [], predR[:0], gtR[:0], gt_t[:0], K)
    assert tuple(empty["mssd"].shape) == (0, k)


@pytest.mark.gpu
def test_eval_bop_end_to_end(gpu, tmp_path):
    from nope_amd import bop, vsd
    from nope_amd.harness import build_model
    from tests.test_vsd import REF_KEYS, _tless_batch
    cad = tmp_path / "models"
    cad.mkdir()
    for oid in range(1, 31):
        v, f = vsd.icosphere(2, 40.0) if oid % 2 == 0 else vsd.box(70.0, 50.0, 40.0 + oid)
        vsd.save_ply(str(cad / f"obj_{oid:06d}.ply"), v, f, binary=oid % 2 == 0)
    m = build_model(device="cuda", save_dir=str(tmp_path / "run"))
    m.load_mesh(str(cad))
    B, H, W = 4, 60, 80
    batch = _tless_batch(B, H, W, m.tless_cad)
    before = m.eval_vsd(batch, "tless")
    out = m.eval_bop(batch, "tless", save_path=str(tmp_path / "e.npz"))
    keys = {f"top {k}, {n}" for k in (1, 3, 5) for n in ("AR_MSSD", "AR_MSPD", "AR_VSD", "AR", "ADD 0.1d", "ADD-S 0.1d", "AR_ADD", "AR_ADD-S")}
    assert set(out) == keys | {"loss/val_tless"}
    assert all(0.0 <= out[k] <= 1.0 for k in keys)
    assert out["loss/val_tless"] == float(m.forward(batch["query"], batch["reference"], batch["gt_relativeR"]))
    # the same retrieval composed by hand: the same bits in every table, and the scores of those tables
    feat, _, _ = m.generate_templates(batch["reference"], batch["all_relativeR"])
    _, idx = m.retrieval(batch["query"], feat)
    tp = batch["template_poses"]
    predR = torch.stack([tp[b, idx[b].to(tp.device)] for b in range(B)])
    ids = batch["obj_id"].tolist()
    errs = bop.pose_errors(m.tless_cad, None, ids, predR, batch["query_pose"], batch["query_translation"], batch["intrinsic"])
    saved = np.load(str(tmp_path / "e.npz"))
    for name in METRICS:
        assert same_bits(saved[name], errs[name].cpu().numpy()), name
    diam_all = bop.mesh_diameters(m.tless_cad)
    diam = np.array([diam_all[o] for o in ids])
    assert np.array_equal(saved["diameter"], diam) and diam[0] == math.sqrt(70.0 ** 2 + 50.0 ** 2 + 41.0 ** 2)
    _, d_gt, d_est = vsd.vsd_error(batch["depth"], m.tless_cad, ids, predR, batch["query_pose"], batch["query_translation"], batch["intrinsic"],
                                   return_depth=True)
    stack = np.stack([np.stack([vsd.vsd_from_depth(batch["depth"][b: b + 1], d_gt[b: b + 1], d_est[b: b + 1], batch["intrinsic"][b: b + 1],
                                                   delta=15, tau=frac * diam[b]).cpu().numpy()[0] for b in range(B)]) for frac in bop.THRESHOLDS])
    assert same_bits(saved["vsd"], stack)
    want = bop.bop_scores(errs, diam, W, vsd_errors=stack)
    assert all(out[k] == want[k] for k in keys)
    # models_info: its diameters and symmetry sets are used (a half turn about z is a symmetry of the boxes: MSSD can only fall)
    info = {str(o): {"diameter": 90.0 + o, "symmetries_discrete": [T4(np.diag([-1.0, -1.0, 1.0]), np.zeros(3)).reshape(-1).tolist()]} for o in (1, 2)}
    (cad / "models_info.json").write_text(json.dumps(info))
    assert sorted(m.load_models_info(str(cad))) == [1, 2]
    m.eval_bop(batch, "tless", save_path=str(tmp_path / "e2.npz"))
    saved2 = np.load(str(tmp_path / "e2.npz"))
    assert np.array_equal(saved2["diameter"], [91.0, 92.0, 91.0, 92.0]) and np.all(saved2["mssd"] <= saved["mssd"])
    assert same_bits(saved2["add"], saved["add"])
    # eval_vsd returns what it returned before eval_bop existed: the host composition of test_vsd.py, and the same after the calls above
    err = vsd.vsd_error(batch["depth"], m.tless_cad, ids, predR, batch["query_pose"], batch["query_translation"], batch["intrinsic"])
    assert set(before) == REF_KEYS | {"loss/val_tless"} and all(before[k] == v for k, v in vsd.vsd_scores(err).items())
    assert m.eval_vsd(batch, "tless") == before
