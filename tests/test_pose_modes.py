"""Pose distribution and distinct pose modes (csrc/kernels_modes.hip, hip.op_pose_modes, PoseConditional.pose_distribution / predict_pose(distinct_deg),
harness.eval_geodesic(distinct_deg)).  DESIGN.md section 4.10.

Every test runs on the interpreter build ("emu") and, marked `gpu`, on the device.  The reference is `ref_modes` below: an f64 NumPy restatement of the
definition (softmax, entropy, the greedy loop over a per-seed distance row).

Radii.  A membership decision is `d <= radius`; the device and NumPy may round d differently, so every radius used against the reference sits in
a gap of the grid's pairwise-distance spectrum, and the test ASSERTS that with the NumPy distance: over all pairs of distinct templates
|d - radius| >= 1e-6 rad (the two computations of d agree to ~1e-8: acos near 0 and pi is the worst).  Under that precondition idx, count and n_modes must
equal the reference exactly.  Radius 180 degrees needs no gap: acos never exceeds pi = radians(180), whatever the rounding.

Bounds of the f32 outputs, from the arithmetic: the f64 sums carry at most N 2^-53 relative error and the device exp / log a few f64 ulp; both vanish
under the one rounding to f32.  prob, mass: 2^-22 |want| + 1e-37 (twice the rounding; the absolute term covers f32 denormals);
entropy: 2^-22 max(1, |want|); score: the input's bits.
"""
import functools
import math

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
REL = 2.0 ** -22
# name: (level, distribution, radius for symmetry 0 / 1, radius for symmetry 2) -- degrees, each in the widest gap of that spectrum
GRIDS = {"l0": (0, "upper", 40.4161, 29.1413), "l1": (1, "all", 24.6384, 23.6949), "l2": (2, "all", 12.5665, 9.9843), "l3": (3, "upper", 6.2965, 8.9311)}
FIELDS = ("prob", "entropy", "idx", "score", "mass", "count", "n_modes")


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


# ---- the reference (f64 NumPy) -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(name):
    from nope_amd import poses
    level, dist = GRIDS[name][:2]
    P = np.ascontiguousarray(poses.get_obj_poses_from_template_level(level, dist)[:, :3, :3], dtype=np.float64)
    P.setflags(write=False)
    return P


def _theta(A, B):
    return np.arccos(np.clip((np.einsum("aij,bij->ab", A, B) - 1.0) / 2.0, -1.0, 1.0))


def distances(A, B, sym):
    """(m, n) distances in radians between the poses A (m, 3, 3) and B (n, 3, 3) under a symmetry class: the op's definition."""
    if sym == 0:
        return _theta(A, B)
    if sym == 1:
        return np.minimum(_theta(A, B), _theta(np.diag([-1.0, 1.0, -1.0]) @ A, B))
    a, b = -np.linalg.inv(A)[:, 2, :], -np.linalg.inv(B)[:, 2, :]
    na, nb = np.maximum(np.linalg.norm(a, axis=1), 1e-8), np.maximum(np.linalg.norm(b, axis=1), 1e-8)
    return np.arccos(np.clip((a @ b.T) / (na[:, None] * nb[None, :]), -1.0, 1.0))


@functools.lru_cache(maxsize=None)
def dmat(name, sym):
    """(N, N) distances between the templates of a grid."""
    D = distances(grid(name), grid(name), sym)
    D.setflags(write=False)
    return D


class SeedRows:
    """D[seed] computed on demand, for a grid too large for its (N, N) matrix; keeps how close any distance it handed out came to `radius_rad`."""

    def __init__(self, P, sym, radius_rad):
        self.P, self.sym, self.radius, self.margin = P, sym, radius_rad, np.inf

    def __getitem__(self, seed):
        row = distances(self.P[seed:seed + 1], self.P, self.sym)[0]
        self.margin = min(self.margin, np.abs(np.delete(row, seed) - self.radius).min())
        return row


def assert_radius_in_gap(name, sym, radius_deg):
    D = dmat(name, sym)
    off = ~np.eye(D.shape[0], dtype=bool)
    margin = np.abs(D[off] - math.radians(radius_deg)).min()
    assert margin >= 1e-6, (name, sym, radius_deg, margin)


def topk_order(s):
    """nope_topk's order of a row without NaN: descending score, ties -> lowest index."""
    return np.lexsort((np.arange(len(s)), -s.astype(np.float64)))


def ref_modes(s, D, temperature, radius_rad, max_modes, fill):
    """One row.  s (N,) f32, D (N, N) f64 -> dict of the op's outputs, prob / entropy / mass in f64."""
    N = len(s)
    s64 = s.astype(np.float64)
    mx = s64.max() if not np.isnan(s64).any() else np.nan
    if not np.isfinite(mx):
        return dict(prob=np.full(N, np.nan), entropy=np.nan, idx=np.full(max_modes, -1), score=np.full(max_modes, np.nan, dtype=np.float32),
                    mass=np.zeros(max_modes), count=np.zeros(max_modes, dtype=int), n_modes=0)
    with np.errstate(under="ignore"):
        e = np.exp((s64 - mx) / temperature)
    p = e / e.sum()
    pos = p > 0
    out = dict(prob=p, entropy=-(p[pos] * np.log(p[pos])).sum(), idx=np.full(max_modes, -1), score=np.full(max_modes, -np.inf, dtype=np.float32),
               mass=np.zeros(max_modes), count=np.zeros(max_modes, dtype=int), n_modes=0)
    alive = np.ones(N, dtype=bool)
    for m in range(max_modes):
        if not alive.any():
            break
        cand = np.flatnonzero(alive)
        seed = cand[np.argmax(s64[cand])]                   # (argmax: the first maximum = the lowest index)
        members = alive & (D[seed] <= radius_rad)
        members[seed] = True
        out["idx"][m], out["score"][m], out["mass"][m], out["count"][m] = seed, s[seed], p[members].sum(), members.sum()
        alive &= ~members
        out["n_modes"] = m + 1
    if fill:
        listed = set(out["idx"][:out["n_modes"]].tolist())
        rest = [n for n in topk_order(s) if n not in listed]
        for m in range(out["n_modes"], max_modes):
            out["idx"][m] = rest[m - out["n_modes"]]
            out["score"][m] = s[out["idx"][m]]
    return out


def close(got, want, floor):
    """|got - want| <= 2^-22 max(|want|, floor) + 1e-37, a NaN where a NaN is wanted."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= REL * np.maximum(np.abs(want[~nan]), floor) + 1e-37))


def to_numpy(got):
    return {f: (None if getattr(got, f) is None else getattr(got, f).cpu().numpy()) for f in FIELDS}


def assert_rows(got, wants, tag=""):
    g = to_numpy(got)
    assert g["idx"].dtype == np.int64 and g["count"].dtype == np.int32 and g["n_modes"].dtype == np.int32 and g["entropy"].dtype == np.float32
    for b, w in enumerate(wants):
        where = (tag, b)
        assert g["n_modes"][b] == w["n_modes"], where
        assert np.array_equal(g["idx"][b], w["idx"]), (where, g["idx"][b], w["idx"])
        assert np.array_equal(g["count"][b], w["count"]), (where, g["count"][b], w["count"])
        assert np.array_equal(g["score"][b], w["score"], equal_nan=True), where                 # the input's bits
        assert close(g["mass"][b], w["mass"], 0.0), (where, g["mass"][b], w["mass"])
        assert close(g["entropy"][b], w["entropy"], 1.0), (where, g["entropy"][b], w["entropy"])
        if g["prob"] is not None:
            assert close(g["prob"][b], w["prob"], 0.0), where


def scores(B, N, seed):
    """Random scores at the real scale (profiles/r15b_bench.json: top1_margin 256 around -2000)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, generator=g) * 300.0 - 2000.0).float()


def run(hip, dev, s, name, sym, shared=True, **kw):
    P = torch.from_numpy(grid(name).copy())
    P = P[None] if shared else P[None].repeat(s.shape[0], 1, 1, 1)
    return hip.op_pose_modes(s.to(dev), P.to(dev), None if sym is None else torch.tensor(sym), **kw)


def equal_bits(a, b):
    """Two PoseModes, or two rows of them: every field bit for bit."""
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. sweep -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_sample"])
@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("B", [1, 3])
def test_sweep(be, B, name, shared):
    hip, dev, _ = be
    N = grid(name).shape[0]
    sym = [0, 1, 2] if B == 3 else [GRIDS[name][0] % 3]           # (B = 1: one class per grid, all three over the four grids)
    s = scores(B, N, 10 * N + B)
    for col, radius in enumerate(GRIDS[name][2:]):
        for c in set(sym):
            assert_radius_in_gap(name, c, radius)
        for temperature in (1.0, 100.0, 1e-3):
            for max_modes, fill in ((0, False), (1, False), (5, False), (5, True), (64, False)):
                if col == 1 and (temperature, max_modes) not in ((1.0, 5), (100.0, 64)):      # the second radius: the mode loop only
                    continue
                got = run(hip, dev, s, name, sym, shared, temperature=temperature, radius_deg=radius, max_modes=max_modes, fill=fill)
                want = [ref_modes(s[b].numpy(), dmat(name, sym[b]), temperature, math.radians(radius), max_modes, fill) for b in range(B)]
                assert tuple(got.idx.shape) == (B, max_modes) and tuple(got.prob.shape) == (B, N)
                assert_rows(got, want, (name, radius, temperature, max_modes, fill))
                ent = got.entropy.cpu().numpy()
                assert np.isfinite(ent).all()                         # (1e-3 underflows every p but one to exactly 0: 0 ln 0 = 0)
                if temperature == 1e-3:
                    assert int((got.prob > 0).sum()) == B and bool((ent == 0).all())


def test_want_prob_false_and_dtypes(be):
    hip, dev, _ = be
    s = scores(2, 26, 3)
    a = run(hip, dev, s, "l0", [0, 2], temperature=50.0, radius_deg=40.4161, max_modes=5)
    P32 = torch.from_numpy(grid("l0").copy()).float()[None]          # any float dtype: converted to f64 (the grid survives f32 within 1e-7)
    b = hip.op_pose_modes(s.double().to(dev), P32, torch.tensor([[0], [2]]), temperature=50.0, radius_deg=40.4161, max_modes=5, want_prob=False)
    assert b.prob is None and b.idx.device == a.idx.device
    for f in ("entropy", "idx", "score", "count", "n_modes"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert close(b.mass.cpu().numpy(), a.mass.cpu().numpy().astype(np.float64), 0.0)


# ---- 2. the planted two-peak score: the reason for the feature ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l1", "l2"])
def test_two_peaks(be, name):
    hip, dev, _ = be
    radius = GRIDS[name][2]
    assert_radius_in_gap(name, 0, radius)
    D = np.degrees(dmat(name, 0))
    a = 17
    b = int(np.argmax(D[a]))
    K = 105.0 / D[a][D[a] > radius].min()
    s = torch.from_numpy(-np.minimum(K * D[a], 100.0 + D[b])).float()[None].repeat(2, 1).contiguous()
    _, top = hip.topk(s.to(dev), 5)
    top = top.cpu().numpy()
    assert (D[a][top] <= radius).all() and not (top == b).any()          # the plain top-5: one basin five times
    assert int(np.flatnonzero(topk_order(s[0].numpy()) == b)[0]) == 7     # (b has rank 7)
    got = run(hip, dev, s, name, None, temperature=10.0, radius_deg=radius, max_modes=5)
    idx, count = got.idx.cpu().numpy(), got.count.cpu().numpy()
    assert (idx[:, 0] == a).all() and (idx[:, 1] == b).all() and (count[:, 0] == 7).all()
    assert_rows(got, [ref_modes(s[r].numpy(), dmat(name, 0), 10.0, math.radians(radius), 5, False) for r in range(2)], name)


# ---- 3. cross-checks against existing ops ---------------------------------------------------------------------------------------------------
def _tied_scores(B, N, seed):
    s = scores(B, N, seed)
    s[:, 40] = s[:, 3] = s[:, 90] = s.max() + 1.0             # three exactly equal maxima
    s[0, 7] = s[0, 100]                                       # and a tie further down the row
    s[0, 11] = float("-inf")                                  # an ordinary score: p = 0, ranks last
    return s


def test_radius_zero_is_topk(be):
    hip, dev, _ = be
    B, N = 3, grid("l1").shape[0]
    assert dmat("l1", 0)[~np.eye(N, dtype=bool)].min() >= 1e-6          # the precondition at radius 0: no two templates coincide
    s = _tied_scores(B, N, 31)
    got = run(hip, dev, s, "l1", None, temperature=100.0, radius_deg=0.0, max_modes=16)
    vals, idx = hip.topk(s.to(dev), 16)
    assert torch.equal(got.idx, idx) and torch.equal(got.score, vals)
    assert idx[:, :3].cpu().tolist() == [[3, 40, 90]] * B
    assert bool((got.count == 1).all()) and bool((got.n_modes == 16).all())
    assert close(got.mass.cpu().numpy(), torch.gather(got.prob, 1, got.idx).cpu().numpy(), 0.0)
    assert float(got.prob[0, 11]) == 0.0
    assert_rows(got, [ref_modes(s[b].numpy(), dmat("l1", 0), 100.0, 0.0, 16, False) for b in range(B)])


@pytest.mark.parametrize("fill", [False, True])
def test_radius_180_is_one_mode(be, fill):
    hip, dev, _ = be
    B, N = 3, grid("l1").shape[0]
    s = _tied_scores(B, N, 32)
    got = run(hip, dev, s, "l1", [0, 1, 2], temperature=100.0, radius_deg=180.0, max_modes=16, fill=fill)
    vals, idx = hip.topk(s.to(dev), 16)
    assert bool((got.n_modes == 1).all()) and bool((got.count[:, 0] == N).all()) and torch.equal(got.idx[:, 0], idx[:, 0])
    assert bool(((got.mass[:, 0].double() - 1.0).abs() <= REL).all())
    assert bool((got.mass[:, 1:] == 0).all()) and bool((got.count[:, 1:] == 0).all())
    if fill:                    # the rest of nope_topk's order (the seed is its first entry)
        assert torch.equal(got.idx[:, 1:], idx[:, 1:]) and torch.equal(got.score[:, 1:], vals[:, 1:])
    else:
        assert bool((got.idx[:, 1:] == -1).all()) and bool((got.score[:, 1:] == float("-inf")).all())
    assert_rows(got, [ref_modes(s[b].numpy(), dmat("l1", c), 100.0, math.pi, 16, fill) for b, c in enumerate([0, 1, 2])])


def test_fill_takes_every_template(be):
    """fill with max_modes = N: every template is listed exactly once, modes first, then nope_topk's order of the rest."""
    hip, dev, _ = be
    N, radius = 26, GRIDS["l0"][2]
    assert_radius_in_gap("l0", 0, radius)
    s = scores(2, N, 33)
    got = run(hip, dev, s, "l0", None, temperature=1.0, radius_deg=radius, max_modes=N, fill=True)
    assert sorted(got.idx[0].cpu().tolist()) == list(range(N)) and 0 < int(got.n_modes[0]) < N
    assert_rows(got, [ref_modes(s[b].numpy(), dmat("l0", 0), 1.0, math.radians(radius), N, True) for b in range(2)])


def test_second_alive_word(be):
    """N = 8192 + 77: a thread owns more than 32 templates, so its alive flags spill into a second LDS word (the grids above stay inside one).
    Haar-random poses; the (N, N) matrix is not built: the reference asks for the seeds' rows only, and those are the only distances that
    decide anything, so the gap precondition is asserted on them.  Then the two radii that need no gap, against nope_topk."""
    from nope_amd.harness import random_rotations
    hip, dev, _ = be
    B, N, radius = 3, 8192 + 77, 20.0
    P = random_rotations(N, torch.Generator().manual_seed(81))
    s = scores(B, N, 82)
    s[:, N - 1] = s.max() + 1.0                    # the best template lives in the second word
    Pd, sd, sym = P[None].to(dev), s.to(dev), [0, 1, 2]
    got = hip.op_pose_modes(sd, Pd, torch.tensor(sym), temperature=100.0, radius_deg=radius, max_modes=8)
    want = []
    for b in range(B):
        rows = SeedRows(P.numpy(), sym[b], math.radians(radius))
        want.append(ref_modes(s[b].numpy(), rows, 100.0, math.radians(radius), 8, False))
        assert rows.margin >= 1e-6, (b, rows.margin)
    assert_rows(got, want)
    assert bool((got.count[:, 0] > 1).all()) and bool((got.idx[:, 0] == N - 1).all())
    vals, idx = hip.topk(sd, 16)
    zero = hip.op_pose_modes(sd, Pd, temperature=100.0, radius_deg=0.0, max_modes=16, want_prob=False)
    for b in range(B):                             # the precondition at radius 0: no template coincides with a seed
        top = idx[b].cpu().numpy()
        rows = distances(P.numpy()[top], P.numpy(), 0)
        rows[np.arange(16), top] = np.inf
        assert rows.min() >= 1e-6
    assert torch.equal(zero.idx, idx) and bool((zero.count == 1).all())
    full = hip.op_pose_modes(sd, Pd, torch.tensor(sym), temperature=100.0, radius_deg=180.0, max_modes=16, fill=True, want_prob=False)
    assert bool((full.n_modes == 1).all()) and bool((full.count[:, 0] == N).all()) and torch.equal(full.idx, idx) and torch.equal(full.score, vals)
    assert bool(((full.mass[:, 0].double() - 1.0).abs() <= REL).all())


# ---- 4. ties -------------------------------------------------------------------------------------------------------------------------------
def test_ties(be):
    hip, dev, _ = be
    name, radius = "l1", GRIDS["l1"][2]
    assert_radius_in_gap(name, 0, radius)
    D = dmat(name, 0)
    i = 57
    far = int(np.argmax(D[i]))
    near = int(np.argsort(D[i])[1])
    assert D[i, far] > math.radians(radius) and D[i, near] <= math.radians(radius) and near != i
    s = scores(2, D.shape[0], 41)
    s[0, i] = s[0, far] = -900.0            # equal maxima in different neighbourhoods
    s[1, i] = s[1, near] = -900.0           # equal maxima inside one neighbourhood
    got = run(hip, dev, s, name, None, temperature=30.0, radius_deg=radius, max_modes=5)
    idx, count = got.idx.cpu().numpy(), got.count.cpu().numpy()
    assert idx[0, 0] == min(i, far) and idx[0, 1] == max(i, far)
    assert idx[1, 0] == min(i, near) and count[1, 0] >= 2 and max(i, near) not in idx[1].tolist()
    assert_rows(got, [ref_modes(s[b].numpy(), D, 30.0, math.radians(radius), 5, False) for b in range(2)])


# ---- 5. undefined rows and padding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "inf", "all_minus_inf"])
@pytest.mark.parametrize("fill", [False, True])
def test_undefined_row(be, kind, fill):
    hip, dev, _ = be
    name, radius = "l1", GRIDS["l1"][2]
    N = grid(name).shape[0]
    s = scores(3, N, 51)
    if kind == "nan":
        s[1, 77] = float("nan")
    elif kind == "inf":
        s[1, N - 1] = float("inf")
    else:
        s[1] = float("-inf")
    sym = [2, 0, 1]
    kw = dict(temperature=100.0, radius_deg=radius, max_modes=64 if not fill else 5, fill=fill)
    got = run(hip, dev, s, name, sym, **kw)
    g = to_numpy(got)
    assert g["n_modes"][1] == 0 and (g["idx"][1] == -1).all() and np.isnan(g["entropy"][1]) and np.isnan(g["prob"][1]).all()
    assert np.isnan(g["score"][1]).all() and (g["mass"][1] == 0).all() and (g["count"][1] == 0).all()
    for b in (0, 2):                     # the other rows: their single-row results, bit for bit
        one = to_numpy(run(hip, dev, s[b:b + 1], name, sym[b:b + 1], **kw))
        assert equal_bits((g[f][b] for f in FIELDS), (one[f][0] for f in FIELDS)), b
        assert g["n_modes"][b] > 1
    for c in sym:
        assert_radius_in_gap(name, c, radius)
    assert_rows(got, [ref_modes(s[b].numpy(), dmat(name, sym[b]), 100.0, math.radians(radius), kw["max_modes"], fill) for b in range(3)])


def test_all_rows_undefined(be):
    """A whole bank can be NaN (f16x2's poison behaviour): no fault, every row reported."""
    hip, dev, _ = be
    got = run(hip, dev, torch.full((3, 642), float("nan")), "l2", None, temperature=1.0, radius_deg=12.5665, max_modes=5, fill=True)
    assert bool((got.n_modes == 0).all()) and bool((got.idx == -1).all()) and bool(got.entropy.isnan().all()) and bool(got.prob.isnan().all())


def test_padded_similarity(be):
    hip, dev, _ = be
    name, radius = "l2", GRIDS["l2"][2]
    N = grid(name).shape[0]
    s = scores(3, N, 52)
    big = torch.full((3, N + 7), float("nan"))
    big[:, :N] = s
    P = torch.from_numpy(grid(name).copy())[None].to(dev)
    kw = dict(temperature=100.0, radius_deg=radius, max_modes=5)
    view = big.to(dev)[:, :N]
    assert view.stride() == (N + 7, 1)
    a = hip.op_pose_modes(view, P, torch.tensor([0, 1, 2]), **kw)
    b = hip.op_pose_modes(s.to(dev), P, torch.tensor([0, 1, 2]), **kw)
    assert equal_bits(to_numpy(a).values(), to_numpy(b).values()) and bool((a.n_modes > 1).all())


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------------------------
BAD_ARGS = [dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=0.0), dict(temperature=-1.0),
            dict(radius_deg=float("nan")), dict(radius_deg=-1e-3), dict(max_modes=-1), dict(max_modes=65), dict(max_modes=27, fill=True),
            dict(n=0)]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments(be, bad):
    hip, dev, _ = be
    bad = dict(bad)
    N = bad.pop("n", 26)
    kw = dict(dict(temperature=1.0, radius_deg=40.0, max_modes=5, fill=False), **bad)
    s = scores(2, 26, 61)[:, :N].contiguous().to(dev)
    P = torch.from_numpy(grid("l0")[:N].copy())[None].to(dev)
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):
        hip.op_pose_modes(s, P, **kw)
    # nothing is written: the same call into outputs that hold a sentinel
    cols = max(kw["max_modes"], 1)
    out = hip.PoseModes(torch.full((2, 26), 7.0, device=dev), torch.full((2,), 7.0, device=dev), torch.full((2, cols), 7, dtype=torch.int64, device=dev),
                        torch.full((2, cols), 7.0, device=dev), torch.full((2, cols), 7.0, device=dev),
                        torch.full((2, cols), 7, dtype=torch.int32, device=dev), torch.full((2,), 7, dtype=torch.int32, device=dev))
    status = torch.full((1,), 7, dtype=torch.int32, device=dev)
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):
        hip._pose_modes_call(s, max(N, 1), P, 0, N, None, kw["temperature"], math.radians(kw["radius_deg"]), kw["max_modes"], kw["fill"], out, status)
    assert all(bool((t == 7).all()) for t in out) and int(status) == 7


def test_shape_errors(be):
    hip, dev, _ = be
    s = scores(2, 26, 62).to(dev)
    P = torch.from_numpy(grid("l0").copy()).to(dev)
    for args in ((s, P[None, :25]), (s, P[None].repeat(3, 1, 1, 1)), (s[0], P[None]), (s, P[None], torch.zeros(3))):
        with pytest.raises(hip.NopeError):
            hip.op_pose_modes(*args, temperature=1.0, radius_deg=40.0)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_deterministic(be):
    hip, dev, _ = be
    N = grid("l3").shape[0]
    s = scores(3, N, 71)
    kw = dict(temperature=100.0, radius_deg=GRIDS["l3"][2], max_modes=64)
    a, b = (to_numpy(run(hip, dev, s, "l3", [0, 1, 2], **kw)) for _ in range(2))
    assert equal_bits(a.values(), b.values())


# ---- 8. plumbing ------------------------------------------------------------------------------------------------------------------------------
_PLUMBING = {}


def _model_and_batch(dev, name):
    """The tiny U-Net of tests/test_refine.py around a StubEncoder, and a batch on the 26 templates of level 0 `upper`; built once per backend.
    The interpreter needs ~15 s per U-Net pass whatever its size, and every call of these tests feeds the network the same inputs: on that
    backend the two methods that run it (the loss forward, encode + generate + retrieve) return their first result again, so the CPU suite
    pays for ONE bank of 26 templates and one loss pass.  What is tested is what happens to the scores afterwards.  The device runs everything."""
    if name in _PLUMBING:
        return _PLUMBING[name]
    from nope_amd import harness
    from nope_amd.model import PoseConditional
    from tests.test_refine import _tiny_unet
    B = 3 if name == "gpu" else 1
    model = PoseConditional(_tiny_unet(3), None, {"similarity_metric": "l2"}, None).to(dev)
    batch = harness.synthetic_batch(B, 0, 8, seed=5, device="cpu", pose_level=0)
    g = torch.Generator().manual_seed(5)
    batch["reference"], batch["query"] = torch.randn(B, 8, 8, 8, generator=g), torch.randn(B, 8, 8, 8, generator=g)
    batch["symmetry"] = torch.tensor([[2], [0], [1]][:B], dtype=torch.float32)
    if name == "emu":
        for attr in ("forward", "_encode_generate_retrieve"):
            def once(*a, _fn=getattr(model, attr), _kept=[], **k):
                if not _kept:
                    _kept.append(_fn(*a, **k))
                return _kept[0]
            setattr(model, attr, once)
    _PLUMBING[name] = model, {k: v.to(dev) for k, v in batch.items()}, B
    return _PLUMBING[name]


def test_predict_pose_distinct(be):
    hip, dev, name = be
    model, batch, B = _model_and_batch(dev, name)
    args = (batch["query"], batch["reference"], batch["all_relativeR"], batch["template_poses"])
    pred0, score0 = model.predict_pose(*args)
    pred1, score1 = model.predict_pose(*args, distinct_deg=None)
    assert pred0.cpu().numpy().tobytes() == pred1.cpu().numpy().tobytes() and score0.cpu().numpy().tobytes() == score1.cpu().numpy().tobytes()
    sym = batch["symmetry"]
    pred, score = model.predict_pose(*args, distinct_deg=40.4161, symmetry=sym, temperature=20.0)
    similarity, nearest_idx, _ = model.generate_and_retrieve(*args[:3])
    modes = hip.op_pose_modes(similarity, batch["template_poses"], sym, temperature=20.0, radius_deg=40.4161, max_modes=5, fill=True)
    rows = torch.arange(B, device=modes.idx.device)[:, None]
    assert bool((modes.idx >= 0).all()) and tuple(modes.idx.shape) == tuple(nearest_idx.shape)
    assert torch.equal(pred, batch["template_poses"][rows, modes.idx]) and torch.equal(score, torch.gather(similarity, 1, modes.idx))
    assert torch.equal(score[:, 0], score0[:, 0])                 # the first seed is the top-1
    dist = model.pose_distribution(similarity, batch["template_poses"], sym, temperature=20.0, radius_deg=40.4161)
    assert torch.equal(dist.idx[:, 0], modes.idx[:, 0]) and tuple(dist.prob.shape) == (B, 26)
    assert bool(((dist.prob.double().sum(1) - 1.0).abs() <= 26 * REL).all())


def test_eval_geodesic_distinct(be, tmp_path):
    from nope_amd import harness
    from nope_amd.metrics import GeodesicError
    hip, dev, name = be
    model, batch, B = _model_and_batch(dev, name)
    sim_a, idx_a, res_a = harness.eval_geodesic(model, batch, save_path=str(tmp_path / "a"))
    sim_b, idx_b, res = harness.eval_geodesic(model, batch, save_path=str(tmp_path / "b"), distinct_deg=40.4161, temperature=20.0)
    assert torch.equal(sim_a, sim_b) and torch.equal(idx_a, idx_b)
    assert {k: v for k, v in res.items() if not k.startswith("modes")} == res_a               # the old keys, the old values
    modes = hip.op_pose_modes(sim_b, batch["template_poses"][:1], batch["symmetry"], temperature=20.0, radius_deg=40.4161, max_modes=5, fill=True)
    _, metric = GeodesicError([15, 30]).from_indices(batch["template_poses"][:1], modes.idx, batch["query_pose"], batch["symmetry"])
    assert sorted(k[len("modes/"):] for k in res if k.startswith("modes/")) == sorted(list(metric) + ["entropy", "n_modes"])
    for k, v in metric.items():
        assert res[f"modes/{k}"] == float(v), k
    assert res["modes/entropy"] == float(modes.entropy.mean()) and res["modes/n_modes"] == float(modes.n_modes.float().mean())
    assert res["modes/n_modes"] > 1
    za, zb = np.load(str(tmp_path / "a.npz")), np.load(str(tmp_path / "b.npz"))
    assert sorted(set(zb.files) - set(za.files)) == ["entropy", "mode_idx", "mode_mass"] and all(za[f].tobytes() == zb[f].tobytes() for f in za.files)
    assert np.array_equal(zb["mode_idx"], modes.idx.cpu().numpy()) and np.array_equal(zb["mode_mass"], modes.mass.cpu().numpy())
    if name != "gpu":
        return
    # with refinement as well (device only: four more U-Net passes): both sets of candidates are refined and reported
    _, _, res_r = harness.eval_geodesic(model, batch, refine_iters=1, distinct_deg=40.4161, temperature=20.0)
    assert sorted(k[len("modes_refined/"):] for k in res_r if k.startswith("modes_refined/")) == sorted(metric)
    assert {k: v for k, v in res_r.items() if not k.startswith(("refined/", "modes_refined/"))} == res
