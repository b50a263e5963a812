"""Coarse-to-fine pose retrieval over nested viewpoint grids (csrc/kernels_search.hip, hip.op_c2f_expand / op_c2f_commit, nope_amd/search.py,
PoseConditional.retrieve_coarse_to_fine / predict_pose(coarse_to_fine), harness.eval_geodesic(coarse_to_fine)).  DESIGN.md section 4.11.

Every op-level and driver-level test runs on the interpreter build ("emu") and, marked `gpu`, on the device; the end-to-end tests need the
U-Net and run on the device only.  The reference is `ref_expand` / `ref_search` below: an f64 NumPy restatement of the definition.

Radii.  Membership is `d <= radius`; the device and NumPy may round d differently (they agree to ~1e-8: acos near 0 and pi is the worst), so
every radius used against the reference sits in a gap of that grid's distance spectrum and the test ASSERTS it with the NumPy distance:
|d - radius| >= 1e-6 rad over all pairs of distinct poses with stage_of <= max_stage.  Under that precondition cand, n_cand, n_dropped,
state and status must equal the reference exactly, and rows bit for bit.  Radius pi needs no gap: acos never exceeds pi.
"""
import functools
import math

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
GRIDS = {"l1all": (1, "all"), "l2": (2, "upper"), "l3": (3, "upper")}
ROT_RADIUS_L1_ALL = 24.6384          # degrees: the gap radius tests/test_pose_modes.py uses on level-1 "all" under the rotation distance
VIEW_RADII_DEG = (22.50, 11.36, 5.86)  # what stage_radii gives on the synthesised upper grids under the viewpoint distance (stages 1, 2, 3)
ROT, VIEW = 0, 1


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


# ---- the reference (f64 NumPy) -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(name):
    """(P (N, 3, 3) f64, stage_of (N,) int32), read-only."""
    from nope_amd import poses
    level, dist = GRIDS[name]
    P = np.ascontiguousarray(poses.get_obj_poses_from_template_level(level, dist)[:, :3, :3], dtype=np.float64)
    st = poses.grid_stages(level, dist)
    P.setflags(write=False)
    st.setflags(write=False)
    return P, st


def distances(A, B, kind):
    """(m, n) radians between A (m, 3, 3) and B (n, 3, 3): the op's definition, restated."""
    with np.errstate(invalid="ignore"):
        if kind == ROT:
            return np.arccos(np.clip((np.einsum("aij,bij->ab", A, B) - 1.0) / 2.0, -1.0, 1.0))
        a, b = A[:, 2, :], B[:, 2, :]
        na, nb = np.maximum(np.linalg.norm(a, axis=1), 1e-8), np.maximum(np.linalg.norm(b, axis=1), 1e-8)
        return np.arccos(np.clip((a @ b.T) / (na[:, None] * nb[None, :]), -1.0, 1.0))


def assert_radius_in_gap(P, stage_of, max_stage, kind, radius_rad):
    Q = P[stage_of <= max_stage]
    D = distances(Q, Q, kind)
    off = ~np.eye(len(Q), dtype=bool)
    margin = np.abs(D[off] - radius_rad).min() if off.any() else np.inf
    assert margin >= 1e-6, (len(Q), kind, radius_rad, margin)


def ref_expand(P, stage_of, max_stage, state, seeds, radius_rad, kind, rel, M):
    """One query.  P (N, 3, 3), stage_of (N,), state (N,) uint8, seeds: a list (empty: stage 0), rel (N, 6) f32 -> the op's outputs."""
    N = len(P)
    elig = (stage_of <= max_stage) & (state == 0)
    seq, bits, pad = [], 0, None
    if len(seeds) == 0:
        seq = np.flatnonzero(elig).tolist()
    else:
        taken = np.zeros(N, dtype=bool)
        for sd in seeds:
            if not 0 <= sd < N:
                bits |= 2
                continue
            if pad is None:
                pad = int(sd)
            with np.errstate(invalid="ignore"):
                m = elig & ~taken & (distances(P[sd:sd + 1], P, kind)[0] <= radius_rad)          # (a NaN compares false)
            m[sd] = False
            seq += np.flatnonzero(m).tolist()
            taken |= m
    kept = seq[:M]
    out_state = state.copy()
    out_state[kept] = 1
    cand = np.full(M, -1, dtype=np.int32)
    cand[:len(kept)] = kept
    rows = np.repeat(rel[(pad or 0):(pad or 0) + 1], M, axis=0)
    rows[:len(kept)] = rel[kept]
    if len(seq) > M:
        bits |= 1
    return dict(cand=cand, n_cand=len(kept), n_dropped=len(seq) - len(kept), state=out_state, rows=rows, status=bits)


def rel_rows(B, N, seed):
    """(B, N, 6) f32 with every bit pattern a row may carry: the op copies bits."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(B, N, 6, generator=g)
    r[:, N // 2, 1] = -0.0
    return r.numpy()


def run_expand(hip, dev, P, stage_of, max_stage, state, seeds, radius_rad, kind, rel, M):
    """P (B|1, N, 3, 3), state (B, N) uint8, seeds (B, n) or None, rel (B, N, 6) -> the outputs as NumPy (state: the updated copy)."""
    st = torch.from_numpy(state.copy()).to(dev)
    sd = None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.int64)).to(dev)
    ex = hip.op_c2f_expand(torch.from_numpy(P.copy()).to(dev), torch.from_numpy(np.array(stage_of)), max_stage, st, sd, torch.from_numpy(rel).to(dev),
                           radius_rad=radius_rad, dist_kind=kind, capacity=M)
    assert ex.cand.dtype == torch.int32 and ex.n_cand.dtype == torch.int32 and ex.rows.dtype == torch.float32 and tuple(ex.rows.shape) == (state.shape[0], M, 6)
    return dict(cand=ex.cand.cpu().numpy(), n_cand=ex.n_cand.cpu().numpy(), n_dropped=ex.n_dropped.cpu().numpy(), state=st.cpu().numpy(),
                rows=ex.rows.cpu().numpy(), status=int(ex.status.cpu()))


def check(got, P, stage_of, max_stage, state, seeds, radius_rad, kind, rel, M, tag=""):
    """got against ref_expand, query by query; returns the references."""
    B, status, wants = state.shape[0], 0, []
    for b in range(B):
        w = ref_expand(P[b if P.shape[0] > 1 else 0], stage_of, max_stage, state[b], [] if seeds is None else list(np.asarray(seeds)[b]), radius_rad,
                       kind, rel[b], M)
        where = (tag, b)
        assert np.array_equal(got["cand"][b], w["cand"]), (where, got["cand"][b], w["cand"])
        assert got["n_cand"][b] == w["n_cand"] and got["n_dropped"][b] == w["n_dropped"], (where, got["n_cand"][b], got["n_dropped"][b], w["n_cand"], w["n_dropped"])
        assert np.array_equal(got["state"][b], w["state"]), where
        assert got["rows"][b].tobytes() == w["rows"].tobytes(), where
        status |= w["status"]
        wants.append(w)
    assert got["status"] == status, (tag, got["status"], status)
    return wants


def mixed_state(B, stage_of, s, seed):
    """(B, N) uint8: what a search holds before stage s -- the coarser levels evaluated -- with a different sprinkling of level-s poses per query."""
    rng = np.random.default_rng(seed)
    state = np.repeat((stage_of < s).astype(np.uint8)[None], B, axis=0)
    for b in range(B):
        state[b, rng.choice(np.flatnonzero(stage_of == s), size=3 + 4 * b, replace=False)] = 1
    return state


def evaluated_seeds(state, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(np.flatnonzero(row == 1), size=n, replace=False) for row in state]).astype(np.int64)


# ---- 1. expand ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l2", "l3"])
def test_stage0_enumeration(be, name):
    hip, dev, _ = be
    P, stage_of = grid(name)
    N, B = len(P), 3
    rel = rel_rows(B, N, 1)
    state = np.zeros((B, N), dtype=np.uint8)
    state[1, [0, 5, 25, N - 1]] = 1
    state[2, ::2] = 1
    for max_stage, M in ((0, 26), (1, 91), (GRIDS[name][0], N)):
        got = run_expand(hip, dev, P[None], stage_of, max_stage, state, None, 0.0, VIEW, rel, M)
        wants = check(got, P[None], stage_of, max_stage, state, None, 0.0, VIEW, rel, M, (name, max_stage))
        assert wants[0]["n_cand"] == M and wants[0]["n_dropped"] == 0 and got["status"] == 0
        assert np.array_equal(got["cand"][0], np.flatnonzero(stage_of <= max_stage))
        assert got["rows"][1, M - 1].tobytes() == rel[1, 0].tobytes()                 # a padded slot without seeds: the row of pose 0


@pytest.mark.parametrize("name", ["l2", "l3"])
def test_expand_viewpoint(be, name):
    """Level-2 upper (341) and level-3 upper (1321), the viewpoint distance at the radii of the issue, B = 3 with different state rows and seeds."""
    from nope_amd import poses
    hip, dev, _ = be
    P, stage_of = grid(name)
    N, B = len(P), 3
    rel = rel_rows(B, N, 2)
    radii = np.degrees(poses.stage_radii(P, stage_of, VIEW))
    assert radii[0] == 0.0 and np.allclose(radii[1:], VIEW_RADII_DEG[:len(radii) - 1], atol=5e-3), radii
    for s in range(1, GRIDS[name][0] + 1):
        radius = math.radians(VIEW_RADII_DEG[s - 1])
        assert_radius_in_gap(P, stage_of, s, VIEW, radius)
        state = mixed_state(B, stage_of, s, 10 * s)
        seeds = evaluated_seeds(state, 3, 11 * s)
        got = run_expand(hip, dev, P[None], stage_of, s, state, seeds, radius, VIEW, rel, 18)
        wants = check(got, P[None], stage_of, s, state, seeds, radius, VIEW, rel, 18, (name, s))
        assert all(0 < w["n_cand"] <= 18 for w in wants) and got["status"] == 0           # 4 to 6 neighbours per seed, fewer where they were evaluated


def test_expand_rotation(be):
    hip, dev, _ = be
    P, stage_of = grid("l1all")
    N, B, radius = len(P), 3, math.radians(ROT_RADIUS_L1_ALL)
    assert_radius_in_gap(P, stage_of, 1, ROT, radius)
    rel = rel_rows(B, N, 3)
    state = mixed_state(B, stage_of, 1, 31)
    seeds = evaluated_seeds(state, 4, 32)
    got = run_expand(hip, dev, P[None], stage_of, 1, state, seeds, radius, ROT, rel, 32)
    wants = check(got, P[None], stage_of, 1, state, seeds, radius, ROT, rel, 32, "rot")
    assert all(w["n_cand"] > 0 for w in wants)
    # the two distances are different things: the same call under the viewpoint distance chooses other poses
    other = run_expand(hip, dev, P[None], stage_of, 1, state, seeds, radius, VIEW, rel, 32)
    assert not np.array_equal(other["cand"], got["cand"])


def test_two_neighbouring_seeds(be):
    """Shared candidates are emitted once, under the first seed; the order is seed by seed, ascending within a seed."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, radius = len(P), math.radians(VIEW_RADII_DEG[0])
    assert_radius_in_gap(P, stage_of, 1, VIEW, radius)
    D = distances(P, P, VIEW)
    lvl0 = np.flatnonzero(stage_of == 0)
    a = int(lvl0[3])
    b = int(lvl0[np.argsort(D[a, lvl0])[1]])                       # its nearest level-0 neighbour
    state = (stage_of == 0).astype(np.uint8)[None]
    near = lambda i: set(np.flatnonzero((stage_of == 1) & (D[i] <= radius)).tolist())
    shared = near(a) & near(b)
    assert shared and near(b) - near(a)
    rel = rel_rows(1, N, 4)
    for seeds in ([[a, b]], [[b, a]], [[a, a]]):
        got = run_expand(hip, dev, P[None], stage_of, 1, state, seeds, radius, VIEW, rel, 16)
        check(got, P[None], stage_of, 1, state, seeds, radius, VIEW, rel, 16, seeds)
        first, second = seeds[0]
        n1 = len(near(first))
        cand = got["cand"][0]
        assert cand[:n1].tolist() == sorted(near(first)) and cand[n1:got["n_cand"][0]].tolist() == sorted(near(second) - near(first))
        assert len(set(cand[:got["n_cand"][0]].tolist())) == got["n_cand"][0]


def test_exclusions(be):
    """stage_of > max_stage is excluded, evaluated poses are excluded, the seed is never emitted -- not even one whose state is 0."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, radius = len(P), math.radians(VIEW_RADII_DEG[0])
    assert_radius_in_gap(P, stage_of, 2, VIEW, radius)
    rel = rel_rows(2, N, 5)
    state = np.zeros((2, N), dtype=np.uint8)                       # nothing evaluated: the seeds themselves are eligible poses
    seeds = np.array([[7, 7], [30, 30]], dtype=np.int64)
    for max_stage in (0, 1, 2):
        got = run_expand(hip, dev, P[None], stage_of, max_stage, state, seeds, radius, VIEW, rel, 64)
        check(got, P[None], stage_of, max_stage, state, seeds, radius, VIEW, rel, 64, max_stage)
        for b in range(2):
            c = got["cand"][b, :got["n_cand"][b]]
            assert (stage_of[c] <= max_stage).all() and seeds[b, 0] not in c and (got["n_cand"][b] > 0 or max_stage == 0) and got["state"][b, seeds[b, 0]] == 0
    seeds = np.array([[7, 30], [30, 7]], dtype=np.int64)
    # evaluated neighbours do not come back
    full = run_expand(hip, dev, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, 64)
    again = run_expand(hip, dev, P[None], stage_of, 2, full["state"], seeds, radius, VIEW, rel, 64)
    check(again, P[None], stage_of, 2, full["state"], seeds, radius, VIEW, rel, 64, "again")
    assert (full["n_cand"] > 20).all() and (full["n_dropped"] == 0).all() and (again["n_cand"] == 0).all() and (again["cand"] == -1).all()


def test_capacity(be):
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, radius = len(P), math.radians(VIEW_RADII_DEG[1])
    assert_radius_in_gap(P, stage_of, 2, VIEW, radius)
    rel = rel_rows(2, N, 6)
    state = np.repeat((stage_of < 2).astype(np.uint8)[None], 2, axis=0)
    seeds = np.array([[40, 3, 60], [40, 3, 60]], dtype=np.int64)       # (the same candidates, other rows: one capacity is "equal" for both)
    count = [ref_expand(P, stage_of, 2, state[b], list(seeds[b]), radius, VIEW, rel[b], N)["n_cand"] for b in range(2)]
    assert count[0] == count[1] and count[0] >= 8, count
    n = count[0]
    for M, bit in ((n - 5, 1), (n, 0), (n + 1, 0), (1, 1)):
        got = run_expand(hip, dev, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, M)
        wants = check(got, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, M, M)
        assert got["status"] == bit and (got["n_dropped"] == max(n - M, 0)).all() and (got["n_cand"] == min(n, M)).all()
        full = ref_expand(P, stage_of, 2, state[0], list(seeds[0]), radius, VIEW, rel[0], N)
        assert np.array_equal(got["cand"][0, :min(n, M)], full["cand"][:min(n, M)])          # below the count: the first M in order
        assert int(got["state"][0].sum()) == int(state[0].sum()) + min(n, M)                  # a dropped pose stays unevaluated
        if M == n + 1:                                                                        # the single pad slot: -1, the first seed's row
            assert (got["cand"][:, n] == -1).all()
            for b in range(2):
                assert got["rows"][b, n].tobytes() == rel[b, seeds[b, 0]].tobytes()


def test_dropped_counted_once(be):
    """A pose two seeds reach and the capacity drops is one dropped pose, not two."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N = len(P)
    rel = rel_rows(1, N, 7)
    state = (stage_of == 0).astype(np.uint8)[None]
    seeds = [[0, 1, 2]]
    got = run_expand(hip, dev, P[None], stage_of, 1, state, seeds, math.pi, VIEW, rel, 10)
    check(got, P[None], stage_of, 1, state, seeds, math.pi, VIEW, rel, 10)
    assert got["n_cand"][0] == 10 and got["n_dropped"][0] == 65 - 10 and got["status"] == 1


def test_per_sample_poses(be):
    """(B, N, 3, 3) poses against the shared (1, N, 3, 3) grid: the same result; and truly different grids per sample."""
    from nope_amd.harness import random_rotations
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, B, radius = len(P), 3, math.radians(VIEW_RADII_DEG[1])
    assert_radius_in_gap(P, stage_of, 2, VIEW, radius)
    rel = rel_rows(B, N, 8)
    state = mixed_state(B, stage_of, 2, 81)
    seeds = evaluated_seeds(state, 3, 82)
    shared = run_expand(hip, dev, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, 18)
    per = run_expand(hip, dev, np.repeat(P[None], B, axis=0), stage_of, 2, state, seeds, radius, VIEW, rel, 18)
    assert all(np.asarray(shared[f]).tobytes() == np.asarray(per[f]).tobytes() for f in shared)
    Q = np.stack([P, random_rotations(N, torch.Generator().manual_seed(83)).numpy(), P[::-1].copy()])
    radius = math.radians(20.0)
    for b in range(B):
        assert_radius_in_gap(Q[b], stage_of, 2, ROT, radius)
    got = run_expand(hip, dev, Q, stage_of, 2, state, seeds, radius, ROT, rel, 40)
    check(got, Q, stage_of, 2, state, seeds, radius, ROT, rel, 40, "per-sample")
    assert not np.array_equal(got["cand"][0], got["cand"][2])


def ring(N):
    """N viewpoints on a great circle, 2 pi / N apart: rotations about x, whose third row is (0, sin a, cos a)."""
    a = 2.0 * np.pi * np.arange(N) / N
    P = np.zeros((N, 3, 3))
    P[:, 0, 0] = 1.0
    P[:, 1, 1], P[:, 1, 2], P[:, 2, 1], P[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return P


@pytest.mark.parametrize("N", [1, 255, 256, 257, 600])
def test_scan_block_edges(be, N):
    """N at and around the workgroup size: the scan's last chunk is partial, exactly full, or one pose long; members straddle the chunk edge."""
    hip, dev, _ = be
    P, stage_of = ring(N), np.zeros(N, dtype=np.int32)
    radius = 2.5 * 2.0 * np.pi / N if N > 1 else 1.0
    assert_radius_in_gap(P, stage_of, 0, VIEW, radius)
    B = 2
    rel = rel_rows(B, N, 9)
    state = np.zeros((B, N), dtype=np.uint8)
    if N > 1:
        state[1, np.random.default_rng(N).choice(N, size=N // 3, replace=False)] = 1
    seeds = np.array([[0, N - 1, min(128, N - 1), min(254, N - 1)], [min(255, N - 1), N // 2, 0, 0]], dtype=np.int64)
    got = run_expand(hip, dev, P[None], stage_of, 0, state, seeds, radius, VIEW, rel, 24)
    wants = check(got, P[None], stage_of, 0, state, seeds, radius, VIEW, rel, 24, N)
    if N == 1:
        assert (got["n_cand"] == 0).all() and (got["cand"] == -1).all()                # the only pose is the seed
    elif N >= 255:
        assert wants[0]["cand"][:4].tolist() == [1, 2, N - 2, N - 1]
    for M in (N, max(N - 1, 1)):                                                        # stage 0: dense flags through every chunk
        got = run_expand(hip, dev, P[None], stage_of, 0, state, None, 0.0, VIEW, rel, M)
        check(got, P[None], stage_of, 0, state, None, 0.0, VIEW, rel, M, (N, M))


def test_bad_seeds(be):
    """A seed of -1 and one of N: bit 1, the seed is skipped; the pad row is the first VALID seed's."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, radius = len(P), math.radians(VIEW_RADII_DEG[1])
    assert_radius_in_gap(P, stage_of, 2, VIEW, radius)
    rel = rel_rows(3, N, 10)
    state = np.repeat((stage_of < 2).astype(np.uint8)[None], 3, axis=0)
    seeds = np.array([[-1, 40, 3], [40, N, 3], [N + 5, -7, -1]], dtype=np.int64)
    got = run_expand(hip, dev, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, 16)
    check(got, P[None], stage_of, 2, state, seeds, radius, VIEW, rel, 16)
    assert got["status"] == 2 and np.array_equal(got["cand"][0], got["cand"][1]) and got["n_cand"][2] == 0
    assert got["rows"][0, 15].tobytes() == rel[0, 40].tobytes() and got["rows"][2, 0].tobytes() == rel[2, 0].tobytes()
    ok = run_expand(hip, dev, P[None], stage_of, 2, state[:1], [[40, 3]], radius, VIEW, rel[:1], 16)
    assert ok["status"] == 0 and np.array_equal(ok["cand"][0], got["cand"][0])


@pytest.mark.parametrize("kind", [ROT, VIEW])
def test_nan_pose(be, kind):
    """A NaN pose is never a member; a NaN seed pose reaches nothing."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    P = P.copy()
    N = len(P)
    radius = math.radians(VIEW_RADII_DEG[1] if kind == VIEW else 20.0)
    assert_radius_in_gap(P, stage_of, 2, kind, radius)
    D = distances(P, P, kind)
    victim = int(np.flatnonzero((stage_of == 2) & (D[40] <= radius))[0])
    P[victim] = np.nan
    P[60, 2, 1] = np.nan
    rel = rel_rows(1, N, 11)
    state = (stage_of < 2).astype(np.uint8)[None]
    seeds = [[40, 60]]
    got = run_expand(hip, dev, P[None], stage_of, 2, state, seeds, radius, kind, rel, 16)
    w = check(got, P[None], stage_of, 2, state, seeds, radius, kind, rel, 16, kind)[0]
    assert victim not in got["cand"][0] and w["n_cand"] > 0 and got["state"][0, victim] == 0
    only = run_expand(hip, dev, P[None], stage_of, 2, state, [[60]], radius, kind, rel, 16)
    assert only["n_cand"][0] == 0 and only["status"] == 0
    got_pi = run_expand(hip, dev, P[None], stage_of, 2, state, [[40]], math.pi, kind, rel, N)          # even at radius pi
    assert victim not in got_pi["cand"][0] and got_pi["n_cand"][0] == int((stage_of == 2).sum()) - 1


BAD_ARGS = [dict(N=0), dict(capacity=0), dict(capacity=-3), dict(n_seeds=17), dict(n_seeds=-1), dict(radius_rad=float("nan")),
            dict(radius_rad=-1e-9), dict(dist_kind=2), dict(dist_kind=-1), dict(poses=None), dict(stage_of=None), dict(state=None), dict(seeds=None),
            dict(rel=None), dict(cand=None), dict(n_cand=None), dict(n_dropped=None), dict(rows=None), dict(status=None)]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments(be, bad):
    """Each NOPE_ERR_ARG case: outputs (and the state) pre-filled with a sentinel are unchanged."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    P, stage_of = P[:26], stage_of[:26]
    B, N, M = 2, 26, 8
    t = dict(poses=torch.from_numpy(P.copy())[None].to(dev), stage_of=torch.from_numpy(stage_of.copy()).to(dev),
             state=torch.full((B, N), 7, dtype=torch.uint8, device=dev), seeds=torch.tensor([[1, 2], [3, 4]], dtype=torch.int64, device=dev),
             rel=torch.from_numpy(rel_rows(B, N, 12)).to(dev))
    out = dict(cand=torch.full((B, M), 7, dtype=torch.int32, device=dev), n_cand=torch.full((B,), 7, dtype=torch.int32, device=dev),
               n_dropped=torch.full((B,), 7, dtype=torch.int32, device=dev), rows=torch.full((B, M, 6), 7.0, device=dev),
               status=torch.full((1,), 7, dtype=torch.int32, device=dev))
    kw = dict(N=N, capacity=M, n_seeds=2, radius_rad=0.5, dist_kind=VIEW)
    kept = dict(t, **out)
    for k_, v in bad.items():
        if k_ in kw:
            kw[k_] = v
    arg = {k_: (None if k_ in bad else v) for k_, v in kept.items()}
    ex = hip.C2FExpand(arg["cand"], arg["n_cand"], arg["n_dropped"], arg["rows"], arg["status"])
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):
        hip._c2f_expand_call(arg["poses"], 0, kw["N"], arg["stage_of"], 0, kept["state"] if "state" not in bad else _NoPtr(kept["state"]), arg["seeds"],
                             kw["n_seeds"], kw["radius_rad"], kw["dist_kind"], arg["rel"], kw["capacity"], ex)
    assert all(bool((v == 7).all()) for v in out.values()) and bool((kept["state"] == 7).all())
    # the same call with nothing wrong goes through (the sentinel state 7 is "not 0": nothing is eligible)
    good = hip._c2f_expand_call(t["poses"], 0, N, t["stage_of"], 0, t["state"], t["seeds"], 2, 0.5, VIEW, t["rel"], M, hip.C2FExpand(**out))
    assert int(good.status) == 0 and bool((good.n_cand == 0).all()) and bool((good.cand == -1).all())


class _NoPtr:
    """Stands in for the state tensor with a NULL pointer: the launch reads its batch size and stream from the tensor it is given."""

    def __init__(self, t):
        self.shape, self.is_cuda, self.device = t.shape, t.is_cuda, t.device

    def data_ptr(self):
        return None


def test_radius_unchecked_without_seeds(be):
    """radius_rad is read with seeds only: stage 0 goes through whatever it holds."""
    hip, dev, _ = be
    P, stage_of = grid("l2")
    state = np.zeros((1, len(P)), dtype=np.uint8)
    got = run_expand(hip, dev, P[None], stage_of, 0, state, None, float("nan"), VIEW, rel_rows(1, len(P), 13), 26)
    assert got["n_cand"][0] == 26 and got["status"] == 0


def test_shape_errors(be):
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N = len(P)
    Pt, st, rel = torch.from_numpy(P.copy())[None].to(dev), torch.from_numpy(stage_of.copy()), torch.from_numpy(rel_rows(2, N, 14)).to(dev)
    state = torch.zeros((2, N), dtype=torch.uint8, device=dev)
    for args in ((Pt[:, :N - 1], st, 0, state, None, rel), (Pt, st[:-1], 0, state, None, rel), (Pt, st, 0, state.int(), None, rel),
                 (Pt, st, 0, state, None, rel[:, :, :5]), (Pt, st, 0, state, torch.zeros((3, 2), dtype=torch.int64), rel), (Pt, st, 0, state[0], None, rel)):
        with pytest.raises(hip.NopeError):
            hip.op_c2f_expand(*args, capacity=8)


def test_deterministic(be):
    hip, dev, _ = be
    P, stage_of = grid("l3")
    N, B = len(P), 3
    rel = rel_rows(B, N, 15)
    state = mixed_state(B, stage_of, 3, 151)
    seeds = evaluated_seeds(state, 16, 152)
    a, b = (run_expand(hip, dev, P[None], stage_of, 3, state, seeds, math.radians(VIEW_RADII_DEG[2]), VIEW, rel, 96) for _ in range(2))
    assert all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in a) and (a["n_cand"] > 16).all()


# ---- 2. commit ---------------------------------------------------------------------------------------------------------------------------------
def test_commit(be):
    """Exact bits (NaN with a payload, -0.0, inf), -1 skipped, and with similarity_ld = N + 3 the padding columns untouched."""
    hip, dev, _ = be
    B, N, M = 3, 341, 300
    rng = np.random.default_rng(16)
    cand = np.full((B, M), -1, dtype=np.int32)
    for b, n in enumerate((300, 17, 0)):
        cand[b, :n] = rng.choice(N, size=n, replace=False)
    cand[1, [2, 9]] = cand[1, [9, 2]]
    bits = rng.integers(0, 2 ** 32, size=(B, M), dtype=np.uint64).astype(np.uint32)
    bits[0, :4] = [0x7fc00001, 0xffc12345, 0x80000000, 0x7f800000]             # two NaNs with payloads, -0.0, +inf
    scores = bits.view(np.float32)
    for pad in (0, 3):
        big = torch.from_numpy(rng.integers(0, 2 ** 32, size=(B, N + pad), dtype=np.uint64).astype(np.uint32).view(np.float32).copy())
        before = big.numpy().view(np.uint32).copy()
        target = big.to(dev)
        view = target[:, :N]
        assert view.stride() == (N + pad, 1)
        ret = hip.op_c2f_commit(torch.from_numpy(scores.copy()).to(dev), torch.from_numpy(cand).to(dev), view)
        assert ret.data_ptr() == view.data_ptr()
        want = before.copy()
        for b in range(B):
            for j in range(M):
                if cand[b, j] >= 0:
                    want[b, cand[b, j]] = bits[b, j]
        assert target.cpu().numpy().view(np.uint32).tobytes() == want.tobytes(), pad
    with pytest.raises(hip.NopeError):
        hip.op_c2f_commit(torch.zeros(B, M).to(dev), torch.zeros(B, M - 1, dtype=torch.int32).to(dev), torch.zeros(B, N).to(dev))
    with pytest.raises(hip.NopeError):
        hip.op_c2f_commit(torch.zeros(B, M).to(dev), torch.zeros(B, M, dtype=torch.int32).to(dev), torch.zeros(B, N).to(dev).double())


# ---- 3. the driver on a planted landscape --------------------------------------------------------------------------------------------------------
def topk_order(s):
    """nope_topk's order of a row without NaN: descending score, ties -> lowest index."""
    return np.lexsort((np.arange(len(s)), -s.astype(np.float64)))


def ref_search(table, P, stage_of, n_stages, seeds, radii, caps, k, kind, rel):
    """coarse_to_fine_search for one query in NumPy: table (N,) f32 = the score `evaluate` gives each pose."""
    N = len(P)
    sim = np.full(N, -np.inf, dtype=np.float32)
    state = np.zeros(N, dtype=np.uint8)
    cands, dropped = [], []
    for s in range(n_stages):
        sd = [] if s == 0 else topk_order(sim)[:seeds].tolist()
        e = ref_expand(P, stage_of, s, state, sd, radii[s], kind, rel, caps[s])
        state = e["state"]
        c = e["cand"][:e["n_cand"]]
        sim[c] = table[c]
        cands.append(e["cand"])
        dropped.append(e["n_dropped"])
    return dict(similarity=sim, evaluated=state, nearest_idx=topk_order(sim)[:k], cand=cands, n_dropped=np.array(dropped))


def view_dirs(P):
    """The unit camera positions: minus the third row (the optical axis looks from the camera at the object).  Angles between them are the
    viewpoint distance; the "upper" grids hold the cameras with z >= 0."""
    v = -P[:, 2, :]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def upper_targets(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(n, 3))
    t[:, 2] = np.abs(t[:, 2])
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def angle_table(P, targets):
    """(len(targets), N) f64: the viewpoint angle of every pose to every target."""
    return np.arccos(np.clip(targets @ view_dirs(P).T, -1.0, 1.0))


def planted_evaluate(table, rel, dev):
    """evaluate(rows, cand) of a planted landscape: the score of a pose is table[b, pose]; it also holds rows to all_relativeR[b, cand]."""
    tab, rel_t = torch.from_numpy(table).to(dev), torch.from_numpy(rel).to(dev)

    def evaluate(rows, cand):
        idx = cand.clamp(min=0).long()
        real = cand >= 0
        picked = torch.gather(rel_t, 1, idx[:, :, None].expand(-1, -1, 6))
        assert torch.equal(rows[real].view(torch.int32), picked[real].view(torch.int32)) and bool(torch.isfinite(rows).all())
        return torch.gather(tab, 1, idx)
    return evaluate


def run_search(hip, dev, table, P, stage_of, rel, **kw):
    from nope_amd.search import coarse_to_fine_search
    return coarse_to_fine_search(planted_evaluate(table, rel, dev), torch.from_numpy(rel).to(dev), torch.from_numpy(P.copy())[None].to(dev), stage_of, **kw)


def assert_search_equal(got, wants, n_stages):
    sim, ev, idx = got.similarity.cpu().numpy(), got.evaluated.cpu().numpy(), got.nearest_idx.cpu().numpy()
    assert got.similarity.dtype == torch.float32 and got.evaluated.dtype == torch.uint8 and got.nearest_idx.dtype == torch.int64
    assert len(got.cand) == n_stages and tuple(got.n_dropped.shape) == (n_stages, len(wants)) and tuple(got.status.shape) == (n_stages,)
    for b, w in enumerate(wants):
        assert sim[b].tobytes() == w["similarity"].tobytes(), b                        # the score bits where evaluated, -inf elsewhere
        assert np.array_equal(ev[b], w["evaluated"]) and np.array_equal(idx[b], w["nearest_idx"]), b
        assert np.isneginf(sim[b][ev[b] == 0]).all() and np.isfinite(sim[b][ev[b] == 1]).all()
        for s in range(n_stages):
            assert np.array_equal(got.cand[s][b].cpu().numpy(), w["cand"][s]), (b, s)
        assert np.array_equal(got.n_dropped[:, b].cpu().numpy(), w["n_dropped"]), b
        assert int(got.n_evaluated[b]) == int(w["evaluated"].sum())


@pytest.mark.parametrize("name", ["l2", "l3"])
def test_driver_unimodal(be, name):
    """score = -viewpoint angle to each of 32 fixed-seed random upper-hemisphere targets, seeds = 3: the NumPy driver's top-1 is the
    exhaustive argmax for all 32 (asserted first), and the device result equals the NumPy driver exactly."""
    from nope_amd import poses
    from nope_amd.search import stage_capacities
    hip, dev, _ = be
    P, stage_of = grid(name)
    N, B, n_stages = len(P), 32, GRIDS[name][0] + 1
    radii = poses.stage_radii(P, stage_of, VIEW)
    for s in range(1, n_stages):
        assert_radius_in_gap(P, stage_of, s, VIEW, radii[s])
    table = (-angle_table(P, upper_targets(B, 2022))).astype(np.float32)
    rel = rel_rows(B, N, 17)
    caps = stage_capacities(stage_of, n_stages, 3, None)
    assert caps == [26] + [18] * (n_stages - 1)
    wants = [ref_search(table[b], P, stage_of, n_stages, 3, radii, caps, 5, VIEW, rel[b]) for b in range(B)]
    for b, w in enumerate(wants):
        assert w["nearest_idx"][0] == topk_order(table[b])[0], b                       # the precondition: the search meets the exhaustive top-1
        assert w["n_dropped"].sum() == 0
    got = run_search(hip, dev, table, P, stage_of, rel, seeds=3)
    assert_search_equal(got, wants, n_stages)
    assert int(got.status.cpu().sum()) == 0
    worst = int(got.n_evaluated.max())
    assert worst <= 26 + 18 * (n_stages - 1) and worst < 0.25 * N, worst               # a fraction of the grid


def test_driver_two_bumps(be):
    """The max of two such terms, targets 111 degrees apart: the search reaches both exhaustive maxima (asserted on the reference first), and
    pose_distribution on the sparse row returns them as its first two modes."""
    from nope_amd import poses
    from nope_amd.model import PoseConditional
    from nope_amd.search import stage_capacities
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N, n_stages = len(P), 3
    el, az = math.radians(30.0), math.radians(17.0)
    t = np.array([[math.cos(el) * math.cos(az + d), math.cos(el) * math.sin(az + d), math.sin(el)] for d in (0.0, math.radians(144.0))])
    assert math.degrees(math.acos(float(t[0] @ t[1]))) > 60.0
    A = angle_table(P, t)
    peaks = [int(np.argmin(A[0])), int(np.argmin(A[1]))]
    table = np.repeat((-np.minimum(A[0], A[1])).astype(np.float32)[None], 2, axis=0)
    rel = rel_rows(2, N, 18)
    radii = poses.stage_radii(P, stage_of, VIEW)
    for s in range(1, n_stages):
        assert_radius_in_gap(P, stage_of, s, VIEW, radii[s])
    caps = stage_capacities(stage_of, n_stages, 4, None)
    wants = [ref_search(table[b], P, stage_of, n_stages, 4, radii, caps, 5, VIEW, rel[b]) for b in range(2)]
    assert all(w["evaluated"][p] == 1 for w in wants for p in peaks) and sorted(wants[0]["nearest_idx"][:2].tolist()) == sorted(peaks)
    got = run_search(hip, dev, table, P, stage_of, rel, seeds=4)
    assert_search_equal(got, wants, n_stages)
    radius_deg = 20.0
    D = distances(P, P, ROT)
    assert np.abs(D[~np.eye(N, dtype=bool)] - math.radians(radius_deg)).min() >= 1e-6 and D[peaks[0], peaks[1]] > math.radians(radius_deg)
    modes = PoseConditional.pose_distribution(None, got.similarity, torch.from_numpy(P.copy())[None].to(dev), temperature=0.05, radius_deg=radius_deg)
    idx = modes.idx.cpu().numpy()
    assert all(sorted(idx[b, :2].tolist()) == sorted(peaks) for b in range(2)) and bool((modes.n_modes >= 2).all())
    assert bool((modes.prob[got.evaluated == 0] == 0).all()) and bool(torch.isfinite(modes.entropy).all())


def test_driver_arguments(be):
    hip, dev, _ = be
    P, stage_of = grid("l2")
    N = len(P)
    rel = rel_rows(1, N, 19)
    table = np.zeros((1, N), dtype=np.float32)
    with pytest.raises(ValueError, match="stage 0"):
        run_search(hip, dev, table, P, np.where(np.arange(N) < 4, 0, 1).astype(np.int32), rel, seeds=3, k=5)
    with pytest.raises(ValueError):
        run_search(hip, dev, table, P, stage_of, rel, seeds=17)
    with pytest.raises(ValueError):
        run_search(hip, dev, table, P, stage_of[:-1], rel)
    # every pose within pi and room for all of them: everything is evaluated, whatever the seeds
    got = run_search(hip, dev, table, P, stage_of, rel, radii_rad=math.pi, capacity=N)
    assert int(got.n_evaluated[0]) == N and bool((got.evaluated == 1).all()) and bool((got.similarity == 0).all())
    # too little room: the overflow is counted and flagged, stage by stage
    got = run_search(hip, dev, table, P, stage_of, rel, radii_rad=math.pi, capacity=[26, 10, 10])
    assert got.n_dropped[:, 0].cpu().tolist() == [0, 55, 295] and got.status.cpu().tolist() == [0, hip.C2F_OVERFLOW, hip.C2F_OVERFLOW]
    assert int(got.n_evaluated[0]) == 46


# ---- 4. host side ----------------------------------------------------------------------------------------------------------------------------------
def test_grid_stages_and_radii():
    from nope_amd import poses
    for level, dist, counts in ((0, "upper", [26]), (1, "upper", [26, 65]), (2, "upper", [26, 65, 250]), (3, "upper", [26, 65, 250, 980]), (2, "all", [42, 120, 480])):
        st = poses.grid_stages(level, dist)
        assert st.dtype == np.int32 and np.bincount(st).tolist() == counts
        fine = poses.get_obj_poses_from_template_level(level, dist, return_cam=True)[:, :3, 3]
        for l in range(level + 1):                                   # the poses of stage <= l are exactly the level-l grid
            coarse = poses.get_obj_poses_from_template_level(l, dist, return_cam=True)[:, :3, 3]
            assert np.array_equal(fine[st <= l], coarse)
        assert np.array_equal(poses.grid_stages_for_size(len(st)), st)
    assert np.array_equal(np.flatnonzero(poses.grid_stages(2, "upper") == 0), poses.load_index_level0_in_level2("upper"))
    with pytest.raises(ValueError):
        poses.grid_stages_for_size(100)
    P, st = grid("l3")
    radii = poses.stage_radii(P, st, VIEW)
    assert np.allclose(np.degrees(radii), (0.0,) + VIEW_RADII_DEG, atol=5e-3)
    for s, (lo, hi) in zip((1, 2, 3), ((18.70, 26.57), (9.44, 12.94), (4.73, 6.43))):          # inside the wide gaps of the distance spectrum
        Q = P[st <= s]
        D = np.degrees(distances(Q, Q, VIEW))[~np.eye(len(Q), dtype=bool)]
        assert not ((D > lo + 0.01) & (D < hi - 0.01)).any() and lo < math.degrees(radii[s]) < hi
        n = (np.degrees(distances(Q, Q, VIEW)) <= math.degrees(radii[s])).sum(1) - 1
        assert 4 <= n.min() and n.max() <= 6
    assert np.allclose(poses.stage_radii(P, st, VIEW, factor=2.5), 2.0 * radii)
    assert np.array_equal(poses.pose_distance(P[:7], P, ROT), distances(P[:7], P, ROT))


def test_grid_stages_from_files(tmp_path):
    """With `root`: the files' own order -- here the synthesised grids, shuffled -- is matched through the camera positions."""
    from nope_amd import poses
    rng = np.random.default_rng(3)
    perms = {}
    for level in range(3):
        cams, objs = poses.synthesize_grid(level)
        perms[level] = rng.permutation(len(cams))
        np.save(tmp_path / f"sphere_poses_level{level}.npy", cams[perms[level]])
        np.save(tmp_path / f"obj_poses_level{level}.npy", objs[perms[level]])
    st = poses.grid_stages(2, "upper", root=str(tmp_path))
    index, _ = poses.get_obj_poses_from_template_level(2, "upper", return_index=True)
    full = np.searchsorted(np.array([42, 162]), np.arange(642), side="right")
    keep = np.isin(perms[2], index)
    assert np.array_equal(st, full[perms[2]][keep]) and np.bincount(st).tolist() == [26, 65, 250]


def test_template_parallel_raises(monkeypatch):
    from nope_amd import model as M
    monkeypatch.setattr(M.ndist, "world", lambda: (0, 2))
    fake = type("Fake", (), {"similarity_metric": "l2", "template_parallel": True})()
    with pytest.raises(NotImplementedError):
        M.PoseConditional.retrieve_coarse_to_fine_from_feat(fake, None, None, None, None)


# ---- 5. end to end (device only: the U-Net) ---------------------------------------------------------------------------------------------------------
_E2E = {}


def _e2e():
    """build_model(u_net_dim=8, encoder="stub") in f32 on 16 x 16 inputs, B = 2, level-2 upper; the exhaustive step and the search, once."""
    if not _E2E:
        from nope_amd import harness
        model = harness.build_model(seed=7, compute_dtype="f32", device="cuda", u_net_dim=8, encoder="stub")
        batch = harness.synthetic_batch(2, 0, 16, seed=7, device="cuda", pose_level=2)
        sim, idx, _ = model.generate_and_retrieve(batch["query"], batch["reference"], batch["all_relativeR"])
        c2f = model.retrieve_coarse_to_fine(batch["query"], batch["reference"], batch["all_relativeR"], batch["template_poses"])
        _E2E.update(model=model, batch=batch, sim=sim, idx=idx, c2f=c2f)
    return _E2E


@pytest.mark.gpu
def test_e2e_scores_and_replay(gpu):
    from nope_amd import poses
    from nope_amd.search import stage_capacities
    from tests.util import MODE_BOUNDS
    e = _e2e()
    c2f, sim = e["c2f"], e["sim"].cpu().numpy()
    P, stage_of = grid("l2")
    assert np.array_equal(e["batch"]["template_poses"][0].cpu().numpy(), P)
    got, ev = c2f.similarity.cpu().numpy(), c2f.evaluated.cpu().numpy().astype(bool)
    # every evaluated entry agrees with the exhaustive similarity: the same arithmetic per sample, only the launch shapes differ, so the
    # suite's own f32 score bound applies (relative to the largest |score|)
    err = np.abs(got[ev].astype(np.float64) - sim[ev]).max() / np.abs(sim).max()
    print("c2f vs exhaustive, relative score error:", err)
    assert err <= MODE_BOUNDS["f32"][1], err
    assert np.isneginf(got[~ev]).all() and np.isfinite(got[ev]).all()
    n_cand = sum((c >= 0).sum(1) for c in c2f.cand)
    assert np.array_equal(c2f.n_evaluated.cpu().numpy(), n_cand.cpu().numpy()) and np.array_equal(ev.sum(1), n_cand.cpu().numpy())
    assert (ev.sum(1) <= 26 + 18 + 18).all() and int(c2f.status.cpu().sum()) == 0
    # replay: the NumPy driver, fed the device's own scores, reproduces every stage's candidates
    radii = poses.stage_radii(P, stage_of, VIEW)
    for s in (1, 2):
        assert_radius_in_gap(P, stage_of, s, VIEW, radii[s])
    rel = e["batch"]["all_relativeR"].cpu().numpy()
    for b in range(2):
        w = ref_search(got[b], P, stage_of, 3, 3, radii, stage_capacities(stage_of, 3, 3, None), 5, VIEW, rel[b])
        for s in range(3):
            assert np.array_equal(c2f.cand[s][b].cpu().numpy(), w["cand"][s]), (b, s)
        assert got[b].tobytes() == w["similarity"].tobytes() and np.array_equal(c2f.nearest_idx[b].cpu().numpy(), w["nearest_idx"])


@pytest.mark.gpu
def test_e2e_everything_evaluated(gpu):
    from tests.util import MODE_BOUNDS
    e = _e2e()
    b = e["batch"]
    N = b["all_relativeR"].shape[1]
    c2f = e["model"].retrieve_coarse_to_fine(b["query"], b["reference"], b["all_relativeR"], b["template_poses"], radii_rad=math.pi, capacity=N)
    assert bool((c2f.evaluated == 1).all()) and c2f.n_evaluated.cpu().tolist() == [N, N]
    sim = e["sim"]
    err = float((c2f.similarity.double() - sim.double()).abs().max() / sim.abs().max())
    assert err <= MODE_BOUNDS["f32"][1], err


@pytest.mark.gpu
def test_e2e_predict_pose(gpu):
    e = _e2e()
    b, model, c2f = e["batch"], e["model"], e["c2f"]
    args = (b["query"], b["reference"], b["all_relativeR"], b["template_poses"])
    pred0, score0 = model.predict_pose(*args)
    pred1, score1 = model.predict_pose(*args, coarse_to_fine=None)
    assert torch.equal(pred0, pred1) and torch.equal(score0, score1)
    assert torch.equal(pred0, b["template_poses"][torch.arange(2, device="cuda")[:, None], e["idx"]])          # the exhaustive answer, as before
    pred, score = model.predict_pose(*args, coarse_to_fine=True)
    rows = torch.arange(2, device="cuda")[:, None]
    assert torch.equal(pred, b["template_poses"].double()[rows, c2f.nearest_idx]) and torch.equal(score, torch.gather(c2f.similarity, 1, c2f.nearest_idx))
    pred_d, _ = model.predict_pose(*args, coarse_to_fine=dict(seeds=2, k=3), distinct_deg=20.0, temperature=50.0)
    assert tuple(pred_d.shape) == (2, 3, 3, 3)
    pred_r, score_r = model.predict_pose(*args, coarse_to_fine=True, refine_iters=1)                           # the refinement reads the sparse row
    assert tuple(pred_r.shape) == (2, 5, 3, 3) and bool(torch.isfinite(score_r).all())


@pytest.mark.gpu
def test_e2e_eval_geodesic(gpu, tmp_path):
    from nope_amd import harness
    from nope_amd.metrics import GeodesicError
    e = _e2e()
    b, model, c2f = e["batch"], e["model"], e["c2f"]
    sim_a, idx_a, res_a = harness.eval_geodesic(model, b, save_path=str(tmp_path / "a"))
    sim_b, idx_b, res = harness.eval_geodesic(model, b, save_path=str(tmp_path / "b"), coarse_to_fine=True)
    assert torch.equal(sim_a, sim_b) and torch.equal(idx_a, idx_b)
    assert {k: v for k, v in res.items() if not k.startswith("c2f/")} == res_a                                  # the old keys, the old values
    _, metric = GeodesicError([15, 30]).from_indices(b["template_poses"][:1], c2f.nearest_idx, b["query_pose"], b["symmetry"])
    assert sorted(k[len("c2f/"):] for k in res if k.startswith("c2f/")) == sorted(list(metric) + ["evaluated_frac", "top1_agree"])
    for k, v in metric.items():
        assert res[f"c2f/{k}"] == float(v), k
    assert res["c2f/evaluated_frac"] == float(c2f.n_evaluated.float().mean()) / 341 and 0.0 < res["c2f/evaluated_frac"] <= 62 / 341
    assert res["c2f/top1_agree"] == float((c2f.nearest_idx[:, 0] == idx_a[:, 0]).float().mean())
    za, zb = np.load(str(tmp_path / "a.npz")), np.load(str(tmp_path / "b.npz"))
    assert sorted(set(zb.files) - set(za.files)) == ["c2f_idx", "c2f_similarity"] and all(za[f].tobytes() == zb[f].tobytes() for f in za.files)
    assert zb["c2f_similarity"].tobytes() == c2f.similarity.cpu().numpy().tobytes() and np.array_equal(zb["c2f_idx"], c2f.nearest_idx.cpu().numpy())
