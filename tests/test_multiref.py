"""Multi-reference pose retrieval (csrc/kernels_multiref.hip, hip.op_multiref_prepare / multiref_similarity / op_multiref_fuse_scores,
PoseConditional.retrieve_multi* / predict_pose_multi, harness.synthetic_batch(n_references) / eval_geodesic(multi_ref)).  DESIGN.md section 4.12.

Every test runs on the interpreter build ("emu") and, marked `gpu`, on the device.  The references are f64 NumPy restatements of the
definitions in include/nope_hip.h, written below; oracle.nope_ref supplies the U-Net bank and `similarity_scores` of the end-to-end test.

Bounds, from the arithmetic:
  dist            1e-8 rad: two f64 evaluations of acos, worst near 0 and pi (tests/test_pose_modes.py)
  all_relativeR   one f32 ulp of f32(T P^T): the f64 dot products differ in their last bits, the one rounding to f32 may then fall either way
  softmax weights 2^-22 |want| + 1e-37: one rounding of an f64 result (tests/test_pose_modes.py's bound for prob)
  uniform weights, nearest weights: exact (nearest under the ASSERTED precondition that best and second-best distance differ by >= 1e-6 rad)
  fused scoring on dyadic data: bit patterns (every product, partial sum and square root is exact in any order)
  fused scoring on random data: 2e-5 relative (max abs difference over max abs), tests/test_gpu_sweeps.py's bound for nope_similarity; the
                  blend adds at most (R + 1) 2^-24 per element
  late fusion on dyadic data: bit patterns
"""
import functools
import math
import re

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
REL = 2.0 ** -22
NT = 256
WEIGHTINGS = ("uniform", "softmax", "nearest")


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


# ---- the reference (f64 NumPy) -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(level):
    from nope_amd import poses
    P = np.ascontiguousarray(poses.get_obj_poses_from_template_level(level, "upper")[:, :3, :3], dtype=np.float64)
    P.setflags(write=False)
    return P


def haar(n, seed):
    from nope_amd.harness import random_rotations
    return random_rotations(n, torch.Generator().manual_seed(seed)).numpy()


def np_distance(T, P, kind):
    """T (N, 3, 3), P (R, 3, 3) -> (R, N) radians: nope_op_c2f_expand's two distances."""
    if kind == 0:
        return np.arccos(np.clip((np.einsum("nij,rij->rn", T, P) - 1.0) / 2.0, -1.0, 1.0))
    a, b = T[:, 2, :], P[:, 2, :]
    na, nb = np.maximum(np.linalg.norm(a, axis=1), 1e-8), np.maximum(np.linalg.norm(b, axis=1), 1e-8)
    return np.arccos(np.clip((b @ a.T) / (nb[:, None] * na[None, :]), -1.0, 1.0))


def np_prepare(T, P, n_refs, weighting, tau_rad, kind):
    """T (B|1, N, 3, 3), P (B, R, 3, 3), n_refs (B,) ints or None -> rel (B, R, N, 6) f64, weights (B, R, N) f64, dist (B, R, N) f64, status."""
    B, R = P.shape[:2]
    N = T.shape[1]
    rel, w, d = np.zeros((B, R, N, 6)), np.zeros((B, R, N)), np.full((B, R, N), np.inf)
    status = 0
    for b in range(B):
        Tb = T[b if T.shape[0] > 1 else 0]
        nr = R if n_refs is None else int(n_refs[b])
        bad = 0
        if nr < 1 or nr > R:
            bad = 2
        elif not np.isfinite(P[b, :nr]).all():
            bad = 1
        status |= bad
        for r in range(R):
            src = r if r < nr else 0
            with np.errstate(invalid="ignore"):
                rel[b, r] = np.einsum("nik,jk->nij", Tb, P[b, src])[:, :2, :].reshape(N, 6)
                if r < nr:
                    d[b, r] = np_distance(Tb, P[b, r:r + 1], kind)[0]
        if bad:
            w[b] = np.nan
            continue
        dv = d[b, :nr]
        if weighting == "uniform":
            w[b, :nr] = 1.0 / nr
        elif weighting == "softmax":
            e = np.exp(-(dv - dv.min(axis=0)) / tau_rad)
            w[b, :nr] = e / e.sum(axis=0)
        else:
            w[b, np.argmin(dv, axis=0), np.arange(N)] = 1.0            # (argmin: the first minimum = the lowest r)
    return rel, w, d, status


def np_fused_scores(q, bank, w):
    """q (B, C, h, w'), bank (B, R, N, C, h, w') as stored, w (B, R, N) f32 -> (B, N) f64: the definition of nope_multiref_similarity in f64."""
    q, bank, w = q.double().numpy(), bank.double().numpy(), w.double().numpy()
    B, R, N = w.shape
    out = np.zeros((B, N))
    for b in range(B):
        tbar = np.zeros(bank.shape[2:])
        for r in range(R):
            on = w[b, r] != 0                                             # (NaN != 0: a NaN weight takes part)
            with np.errstate(invalid="ignore", over="ignore"):
                tbar[on] += w[b, r, on, None, None, None] * bank[b, r, on]
        with np.errstate(invalid="ignore", over="ignore"):
            out[b] = -np.sqrt(((q[b][None] - tbar) ** 4).sum(axis=1)).reshape(N, -1).sum(axis=1)
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got, want):
    """f32 tensors equal as bit patterns (-0.0 is not 0.0); a NaN matches any NaN."""
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    if got.shape != want.shape:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


def ulp_apart(got, want):
    """The largest distance in f32 ulps between two finite f32 arrays of one sign pattern."""
    g, w = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    gi, wi = g.view(np.int32).astype(np.int64), w.view(np.int32).astype(np.int64)
    gi, wi = np.where(gi < 0, -(gi & 0x7fffffff), gi), np.where(wi < 0, -(wi & 0x7fffffff), wi)
    return int(np.abs(gi - wi).max())


def close(got, want):
    """|got - want| <= 2^-22 |want| + 1e-37, a NaN where a NaN is wanted."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= REL * np.abs(want[~nan]) + 1e-37))


# ---- 1. prepare ----------------------------------------------------------------------------------------------------------------------------
def _prepare_inputs(level, R, B=3, seed=11):
    T = grid(level)[None]                                       # pose_stride_b = 0
    P = haar(B * R, seed + 100 * R + level).reshape(B, R, 3, 3)
    return T, P


@pytest.mark.parametrize("n_refs", [None, (1, 2, 3)], ids=["all", "padded"])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("level", [0, 1])
def test_prepare(be, level, R, n_refs):
    hip, dev, _ = be
    T, P = _prepare_inputs(level, R)
    B, N = 3, T.shape[1]
    assert N == (26, 91)[level]
    nr = None if n_refs is None else [min(x, R) for x in n_refs]
    tau = 30.0
    for kind in (0, 1):
        for weighting in WEIGHTINGS:
            got = hip.op_multiref_prepare(torch.from_numpy(T.copy()).to(dev), torch.from_numpy(P).to(dev), None if nr is None else torch.tensor(nr),
                                          weighting=weighting, tau_deg=tau, dist_kind=kind, want_dist=True)
            rel, w, d, status = np_prepare(T, P, nr, weighting, math.radians(tau), kind)
            where = (level, R, n_refs, kind, weighting)
            assert int(got.status) == status == 0, where
            assert tuple(got.all_relativeR.shape) == (B, R, N, 6) and got.all_relativeR.dtype == torch.float32 and got.dist.dtype == torch.float64
            gd, gw, grel = got.dist.cpu().numpy(), got.weights.cpu().numpy(), got.all_relativeR.cpu().numpy()
            valid = np.isfinite(d)
            assert np.array_equal(np.isposinf(gd), ~valid), where                      # a padded reference: +inf, weight 0, the rows of reference 0
            assert np.abs(gd[valid] - d[valid]).max() <= 1e-8, where
            assert ulp_apart(grel, rel.astype(np.float32)) <= 1, where
            for b in range(B):
                for r in range(R if nr is None else nr[b], R):
                    assert np.array_equal(grel[b, r], grel[b, 0]) and (gw[b, r] == 0).all(), (where, b, r)
            if weighting == "uniform":
                assert np.array_equal(gw, w.astype(np.float32)), where
            elif weighting == "softmax":
                assert close(gw, w), where
                assert np.abs(gw.astype(np.float64).sum(axis=1) - 1.0).max() <= R * 2.0 ** -24, where
            else:
                ds = np.sort(d, axis=1)
                if R > 1:                                                               # the precondition: no near tie, none left out
                    gap = ds[:, 1] - ds[:, 0]
                    assert gap[np.isfinite(gap)].min() >= 1e-6 and (np.isfinite(gap) | np.isposinf(ds[:, 1])).all(), where
                assert np.array_equal(gw, w.astype(np.float32)), where
    if R == 1:                                                                          # the single-reference rows of the loader
        from nope_amd import poses
        for b in range(B):
            want = poses.all_relative_poses(T[0], P[b, 0]).numpy()
            assert ulp_apart(grel[b, 0], want) <= 1


def test_prepare_per_sample_grid_and_optional_outputs(be):
    hip, dev, _ = be
    B, R, N = 2, 3, 26
    T = np.stack([grid(0), haar(N, 5)])                        # one grid per sample
    P = haar(B * R, 6).reshape(B, R, 3, 3)
    got = hip.op_multiref_prepare(torch.from_numpy(T).float().to(dev), torch.from_numpy(P).to(dev), weighting="softmax", tau_deg=20.0,
                                  dist_kind=hip.C2F_VIEWPOINT, want_rel=False)
    assert got.all_relativeR is None and got.dist is None
    _, w, _, _ = np_prepare(T.astype(np.float32).astype(np.float64), P, None, "softmax", math.radians(20.0), 1)      # (any float dtype: converted to f64)
    assert close(got.weights.cpu().numpy(), w)
    again = hip.op_multiref_prepare(torch.from_numpy(T).float().to(dev), torch.from_numpy(P).to(dev), weighting="softmax", tau_deg=20.0,
                                    dist_kind=hip.C2F_VIEWPOINT, want_rel=False)
    assert got.weights.cpu().numpy().tobytes() == again.weights.cpu().numpy().tobytes()                             # run to run


def test_prepare_nearest_tie(be):
    """Two identical reference poses: an exact tie, which goes to the lower r."""
    hip, dev, _ = be
    T, P = _prepare_inputs(0, 3, B=2)
    P = P.copy()
    P[0, 2] = P[0, 0]
    P[1, 2] = P[1, 1]
    for kind in (0, 1):
        got = hip.op_multiref_prepare(torch.from_numpy(T.copy()).to(dev), torch.from_numpy(P).to(dev), weighting="nearest", dist_kind=kind, want_dist=True)
        w, d = got.weights.cpu().numpy(), got.dist.cpu().numpy()
        assert np.array_equal(d[0, 2], d[0, 0]) and np.array_equal(d[1, 2], d[1, 1])
        assert (w[:, 2] == 0).all() and (w.sum(axis=1) == 1).all()
        assert (w[0, 0] == 1).any() and (w[1, 1] == 1).any()                  # the tied pair does win somewhere: at its lower r
        _, want, _, _ = np_prepare(T, P, None, "nearest", 1.0, kind)
        assert np.array_equal(w, want.astype(np.float32))


def test_prepare_status(be):
    hip, dev, _ = be
    T, P = _prepare_inputs(0, 3)
    Td = torch.from_numpy(T.copy()).to(dev)
    bad = P.copy()
    bad[1, 1, 2, 0] = np.nan
    for weighting in WEIGHTINGS:
        got = hip.op_multiref_prepare(Td, torch.from_numpy(bad).to(dev), weighting=weighting)
        clean = hip.op_multiref_prepare(Td, torch.from_numpy(P).to(dev), weighting=weighting)
        w = got.weights.cpu().numpy()
        assert int(got.status) == hip.MULTIREF_BAD_POSE and np.isnan(w[1]).all()
        for b in (0, 2):                                                      # that sample only
            assert w[b].tobytes() == clean.weights[b].cpu().numpy().tobytes()
            assert got.all_relativeR[b].cpu().numpy().tobytes() == clean.all_relativeR[b].cpu().numpy().tobytes()
    # the NaN sits in a PADDED reference: not an error
    got = hip.op_multiref_prepare(Td, torch.from_numpy(bad).to(dev), torch.tensor([3, 1, 3]), weighting="uniform")
    assert int(got.status) == 0 and bool((got.weights[1, 0] == 1).all()) and bool((got.weights[1, 1:] == 0).all())
    bad[1, 1, 2, 0] = np.inf
    assert int(hip.op_multiref_prepare(Td, torch.from_numpy(bad).to(dev), weighting="nearest").status) == hip.MULTIREF_BAD_POSE
    for count in (0, 4, -1):
        got = hip.op_multiref_prepare(Td, torch.from_numpy(P).to(dev), torch.tensor([3, 2, count]), weighting="softmax")
        w = got.weights.cpu().numpy()
        assert int(got.status) == hip.MULTIREF_BAD_COUNT and np.isnan(w[2]).all() and np.isfinite(w[:2]).all(), count
        assert bool(torch.isfinite(got.all_relativeR).all())
    got = hip.op_multiref_prepare(Td, torch.from_numpy(bad).to(dev), torch.tensor([3, 3, 0]), weighting="softmax")
    assert int(got.status) == hip.MULTIREF_BAD_POSE | hip.MULTIREF_BAD_COUNT
    # the fused row of such a sample is NaN and ranks first
    per_ref = torch.zeros(3, 3, 26).to(dev)
    fused = hip.op_multiref_fuse_scores(per_ref, got.weights)
    assert bool(fused[1].isnan().all()) and bool(fused[2].isnan().all()) and bool(torch.isfinite(fused[0]).all())


BAD_PREPARE = [dict(R=0), dict(R=9), dict(N=0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=0.0), dict(tau=-1.0), dict(weighting=3),
               dict(weighting=-1), dict(kind=2), dict(kind=-1), dict(no="poses"), dict(no="refs"), dict(no="weights"), dict(no="status")]


@pytest.mark.parametrize("bad", BAD_PREPARE, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_prepare_bad_arguments(be, bad):
    """NOPE_ERR_ARG, and nothing written: the outputs hold a sentinel afterwards."""
    hip, dev, _ = be
    B, R, N = 2, 3, 26
    T = torch.from_numpy(grid(0).copy())[None].to(dev)
    P = torch.from_numpy(haar(B * 9, 3).reshape(B, 9, 3, 3)).to(dev)          # (room for R = 9)
    out = hip.MultiRefPrep(torch.full((B, 9, N, 6), 7.0, device=dev), torch.full((B, 9, N), 7.0, device=dev),
                           torch.full((B, 9, N), 7.0, dtype=torch.float64, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev))
    kw = dict(R=R, N=N, tau=0.5, weighting=1, kind=0)
    kw.update({k: v for k, v in bad.items() if k != "no"})
    ptr = dict(poses=T.data_ptr(), refs=P.data_ptr(), weights=out.weights.data_ptr(), status=out.status.data_ptr())
    if "no" in bad:
        ptr[bad["no"]] = None
    l = hip.lib()
    code = l.dll.nope_op_multiref_prepare(ptr["poses"], 0, kw["N"], ptr["refs"], kw["R"], None, kw["weighting"], kw["tau"], kw["kind"],
                                          out.all_relativeR.data_ptr(), ptr["weights"], out.dist.data_ptr(), ptr["status"], B, 0)
    assert code == -1, code
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):
        l.check(code, "nope_op_multiref_prepare")
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)
    if "tau" in bad:                                                           # tau is read under softmax only
        ok = hip._multiref_prepare_call(T, 0, N, P[:, :R].contiguous(), R, None, 0, kw["tau"], 0, out)
        assert int(ok.status) == 0 and bool((ok.weights.view(-1)[:B * R * N] == np.float32(1.0 / 3)).all())
    elif "no" not in bad and "R" not in bad and "N" not in bad:
        with pytest.raises(hip.NopeError, match=r"\(-1\)"):                    # the same through the binding
            hip._multiref_prepare_call(T, 0, N, P[:, :R].contiguous(), R, None, kw["weighting"], kw["tau"], kw["kind"], out)


def test_prepare_shape_errors(be):
    hip, dev, _ = be
    T = torch.from_numpy(grid(0).copy())[None].to(dev)
    P = torch.from_numpy(haar(6, 3).reshape(2, 3, 3, 3)).to(dev)
    for args, kw in (((T[0], P), {}), ((T.repeat(3, 1, 1, 1), P), {}), ((T, P[0]), {}), ((T, P, torch.zeros(3)), {}), ((T, P), dict(weighting="best"))):
        with pytest.raises(hip.NopeError):
            hip.op_multiref_prepare(*args, **kw)


# ---- 2. fused scoring, exact arithmetic -----------------------------------------------------------------------------------------------------
# weight patterns (they sum to 1) per R; the solver is a reference with the smallest non-zero weight: its d makes the fused difference D
PATTERNS = {1: [(1.0,)], 2: [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)], 3: [(0.5, 0.25, 0.25), (0.0, 0.5, 0.5), (0.25, 0.5, 0.25), (0.0, 0.0, 1.0), (0.5, 0.5, 0.0), (1.0, 0.0, 0.0)],
            8: [(0.25, 0.25, 0.25, 0.25, 0, 0, 0, 0), (0, 0.5, 0, 0.25, 0, 0, 0.25, 0), (0, 0, 0, 0, 0.5, 0, 0, 0.5), (0.25, 0, 0.25, 0, 0.25, 0, 0.25, 0)]}
_CASES = {}


def _hw(HW):
    return (HW // 4, 4) if HW % 4 == 0 else (1, HW)


def exact_case(seed, dt, B, R, N, C, HW, dead_last=False):
    """q (B, C, h, w) f32, integer-valued in [-64, 64]; bank (B, R, N, C, h, w) of type dt: t[r] = q except in one channel per pixel, where it is
    q + d_r, d_r a multiple of 4; weights (B, R, N) from {0, 1/4, 1/2, 1} summing to 1; the f64 scores (B, N) as f32.  The fused difference
    D = sum_r w_r d_r is planted per pixel: in {0, +-1, +-2, +-4} (16-bit banks) or [-8, 8] (f32), as far as the pattern's smallest weight allows
    (w = 1: multiples of 4, w = 1/2: even).  Template N // 2 of the last sample is a match that exists only in the blend (R >= 2: d = (+4, -4)
    under w = (1/2, 1/2)).  dead_last: the last reference has weight 0 everywhere (R >= 2)."""
    key = (seed, dt, B, R, N, C, HW, dead_last)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(seed)
    pats = [p for p in PATTERNS[R] if not (dead_last and p[-1] != 0)] if R > 1 else PATTERNS[1]
    pat = torch.tensor(pats, dtype=torch.float64)[torch.randint(0, len(pats), (B, N), generator=g)]          # (B, N, R)
    blend_only = R >= 2 and not (dead_last and R == 2)          # (R = 2 with a dead last reference: an ordinary match in reference 0)
    if blend_only:
        pat[B - 1, N // 2] = torch.tensor([0.5, 0.5] + [0.0] * (R - 2), dtype=torch.float64)
    wmin = torch.where(pat > 0, pat, torch.full_like(pat, 2.0)).min(dim=2)
    solver, smallest = wmin.indices, wmin.values                                                            # (B, N)
    allowed = (-4, -2, -1, 0, 1, 2, 4) if dt != "f32" else tuple(range(-8, 9))
    D = torch.tensor(allowed, dtype=torch.float64)[torch.randint(0, len(allowed), (B, N, HW), generator=g)]
    step = (1.0 / smallest)[..., None]                                                                      # D must be a multiple of 4 w_solver
    D = torch.where(step == 1, (D / 4).round() * 4, torch.where(step == 2, (D / 2).round() * 2, D))
    D[B - 1, N // 2] = 0
    d = torch.randint(-4, 5, (B, N, R, HW), generator=g).double() * 4
    if blend_only:
        d[B - 1, N // 2, 0], d[B - 1, N // 2, 1] = 4.0, -4.0
    is_solver = torch.nn.functional.one_hot(solver, R).bool()[..., None]                                    # (B, N, R, 1)
    others = (pat[..., None] * d).masked_fill(is_solver, 0.0).sum(dim=2)                                    # (B, N, HW)
    d_solver = (D - others) / smallest[..., None]
    d = torch.where(is_solver, d_solver[:, :, None, :], d)
    if blend_only:
        assert float(d[B - 1, N // 2, 0, 0]) == 4.0 and float(d[B - 1, N // 2, 1, 0]) == -4.0
    assert bool((d % 4 == 0).all()) and float(d.abs().max()) <= 112 and torch.equal((pat[..., None] * d).sum(dim=2), D)
    q = torch.randint(-64, 65, (B, C, HW), generator=g).float()
    ch = torch.randint(0, C, (B, 1, N, 1, HW), generator=g).expand(B, R, N, 1, HW)
    bank = q[:, None, None].repeat(1, R, N, 1, 1)
    bank.scatter_add_(3, ch, d.permute(0, 2, 1, 3)[:, :, :, None, :].float())
    h, w = _hw(HW)
    q, bank = q.reshape(B, C, h, w), bank.reshape(B, R, N, C, h, w).to(DT[dt])
    assert torch.equal(bank.float().to(DT[dt]), bank) and float(bank.float().abs().max()) <= 256
    weights = pat.permute(0, 2, 1).float().contiguous()
    want64 = np_fused_scores(q, bank, weights)
    assert np.array_equal(want64, -(D.numpy() ** 2).sum(axis=2))                                           # the restatement is exact on this data
    want = torch.from_numpy(want64).float()
    assert bits(want)[B - 1, N // 2] == bits(torch.tensor([-0.0]))[0] and int((want[B - 1] == 0).sum()) == 1
    _CASES[key] = q, bank, weights, want
    return _CASES[key]


_LINE = re.compile(r"mrsim (reg|lds) (\w+) LV (\d+) CMAX (\d+) RT (\d+) R (\d+) P (\d+) hpi (\d+) groups (\d+) nsplit (\d+)$")
_FIELDS = ("form", "dt", "LV", "CMAX", "RT", "R", "P", "hpi", "groups", "nsplit")


def traced(capfd, fn):
    """fn() and the fields of the ONE NOPE_SIM_TRACE line it printed."""
    capfd.readouterr()
    out = fn()
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("mrsim ")]
    assert len(lines) == 1, lines
    m = _LINE.match(lines[0])
    assert m, lines[0]
    return out, {k: (v if k in ("form", "dt") else int(v)) for k, v in zip(_FIELDS, m.groups())}


def want_line(dt, B, R, N, C, HW, mingroups=1):
    """The dispatch of launch_multiref_similarity: nope_similarity's forms and grid."""
    lv = 4 if dt == "f32" else 8
    P = HW // lv
    if P <= NT and NT % P == 0 and C <= 16:
        hpi = NT // P
        groups = -(-N // hpi)
        return dict(form="reg", dt=dt, LV=lv, CMAX=8 if C <= 8 else 16, RT={1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8), R=R, P=P, hpi=hpi, groups=groups,
                    nsplit=max(1, min(4096 // B, groups // mingroups, groups)))
    return dict(form="lds", dt=dt, LV=lv, CMAX=0, RT=0, R=R, P=P, hpi=1, groups=N, nsplit=min(-(-4096 // B), N))


def run_exact(be, monkeypatch, capfd, dt, B, R, N, C, HW, seed, mingroups=None):
    hip, dev, _ = be
    q, bank, weights, want = exact_case(seed, dt, B, R, N, C, HW)
    monkeypatch.setenv("NOPE_SIM_TRACE", "1")
    if mingroups is None:
        monkeypatch.delenv("NOPE_SIM_MINGROUPS", raising=False)
    else:
        monkeypatch.setenv("NOPE_SIM_MINGROUPS", str(mingroups))
    got, line = traced(capfd, lambda: hip.multiref_similarity(q.to(dev), bank.to(dev), weights.to(dev)))
    assert line == want_line(dt, B, R, N, C, HW, mingroups or 1), line
    what = (dt, B, R, N, C, HW, mingroups, line)
    assert same_bits(got, want), (what, (bits(got.cpu()) != bits(want)).nonzero()[:4].tolist())
    assert bits(got)[B - 1, N // 2] == bits(torch.tensor([-0.0]))[0], what              # the match that exists only in the blend: -0.0
    assert int(hip.topk(got, 1)[1][B - 1, 0]) == N // 2, what
    if R >= 2:                                                                          # ... and in no single reference: scoring per reference and averaging fails
        per_ref = hip.similarity(q.to(dev), bank.view(B, R * N, *bank.shape[3:]).to(dev)).view(B, R, N)
        late = hip.op_multiref_fuse_scores(per_ref, weights.to(dev))
        assert float(late[B - 1, N // 2]) == -16.0 * HW and float(per_ref[B - 1, 0, N // 2]) == -16.0 * HW, what
    return line


# (C, HW, N): the smallest shapes that reach each form -- per bank type the lane count P = HW / (4 | 8) decides
SHAPES = [(8, 64, 37), (8, 256, 11), (8, 1024, 5), (5, 64, 37), (12, 64, 37), (8, 144, 7), (20, 64, 7)]


# every R on the channel forms (the slot blocks depend on both C and R); R = 2 and 3 on every shape
FORM_CASES = [(c, hw, n, r) for c, hw, n in SHAPES for r in (1, 2, 3, 8) if r in (2, 3) or (c, hw) in ((8, 64), (5, 64), (12, 64))]


@pytest.mark.parametrize("C,HW,N,R", FORM_CASES, ids=[f"C{c}_HW{hw}_N{n}_R{r}" for c, hw, n, r in FORM_CASES])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_exact_forms(be, monkeypatch, capfd, dt, C, HW, N, R):
    line = run_exact(be, monkeypatch, capfd, dt, 2, R, N, C, HW, seed=1000 + 7 * R + C + HW)
    assert line["form"] == ("lds" if HW == 144 or C == 20 else "reg")


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_exact_several_groups_per_workgroup(be, monkeypatch, capfd, dt, R):
    """NOPE_SIM_MINGROUPS = 3: a workgroup walks four (or three) groups -- the prefetch of group g + nsplit, the peeled last group, the
    double-buffered partials -- and the last group is ragged."""
    hpi = 16 if dt == "f32" else 32
    line = run_exact(be, monkeypatch, capfd, dt, 2, R, 7 * hpi + 5, 8, 64, seed=2000 + R, mingroups=3)
    assert line["groups"] == 8 and line["nsplit"] == 2
    line = run_exact(be, monkeypatch, capfd, dt, 1, R, 5 * (NT // (512 // (4 if dt == "f32" else 8))) + 1, 8, 512, seed=2100 + R, mingroups=3)
    assert line["groups"] == 6 and line["nsplit"] == 2 and line["P"] >= 64


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_unsupported_shapes(be, dt):
    hip, dev, _ = be
    q = torch.zeros(1, 17, 32, 32)
    bank = torch.zeros(1, 1, 1, 17, 32, 32, dtype=DT[dt])
    with pytest.raises(hip.NopeError, match=r"\(-2\)|unsupported|not supported"):
        hip.multiref_similarity(q.to(dev), bank.to(dev), torch.ones(1, 1, 1).to(dev))
    vec = 4 if dt == "f32" else 8
    q = torch.zeros(1, 8, 1, vec + 2)
    with pytest.raises(hip.NopeError):
        hip.multiref_similarity(q.to(dev), torch.zeros(1, 2, 3, 8, 1, vec + 2, dtype=DT[dt]).to(dev), torch.ones(1, 2, 3).to(dev))
    q = torch.zeros(1, 8, 8, 8)
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):                          # R = 9
        hip.multiref_similarity(q.to(dev), torch.zeros(1, 9, 2, 8, 8, 8, dtype=DT[dt]).to(dev), torch.ones(1, 9, 2).to(dev))
    with pytest.raises(hip.NopeError):                                           # weights of another shape
        hip.multiref_similarity(q.to(dev), torch.zeros(1, 2, 3, 8, 8, 8, dtype=DT[dt]).to(dev), torch.ones(1, 3, 2).to(dev))


PROBE_W = {1: (1.0,), 2: (0.5, 0.5), 3: (0.5, 0.25, 0.25), 8: (0.25, 0.25, 0.25, 0.25, 0.0, 0.0, 0.0, 0.0)}


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("C,HW", [(8, 64), (12, 64), (8, 256), (8, 144)])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_one_element_probes(be, dt, C, HW, R):
    """Template n differs from q in ONE element of reference n mod R only, by 4: the score is -(4 w[n mod R])^2, -0.0 under a zero weight.  A
    kernel that drops, swaps or double-counts a (reference, channel, lane, word, half-word) position fails on exactly that column."""
    hip, dev, _ = be
    E = C * HW
    N = min(E, 256)
    g = torch.Generator().manual_seed(31 + R)
    q = torch.randint(-64, 65, (1, E), generator=g).float()
    bank = q[:, None, None].repeat(1, R, N, 1)
    n = torch.arange(N)
    elem = (n * (E // N) + n // 7) % E                          # spread over the channels, lanes and words
    bank[0, n % R, n, elem] += 4.0
    w = torch.tensor(PROBE_W[R])
    weights = w[None, :, None].repeat(1, 1, N).contiguous()
    h, wd = _hw(HW)
    got = hip.multiref_similarity(q.reshape(1, C, h, wd).to(dev), bank.reshape(1, R, N, C, h, wd).to(DT[dt]).to(dev), weights.to(dev))
    want = -((4.0 * w[n % R]) ** 2)[None]
    assert same_bits(got, want), (bits(got.cpu()) != bits(want)).nonzero()[:4].tolist()
    if R == 8:
        assert int((bits(got) == bits(torch.tensor([-0.0]))[0]).sum()) == N // 2


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("C,HW", [(8, 64), (12, 64), (8, 144)])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_zero_weight_reference_is_not_read(be, dt, C, HW, fill):
    """A reference bank full of NaN / inf under weight 0 leaves every score's bits alone; so does one zero-weight (b, r, n) plane."""
    hip, dev, _ = be
    for R in (2, 3, 8):
        q, bank, weights, want = exact_case(3000 + R, dt, 2, R, 21, C, HW, dead_last=True)
        assert bool((weights[:, R - 1] == 0).all())
        poisoned = bank.clone()
        poisoned[:, R - 1] = fill
        zero = (weights == 0)[..., None, None, None].expand_as(bank)
        scattered = torch.where(zero, torch.full_like(bank, fill), bank)         # every zero-weight plane, wherever it sits
        for bk in (poisoned, scattered):
            got = hip.multiref_similarity(q.to(dev), bk.to(dev), weights.to(dev))
            assert same_bits(got, want), (dt, C, HW, R, fill)


@pytest.mark.parametrize("C,HW", [(8, 64), (8, 144)])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_nan_weight_is_not_zero(be, dt, C, HW):
    hip, dev, _ = be
    for R in (1, 3):
        q, bank, weights, want = exact_case(3100 + R, dt, 2, R, 21, C, HW)
        weights = weights.clone()
        weights[1, R - 1, 13] = float("nan")
        want = want.clone()
        want[1, 13] = float("nan")
        got = hip.multiref_similarity(q.to(dev), bank.to(dev), weights.to(dev))
        assert same_bits(got, want) and int(got.isnan().sum()) == 1                # exactly that column
        assert int(hip.topk(got, 1)[1][1, 0]) == 13                                # visible: it ranks first


def test_similarity_out_and_ld(be):
    hip, dev, _ = be
    q, bank, weights, want = exact_case(3200, "f32", 2, 3, 21, 8, 64)
    out = torch.full((2, 30), 7.0).to(dev)
    got = hip.multiref_similarity(q.to(dev), bank.to(dev), weights.to(dev), out=out)
    assert got is out and same_bits(out[:, :21], want) and bool((out[:, 21:] == 7).all())


# ---- 3. fused scoring, random data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,HW", [(8, 64), (8, 144)])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_random_data(be, dt, C, HW):
    hip, dev, _ = be
    B, R, N = 2, 4, 19
    g = torch.Generator().manual_seed(41)
    h, w = _hw(HW)
    q = torch.randn(B, C, h, w, generator=g)
    bank = torch.randn(B, R, N, C, h, w, generator=g).to(DT[dt])
    T = haar(N, 42)[None]
    P = haar(B * R, 43).reshape(B, R, 3, 3)
    weights = hip.op_multiref_prepare(torch.from_numpy(T).to(dev), torch.from_numpy(P).to(dev), torch.tensor([4, 3]), weighting="softmax", tau_deg=30.0).weights
    assert close(weights.cpu().numpy(), np_prepare(T, P, [4, 3], "softmax", math.radians(30.0), 0)[1])
    got = hip.multiref_similarity(q.to(dev), bank.to(dev), weights).cpu().double().numpy()
    want = np_fused_scores(q, bank, weights.cpu())
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"multiref_similarity {dt} C {C} HW {HW}: relative error {err:.3e}")
    assert err <= 2e-5, err


@pytest.mark.parametrize("C,HW", [(8, 64), (12, 64), (8, 1024), (8, 144)])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_identical_banks_equal_single_reference(be, dt, C, HW):
    """R identical banks under uniform weights 1 / R (R = 2, 4: exact in f32) are the R = 1 call bit for bit, and R = 1 with weight 1 ranks as nope_similarity."""
    hip, dev, _ = be
    B, N = 2, 19
    g = torch.Generator().manual_seed(51)
    h, w = _hw(HW)
    q = torch.randn(B, C, h, w, generator=g).to(dev)
    one = torch.randn(B, 1, N, C, h, w, generator=g).to(DT[dt]).to(dev)
    base = hip.multiref_similarity(q, one, torch.ones(B, 1, N).to(dev))
    plain = hip.similarity(q, one[:, 0])                       # the same definition from another kernel: equal to rounding (1 ulp seen on the device)
    assert float((base - plain).abs().max() / plain.abs().max()) <= 2e-5 and torch.equal(hip.topk(base, 5)[1], hip.topk(plain, 5)[1])
    for R in (2, 4):
        got = hip.multiref_similarity(q, one.repeat(1, R, 1, 1, 1, 1), torch.full((B, R, N), 1.0 / R).to(dev))
        assert same_bits(got, base), (dt, C, HW, R)


# ---- 4. late fusion -------------------------------------------------------------------------------------------------------------------------
def test_fuse_scores(be):
    hip, dev, _ = be
    B, R, N = 3, 8, 300                                        # more than one workgroup per row
    g = torch.Generator().manual_seed(61)
    s = -torch.randint(0, 1 << 16, (B, R, N), generator=g).float()          # (sums below 2^19 with three fraction bits: exact in f32)
    w = torch.tensor([0.0, 0.125, 0.25, 0.5, 1.0])[torch.randint(0, 5, (B, R, N), generator=g)]
    want = (w.double() * s.double()).sum(dim=1)
    assert torch.equal(want.float().double(), want)            # exact on this data
    s[0, 2, 5], w[0, 2, 5] = float("-inf"), 0.0                # ignored under a zero weight ...
    s[1, 0, 7], w[1, 0, 7] = float("nan"), 0.0
    s[0, 3, 9], w[0, 3, 9] = float("inf"), 0.0
    want[0, 5], want[1, 7], want[0, 9] = [(w[b, :, n].double() * torch.nan_to_num(s[b, :, n], 0.0, 0.0, 0.0).double()).sum() for b, n in ((0, 5), (1, 7), (0, 9))]
    s[2, 1, 11], w[2, 1, 11] = float("-inf"), 0.5              # ... and propagated under a non-zero one
    s[2, 4, 12], w[2, 4, 12] = float("nan"), 0.25
    w[1, 6, 13] = float("nan")
    want[2, 11], want[2, 12], want[1, 13] = float("-inf"), float("nan"), float("nan")
    out = torch.full((B, N + 9), 7.0).to(dev)
    got = hip.op_multiref_fuse_scores(s.to(dev), w.to(dev), out=out)
    assert got is out and same_bits(out[:, :N], want.float()) and bool((out[:, N:] == 7).all())
    assert same_bits(hip.op_multiref_fuse_scores(s.to(dev), w.to(dev)), want.float())
    one = hip.op_multiref_fuse_scores(s[:, :1].contiguous().to(dev), torch.ones(B, 1, N).to(dev))
    assert same_bits(one, s[:, 0])
    for args in ((s[0], w[0]), (s, w[:, :2])):
        with pytest.raises(hip.NopeError):
            hip.op_multiref_fuse_scores(args[0].to(dev), args[1].to(dev))
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):        # R = 9
        hip.op_multiref_fuse_scores(torch.zeros(1, 9, 4).to(dev), torch.zeros(1, 9, 4).to(dev))


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
SMOKE_BOUNDS = {"f32": 1e-6, "f16x2": 1e-5, "bf16x3": 5e-6, "f16": 3e-4, "bf16": 2e-3}       # __graft_entry__.smoke's score bounds
_E2E = {}


def _memoize(fn):
    """The interpreter needs many seconds per U-Net pass: on that backend a call with inputs it has seen returns the first result again (the
    network is a pure function of them).  The device runs everything."""
    kept = {}

    def wrapped(*a):
        key = tuple(t.detach().cpu().numpy().tobytes() for t in a)
        if key not in kept:
            kept[key] = fn(*a)
        return kept[key]
    return wrapped


def _e2e(dev, name, cdt="f32"):
    """smoke()'s tiny network (u_net_dim 32 around a StubEncoder(8), 16 x 16 maps) and a batch with B = 2, R = 3, N = 6; built once per backend and mode."""
    if (name, cdt) in _E2E:
        return _E2E[(name, cdt)]
    from nope_amd import harness
    from nope_amd.model import PoseConditional
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    B, R, N = 2, 3, 6
    u = UNet(u_net_dim=32, rot_representation_dim=6, encoder=harness.StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
    synth_init_(u, 2022)
    sd = {k: v.clone() for k, v in u.own_state_dict().items()}
    model = PoseConditional(u, None, {"similarity_metric": "l2"}, None).to(dev)
    batch = harness.synthetic_batch(B, N, 16, seed=9, device="cpu", n_references=R)
    g = torch.Generator().manual_seed(9)
    batch["query"] = torch.randn(B, 8, 16, 16, generator=g)
    batch["references"] = torch.randn(B, R, 8, 16, 16, generator=g)
    batch["reference"] = batch["references"][:, 0].contiguous()
    if name == "emu":
        model._generate_templates_from_feat = _memoize(model._generate_templates_from_feat)
        model.forward = _memoize(model.forward)
    _E2E[(name, cdt)] = model, sd, {k: v.to(dev) for k, v in batch.items()}
    return _E2E[(name, cdt)]


E2E_CASES = [pytest.param("emu", "f32")] + [pytest.param("gpu", c, marks=pytest.mark.gpu) for c in SMOKE_BOUNDS]      # the interpreter runs the f32 mode


@pytest.mark.parametrize("backend,cdt", E2E_CASES)
def test_e2e_retrieve_multi(request, monkeypatch, backend, cdt):
    from oracle import nope_ref
    hip, dev, name = request.getfixturevalue(backend), ("cuda" if backend == "gpu" else "cpu"), backend
    if cdt == "f16x2":
        monkeypatch.setenv("NOPE_CONV_PP", "11")             # as smoke(): a dozen hypotheses would not reach the ping-pong kernels otherwise
    model, sd, b = _e2e(dev, name, cdt)
    B, R, N = 2, 3, 6
    q, refs, P, T = b["query"], b["references"], b["reference_poses"], b["template_poses"][:1]
    n_refs = torch.tensor([3, 2])
    want_bank = None
    if cdt == "f16x2":                                       # the handle re-centres its layers' range shifts after the first passes, and a re-centred
        for _ in range(4):                                   # layer rounds differently: compare passes of the settled handle
            model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs)
    for fusion in ("feature", "score"):
        for weighting in ("softmax", "nearest"):
            res = model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, fusion=fusion, weighting=weighting, tau_deg=40.0, return_per_reference=True)
            # the hand composition, bit for bit
            prep = hip.op_multiref_prepare(T, P, n_refs, weighting=weighting, tau_deg=40.0)
            bank = model.generate_templates_from_feat(refs.reshape(B * R, 8, 16, 16), prep.all_relativeR.reshape(B * R, N, 6)).view(B, R, N, 8, 16, 16)
            per_ref = hip.similarity(q, bank.view(B, R * N, 8, 16, 16)).view(B, R, N)
            sim = hip.multiref_similarity(q, bank, prep.weights) if fusion == "feature" else hip.op_multiref_fuse_scores(per_ref, prep.weights)
            _, idx = hip.topk(sim, 5)
            assert torch.equal(res.bank, bank) and same_bits(res.similarity, sim) and torch.equal(res.nearest_idx, idx)
            assert same_bits(res.per_reference, per_ref) and same_bits(res.weights, prep.weights)
            assert bool((res.weights[1, 2] == 0).all()) and bool(torch.isfinite(res.similarity).all())
            # the oracle: a bank per reference, a NumPy blend, similarity_scores
            if want_bank is None:                 # (the relative poses do not depend on the weighting: one oracle bank)
                want_bank = nope_ref.generate_templates(sd, refs.cpu().reshape(B * R, 8, 16, 16), prep.all_relativeR.cpu().reshape(B * R, N, 6)).view(B, R, N, 8, 16, 16)
            w64 = prep.weights.cpu().double()
            if fusion == "feature":
                blend = (w64[..., None, None, None] * want_bank.double()).sum(dim=1)
                want = nope_ref.similarity_scores(q.cpu().double(), blend)
            else:
                want = (w64 * nope_ref.similarity_scores(q.cpu().double(), want_bank.double().view(B, R * N, 8, 16, 16)).view(B, R, N)).sum(dim=1)
            err = float((res.similarity.cpu().double() - want).abs().max() / want.abs().max())
            print(f"retrieve_multi[{cdt}, {fusion}, {weighting}]: score rel err {err:.2e}")
            assert err < SMOKE_BOUNDS[cdt], (cdt, fusion, weighting, err)
    assert model.retrieve_multi_from_feat(q, refs, P, T, return_per_reference=False).per_reference is None
    # R = 1 with weight 1: the single-reference path on the same bank
    sim1, idx1 = model.retrieval_from_feat(q, res.bank[:, 0])
    fused1 = hip.multiref_similarity(q, res.bank[:, :1], torch.ones(B, 1, N).to(dev))
    assert torch.equal(hip.topk(fused1, 5)[1], idx1) and float((fused1 - sim1).abs().max() / sim1.abs().max()) <= 2e-5
    if name == "gpu":                                    # ... and through the driver (one more U-Net pass: the device only)
        one = model.retrieve_multi_from_feat(q, refs[:, :1], P[:, :1], T, weighting="uniform")
        assert bool((one.weights == 1).all())
        sim1, idx1 = model.retrieval_from_feat(q, one.bank[:, 0])
        assert torch.equal(one.nearest_idx, idx1) and float((one.similarity - sim1).abs().max() / sim1.abs().max()) <= 2e-5
    with pytest.raises(ValueError):
        model.retrieve_multi_from_feat(q, refs, P, T, fusion="both")


def test_e2e_predict_pose_multi(be):
    hip, dev, name = be
    model, _, b = _e2e(dev, name)
    q, refs, P, T = b["query"], b["references"], b["reference_poses"], b["template_poses"][:1]
    res = model.retrieve_multi(q, refs, P, T)                                       # (the StubEncoder hands the embeddings through)
    same = model.retrieve_multi_from_feat(q, refs, P, T)
    assert same_bits(res.similarity, same.similarity) and torch.equal(res.nearest_idx, same.nearest_idx)
    pred, score = model.predict_pose_multi(q, refs, P, T)
    assert tuple(pred.shape) == (2, 5, 3, 3) and pred.dtype == torch.float64
    assert torch.equal(pred, T.to(pred.device)[0, res.nearest_idx]) and torch.equal(score, torch.gather(res.similarity, 1, res.nearest_idx))
    assert torch.equal(pred[:, 0], T.to(pred.device)[0, res.nearest_idx[:, 0]])
    sym = torch.tensor([0, 2])
    pred_d, score_d = model.predict_pose_multi(q, refs, P, T, distinct_deg=60.0, symmetry=sym, temperature=20.0)
    modes = hip.op_pose_modes(res.similarity, T, sym, temperature=20.0, radius_deg=60.0, max_modes=5, fill=True)
    assert torch.equal(pred_d, T.to(pred.device)[0, modes.idx]) and torch.equal(score_d, torch.gather(res.similarity, 1, modes.idx))
    assert torch.equal(score_d[:, 0], score[:, 0])                                  # the first seed is the top-1
    dist = model.pose_distribution(res.similarity, T, sym, temperature=20.0, radius_deg=60.0)
    assert torch.equal(dist.idx[:, 0], modes.idx[:, 0])
    model.template_parallel = True
    try:
        from nope_amd import dist as ndist
        world = ndist.world
        ndist.world = lambda: (0, 2)
        for call in (lambda: model.retrieve_multi(q, refs, P, T), lambda: model.retrieve_multi_from_feat(q, refs, P, T),
                     lambda: model.generate_templates_multi_from_feat(refs, torch.zeros(2, 3, 6, 6)), lambda: model.predict_pose_multi(q, refs, P, T)):
            with pytest.raises(NotImplementedError):
                call()
    finally:
        ndist.world = world
        model.template_parallel = False


def test_e2e_eval_geodesic(be, tmp_path):
    from nope_amd import harness
    from nope_amd.metrics import GeodesicError
    hip, dev, name = be
    model, _, b = _e2e(dev, name)
    sim_a, idx_a, res_a = harness.eval_geodesic(model, b, save_path=str(tmp_path / "a"))
    kw = dict(fusion="score", weighting="softmax", tau_deg=40.0)
    sim_b, idx_b, res = harness.eval_geodesic(model, b, save_path=str(tmp_path / "b"), multi_ref=kw)
    assert same_bits(sim_a, sim_b) and torch.equal(idx_a, idx_b)
    assert {k: v for k, v in res.items() if not k.startswith("multi/")} == res_a                     # the old keys, the old values
    mr = model.retrieve_multi(b["query"], b["references"], b["reference_poses"], b["template_poses"][:1], **kw)
    _, metric = GeodesicError([15, 30]).from_indices(b["template_poses"][:1], mr.nearest_idx, b["query_pose"], b["symmetry"])
    assert sorted(k[len("multi/"):] for k in res if k.startswith("multi/")) == sorted(list(metric) + ["top1_agree"])
    for k, v in metric.items():
        assert res[f"multi/{k}"] == float(v), k
    assert res["multi/top1_agree"] == float((mr.nearest_idx[:, 0] == idx_a[:, 0]).float().mean())
    za, zb = np.load(str(tmp_path / "a.npz")), np.load(str(tmp_path / "b.npz"))
    assert sorted(set(zb.files) - set(za.files)) == ["multi_similarity"] and all(za[f].tobytes() == zb[f].tobytes() for f in za.files)
    assert zb["multi_similarity"].tobytes() == mr.similarity.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        harness.eval_geodesic(model, {k: v for k, v in b.items() if k != "references"}, multi_ref={})


def test_synthetic_batch_references():
    from nope_amd import harness
    for kw in (dict(), dict(pose_level=0), dict(gt_templates=True)):
        a = harness.synthetic_batch(2, 7, 16, seed=4, **kw)
        b = harness.synthetic_batch(2, 7, 16, seed=4, n_references=3, **kw)
        assert set(b) == set(a) and tuple(b["references"].shape) == (2, 3, 3, 16, 16) and tuple(b["reference_poses"].shape) == (2, 3, 3, 3)
        assert tuple(a["references"].shape) == (2, 1, 3, 16, 16)
        for k in a:
            if k not in ("references", "reference_poses"):
                assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), k                            # every existing tensor keeps its bits
        assert torch.equal(b["references"][:, 0], b["reference"]) and torch.equal(a["references"][:, 0], a["reference"])
        assert torch.equal(b["reference_poses"][:, 0], a["reference_poses"][:, 0])
        # index 0 is the pose all_relativeR was made from, and the extras are rotations
        P = b["reference_poses"]
        rel = (b["template_poses"][:, :, None] @ P[:, None, :1].transpose(-1, -2))[:, :, 0, :2].reshape(2, -1, 6).float()
        assert float((rel - b["all_relativeR"]).abs().max()) <= 1e-6
        eye = torch.eye(3, dtype=torch.float64)
        assert float((P @ P.transpose(-1, -2) - eye).abs().max()) <= 1e-12 and float((torch.linalg.det(P) - 1).abs().max()) <= 1e-12
