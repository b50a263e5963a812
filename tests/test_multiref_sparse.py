"""Multi-reference retrieval from the M nearest references per pose (csrc/kernels_multiref.hip: multiref_select / multiref_gather,
hip.op_multiref_select / op_multiref_gather, PoseConditional.retrieve_multi_from_feat(max_refs=...), retrieve_multi_coarse_to_fine*,
refine_multi_from_feat, predict_pose_multi, the harness's --max-refs).  DESIGN.md section 4.13.

Every test runs on the interpreter build ("emu") and, marked `gpu`, on the device, unless it says otherwise.  The reference of the select is
an f64 NumPy restatement of include/nope_hip.h, written below on top of tests/test_multiref.py's restatement of the distances.

Bounds, from the arithmetic (tests/test_multiref.py's for nope_op_multiref_prepare, whose device functions the select shares):
  dist            1e-8 rad
  all_relativeR   one f32 ulp
  softmax weights 2^-22 |want| + 1e-37
  uniform / nearest weights, src: exact, under the ASSERTED precondition that the distances of one slot lie >= 1e-6 rad apart
  gather          bit patterns
  drivers         bit patterns against their hand composition; SMOKE_BOUNDS[mode] against the oracle; 2 SMOKE_BOUNDS[mode] between two device
                  paths that each lie within SMOKE_BOUNDS of one oracle value (the triangle inequality) or that differ by their launch plan
"""
import math

import numpy as np
import pytest
import torch

from tests.test_multiref import SMOKE_BOUNDS, WEIGHTINGS, _e2e, bits, close, grid, haar, np_distance, same_bits, ulp_apart
from tests.test_refine import CLAMP_DEG, DAMPING, H_FD, _tiny_unet, angle_deg, expm, gs

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
CAND = np.array([[5, 2, 19, 2, 0, -1, -1], [25, 1, 7, 3, 3, 11, -1], [4, 4, 9, 20, 13, 6, -1]], dtype=np.int32)     # scrambled, a duplicate, trailing -1


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


def sync(dev):
    if dev == "cuda":
        torch.cuda.synchronize()


# ---- the reference (f64 NumPy) -------------------------------------------------------------------------------------------------------------
def np_rows(Tp, Pr):
    return (Tp @ Pr.T)[:2].reshape(6)


def np_select(T, P, n_refs, cand, M, weighting, tau_rad, kind):
    """T (B|1, N, 3, 3), P (B, R, 3, 3), n_refs (B,) or None, cand (B, S) or None -> src (B, M, S), rel (B, M, S, 6), weights, dist (f64),
    status, and the smallest gap between two distances of one valid slot."""
    B, R = P.shape[:2]
    N = T.shape[1]
    S = N if cand is None else cand.shape[1]
    src, rel = np.zeros((B, M, S), dtype=np.int32), np.zeros((B, M, S, 6))
    w, d = np.zeros((B, M, S)), np.full((B, M, S), np.inf)
    status, gap = 0, np.inf
    for b in range(B):
        Tb = T[b if T.shape[0] > 1 else 0]
        nr = R if n_refs is None else int(n_refs[b])
        bad = 0
        if nr < 1 or nr > R:
            bad = 2
        elif not np.isfinite(P[b, :nr]).all():
            bad = 1
        status |= bad
        nrc = min(max(nr, 0), R)
        with np.errstate(invalid="ignore"):
            dall = np_distance(Tb, P[b], kind)
        for s in range(S):
            p = s if cand is None else int(cand[b, s])
            if p < -1 or p >= N:
                status |= 4
            if p < 0 or p >= N:
                rel[b, :, s] = np_rows(Tb[0], P[b, 0])
                continue
            dv = dall[:nrc, p]
            order = sorted(range(nrc), key=lambda r: (bool(np.isnan(dv[r])), 0.0 if np.isnan(dv[r]) else dv[r], r))
            fin = np.sort(dv[np.isfinite(dv)])
            if len(fin) > 1:
                gap = min(gap, float(np.diff(fin).min()))
            Mv = min(M, nrc)
            kept = order[:Mv]
            for m in range(M):
                r = kept[m] if m < Mv else (kept[0] if Mv else 0)
                src[b, m, s] = r
                with np.errstate(invalid="ignore"):
                    rel[b, m, s] = np_rows(Tb[p], P[b, r])
                if m < Mv:
                    d[b, m, s] = dv[r]
            if Mv:
                if weighting == "uniform":
                    w[b, :Mv, s] = 1.0 / Mv
                elif weighting == "softmax":
                    e = np.exp(-(dv[kept] - dv[kept[0]]) / tau_rad)
                    w[b, :Mv, s] = e / e.sum()
                else:
                    w[b, 0, s] = 1.0
        if bad:
            w[b] = np.nan
    return src, rel, w, d, status, gap


def _inputs(level, R, B=3, seed=11):
    """tests/test_multiref.py's _prepare_inputs: one grid for every sample (pose_stride_b = 0), Haar references from a fixed seed.  The seed
    was checked on the CPU: the precondition asserted in test_select holds for every case."""
    return grid(level)[None], haar(B * R, seed + 100 * R + level).reshape(B, R, 3, 3)


def _select(hip, dev, T, P, nr, cand, M, **kw):
    return hip.op_multiref_select(torch.from_numpy(np.array(T)).to(dev), torch.from_numpy(P).to(dev), None if nr is None else torch.tensor(nr),
                                  max_refs=M, cand=None if cand is None else torch.from_numpy(cand).to(dev), **kw)


# ---- 1. select -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cand", [False, True], ids=["grid", "cand"])
@pytest.mark.parametrize("n_refs", [None, (1, 2, 3)], ids=["all", "padded"])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("level", [0, 1])
def test_select(be, level, R, n_refs, with_cand):
    hip, dev, _ = be
    T, P = _inputs(level, R)
    B, N = 3, T.shape[1]
    assert N == (26, 91)[level]                       # no multiple of 64: partial waves
    nr = None if n_refs is None else [min(x, R) for x in n_refs]
    cand = CAND if with_cand else None
    S = N if cand is None else cand.shape[1]
    tau = 30.0
    for M in sorted({1, min(2, R), R}):
        for kind in (0, 1):
            for weighting in WEIGHTINGS:
                got = _select(hip, dev, T, P, nr, cand, M, weighting=weighting, tau_deg=tau, dist_kind=kind, want_dist=True)
                src, rel, w, d, status, gap = np_select(T, P, nr, cand, M, weighting, math.radians(tau), kind)
                where = (level, R, n_refs, with_cand, M, kind, weighting)
                assert gap >= 1e-6, where                                            # the precondition on the inputs: no near tie in any slot
                assert int(got.status) == status == 0, where
                assert tuple(got.src.shape) == (B, M, S) and got.src.dtype == torch.int32 and tuple(got.all_relativeR.shape) == (B, M, S, 6)
                assert got.all_relativeR.dtype == torch.float32 and got.weights.dtype == torch.float32 and got.dist.dtype == torch.float64
                gd, gw, grel = got.dist.cpu().numpy(), got.weights.cpu().numpy(), got.all_relativeR.cpu().numpy()
                assert np.array_equal(got.src.cpu().numpy(), src), where
                valid = np.isfinite(d)
                assert np.array_equal(np.isposinf(gd), ~valid), where
                assert np.abs(gd[valid] - d[valid]).max() <= 1e-8, where
                assert ulp_apart(grel, rel.astype(np.float32)) <= 1, where
                assert (gw[~valid] == 0).all(), where                                # slots m >= Mv and padded candidates: exactly 0
                if weighting == "softmax":
                    assert close(gw, w), where
                else:
                    assert np.array_equal(gw, w.astype(np.float32)), where
                again = _select(hip, dev, T, P, nr, cand, M, weighting=weighting, tau_deg=tau, dist_kind=kind, want_dist=True)
                assert all(a.cpu().numpy().tobytes() == b_.cpu().numpy().tobytes() for a, b_ in zip(got, again)), where      # run to run


def test_select_per_sample_grid_and_optional_outputs(be):
    hip, dev, _ = be
    B, R, N = 2, 3, 26
    T = np.stack([grid(0), haar(N, 5)])                        # one grid per sample: pose_stride_b = N * 9
    P = haar(B * R, 6).reshape(B, R, 3, 3)
    got = _select(hip, dev, T, P, None, None, 2, weighting="softmax", tau_deg=20.0, dist_kind=hip.C2F_VIEWPOINT, want_rel=False)
    assert got.all_relativeR is None and got.dist is None
    src, _, w, _, _, gap = np_select(T, P, None, None, 2, "softmax", math.radians(20.0), 1)
    assert gap >= 1e-6 and np.array_equal(got.src.cpu().numpy(), src) and close(got.weights.cpu().numpy(), w)


def test_select_planted_ties(be):
    """Two identical reference poses: the lower r comes first; M = 1 takes it; M = 2 keeps both in r order under bit-equal softmax weights."""
    hip, dev, _ = be
    T, P = _inputs(0, 3, B=2)
    P = P.copy()
    P[0, 2] = P[0, 0]
    P[1, 2] = P[1, 1]
    lo = (0, 1)
    for kind in (0, 1):
        one = _select(hip, dev, T, P, None, None, 1, weighting="nearest", dist_kind=kind)
        two = _select(hip, dev, T, P, None, None, 2, weighting="softmax", dist_kind=kind, want_dist=True)
        full = _select(hip, dev, T, P, None, None, 3, weighting="softmax", dist_kind=kind, want_dist=True)
        s1, s2, s3 = one.src.cpu().numpy(), two.src.cpu().numpy(), full.src.cpu().numpy()
        d3, w2 = full.dist.cpu().numpy(), two.weights.cpu().numpy()
        for b in range(2):
            assert not (s1[b] == 2).any() and (s1[b, 0] == lo[b]).any()                       # the tied pair wins somewhere: at its lower r
            first = s3[b, 0] == lo[b]                                                          # slots led by the tied pair
            assert first.any() and (s3[b, 1][first] == 2).all()
            assert np.array_equal(d3[b, 0][first], d3[b, 1][first])
            assert (s2[b, 1][first] == 2).all() and w2[b, 0][first].tobytes() == w2[b, 1][first].tobytes()
            assert (w2[b, 0][first] == 0.5).all()
            third = s3[b, 2] == 2                                                              # ... and when the pair comes last, r order again
            assert (s3[b, 1][third] == lo[b]).all()
        want = np_select(T, P, None, None, 3, "softmax", math.radians(30.0), kind)[0]
        assert np.array_equal(s3, want)


@pytest.mark.parametrize("n_refs", [None, (1, 2, 3)], ids=["all", "padded"])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_select_all_against_prepare(be, R, n_refs):
    """M = R: the selection is a permutation of nope_op_multiref_prepare's outputs."""
    hip, dev, _ = be
    T, P = _inputs(1, R)
    nr = None if n_refs is None else [min(x, R) for x in n_refs]
    Td, Pd, nrd = torch.from_numpy(T.copy()).to(dev), torch.from_numpy(P).to(dev), None if nr is None else torch.tensor(nr)
    for kind in (0, 1):
        for weighting in WEIGHTINGS:
            sel = hip.op_multiref_select(Td, Pd, nrd, max_refs=R, weighting=weighting, tau_deg=25.0, dist_kind=kind, want_dist=True)
            prep = hip.op_multiref_prepare(Td, Pd, nrd, weighting=weighting, tau_deg=25.0, dist_kind=kind, want_dist=True)
            src = sel.src.cpu().long()
            rows = torch.gather(prep.all_relativeR.cpu(), 1, src[..., None].expand(-1, -1, -1, 6))
            assert bits(sel.all_relativeR).equal(bits(rows)), (R, n_refs, kind, weighting)
            dist, w = torch.gather(prep.dist.cpu(), 1, src), torch.gather(prep.weights.cpu(), 1, src)
            live = torch.isfinite(sel.dist.cpu())
            for b in range(3):                              # slot m is live exactly for m < n_refs[b]
                assert bool(live[b, :R if nr is None else nr[b]].all()) and not bool(live[b, R if nr is None else nr[b]:].any())
            assert sel.dist.cpu()[live].numpy().tobytes() == dist[live].numpy().tobytes()
            gw = sel.weights.cpu()
            assert bool((gw[~live] == 0).all())
            if weighting == "softmax":                      # another summation order: ascending m, not ascending r
                assert close(gw[live].numpy(), w[live].double().numpy())
            else:
                assert torch.equal(gw[live], w[live])


def test_select_padding_and_status(be):
    hip, dev, _ = be
    T, P = _inputs(0, 3)
    N = T.shape[1]
    # n_refs[b] < M: the slots m >= n_refs[b] repeat slot 0 under weight 0
    got = _select(hip, dev, T, P, [1, 2, 3], None, 3, weighting="uniform", want_dist=True)
    src, w, rel, d = got.src.cpu().numpy(), got.weights.cpu().numpy(), got.all_relativeR.cpu().numpy(), got.dist.cpu().numpy()
    for b, nr in enumerate((1, 2, 3)):
        assert (w[b, :nr] == np.float32(1.0 / nr)).all() and (w[b, nr:] == 0).all() and np.isposinf(d[b, nr:]).all() and np.isfinite(d[b, :nr]).all()
        for m in range(nr, 3):
            assert np.array_equal(src[b, m], src[b, 0]) and rel[b, m].tobytes() == rel[b, 0].tobytes()
        assert (src[b, :nr] < nr).all()
    # cand == -1: all weights 0, src 0, the finite rows of pose 0 against reference 0, dist +inf
    for weighting in WEIGHTINGS:
        got = _select(hip, dev, T, P, None, CAND, 2, weighting=weighting, want_dist=True)
        pad = torch.from_numpy(CAND < 0)
        assert int(got.status) == 0
        for m in range(2):
            assert bool((got.weights.cpu()[:, m][pad] == 0).all()) and bool((got.src.cpu()[:, m][pad] == 0).all())
            assert bool(torch.isposinf(got.dist.cpu()[:, m][pad]).all()) and bool(torch.isfinite(got.all_relativeR).all())
            for b in range(3):
                want = np_rows(T[0, 0], P[b, 0]).astype(np.float32)
                assert ulp_apart(got.all_relativeR.cpu().numpy()[b, m][CAND[b] < 0], np.broadcast_to(want, (int((CAND[b] < 0).sum()), 6))) <= 1
        assert bool((got.weights.cpu().sum(dim=1)[~pad] - 1).abs().max() <= 2 * 2.0 ** -24)
    # cand below -1 or >= N: as padding, and status bit 2
    clean = _select(hip, dev, T, P, None, CAND, 2, want_dist=True)
    for wrong in (-2, N):
        c = CAND.copy()
        c[1, 2] = wrong
        got = _select(hip, dev, T, P, None, c, 2, want_dist=True)
        assert int(got.status) == hip.MULTIREF_BAD_CAND == 4
        assert bool((got.weights[1, :, 2] == 0).all()) and bool((got.src[1, :, 2] == 0).all()) and bool(torch.isposinf(got.dist[1, :, 2]).all())
        keep = torch.ones(3, 7, dtype=torch.bool)
        keep[1, 2] = False
        for a, b_ in ((got.weights, clean.weights), (got.src, clean.src), (got.dist, clean.dist)):
            assert a.cpu()[:, 0][keep].numpy().tobytes() == b_.cpu()[:, 0][keep].numpy().tobytes()
    # status bits 0 and 1: that sample's weights are all NaN, the other samples keep their bits, src stays inside [0, R)
    bad = P.copy()
    bad[1, 1, 2, 0] = np.nan
    for weighting in WEIGHTINGS:
        got = _select(hip, dev, T, bad, None, None, 2, weighting=weighting)
        ok = _select(hip, dev, T, P, None, None, 2, weighting=weighting)
        w = got.weights.cpu().numpy()
        assert int(got.status) == hip.MULTIREF_BAD_POSE and np.isnan(w[1]).all()
        for b in (0, 2):
            assert w[b].tobytes() == ok.weights[b].cpu().numpy().tobytes()
            assert got.all_relativeR[b].cpu().numpy().tobytes() == ok.all_relativeR[b].cpu().numpy().tobytes()
        assert bool(((got.src >= 0) & (got.src < 3)).all())
    got = _select(hip, dev, T, bad, [3, 1, 3], None, 1, weighting="uniform")          # the NaN sits in a PADDED reference: not an error
    assert int(got.status) == 0 and bool((got.weights == 1).all()) and bool((got.src[1] == 0).all())
    for count in (0, 4, -1):
        got = _select(hip, dev, T, P, [3, 2, count], None, 2, weighting="softmax")
        w = got.weights.cpu().numpy()
        assert int(got.status) == hip.MULTIREF_BAD_COUNT and np.isnan(w[2]).all() and np.isfinite(w[:2]).all(), count
        assert bool(torch.isfinite(got.all_relativeR).all()) and bool(((got.src >= 0) & (got.src < 3)).all())
    got = _select(hip, dev, T, bad, [3, 3, 0], CAND, 2)
    assert int(got.status) == hip.MULTIREF_BAD_POSE | hip.MULTIREF_BAD_COUNT


BAD_SELECT = [dict(R=0), dict(R=9), dict(N=0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=0.0), dict(tau=-1.0), dict(weighting=3),
              dict(weighting=-1), dict(kind=2), dict(kind=-1), dict(M=0), dict(M=4), dict(S=0), dict(no="poses"), dict(no="refs"), dict(no="src"),
              dict(no="weights"), dict(no="status")]


@pytest.mark.parametrize("bad", BAD_SELECT, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_select_bad_arguments(be, bad):
    """NOPE_ERR_ARG, and nothing written: the outputs hold a sentinel afterwards."""
    hip, dev, _ = be
    B, R, N = 2, 3, 26
    T = torch.from_numpy(grid(0).copy())[None].to(dev)
    P = torch.from_numpy(haar(B * 9, 3).reshape(B, 9, 3, 3)).to(dev)          # (room for R = 9)
    cand = torch.zeros(B, 7, dtype=torch.int32, device=dev)
    out = hip.MultiRefSelect(torch.full((B, 9, N, 6), 7.0, device=dev), torch.full((B, 9, N), 7.0, device=dev),
                             torch.full((B, 9, N), 7.0, dtype=torch.float64, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev),
                             torch.full((B, 9, N), 7, dtype=torch.int32, device=dev))
    kw = dict(R=R, N=N, tau=0.5, weighting=1, kind=0, M=2, S=7)
    kw.update({k: v for k, v in bad.items() if k != "no"})
    ptr = dict(poses=T.data_ptr(), refs=P.data_ptr(), src=out.src.data_ptr(), weights=out.weights.data_ptr(), status=out.status.data_ptr())
    if "no" in bad:
        ptr[bad["no"]] = None
    l = hip.lib()
    for cp in ((cand.data_ptr(),) if "S" in bad else (cand.data_ptr(), None)):       # S is read with a candidate list only
        code = l.dll.nope_op_multiref_select(ptr["poses"], 0, kw["N"], ptr["refs"], kw["R"], None, cp, kw["S"], kw["M"], kw["weighting"], kw["tau"],
                                             kw["kind"], ptr["src"], out.all_relativeR.data_ptr(), ptr["weights"], out.dist.data_ptr(), ptr["status"], B, 0)
        assert code == -1, code
    with pytest.raises(hip.NopeError, match=r"\(-1\)"):
        l.check(code, "nope_op_multiref_select")
    sync(dev)
    assert all(bool((t == 7).all()) for t in out)
    if "S" in bad:                                                             # without a list S = 0 is not read
        ok = hip._multiref_select_call(T, 0, N, P[:, :R].contiguous(), R, None, None, 0, 2, 0, 0.5, 0, out)
        assert int(ok.status) == 0 and bool((ok.weights.view(-1)[:B * 2 * N] == 0.5).all())
    elif "tau" in bad:                                                         # tau is read under softmax only
        ok = hip._multiref_select_call(T, 0, N, P[:, :R].contiguous(), R, None, None, N, 3, 0, kw["tau"], 0, out)
        assert int(ok.status) == 0 and bool((ok.weights.view(-1)[:B * R * N] == np.float32(1.0 / 3)).all())
    elif "M" in bad:                                                           # the same through the binding
        with pytest.raises(hip.NopeError, match=r"\(-1\)"):
            hip.op_multiref_select(T, P[:, :R].contiguous(), max_refs=kw["M"])


def test_select_shape_errors(be):
    hip, dev, _ = be
    T = torch.from_numpy(grid(0).copy())[None].to(dev)
    P = torch.from_numpy(haar(6, 3).reshape(2, 3, 3, 3)).to(dev)
    for args, kw in (((T[0], P), {}), ((T.repeat(3, 1, 1, 1), P), {}), ((T, P[0]), {}), ((T, P, torch.zeros(3)), {}), ((T, P), dict(weighting="best")),
                     ((T, P), dict(cand=torch.zeros(3, 4, dtype=torch.int32))), ((T, P), dict(cand=torch.zeros(4, dtype=torch.int32)))):
        with pytest.raises(hip.NopeError):
            hip.op_multiref_select(*args, max_refs=1, **kw)


# ---- 2. gather -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8 * 12 * 12, 8 * 16 * 16])
def test_gather_bit_patterns(be, L):
    """Random words as f32 (NaN payloads among them), an inf plane; src = 7 in the last sample; a source outside [0, R): a NaN row."""
    hip, dev, _ = be
    B, R, J = 3, 8, 6
    g = torch.Generator().manual_seed(L)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, R, L), generator=g, dtype=torch.int64).to(torch.int32)
    words[0, 1] = 0x7fc12345                                                   # a quiet NaN with a payload
    words[1, 2, ::2] = 0x7fa00001                                              # signalling NaNs
    feats = words.view(torch.float32).clone()
    feats[2, 7] = float("inf")
    feats[2, 0] = -float("inf")
    src = torch.tensor([[1, 0, 7, 1, 3, 5], [2, 2, 6, 0, 7, 4], [7, 0, 3, 7, 1, 6]], dtype=torch.int32)
    got = hip.op_multiref_gather(feats.to(dev), src.to(dev))
    assert tuple(got.shape) == (B, J, L) and got.dtype == torch.float32
    want = torch.gather(bits(feats), 1, src.long()[..., None].expand(-1, -1, L))
    assert torch.equal(bits(got), want)
    shaped = hip.op_multiref_gather(feats.view(B, R, L // 4, 2, 2).to(dev), src.view(B, 2, 3).to(dev))       # (B, R, C, h, w) and (B, M, S)
    assert tuple(shaped.shape) == (B, J, L // 4, 2, 2) and torch.equal(bits(shaped).view(B, J, L), want)
    for wrong in (-1, R):
        s2 = src.clone()
        s2[1, 3] = wrong
        got = hip.op_multiref_gather(feats.to(dev), s2.to(dev)).cpu()
        assert bool(torch.isnan(got[1, 3]).all())
        keep = torch.ones(B, J, dtype=torch.bool)
        keep[1, 3] = False
        assert torch.equal(bits(got)[keep], want[keep])                        # its neighbours are untouched


@pytest.mark.parametrize("bad", [dict(L=6), dict(L=0), dict(B=0), dict(R=0), dict(J=0), dict(no="feats"), dict(no="src"), dict(no="out")],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_gather_bad_arguments(be, bad):
    hip, dev, _ = be
    feats, src = torch.zeros(2, 3, 8, device=dev), torch.zeros(2, 4, dtype=torch.int32, device=dev)
    out = torch.full((2, 4, 8), 7.0, device=dev)
    kw = dict(B=2, R=3, J=4, L=8)
    kw.update({k: v for k, v in bad.items() if k != "no"})
    ptr = dict(feats=feats.data_ptr(), src=src.data_ptr(), out=out.data_ptr())
    if "no" in bad:
        ptr[bad["no"]] = None
    code = hip.lib().dll.nope_op_multiref_gather(ptr["feats"], ptr["src"], ptr["out"], kw["B"], kw["R"], kw["J"], kw["L"], 0)
    assert code == -1, code
    sync(dev)
    assert bool((out == 7).all())
    if bad == dict(L=6):
        with pytest.raises(hip.NopeError, match=r"\(-1\)"):
            hip.op_multiref_gather(torch.zeros(2, 3, 6, device=dev), src)
        for wrong in (torch.zeros(2, 4, 7, device=dev), torch.zeros(2, 4, 8, dtype=torch.float64, device=dev), torch.zeros(2, 8, 8, device=dev)[:, ::2]):
            with pytest.raises(hip.NopeError, match="out"):                    # a wrong-sized `out` is refused, not written past its end
                hip.op_multiref_gather(feats, src, out=wrong)


# ---- 3. the driver on smoke()'s tiny network ----------------------------------------------------------------------------------------------------
def _memo_forward(model):
    """The interpreter needs many seconds per U-Net pass: a forward_hypotheses call with inputs it has seen returns the first result again."""
    inner, kept = model.u_net.forward_hypotheses, {}

    def wrapped(x, poses, out=None, out_dtype="f32", defer_range_check=False):
        key = (x.detach().cpu().numpy().tobytes(), poses.detach().cpu().numpy().tobytes(), out_dtype)
        if key not in kept:
            kept[key] = inner(x, poses, out_dtype=out_dtype, defer_range_check=defer_range_check).clone()
        if out is not None:
            out.copy_(kept[key])
            return out
        return kept[key].clone()
    return wrapped


class _Counting:
    """Counts the hypotheses that go through u_net.forward_hypotheses."""

    def __init__(self, model, monkeypatch):
        self.n, inner = 0, model.u_net.forward_hypotheses

        def wrapped(x, poses, *a, **kw):
            self.n += poses.shape[0] * poses.shape[1]
            return inner(x, poses, *a, **kw)
        monkeypatch.setattr(model.u_net, "forward_hypotheses", wrapped, raising=False)


def _compose(hip, model, q, refs, sel, fusion):
    """select -> gather -> forward_hypotheses with one pose per source -> scoring -> top-k, written out."""
    B, M, S = sel.src.shape
    x = hip.op_multiref_gather(refs, sel.src).view(B * M * S, *refs.shape[2:])
    bank = model.u_net.forward_hypotheses(x, sel.all_relativeR.view(B * M * S, 1, 6)).view(B, M, S, *refs.shape[2:])
    per = hip.similarity(q, bank.view(B, M * S, *refs.shape[2:])).view(B, M, S)
    if M == 1:
        sim = hip.similarity(q, bank.view(B, S, *refs.shape[2:]))
    else:
        sim = hip.multiref_similarity(q, bank, sel.weights) if fusion == "feature" else hip.op_multiref_fuse_scores(per, sel.weights)
    return bank, per, sim


E2E_CASES = [pytest.param("emu", "f32")] + [pytest.param("gpu", c, marks=pytest.mark.gpu) for c in SMOKE_BOUNDS]      # the interpreter runs the f32 mode


@pytest.mark.parametrize("backend,cdt", E2E_CASES)
def test_e2e_retrieve_multi_sparse(request, monkeypatch, backend, cdt):
    from oracle import nope_ref
    hip, dev, name = request.getfixturevalue(backend), ("cuda" if backend == "gpu" else "cpu"), backend
    if cdt == "f16x2":
        monkeypatch.setenv("NOPE_CONV_PP", "11")             # as smoke(): a dozen hypotheses would not reach the ping-pong kernels otherwise
    model, sd, b = _e2e(dev, name, cdt)
    if name == "emu":
        monkeypatch.setattr(model.u_net, "forward_hypotheses", _memo_forward(model), raising=False)
    B, R, N = 2, 3, 6
    q, refs, P, T = b["query"], b["references"], b["reference_poses"], b["template_poses"][:1]
    n_refs = torch.tensor([3, 2])
    bound = SMOKE_BOUNDS[cdt]
    if cdt == "f16x2":                                       # the handle re-centres its layers' range shifts after the first passes: compare
        for _ in range(4):                                   # passes of the settled handle, as the dense test does
            model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, max_refs=2)
            model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs)
    dense = {w: model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, fusion="feature", weighting=w, tau_deg=40.0) for w in ("softmax", "nearest")}
    none = model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, fusion="feature", weighting="softmax", tau_deg=40.0, max_refs=None)
    assert same_bits(none.similarity, dense["softmax"].similarity) and torch.equal(none.bank, dense["softmax"].bank) and none.src is None
    rel = lambda a, w: float((a.cpu().double() - w.cpu().double()).abs().max() / w.cpu().double().abs().max())
    for M in (1, 2, 3):
        want_bank = None
        for fusion in ("feature", "score"):
            for weighting in ("softmax", "nearest"):
                res = model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, fusion=fusion, weighting=weighting, tau_deg=40.0,
                                                     return_per_reference=True, max_refs=M)
                sel = hip.op_multiref_select(T, P, n_refs, max_refs=M, weighting=weighting, tau_deg=40.0)
                bank, per, sim = _compose(hip, model, q, refs, sel, fusion)
                _, idx = hip.topk(sim, 5)
                assert torch.equal(res.bank, bank) and same_bits(res.similarity, sim) and torch.equal(res.nearest_idx, idx)
                assert same_bits(res.per_reference, per) and same_bits(res.weights, sel.weights) and torch.equal(res.src, sel.src)
                assert tuple(res.bank.shape) == (B, M, N, 8, 16, 16) and bool(torch.isfinite(res.similarity).all())
                # the oracle: one map per gathered source, a NumPy blend, similarity_scores
                if want_bank is None:
                    x = hip.op_multiref_gather(refs, sel.src).cpu().reshape(B * M * N, 8, 16, 16)
                    want_bank = nope_ref.generate_templates(sd, x, sel.all_relativeR.cpu().reshape(B * M * N, 1, 6)).view(B, M, N, 8, 16, 16)
                w64 = sel.weights.cpu().double()
                if fusion == "feature" or M == 1:
                    want = nope_ref.similarity_scores(q.cpu().double(), (w64[..., None, None, None] * want_bank.double()).sum(dim=1))
                else:
                    want = (w64 * nope_ref.similarity_scores(q.cpu().double(), want_bank.double().view(B, M * N, 8, 16, 16)).view(B, M, N)).sum(dim=1)
                err = rel(res.similarity, want)
                print(f"retrieve_multi[{cdt}, max_refs {M}, {fusion}, {weighting}]: score rel err {err:.2e}")
                assert err < bound, (cdt, M, fusion, weighting, err)
                # against the dense path: both lie within `bound` of one oracle value
                pair = dense["softmax"] if (M == R and weighting == "softmax") else dense["nearest"] if M == 1 else None
                if pair is not None and fusion == "feature":
                    between = rel(res.similarity, pair.similarity)
                    print(f"retrieve_multi[{cdt}, max_refs {M}, {weighting}]: sparse against dense {between:.2e}")
                    assert between <= 2 * bound, (cdt, M, weighting, between)
                    top2 = want.topk(2, dim=1).values
                    sure = ((top2[:, 0] - top2[:, 1]) / want.abs().max() > 2 * bound)
                    assert torch.equal(res.nearest_idx[:, 0].cpu()[sure], pair.nearest_idx[:, 0].cpu()[sure])
    # the U-Net sees B M N hypotheses for the sparse call, B R N for the dense one
    if "_generate_templates_from_feat" in vars(model):                             # (the interpreter's memo of the dense bank would hide its forwards)
        monkeypatch.delattr(model, "_generate_templates_from_feat")
    count = _Counting(model, monkeypatch)
    model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs, max_refs=2)
    assert count.n == B * 2 * N
    count.n = 0
    model.retrieve_multi_from_feat(q, refs, P, T, n_refs=n_refs)
    assert count.n == B * R * N
    assert model.retrieve_multi_from_feat(q, refs, P, T, max_refs=1).per_reference is None
    for wrong in (0, 4, -1):
        with pytest.raises(ValueError):
            model.retrieve_multi_from_feat(q, refs, P, T, max_refs=wrong)
    # positional construction with five fields keeps working
    from nope_amd.model import MultiRefResult
    assert MultiRefResult(1, 2, 3, 4, 5).src is None


@pytest.mark.gpu
def test_sparse_chunked_forwards(gpu):
    """max_hypotheses_per_launch below B M N: the sparse path chunks its sources -- to rounding the same scores (another launch plan)."""
    from nope_amd.model import PoseConditional
    model, _, b = _e2e("cuda", "gpu")
    q, refs, P, T = b["query"], b["references"], b["reference_poses"], b["template_poses"][:1]
    whole = model.retrieve_multi_from_feat(q, refs, P, T, max_refs=2)
    small = PoseConditional(model.u_net, None, {"similarity_metric": "l2"}, None, max_hypotheses_per_launch=5).cuda()
    parts = small.retrieve_multi_from_feat(q, refs, P, T, max_refs=2)
    assert torch.equal(parts.src, whole.src) and same_bits(parts.weights, whole.weights)
    assert float((parts.similarity - whole.similarity).abs().max() / whole.similarity.abs().max()) <= 2 * SMOKE_BOUNDS["f32"]


# ---- 4. coarse to fine ---------------------------------------------------------------------------------------------------------------------------
def _stub_forward(x, poses, out=None, out_dtype="f32", defer_range_check=False):
    """In place of the U-Net on the interpreter: a cheap pure function of (source, pose)."""
    y = x[:, None] * poses[..., 0, None, None, None] + poses[..., 1:4].sum(-1)[..., None, None, None] + 0.25 * x[:, None].flip(-1) * poses[..., 5, None, None, None]
    if out is not None:
        out.copy_(y)
        return out
    return y


@pytest.mark.parametrize("M", [1, 2])
def test_coarse_to_fine_multi(be, monkeypatch, M):
    from nope_amd import poses, search
    hip, dev, name = be
    model, _, b = _e2e(dev, name)
    if name == "emu":
        monkeypatch.setattr(model.u_net, "forward_hypotheses", _stub_forward, raising=False)
    B, R = 2, 3
    q, refs, P = b["query"], b["references"], b["reference_poses"]
    T = torch.from_numpy(grid(1).copy())[None].to(dev)
    N = T.shape[1]
    stage_of = poses.grid_stages(1, "upper")
    n_refs = torch.tensor([3, 2])
    kw = dict(n_refs=n_refs, max_refs=M, fusion="score", weighting="softmax", tau_deg=40.0)
    got = model.retrieve_multi_coarse_to_fine_from_feat(q, refs, P, T, stage_of=stage_of, seeds=3, **kw)

    def evaluate(rows, cand):                                   # written out: `rows` is not used
        sel = hip.op_multiref_select(T, P, n_refs, max_refs=M, cand=cand, weighting="softmax", tau_deg=40.0)
        return _compose(hip, model, q, refs, sel, "score")[2]
    rows = hip.op_multiref_select(T, P, n_refs, max_refs=1, weighting="nearest").all_relativeR.view(B, N, 6)
    want = search.coarse_to_fine_search(evaluate, rows, T, stage_of, seeds=3)
    assert same_bits(got.similarity, want.similarity) and torch.equal(got.nearest_idx, want.nearest_idx) and torch.equal(got.evaluated, want.evaluated)
    assert all(torch.equal(a, c) for a, c in zip(got.cand, want.cand)) and int(got.status.max()) == 0
    state = got.evaluated.cpu() != 0
    assert bool(torch.isneginf(got.similarity.cpu()[~state]).all()) and bool(torch.isfinite(got.similarity.cpu()[state]).all())
    assert 26 <= int(got.n_evaluated.min()) and int(got.n_evaluated.max()) < N
    full = model.retrieve_multi_from_feat(q, refs, P, T, k=5, **kw)
    diff = (got.similarity.cpu()[state] - full.similarity.cpu()[state]).abs().max() / full.similarity.abs().max().cpu()
    print(f"c2f multi[{name}, max_refs {M}]: evaluated {got.n_evaluated.cpu().tolist()} of {N}, against the exhaustive call {float(diff):.2e}")
    assert float(diff) <= 2 * SMOKE_BOUNDS["f32"]              # (another batch size takes another launch plan)
    every = model.retrieve_multi_coarse_to_fine_from_feat(q, refs, P, T, stage_of=stage_of, seeds=3, capacity=N, radii_rad=math.pi, **kw)
    assert bool((every.evaluated != 0).all()) and bool(torch.isfinite(every.similarity).all())
    assert float((every.similarity - full.similarity).abs().max() / full.similarity.abs().max()) <= 2 * SMOKE_BOUNDS["f32"]
    through = model.retrieve_multi_coarse_to_fine(q, refs, P, T, stage_of=stage_of, seeds=3, **kw)      # (the StubEncoder hands the embeddings through)
    assert same_bits(through.similarity, got.similarity)


# ---- 5. refinement ---------------------------------------------------------------------------------------------------------------------------------
def _planted_multi(hip, dev, model, B, seed):
    """R = 3 references; a per-sample grid whose vertices 1 and 4 lie 4 and 8 degrees off the planted pose Q and whose vertex 6 IS Q; the
    query is the network's output at Q from the nearest reference r* of those vertices -- slot 0 of vertex 6 in a forward of the very shape
    the refinement's first iteration runs, so that candidate's residual is exactly zero."""
    R, N, k = 3, 8, 3
    g = torch.Generator().manual_seed(200 + seed)
    feats = torch.randn(B, R, 8, 8, 8, generator=g).to(dev)
    T, P = haar(B * N, 300 + seed).reshape(B, N, 3, 3).copy(), haar(B * R, 400 + seed).reshape(B, R, 3, 3)
    idx = torch.tensor([[1, 4, 6]] * B)
    for b in range(B):
        for j, deg in ((1, 4.0), (4, 8.0)):
            ax = torch.randn(3, generator=g, dtype=torch.float64).numpy()
            T[b, j] = expm(math.radians(deg) * ax / np.linalg.norm(ax)) @ T[b, 6]
        d = np_distance(T[b], P[b], 0)                                              # (R, N)
        near = d[:, [1, 4, 6]].argmin(axis=0)
        assert (near == near[0]).all() and np.diff(np.sort(d[:, [1, 4, 6]], axis=0), axis=0).min() >= 1e-6      # one r* for the three, no near tie
    Td, Pd = torch.from_numpy(T).to(dev), torch.from_numpy(P).to(dev)
    sel = hip.op_multiref_select(Td, Pd, max_refs=1, cand=idx.to(dev), weighting="nearest")
    x = hip.op_multiref_gather(feats, sel.src).view(B * k, 8, 8, 8)
    seven = hip.op_refine_init(sel.all_relativeR.view(B, k, 6), torch.arange(k).expand(B, k).contiguous().to(dev), H_FD)[2]
    maps = torch.empty(B * k, 7, 8, 8, 8, device=dev)
    model._forward_poses(x, seven.view(B * k, 7, 6), maps)
    q = maps.view(B, k, 7, 8, 8, 8)[:, 2, 0].contiguous()
    truth = [gs(sel.all_relativeR[b, 0, 2].cpu().numpy()) for b in range(B)]
    return feats, Td, Pd, idx.to(dev), q, sel, x, truth, maps.view(B, k, 7, 8, 8, 8)


def test_refine_multi(be, monkeypatch):
    from nope_amd.model import PoseConditional
    hip, dev, name = be
    model = PoseConditional(_tiny_unet(3), None, {"similarity_metric": "l2"}, None).to(dev)
    if name == "emu":
        monkeypatch.setattr(model.u_net, "forward_hypotheses", _memo_forward(model), raising=False)
    B, iters, tol = (2, 3, 0.005) if name == "gpu" else (1, 2, 0.02)
    feats, T, P, idx, q, sel, x, truth, first = _planted_multi(hip, dev, model, B, 3)
    r = model.refine_multi_from_feat(q, feats, P, T, idx, iters=iters, fd_step=H_FD, max_step_deg=CLAMP_DEG, damping=DAMPING)
    traj, order = r.trajectory.cpu().numpy(), r.order.cpu()
    worst = max(angle_deg(traj[iters, b, j], truth[b]) for b in range(B) for j in range(3))
    print(f"refine_multi[{name}]: final error <= {worst:.2e} deg after {iters} iterations, accepted {r.accepted.cpu().tolist()}, order {order.tolist()}")
    assert worst <= tol
    for b in range(B):
        for pos in range(3):
            assert bool(r.accepted[b, pos]) == (int(order[b, pos]) != 2)          # the candidate ON the grid answer is not "accepted"
        assert angle_deg(r.relR[b, 0].cpu().numpy(), truth[b]) <= tol
    # score_init is, by construction, the score of slot 0 of each group of seven in the first iteration's forward; _planted_multi ran that
    # very forward (same sources, same poses, same shape: `first`), so the baseline is known bit for bit, in the final order.  A neighbour's
    # slot, or the fused row's score, would differ in the first digits.
    base = hip.similarity(q, first[:, :, 0].contiguous())
    assert same_bits(r.score_init, torch.gather(base, 1, order.to(dev)))
    for slot in range(1, 7):
        assert not same_bits(torch.gather(hip.similarity(q, first[:, :, slot].contiguous()), 1, order.to(dev)), r.score_init)
    # ... and it is the single-reference score of the grid pose through src: a forward of ANOTHER shape (one pose per source), so equal to
    # rounding only.  Both scores are -sum_p ||q - t||_4^2 of maps within eps = SMOKE_BOUNDS of the f64 network, relative to the maps, and
    # ||a + d||^2 - ||a||^2 <= (2 ||a|| + ||d||) ||d||: against the score's own magnitude s = sum_p ||q - t||^2 the two may differ by
    # 2 eps (2 sqrt(S0 / s) + 2 eps S0 / s), S0 = sum_p ||t||^2 the maps' score against a zero query -- 2 eps times a factor that is 1 for
    # unrelated embeddings (s ~ S0: smoke()'s setting) and grows as the planted query cancels.  Per candidate; the candidate ON the
    # answer has s = 0 and is covered by the bit pattern above.
    maps_of_src = model.u_net.forward_hypotheses(x, sel.all_relativeR.view(B * 3, 1, 6)).view(B, 3, 8, 8, 8)
    single = hip.similarity(q, maps_of_src)
    s0 = hip.similarity(torch.zeros_like(q), maps_of_src).abs()
    eps = SMOKE_BOUNDS["f32"]
    for j in (0, 1):
        sj, ratio = single[:, j].abs().double(), (s0[:, j] / single[:, j].abs()).double()
        err = (base[:, j] - single[:, j]).abs().double() / sj
        bound = 2 * eps * (2 * ratio.sqrt() + 2 * eps * ratio)
        print(f"refine_multi[{name}]: candidate {j}: score_init against the one-pose forward {err.cpu().tolist()} of the score, bound {bound.cpu().tolist()}")
        assert bool((err <= bound).all())
    assert bool((r.score >= r.score_init).all())
    want = torch.from_numpy(np.stack([np.stack([traj[iters, b, j] @ gs(sel.all_relativeR[b, 0, j].cpu().numpy()).T @ T[b, idx[b, j]].cpu().numpy()
                                               for j in range(3)]) for b in range(B)]))
    for b in range(B):
        for pos in range(3):
            if bool(r.accepted[b, pos]):
                assert np.abs(r.pred_R[b, pos].cpu().numpy() - want[b, order[b, pos]].numpy()).max() <= 1e-6


# ---- 6. predict_pose_multi and the harness -------------------------------------------------------------------------------------------------------
def test_predict_pose_multi_defaults_and_shards(be, monkeypatch):
    hip, dev, name = be
    model, _, b = _e2e(dev, name)
    if name == "emu":
        monkeypatch.setattr(model.u_net, "forward_hypotheses", _memo_forward(model), raising=False)
    q, refs, P, T = b["query"], b["references"], b["reference_poses"], b["template_poses"][:1]
    res = model.retrieve_multi(q, refs, P, T)
    pred, score = model.predict_pose_multi(q, refs, P, T, max_refs=None, coarse_to_fine=None, refine_iters=0)
    assert torch.equal(pred, T.to(pred.device)[0, res.nearest_idx]) and torch.equal(score, torch.gather(res.similarity, 1, res.nearest_idx))
    one = model.retrieve_multi(q, refs, P, T, max_refs=1)
    pred1, score1 = model.predict_pose_multi(q, refs, P, T, max_refs=1)
    assert torch.equal(pred1, T.to(pred.device)[0, one.nearest_idx]) and torch.equal(score1, torch.gather(one.similarity, 1, one.nearest_idx))
    with pytest.raises(TypeError):                           # a keyword the staged branch does not know is not dropped
        model.predict_pose_multi(q, refs, P, T, coarse_to_fine=True, return_per_reference=True)
    from nope_amd import dist as ndist
    monkeypatch.setattr(model, "template_parallel", True)
    monkeypatch.setattr(ndist, "world", lambda: (0, 2))
    idx = res.nearest_idx
    for call in (lambda: model.retrieve_multi(q, refs, P, T, max_refs=1), lambda: model.retrieve_multi_from_feat(q, refs, P, T, max_refs=1),
                 lambda: model.retrieve_multi_coarse_to_fine(q, refs, P, T), lambda: model.retrieve_multi_coarse_to_fine_from_feat(q, refs, P, T),
                 lambda: model.refine_multi_from_feat(q, refs, P, T, idx), lambda: model.predict_pose_multi(q, refs, P, T, max_refs=1, refine_iters=1)):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.gpu
def test_predict_pose_multi_refined(gpu):
    """max_refs = 1 with three iterations on a planted batch: the top-1 moves from the grid vertex towards the planted pose."""
    from nope_amd.model import PoseConditional
    hip, dev = gpu, "cuda"
    model = PoseConditional(_tiny_unet(3), None, {"similarity_metric": "l2"}, None).to(dev)
    B = 2
    feats, T, P, _, q, _, _, _, _ = _planted_multi(hip, dev, model, B, 3)
    want = T[:, 6].cpu().numpy()                                                   # the planted pose Q ...
    T = T.clone()
    T[:, 6] = torch.from_numpy(haar(B, 77)).to(dev)                                 # ... which is no vertex of this grid: 1 and 4 lie 4 and 8 degrees off
    grid_pred, grid_score = model.predict_pose_multi(q, feats, P, T, max_refs=1, k=3)
    pred, score = model.predict_pose_multi(q, feats, P, T, max_refs=1, k=3, refine_iters=3, fd_step=H_FD, max_step_deg=CLAMP_DEG, damping=DAMPING)
    for b in range(B):
        before, after = angle_deg(grid_pred[b, 0].cpu().numpy(), want[b]), angle_deg(pred[b, 0].cpu().numpy(), want[b])
        print(f"predict_pose_multi[max_refs 1] sample {b}: grid top-1 {before:.4f} deg, refined {after:.4f} deg")
        assert after < before
    assert bool((score[:, 0] >= grid_score[:, 0]).all())


@pytest.mark.gpu
def test_harness_cli_max_refs(gpu, capsys):
    import json
    from nope_amd import harness
    harness.main(["--batch", "1", "--size", "64", "--pose-level", "1", "--references", "3", "--max-refs", "1", "--coarse-to-fine", "--refine", "2"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "multi/top1, median" in res and "multi/top1_agree" in res and "multi/evaluated_frac" in res
    assert any(k.startswith("multi_refined/") for k in res) and any(k.startswith("c2f/") for k in res) and any(k.startswith("refined/") for k in res)
