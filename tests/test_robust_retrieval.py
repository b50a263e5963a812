"""Occlusion-robust retrieval: masked and trimmed template scoring (csrc/kernels_robust.hip, hip.robust_similarity / op_residual_maps /
op_pool_mask, PoseConditional.retrieval*(robust=...) / retrieve_robust, harness.occlude_queries / eval_geodesic(robust)).  DESIGN.md section 4.14.

Every test runs on the interpreter build ("emu") and, marked `gpu`, on the device.  The references are f64 NumPy restatements of the
definitions in include/nope_hip.h, written below; the number of trimmed terms is computed with np.float32, as the definition says.

Bounds, from the arithmetic:
  scores on dyadic data        bit patterns, -0.0 included: q is integer-valued and a template differs from it in ONE channel per pixel by a small
                               integer D, so d = D^2, and every product, partial sum and square root is exact in any order
  scores on random data        2e-5 relative (max abs difference over max abs), tests/test_gpu_sweeps.py's bound for nope_similarity: the trimmed
                               form needed no more.  Observed on the interpreter build over the shape list below: 1.7e-7 (f32 / bf16 / f16
                               banks alike: the bank's rounding is in the reference too)
  residual maps, dyadic        bit patterns
  residual maps, random        2^-22 relative per element for every bank type: the planes are evaluated in f64 and rounded once, so the error
                               against the f64 reference is one f32 rounding, 2^-24 (observed: 5.9e-8 <= 2^-24, all three bank types)
  pool mask                    exact (uint8: integer sums; f32: dyadic planes, whose sums and means are exact)
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTS = ["f32", "bf16", "f16"]
SHAPES = [(4, 4), (8, 8), (16, 16), (32, 32)]
OUTSIDE = (4, 12)                    # 48 pixels: 12 (f32) or 6 (16-bit) lanes per hypothesis do not divide 256 -> the generic form
RANDOM_BOUND = 2e-5
REL = 2.0 ** -22


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


# ---- the reference (f64 NumPy) -------------------------------------------------------------------------------------------------------------
def np_d(q, bank):
    """q (B, C, h, w) f32, bank (B|1, N, C, h, w) as stored -> d (B, N, h w) f64."""
    q64, bk = q.double().numpy(), bank.double().numpy()
    if bk.shape[0] == 1 and q64.shape[0] > 1:
        bk = np.broadcast_to(bk, (q64.shape[0],) + bk.shape[1:])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(((q64[:, None] - bk) ** 4).sum(axis=2)).reshape(q64.shape[0], bk.shape[1], -1)


def kept(a, trim):
    """m = a - min(a - 1, floorf(trim * (float)a)), the product in f32."""
    t = min(a - 1, int(np.floor(np.float32(trim) * np.float32(a))))
    return a - t


def np_robust(q, bank, mask=None, trim=0.0):
    """The definition of nope_robust_similarity in f64 -> (B, N) f64."""
    d = np_d(q, bank)
    B, N, HW = d.shape
    out = np.zeros((B, N))
    for b in range(B):
        A = np.ones(HW, dtype=bool) if mask is None else (mask[b].reshape(-1).numpy() != 0)
        a = int(A.sum())
        if a == 0:
            out[b] = np.nan
            continue
        m = kept(a, trim)
        for n in range(N):
            row = d[b, n, A]
            out[b, n] = np.nan if np.isnan(row).any() else -np.sort(row)[:m].sum()
    return out


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got, want):
    """f32 tensors equal as bit patterns (-0.0 is not 0.0); a NaN matches any NaN."""
    got = got.detach().cpu().float()
    want = torch.as_tensor(np.asarray(want)).float() if not isinstance(want, torch.Tensor) else want.detach().cpu().float()
    if got.shape != want.shape:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def dyadic_case(seed, dt, B, N, C, h, w, ties=None, shared=False):
    """q (B, C, h, w) f32, integer-valued in [-64, 64]; bank (B|1, N, C, h, w) of type dt: q[0 if shared else b] except in ONE channel per
    pixel, where it is q + D, D a small integer, so d = D^2 exactly (16-bit banks: |q + D| <= 68 is an integer the type holds).  D comes from
    few values, so a row is full of ties on both sides of any position; ties = "all": every d of a row is the same value."""
    g = torch.Generator().manual_seed(seed)
    HW = h * w
    q = torch.randint(-64, 65, (B, C, HW), generator=g).float()
    if shared:
        q = q[:1].repeat(B, 1, 1)                     # (one bank for every query: the queries must agree for d to stay D^2)
    Bb = 1 if shared else B
    allowed = (-4, -2, -1, 0, 1, 2, 4) if dt != "f32" else tuple(range(-8, 9))
    D = torch.tensor(allowed)[torch.randint(0, len(allowed), (Bb, N, HW), generator=g)].float()
    if ties == "all":
        D = torch.tensor(allowed)[torch.randint(0, len(allowed), (Bb, N, 1), generator=g)].float().abs().clamp(min=1).repeat(1, 1, HW)
    ch = torch.randint(0, C, (Bb, N, HW), generator=g)
    bank = q[:Bb, None].repeat(1, N, 1, 1)
    bank.scatter_add_(2, ch[:, :, None, :], D[:, :, None, :])
    if N > 2 and ties is None:
        bank[Bb - 1, N // 2] = q[Bb - 1]              # a planted match: every d is 0, the score is -0.0
    return q.reshape(B, C, h, w), bank.reshape(Bb, N, C, h, w).to(DT[dt])


def make_mask(kind, B, h, w, seed=5):
    """"ones" | "rect" | "random" (a count that is a multiple of nothing convenient) | "one" (a = 1) | "zero" | ("count", a): exactly a pixels."""
    g = torch.Generator().manual_seed(seed)
    HW = h * w
    m = torch.zeros(B, HW, dtype=torch.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "rect":
        m = m.reshape(B, h, w)
        m[:, h // 4:h - h // 8, 1:w - 1] = 1
        m = m.reshape(B, HW)
    elif kind == "one":
        for b in range(B):
            m[b, int(torch.randint(0, HW, (1,), generator=g))] = 7             # (any non-zero byte counts)
    elif kind == "zero":
        pass
    else:
        for b in range(B):
            a = kind[1] if isinstance(kind, tuple) else max(1, min(HW - 1, (HW * 5) // 9 + 2 * b + 1))
            m[b, torch.randperm(HW, generator=g)[:a]] = 1
    return m.reshape(B, h, w)


# (B, N, mask, trim): N in {1, 5, 13} (the tail group), B in {1, 3}, every mask and every trim value of the issue
COMBOS = [(1, 1, "ones", 0.25), (3, 5, "rect", 0.5), (3, 13, "random", 0.25), (1, 13, "one", 0.999), (3, 5, "random", 0.0), (1, 5, None, 0.999),
          (3, 13, None, 0.5), (1, 5, "zero", 0.25), (3, 1, ("count", 10), 0.7), (1, 13, ("count", 37), 0.3), (3, 5, "rect", 0.0)]


def combos_for(h, w):
    out = []
    for B, N, mk, trim in COMBOS:
        if isinstance(mk, tuple) and mk[1] > h * w:
            mk = ("count", h * w - 3)
        out.append((B, N, mk, trim))
    return out


def test_kept_terms_rule():
    """The f32 rule differs from an f64 product: f32(0.7) * 10 rounds to 7.0f, while the same product in f64 is 6.99999988."""
    assert kept(10, 0.7) == 3 and 10 - math.floor(float(np.float32(0.7)) * 10) == 4
    assert kept(37, 0.3) == 26 and kept(16, 0.999) == 1 and kept(1, 0.999) == 1 and kept(1024, 0.25) == 768 and kept(5, 0.0) == 5


# ---- 1. dyadic data: bit patterns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("h,w", SHAPES + [OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_dyadic_bits(be, dt, h, w, C):
    hip, dev, _ = be
    for i, (B, N, mk, trim) in enumerate(combos_for(h, w)):
        q, bank = dyadic_case(100 + i, dt, B, N, C, h, w)
        mask = None if mk is None else make_mask(mk, B, h, w, seed=i)
        want = np_robust(q, bank, mask, trim)
        got = hip.robust_similarity(q.to(dev), bank.to(dev), None if mask is None else mask.to(dev), trim)
        assert same_bits(got, want), (dt, h, w, C, B, N, mk, trim, got.cpu().tolist(), want.tolist())
        if mk == "zero":
            assert bool(torch.isnan(got).all())
        elif N > 2 and mk != "one":
            assert int(bits(got)[B - 1, N // 2]) == int(bits(torch.tensor([-0.0]))[0])          # the planted match: -0.0


@pytest.mark.parametrize("h,w", [(8, 8), (32, 32), OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_dyadic_heavy_ties(be, dt, h, w):
    """Every d of a row equal (the m-th position lies inside ONE run of equal values), and rows of few distinct values under every trim: a
    selection that miscounts ties returns a neighbouring value or a wrong count of it."""
    hip, dev, _ = be
    for trim in (0.25, 0.5, 0.999):
        q, bank = dyadic_case(200, dt, 2, 5, 8, h, w, ties="all")
        want = np_robust(q, bank, None, trim)
        assert same_bits(hip.robust_similarity(q.to(dev), bank.to(dev), None, trim), want), (dt, h, w, trim)
        d0 = np_d(q, bank)
        assert (d0.min(axis=2) == d0.max(axis=2)).all() and (want < 0).all()
        mask = make_mask("random", 2, h, w)
        q, bank = dyadic_case(201, dt, 2, 5, 8, h, w)
        assert same_bits(hip.robust_similarity(q.to(dev), bank.to(dev), mask.to(dev), trim), np_robust(q, bank, mask, trim)), (dt, h, w, trim)


@pytest.mark.parametrize("dt", DTS)
def test_shared_bank_out_and_col_offset(be, dt):
    hip, dev, _ = be
    B, N, C, h, w = 3, 5, 8, 8, 8
    q, bank = dyadic_case(300, dt, B, N, C, h, w, shared=True)
    assert bank.shape[0] == 1
    mask = make_mask("random", B, h, w)
    want = np_robust(q, bank, mask, 0.25)
    assert same_bits(hip.robust_similarity(q.to(dev), bank.to(dev), mask.to(dev), 0.25), want)
    sentinel = torch.full((B, 11), 0.0).view(torch.int32).fill_(0x7fc12345).view(torch.float32)          # a NaN payload: any write shows
    out = sentinel.clone().to(dev)
    got = hip.robust_similarity(q.to(dev), bank.to(dev), mask.to(dev), 0.25, out=out, col_offset=4)
    assert got is out and same_bits(out[:, 4:9], want)
    keep = [0, 1, 2, 3, 9, 10]
    assert torch.equal(bits(out)[:, keep], bits(sentinel)[:, keep])


# ---- 2. random data ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("h,w", SHAPES + [OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_random_data(be, dt, h, w, C):
    """2e-5 relative, nope_similarity's bound: the trimmed form needs no more (observed on the interpreter build: at most 1.7e-7)."""
    hip, dev, _ = be
    g = torch.Generator().manual_seed(41)
    worst = 0.0
    for B, N, mk, trim in ((3, 13, None, 0.25), (1, 5, "random", 0.5), (3, 5, "rect", 0.0), (1, 13, None, 0.0)):
        q = torch.randn(B, C, h, w, generator=g)
        bank = torch.randn(B, N, C, h, w, generator=g).to(DT[dt])
        mask = None if mk is None else make_mask(mk, B, h, w)
        got = hip.robust_similarity(q.to(dev), bank.to(dev), None if mask is None else mask.to(dev), trim).cpu().double().numpy()
        err = rel_err(got, np_robust(q, bank, mask, trim))
        worst = max(worst, err)
        assert err <= RANDOM_BOUND, (dt, h, w, C, B, N, mk, trim, err)
    print(f"robust_similarity {dt} {h}x{w} C {C}: relative error {worst:.3e}")


# ---- 3. selects and NaN rules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(4, 4), (16, 16), (32, 32), OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_masked_out_pixels_do_not_leak(be, dt, h, w):
    hip, dev, _ = be
    B, N, C = 2, 5, 8
    q, bank = dyadic_case(400, dt, B, N, C, h, w)
    mask = make_mask("random", B, h, w)
    off = (mask == 0)
    for trim in (0.0, 0.5):
        want = hip.robust_similarity(q.to(dev), bank.to(dev), mask.to(dev), trim).cpu()
        assert same_bits(want, np_robust(q, bank, mask, trim))
        for fill in (float("nan"), float("inf"), -float("inf")):
            pb = torch.where(off[:, None, None].expand_as(bank), torch.full_like(bank, fill), bank)
            pq = torch.where(off[:, None].expand_as(q), torch.full_like(q, fill), q)
            for qq, bb in ((q, pb), (pq, bank), (pq, pb)):
                got = hip.robust_similarity(qq.to(dev), bb.to(dev), mask.to(dev), trim)
                assert torch.equal(bits(got), bits(want)), (dt, h, w, trim, fill)


@pytest.mark.parametrize("h,w", [(4, 4), (16, 16), (32, 32), OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_nan_and_inf_in_active_pixels(be, dt, h, w):
    hip, dev, _ = be
    B, N, C = 2, 5, 8
    q, bank = dyadic_case(500, dt, B, N, C, h, w)
    mask = make_mask("random", B, h, w)
    on = mask[1].reshape(-1).nonzero().reshape(-1)
    p = int(on[len(on) // 2])
    for trim in (0.0, 0.5):
        clean = np_robust(q, bank, mask, trim)
        nb = bank.clone().reshape(B, N, C, -1)
        nb[1, 3, 2, p] = float("nan")                       # one NaN in an active pixel of ONE hypothesis
        nb = nb.reshape(bank.shape)
        got = hip.robust_similarity(q.to(dev), nb.to(dev), mask.to(dev), trim)
        want = clean.copy()
        want[1, 3] = np.nan
        assert same_bits(got, want) and int(torch.isnan(got).sum()) == 1, (dt, h, w, trim)
        ib = bank.clone().reshape(B, N, C, -1)
        ib[1, 3, 2, p] = float("inf")                       # d = +inf: the largest value of its row
        ib = ib.reshape(bank.shape)
        got = hip.robust_similarity(q.to(dev), ib.to(dev), mask.to(dev), trim).cpu()
        want = np_robust(q, ib, mask, trim)
        assert same_bits(got, want)
        if trim == 0.0:
            assert float(got[1, 3]) == -float("inf")        # kept: -inf, not NaN
        else:
            assert math.isfinite(float(got[1, 3]))          # trimmed: finite
    # a row whose KEPT terms end in +inf under a trim: m reaches into the infinite values
    ib = bank.clone().reshape(B, N, C, -1)
    ib[1, 3, 2, on[: len(on) - 1]] = float("inf")           # all but one active pixel
    ib = ib.reshape(bank.shape)
    got = hip.robust_similarity(q.to(dev), ib.to(dev), mask.to(dev), 0.25).cpu()
    assert same_bits(got, np_robust(q, ib, mask, 0.25)) and float(got[1, 3]) == -float("inf")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_poisoned_bank_scores_nan(be, dt):
    """A bank the f16x2 range check poisoned (all NaN) still scores NaN, under a trim as well: NaNs are never trimmed away as the largest."""
    hip, dev, _ = be
    q, bank = dyadic_case(600, dt, 2, 5, 8, 16, 16)
    bank[1] = float("nan")
    for trim, mk in ((0.5, None), (0.25, "random"), (0.0, "rect")):
        mask = None if mk is None else make_mask(mk, 2, 16, 16).to(dev)
        got = hip.robust_similarity(q.to(dev), bank.to(dev), mask, trim).cpu()
        assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[0]).any())


# ---- 4. trim = 0, no mask: nope_similarity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("h,w", SHAPES + [OUTSIDE])
@pytest.mark.parametrize("dt", DTS)
def test_no_trim_no_mask_is_similarity(be, dt, h, w, C):
    hip, dev, _ = be
    q, bank = dyadic_case(700, dt, 3, 13, C, h, w)
    assert torch.equal(bits(hip.robust_similarity(q.to(dev), bank.to(dev))), bits(hip.similarity(q.to(dev), bank.to(dev))))
    g = torch.Generator().manual_seed(71)
    q = torch.randn(3, C, h, w, generator=g).to(dev)
    bank = torch.randn(3, 13, C, h, w, generator=g).to(DT[dt]).to(dev)
    assert rel_err(hip.robust_similarity(q, bank).cpu().numpy(), hip.similarity(q, bank).cpu().numpy()) <= RANDOM_BOUND


# ---- 5. the planted occlusion -------------------------------------------------------------------------------------------------------------------
def planted():
    """Bank of seeded random maps, 16 x 16, C = 8, N = 13.  The query equals bank[n*] outside a rectangle O covering 20 % of the pixels (4 rows
    of 13: 52 of 256 = 20.3 %) and is large noise inside; the decoy bank[n'] equals bank[n*] + eps outside O and the query's noise inside."""
    g = torch.Generator().manual_seed(2024)
    N, C, h, w, star, decoy = 13, 8, 16, 16, 9, 4
    bank = torch.randn(1, N, C, h, w, generator=g)
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[5:9, 2:15] = True
    noise = torch.randn(C, h, w, generator=g) * 8.0
    q = torch.where(inside, noise, bank[0, star])[None].contiguous()
    bank[0, decoy] = torch.where(inside, noise, bank[0, star] + 0.1)
    mask = (~inside).to(torch.uint8)[None].contiguous()
    return q, bank, mask, star, decoy


@pytest.mark.parametrize("dt", ["f32"])
def test_planted_occlusion(be, dt):
    """The test that fails without the feature: the plain metric prefers the decoy that reproduces the occluder, the robust score the true match."""
    hip, dev, name = be
    q, bank, mask, star, decoy = planted()
    assert abs(float((mask == 0).sum()) / 256 - 0.2) < 0.01
    # the precondition, on the f64 reference alone
    plain = np_robust(q, bank)[0]
    order = np.argsort(-plain)
    gap = (plain[order[0]] - plain[order[1]]) / np.abs(plain).max()
    assert order[0] == decoy and order[1] == star and gap > 10 * RANDOM_BOUND, (order[:3], gap)
    trimmed, masked = np_robust(q, bank, None, 0.25)[0], np_robust(q, bank, mask, 0.0)[0]
    assert int(np.argmax(trimmed)) == star and trimmed[star] == 0.0 and np.sort(trimmed)[-2] < -1.0
    assert int(np.argmax(masked)) == star and masked[star] == 0.0 and np.sort(masked)[-2] < -1.0
    # the device
    qd, bd, md = q.to(dev), bank.to(dev), mask.to(dev)
    assert int(hip.topk(hip.similarity(qd, bd), 1)[1][0, 0]) == decoy
    r = hip.robust_similarity(qd, bd, None, 0.25)
    assert int(hip.topk(r, 1)[1][0, 0]) == star and int(bits(r)[0, star]) == int(bits(torch.tensor([-0.0]))[0])
    rm = hip.robust_similarity(qd, bd, md, 0.0)
    assert int(hip.topk(rm, 1)[1][0, 0]) == star
    # the same through the model
    model = stub_model(dev)
    _, idx = model.retrieval_from_feat(qd, bd)
    assert int(idx[0, 0]) == decoy
    sim_t, idx_t = model.retrieval_from_feat(qd, bd, robust={"trim": 0.25})
    assert int(idx_t[0, 0]) == star and torch.equal(bits(sim_t), bits(r))
    sim_m, idx_m = model.retrieval_from_feat(qd, bd, robust={"mask": md, "trim": 0.0})
    assert int(idx_m[0, 0]) == star and torch.equal(bits(sim_m), bits(rm))
    vals, idx_k = model.retrieval_topk_from_feat(qd, bd, robust={"mask": md.bool(), "trim": 0.25})
    assert int(idx_k[0, 0]) == star and int(bits(vals)[0, 0]) == int(bits(torch.tensor([-0.0]))[0])


def stub_model(dev, u_net_dim=8, channels=8):
    from nope_amd.harness import StubEncoder
    from nope_amd.model import PoseConditional
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    u = UNet(u_net_dim=u_net_dim, rot_representation_dim=6, encoder=StubEncoder(channels), pose_mlp_name="single_layer", compute_dtype="f32")
    synth_init_(u, 2022)
    return PoseConditional(u, None, {"similarity_metric": "l2"}, None).to(dev)


def stand_in_network(model):
    """The interpreter build needs ~13 s per U-Net pass and ~0.4 s per hypothesis on top: on that backend the host-side tests replace the
    network by a pure per-hypothesis function of (reference map, pose) -- what they check is the scoring and the plumbing around it.  The
    device runs the U-Net."""
    def hypotheses(x, poses, out=None, out_dtype="f32", defer_range_check=False):
        p = poses.float()
        C = x.shape[1]
        shift = p[..., torch.arange(C) % p.shape[-1]]                                         # (B, N, C)
        y = x.float()[:, None] * (1.0 + 0.5 * p[..., 0])[..., None, None, None] + shift[..., None, None]
        if out is None:
            return y.to(DT[out_dtype])
        out.copy_(y)
        return out
    model.u_net.forward_hypotheses = hypotheses
    model.u_net.forward = lambda x, pose: hypotheses(x, pose[:, None])[:, 0]
    return model


# ---- 6. residual maps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(4, 4), (16, 16), (5, 7)])
@pytest.mark.parametrize("dt", DTS)
def test_residual_maps(be, dt, h, w):
    """Dyadic: bit patterns.  Random: 2^-22 relative per element (f64 arithmetic rounded once: observed 5.9e-8 <= 2^-24 for all three bank types).  An index
    outside [0, N) gives a NaN plane; a plane summed in f64 reproduces the plain score to nope_similarity's bound."""
    hip, dev, _ = be
    B, N, C = 3, 5, 8
    q, bank = dyadic_case(800, dt, B, N, C, h, w)
    got = hip.op_residual_maps(q.to(dev), bank.to(dev))
    assert tuple(got.shape) == (B, N, h, w) and same_bits(got, np_d(q, bank).reshape(B, N, h, w))
    g = torch.Generator().manual_seed(81)
    q = torch.randn(B, C, h, w, generator=g)
    bank = torch.randn(B, N, C, h, w, generator=g).to(DT[dt])
    idx = torch.tensor([[4, 0, 2], [1, 1, 7], [-1, 3, 4]])
    want = np_d(q, bank)
    got = hip.op_residual_maps(q.to(dev), bank.to(dev), idx.to(dev)).cpu().double().numpy().reshape(B, 3, -1)
    worst = 0.0
    for b in range(B):
        for j in range(3):
            n = int(idx[b, j])
            if n < 0 or n >= N:
                assert np.isnan(got[b, j]).all()
                continue
            e = np.abs(got[b, j] - want[b, n]) / want[b, n]
            worst = max(worst, float(e.max()))
            assert (e <= REL).all(), (dt, b, j, float(e.max()))
    print(f"op_residual_maps {dt} {h}x{w}: relative error {worst:.3e}")
    if (h * w) % 8 == 0:
        plain = hip.similarity(q.to(dev), bank.to(dev)).cpu().double().numpy()
        full = hip.op_residual_maps(q.to(dev), bank.to(dev)).cpu().double().numpy().reshape(B, N, -1)
        assert rel_err(-full.sum(axis=2), plain) <= RANDOM_BOUND
    shared = hip.op_residual_maps(q.to(dev), bank[:1].to(dev), idx[:, :2].clamp(0, N - 1).to(dev)).cpu().double().numpy().reshape(B, 2, -1)
    ws = np_d(q, bank[:1])
    for b in range(B):
        for j in range(2):
            n = int(idx[b, j].clamp(0, N - 1))
            assert (np.abs(shared[b, j] - ws[b, n]) <= REL * ws[b, n]).all()


# ---- 7. pool mask -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sh,Sw,H,W", [(32, 32, 4, 4), (64, 64, 16, 16), (32, 64, 4, 16), (48, 32, 16, 4)])
def test_pool_mask(be, Sh, Sw, H, W):
    hip, dev, _ = be
    B = 3
    g = torch.Generator().manual_seed(91)
    ch, cw = Sh // H, Sw // W
    area = ch * cw
    for threshold in (0.5, 0.25, 1.0, 0.3):
        min_sum = math.ceil(Fraction(threshold) * 255 * area)
        cover = torch.randint(0, 256, (B, Sh, Sw), generator=g, dtype=torch.uint8)
        cells = cover.reshape(B, H, ch, W, cw)
        # cells whose sum sits exactly at min_sum, one below and one above: a constant cell with single bytes moved
        planted_sums = {}
        for (hh, ww, delta) in ((0, 0, 0), (H - 1, W - 1, -1), (1, 2, 1)):
            total = min_sum + delta
            if not 0 <= total <= 255 * area:
                continue
            base, rem = divmod(total, area)
            cell = torch.full((area,), base, dtype=torch.int64)
            cell[:rem] += 1
            cells[0, hh, :, ww, :] = cell.reshape(ch, cw).to(torch.uint8)
            planted_sums[(hh, ww)] = total
        cover = cells.reshape(B, Sh, Sw).contiguous()
        sums = cover.numpy().astype(np.int64).reshape(B, H, ch, W, cw).sum(axis=(2, 4))
        want = (sums >= min_sum).astype(np.uint8)
        got = hip.op_pool_mask(cover.to(dev), (H, W), threshold)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), threshold
        assert (0, 0) in planted_sums and (H - 1, W - 1) in planted_sums
        for (hh, ww), total in planted_sums.items():
            assert sums[0, hh, ww] == total and want[0, hh, ww] == (1 if total >= min_sum else 0)
    # f32 visibility on dyadic planes: multiples of 1/8, so sums and means are exact
    vis = torch.randint(0, 9, (B, Sh, Sw), generator=g).float() / 8
    vis[1, :ch, :cw] = 0.5                                   # a mean exactly at the threshold counts
    means = vis.double().numpy().reshape(B, H, ch, W, cw).sum(axis=(2, 4)) / area
    for threshold in (0.5, 0.625):
        got = hip.op_pool_mask(vis.to(dev), (H, W), threshold)
        assert np.array_equal(got.cpu().numpy(), (means >= threshold).astype(np.uint8))
    assert int(hip.op_pool_mask(vis.to(dev), (H, W), 0.5)[1, 0, 0]) == 1
    with pytest.raises(hip.NopeError):
        hip.op_pool_mask(vis.to(dev), (H + 1, W), 0.5)
    with pytest.raises(hip.NopeError):
        hip.op_pool_mask(vis.double().to(dev), (H, W), 0.5)


# ---- 8. host side -------------------------------------------------------------------------------------------------------------------------------
def test_robust_none_is_todays_path(be):
    hip, dev, _ = be
    model = stub_model(dev)
    g = torch.Generator().manual_seed(11)
    q = torch.randn(2, 8, 16, 16, generator=g).to(dev)
    bank = torch.randn(2, 7, 8, 16, 16, generator=g).to(dev)
    sim0, idx0 = model.retrieval_from_feat(q, bank)
    sim1, idx1 = model.retrieval_from_feat(q, bank, robust=None)
    assert torch.equal(bits(sim0), bits(sim1)) and torch.equal(idx0, idx1)
    assert torch.equal(bits(sim0), bits(hip.similarity(q, bank)))
    v0, i0 = model.retrieval_topk_from_feat(q, bank)
    v1, i1 = model.retrieval_topk_from_feat(q, bank, robust=None)
    assert torch.equal(bits(v0), bits(v1)) and torch.equal(i0, i1)
    # the robust row feeds pose_distribution unchanged
    from nope_amd.harness import random_rotations
    sim_r, _ = model.retrieval_from_feat(q, bank, robust={"trim": 0.25})
    modes = model.pose_distribution(sim_r, random_rotations(7, torch.Generator().manual_seed(1))[None].to(dev), temperature=10.0)
    assert tuple(modes.prob.shape) == (2, 7) and bool(torch.isfinite(modes.entropy).all())


def test_not_implemented_combinations(be, monkeypatch):
    hip, dev, _ = be
    from nope_amd import model as M
    model = stub_model(dev)
    robust = {"trim": 0.25}
    x = torch.zeros(1, 8, 8, 8).to(dev)
    rel = torch.zeros(1, 4, 6).to(dev)
    tp = torch.eye(3)[None, None].repeat(1, 4, 1, 1).to(dev)
    with pytest.raises(NotImplementedError):
        model.predict_pose(x, x, rel, tp, refine_iters=1, robust=robust)
    with pytest.raises(NotImplementedError):
        model.retrieve_multi_from_feat(x, x[:, None], tp[:, :1], tp, robust=robust)
    with pytest.raises(NotImplementedError):
        model.retrieve_multi_coarse_to_fine_from_feat(x, x[:, None], tp[:, :1], tp, robust=robust)
    with pytest.raises(NotImplementedError):
        model.predict_pose_multi(x, x[:, None], tp[:, :1], tp, robust=robust)
    monkeypatch.setattr(M.ndist, "world", lambda: (0, 2))
    model.template_parallel = True
    try:
        for call in (lambda: model.retrieval_from_feat(x, x[:, None], shard=False, robust=robust),
                     lambda: model.retrieval_topk_from_feat(x, x[:, None], shard=False, robust=robust),
                     lambda: model.retrieve_robust(x, x, rel, trim=0.25)):
            with pytest.raises(NotImplementedError):
                call()
    finally:
        model.template_parallel = False


def test_argument_errors(be):
    hip, dev, name = be
    q = torch.zeros(2, 8, 4, 4).to(dev)
    bank = torch.zeros(2, 3, 8, 4, 4).to(dev)
    for trim in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(hip.NopeError):
            hip.robust_similarity(q, bank, None, trim)
    # the C entry refuses it as well (NOPE_ERR_ARG), before anything is written
    out = torch.full((2, 3), 7.0).to(dev)
    l = hip.lib()
    for trim in (1.0, -0.5, float("nan")):
        assert l.dll.nope_robust_similarity(q.data_ptr(), bank.data_ptr(), 0, None, trim, out.data_ptr(), 2, 3, 8, 4, 4, 3 * 8 * 16, 3, None) == -1
    assert bool((out == 7).all())
    for bad in (torch.ones(2, 4, 5, dtype=torch.uint8), torch.ones(1, 4, 4, dtype=torch.uint8), torch.ones(2, 16, dtype=torch.uint8),
                torch.ones(2, 4, 4), torch.ones(2, 4, 4, dtype=torch.int32)):
        with pytest.raises(hip.NopeError):
            hip.robust_similarity(q, bank, bad.to(dev), 0.0)
    with pytest.raises(hip.NopeError):
        hip.robust_similarity(q, torch.zeros(2, 3, 8, 4, 5).to(dev))
    with pytest.raises(hip.NopeError):
        hip.op_residual_maps(q, bank, torch.zeros(3, 2, dtype=torch.int64).to(dev))
    if name == "gpu":                                   # a CPU tensor on the GPU path is an error, never a detour
        with pytest.raises(hip.NopeError):
            hip.robust_similarity(q.cpu(), bank.cpu())
        with pytest.raises(hip.NopeError):
            hip.robust_similarity(q, bank, torch.ones(2, 4, 4, dtype=torch.uint8))
        with pytest.raises(hip.NopeError):
            hip.op_residual_maps(q.cpu(), bank.cpu())
        with pytest.raises(hip.NopeError):
            hip.op_pool_mask(torch.ones(1, 8, 8), (4, 4))
    model = stub_model(dev)
    with pytest.raises(TypeError):
        model.retrieval_from_feat(q, bank, robust={"trim": 0.25, "masks": None})
    with pytest.raises(hip.NopeError):
        model.retrieval_from_feat(q, bank, robust={"trim": 1.0})


_C2F = {}


def _c2f_case(dev, name):
    """A u_net_dim 8 network around a StubEncoder(8) on 8 x 8 maps, B = 1, the level-1 upper grid (91 poses), a random mask: built once per backend."""
    if name not in _C2F:
        from nope_amd import harness
        model = stub_model(dev) if name == "gpu" else stand_in_network(stub_model(dev))
        batch = harness.synthetic_batch(1, 0, 8, seed=7, device="cpu", pose_level=1)
        g = torch.Generator().manual_seed(7)
        batch["query"] = torch.randn(1, 8, 8, 8, generator=g)
        batch["reference"] = torch.randn(1, 8, 8, 8, generator=g)
        _C2F[name] = model, {k: v.to(dev) for k, v in batch.items()}, make_mask("random", 1, 8, 8).to(dev)
    return _C2F[name]


def test_coarse_to_fine_robust_matches_exhaustive(be):
    """On a level-1 grid every column the search evaluates holds the bits of the exhaustive robust row; retrieve_robust is
    generate_and_retrieve with the robust score."""
    hip, dev, name = be
    model, b, mask = _c2f_case(dev, name)
    robust = {"mask": mask, "trim": 0.25}
    N = b["all_relativeR"].shape[1]
    sim, idx, bank = model.retrieve_robust(b["query"], b["reference"], b["all_relativeR"], mask=mask, trim=0.25)
    assert tuple(sim.shape) == (1, N) and torch.equal(bits(sim), bits(hip.robust_similarity(b["query"], bank, mask, 0.25)))
    assert torch.equal(idx, hip.topk(sim, 5)[1])
    plain, _, bank0 = model.generate_and_retrieve(b["query"], b["reference"], b["all_relativeR"])
    assert torch.equal(bits(bank0), bits(bank)) and not torch.equal(bits(plain), bits(sim))
    c2f = model.retrieve_coarse_to_fine(b["query"], b["reference"], b["all_relativeR"], b["template_poses"], robust=robust)
    ev = c2f.evaluated.cpu().bool()
    assert 26 <= int(ev.sum()) < N
    full, got = sim.cpu(), c2f.similarity.cpu()
    err = float((got[ev].double() - full[ev].double()).abs().max() / full.abs().max())
    print("c2f robust vs exhaustive robust row, relative error:", err)
    assert torch.equal(bits(got)[ev], bits(full)[ev]), err
    assert bool(torch.isneginf(got[~ev]).all())
    pred, score = model.predict_pose(b["query"], b["reference"], b["all_relativeR"], b["template_poses"], robust=robust)
    assert torch.equal(bits(score), bits(torch.gather(sim, 1, idx)))
    pred_c, score_c = model.predict_pose(b["query"], b["reference"], b["all_relativeR"], b["template_poses"], coarse_to_fine=True, robust=robust)
    assert torch.equal(bits(score_c), bits(torch.gather(c2f.similarity, 1, c2f.nearest_idx)))


# ---- 9. harness -----------------------------------------------------------------------------------------------------------------------------------
def test_harness_occlude_and_eval(be):
    hip, dev, name = be
    from nope_amd import harness
    clean = harness.synthetic_batch(1, 8, 64, seed=3, device=dev)
    batch, vis = harness.occlude_queries(clean, 0.2, 3)
    assert tuple(vis.shape) == (1, 64, 64) and vis.dtype == torch.float32 and abs(float((vis == 0).float().mean()) - 0.2) < 0.01
    assert set(vis.unique().cpu().tolist()) == {0.0, 1.0}
    outside = (vis[:, None] == 1).expand_as(batch["query"])
    assert torch.equal(batch["query"][outside], clean["query"][outside]) and not torch.equal(batch["query"], clean["query"])
    again, _ = harness.occlude_queries(clean, 0.2, 3)
    assert torch.equal(again["query"], batch["query"]) and torch.equal(batch["reference"], clean["reference"])
    model = harness.build_model(seed=7, compute_dtype="f32", device=dev, u_net_dim=8, encoder="stub")
    if name == "emu":
        stand_in_network(model)
    sim_a, idx_a, res_a = harness.eval_geodesic(model, batch)
    sim_b, idx_b, res = harness.eval_geodesic(model, batch, robust={"trim": 0.25, "use_mask": True})
    assert torch.equal(bits(sim_a), bits(sim_b)) and torch.equal(idx_a, idx_b)
    assert {k: v for k, v in res.items() if not k.startswith("robust/")} == res_a                     # the old keys, the old values
    rk = sorted(k for k in res if k.startswith("robust/"))
    assert "robust/top1_agree" in rk and len(rk) == len(res_a) and all(math.isfinite(res[k]) for k in rk)


# ---- 10. determinism ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_deterministic(be, dt):
    hip, dev, _ = be
    g = torch.Generator().manual_seed(13)
    q = torch.randn(3, 8, 32, 32, generator=g).to(dev)
    bank = torch.randn(3, 13, 8, 32, 32, generator=g).to(DT[dt]).to(dev)
    mask = make_mask("random", 3, 32, 32).to(dev)
    a = hip.robust_similarity(q, bank, mask, 0.25)
    b = hip.robust_similarity(q, bank, mask, 0.25)
    assert torch.equal(bits(a), bits(b)) and bool(torch.isfinite(a).all())
