"""Sub-grid pose refinement (csrc/kernels_refine.hip, PoseConditional.refine_from_feat / predict_pose, harness.eval_geodesic(refine_iters)).

Every test runs on the interpreter build ("emu") and, marked `gpu`, on the device (the host-side chunking check: device only).  The
interpreter needs ~15 s for one U-Net pass whatever its size, so its cases are cut to the fewest passes that still reach every kernel.  The kernels are checked against NumPy restatements
(f64, the normal equations in extended precision), the whole path on planted problems: the query embedding is the network's own output at
a known off-grid pose, so the answer is known.

Bounds.  Normal equations, per entry: 2 (C h w + 8) 2^-53 sum|terms| -- the worst case of ANY summation order of C h w terms plus the
roundings of a term; the sum of |terms| is computed here.  3x3 algebra (Gram-Schmidt, exponential map, clamp, solve, poses): 1e-12
absolute -- a few dozen f64 operations on O(1) numbers with margin for the device's sin / cos.  Planted convergence: the same loop on
the oracle in f64; the f32 and f64 trajectories of the CPU study stay within 0.0026 degrees of each other, the
device's f32 forward carries the same kind of noise but not the same bits: 0.02 degrees per iteration; the final error against the
planted pose <= 0.005 degrees (15x the worst f32 CPU value after 3 iterations; 0.02 degrees for the 2 iterations of the CPU suite).
"""
import math

import numpy as np
import pytest
import torch

from oracle import nope_ref as R
from tests.util import StubEncoder

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
H_FD, CLAMP_DEG, DAMPING = 1e-2, 10.0, 1e-6


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu"), request.param


# ---- NumPy restatements (f64) ----------------------------------------------------------------------------------------------------------
def gs(a):
    """rotation_6d_to_matrix on the six numbers a (first two rows)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b1 = a[:3] / max(np.linalg.norm(a[:3]), 1e-12)
    b2 = a[3:6] - np.dot(b1, a[3:6]) * b1
    b2 = b2 / max(np.linalg.norm(b2), 1e-12)
    return np.stack([b1, b2, np.cross(b1, b2)])


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def expm(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    if t < 1e-6:
        return np.eye(3) + skew(w) + 0.5 * skew(w) @ skew(w)
    K = skew(w / t)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def seven(Rm, h=H_FD):
    """The seven poses of a candidate as (7, 6) f64 (not yet rounded to f32)."""
    rows = [Rm[:2].reshape(6)]
    for a in range(3):
        for sgn in (1.0, -1.0):
            w = np.zeros(3)
            w[a] = sgn * h
            rows.append((expm(w) @ Rm)[:2].reshape(6))
    return np.stack(rows)


def angle_deg(A, B):
    M = A @ B.T
    # atan2 form: accurate near 0, where acos((tr - 1) / 2) loses half the digits
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return math.degrees(math.atan2(s, 0.5 * (np.trace(M) - 1.0)))


def gn_step(ne, Rm, max_step=math.radians(CLAMP_DEG), damping=DAMPING):
    A = np.array([[ne[0], ne[1], ne[2]], [ne[1], ne[3], ne[4]], [ne[2], ne[4], ne[5]]])
    w = np.linalg.solve(A + damping * np.diag(np.diag(A)), -ne[6:9])
    n = np.linalg.norm(w)
    clamped = n > max_step
    if clamped:
        w = w * (max_step / n)
    return gs((expm(w) @ Rm)[:2].reshape(6)), w, clamped


def assert_poses(poses_f32, Rm, h=H_FD):
    """poses (7, 6) f32 from the device against the f64 restatement: the correctly rounded f32 of a value within 1e-12."""
    want = seven(Rm, h)
    got = poses_f32.astype(np.float64)
    assert np.all(np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-12), np.abs(got - want).max()


def normal_eq_ref(q, maps, h):
    """(ne (B,k,10), sum of |terms| (B,k,10)) in extended precision."""
    L = np.longdouble
    q, m = q.astype(L), maps.astype(L)
    r = m[:, :, 0] - q[:, None]
    J = [(m[:, :, 1 + 2 * a] - m[:, :, 2 + 2 * a]) / L(2.0 * h) for a in range(3)]
    terms = [J[0] * J[0], J[0] * J[1], J[0] * J[2], J[1] * J[1], J[1] * J[2], J[2] * J[2], J[0] * r, J[1] * r, J[2] * r, r * r]
    ne = np.stack([t.sum(axis=(2, 3)) for t in terms], -1)
    mag = np.stack([np.abs(t).sum(axis=(2, 3)) for t in terms], -1)
    return ne, mag


# ---- 1. normal equations ------------------------------------------------------------------------------------------------------------------
NE_SHAPES = [(1, 1, 8, 8, 8), (2, 3, 8, 32, 32), (1, 5, 4, 16, 16), (2, 2, 3, 4, 4),
             (1, 2, 2, 4, 260),        # 1040 pixels: two pixel slices, the second one ragged
             (1, 1, 1, 32, 96)]        # 3072 pixels: three full slices


@pytest.mark.parametrize("shape", NE_SHAPES)
def test_normal_equations(be, shape):
    hip, dev, _ = be
    B, k, C, H, W = shape
    g = torch.Generator().manual_seed(11 + B * k * C + H * W)
    q = torch.randn(B, C, H, W, generator=g)
    maps = q[:, None, None] + 0.3 * torch.randn(B, k, 7, C, H, W, generator=g)
    # planted: candidate (0, 0) has t_{+y} = t_{-y}; the last candidate has t0 = q; with B * k > 2 a middle candidate holds one NaN
    maps[0, 0, 4] = maps[0, 0, 3]
    maps[B - 1, k - 1, 0] = q[B - 1]
    nan_at = None
    if B * k > 2:
        nan_at = (0, 1) if k > 1 else (1, 0)
        maps[nan_at[0], nan_at[1], 5, C - 1, H - 1, W // 2] = float("nan")
    got = hip.op_refine_normal_eq(q.to(dev), maps.to(dev), H_FD).cpu().numpy()
    assert got.shape == (B, k, 10) and got.dtype == np.float64
    want, mag = normal_eq_ref(q.numpy().reshape(B, C, H * W), maps.numpy().reshape(B, k, 7, C, H * W), H_FD)
    bound = 2.0 * (C * H * W + 8) * 2.0 ** -53 * mag
    for b in range(B):
        for j in range(k):
            if nan_at == (b, j):
                assert np.isnan(got[b, j]).any()
                continue
            err = np.abs(got[b, j].astype(np.longdouble) - want[b, j])
            print(f"normal_eq {shape} cand ({b},{j}): max err / bound {float((err / np.maximum(bound[b, j], 1e-300)).max()):.3f}")
            assert np.all(err <= bound[b, j]), (b, j, err, bound[b, j])
    if nan_at != (0, 0):
        assert np.all(got[0, 0, [1, 3, 4, 7]] == 0.0)          # row and column y of A, and g_y: exactly zero
    if nan_at != (B - 1, k - 1):
        assert np.all(got[B - 1, k - 1, 6:] == 0.0)            # g = 0 and cost = 0 exactly
    if nan_at is not None:                                     # the NaN poisons its own candidate only
        others = np.ones((B, k), dtype=bool)
        others[nan_at] = False
        assert np.isfinite(got[others]).all()


def test_normal_equations_unsupported_size(be):
    hip, dev, _ = be
    q, maps = torch.zeros(1, 2, 4, 6), torch.zeros(1, 1, 7, 2, 4, 6)          # h w = 24
    with pytest.raises(hip.NopeError, match=r"\(-6\)"):
        hip.op_refine_normal_eq(q.to(dev), maps.to(dev), H_FD)


# ---- 2. init and step -----------------------------------------------------------------------------------------------------------------------
def test_init(be):
    hip, dev, _ = be
    g = torch.Generator().manual_seed(21)
    B, N, k = 3, 9, 4
    rel = torch.randn(B, N, 6, generator=g)                                    # not orthonormal: Gram-Schmidt has work to do
    idx = torch.randint(0, N, (B, k), generator=g)
    idx[0, 1] = idx[0, 0]                                                      # a repeated index
    dR, dR0, poses, status = hip.op_refine_init(rel.to(dev), idx.to(dev), H_FD)
    assert torch.equal(dR, dR0) and dR.dtype == torch.float64 and poses.dtype == torch.float32 and tuple(poses.shape) == (B, 7 * k, 6)
    assert int(status.abs().sum()) == 0
    assert torch.equal(poses.view(B, k, 7, 6)[:, :, 0].cpu(), dR.cpu()[:, :, :2].reshape(B, k, 6).float())      # row 0: f32(first two rows)
    dRn, pn = dR.cpu().numpy(), poses.cpu().numpy().reshape(B, k, 7, 6)
    for b in range(B):
        for j in range(k):
            want = gs(rel[b, idx[b, j]].numpy())
            assert np.abs(dRn[b, j] - want).max() <= 1e-12
            assert_poses(pn[b, j], dRn[b, j])
    # an index outside the grid is reported per candidate and never read out of bounds
    bad = idx.clone()
    bad[1, 2] = N
    bad[2, 0] = -1
    st = hip.op_refine_init(rel.to(dev), bad.to(dev), H_FD)[3].cpu()
    assert st[1, 2] == hip.REFINE_BAD_INDEX and st[2, 0] == hip.REFINE_BAD_INDEX and int((st != 0).sum()) == 2


def _random_rot(g):
    return gs(torch.randn(6, generator=g, dtype=torch.float64).numpy())


def test_step(be):
    hip, dev, _ = be
    g = torch.Generator().manual_seed(22)
    B, k = 2, 6
    n = B * k
    dR0 = np.stack([_random_rot(g) for _ in range(n)]).reshape(B, k, 3, 3)
    ne = np.zeros((B, k, 10))
    for c in range(n):
        J = torch.randn(20, 3, generator=g, dtype=torch.float64).numpy()
        A = J.T @ J
        gvec = torch.randn(3, generator=g, dtype=torch.float64).numpy() * (0.5 if c % 2 == 0 else 40.0)      # inside / beyond the clamp
        ne[c // k, c % k] = [A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2], *gvec, 1.0 + c]
    # the cases that must not move dR: singular A (a zero row and column; all zero), g = 0, a non-finite entry anywhere
    no_step = {(0, 1): hip.REFINE_SINGULAR, (0, 3): hip.REFINE_SINGULAR, (1, 0): hip.REFINE_ZERO_STEP, (1, 2): hip.REFINE_NONFINITE,
               (1, 4): hip.REFINE_NONFINITE}
    ne[0, 1, [1, 3, 4]] = 0.0
    ne[0, 3, :6] = 0.0
    ne[1, 0, 6:9] = 0.0
    ne[1, 2, 2] = float("nan")
    ne[1, 4, 9] = float("inf")
    dR = torch.from_numpy(dR0.copy()).to(dev)
    poses = torch.full((B, 7 * k, 6), float("nan"), dtype=torch.float32, device=dev)
    status = hip.op_refine_step(torch.from_numpy(ne).to(dev), dR, poses, H_FD, math.radians(CLAMP_DEG), DAMPING).cpu().numpy()
    got, pn = dR.cpu().numpy(), poses.cpu().numpy().reshape(B, k, 7, 6)
    seen_clamped = seen_free = 0
    for b in range(B):
        for j in range(k):
            assert_poses(pn[b, j], got[b, j])
            if (b, j) in no_step:
                assert status[b, j] == no_step[(b, j)]
                assert got[b, j].tobytes() == dR0[b, j].tobytes()              # bit for bit
                continue
            want, w, clamped = gn_step(ne[b, j], dR0[b, j])
            assert status[b, j] == (hip.REFINE_CLAMPED if clamped else 0)
            assert np.abs(got[b, j] - want).max() <= 1e-12, (b, j, np.abs(got[b, j] - want).max())
            assert np.abs(got[b, j] @ got[b, j].T - np.eye(3)).sum(axis=1).max() <= 1e-14
            if clamped:                    # lands on the clamp, direction kept
                seen_clamped += 1
                M = got[b, j] @ dR0[b, j].T
                axis = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
                assert abs(angle_deg(got[b, j], dR0[b, j]) - CLAMP_DEG) <= 1e-10
                assert np.abs(axis / np.linalg.norm(axis) - w / np.linalg.norm(w)).max() <= 1e-10
            else:
                seen_free += 1
    assert seen_clamped >= 2 and seen_free >= 2


# ---- 3. select ----------------------------------------------------------------------------------------------------------------------------
def test_select(be):
    hip, dev, _ = be
    g = torch.Generator().manual_seed(23)
    B, k, N = 3, 5, 12
    nan = float("nan")
    idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(B)])
    sim = torch.randn(B, N, generator=g)
    old = torch.gather(sim, 1, idx).clone()
    # sample 0: better / equal / NaN / worse / better -- sample 1: ties between final scores -- sample 2: a NaN retrieval score, all worse
    old[0] = torch.tensor([-5.0, -4.0, -3.0, -2.0, -6.0]); new0 = [-1.0, -4.0, nan, -2.5, -5.5]
    old[1] = torch.tensor([-3.0, -3.0, -7.0, -3.0, -9.0]); new1 = [-3.5, -2.0, -3.0, -3.0, -2.0]
    old[2] = torch.tensor([-1.0, nan, -2.0, -3.0, -4.0]); new2 = [-1.5, 0.0, -2.5, -3.0, -4.5]
    sim.scatter_(1, idx, old)
    new = torch.tensor([new0, new1, new2])
    dR = torch.from_numpy(np.stack([_random_rot(g) for _ in range(B * k)]).reshape(B, k, 3, 3))
    dR0 = torch.from_numpy(np.stack([_random_rot(g) for _ in range(B * k)]).reshape(B, k, 3, 3))
    tpl = torch.from_numpy(np.stack([_random_rot(g) for _ in range(B * N)]).reshape(B, N, 3, 3))
    for shared in (False, True):
        T = tpl[:1] if shared else tpl
        r = hip.op_refine_select(dR.to(dev), dR0.to(dev), new.to(dev), sim.to(dev), idx.to(dev), T.to(dev))
        for b in range(B):
            acc = [bool(new[b, j] > old[b, j]) for j in range(k)]             # strict; False with a NaN on either side
            fin = [float(new[b, j]) if acc[j] else float(old[b, j]) for j in range(k)]
            key = [math.inf if f != f else f for f in fin]
            order = sorted(range(k), key=lambda j: (-key[j], j))              # descending, ties -> the lower retrieval rank
            assert r.order[b].cpu().tolist() == order
            assert r.accepted[b].cpu().tolist() == [acc[j] for j in order]
            for pos, j in enumerate(order):
                assert np.array_equal(np.float32(fin[j]), r.score[b, pos].cpu().numpy(), equal_nan=True)
                assert np.array_equal(old[b, j].numpy(), r.score_init[b, pos].cpu().numpy(), equal_nan=True)
                keep = (dR if acc[j] else dR0)[b, j]
                assert torch.equal(r.dR[b, pos].cpu(), keep) and torch.equal(r.rot6d[b, pos].cpu(), keep[:2].reshape(6).float())
                Tj = T[0 if shared else b, idx[b, j]].numpy()
                if acc[j]:
                    want = (dR[b, j].numpy() @ dR0[b, j].numpy().T) @ Tj
                    assert np.abs(r.pred_R[b, pos].cpu().numpy() - want).max() <= 1e-12
                else:
                    assert r.pred_R[b, pos].cpu().numpy().tobytes() == Tj.tobytes()       # reverted: the grid pose itself
        assert r.accepted[0].cpu().tolist().count(True) == 2 and not bool(r.accepted[2].any())
    assert hip.op_refine_select(dR.to(dev), dR0.to(dev), new.to(dev), sim.to(dev), idx.to(dev)).pred_R is None


# ---- 4. planted convergence through the whole path ---------------------------------------------------------------------------------------
def _tiny_unet(seed, cdt="f32"):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    u = UNet(u_net_dim=8, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
    synth_init_(u, seed)
    return u


def _oracle_refine(forward64, x64, q64, start, iters):
    """The loop of refine_from_feat on the oracle in f64, for one candidate: x64 (1,C,h,w), q64 (C,h,w), start (3,3) -> [dR after every iteration]."""
    Rm, out = start.copy(), []
    for _ in range(iters):
        poses = torch.from_numpy(seven(Rm).astype(np.float32)).double()        # the poses travel as f32 rows
        t = forward64(x64.expand(7, -1, -1, -1), poses).numpy().reshape(7, -1)
        r = t[0] - q64.reshape(-1)
        J = np.stack([(t[1 + 2 * a] - t[2 + 2 * a]) / (2 * H_FD) for a in range(3)], 1)
        A, gv = J.T @ J, J.T @ r
        Rm = gn_step(np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2], *gv, r @ r]), Rm)[0]
        out.append(Rm)
    return out


def _planted_case(hip, dev, model, forward64, B, starts_deg, iters, seed, traj_tol, final_tol, tag, query64=None):
    """Queries = the network at dR_true; candidate j of every sample starts starts_deg[j] away from it.  forward64: the oracle in f64 (the
    trajectory is compared with its loop), or None: only the final error is bounded.  Returns the result."""
    g = torch.Generator().manual_seed(100 + seed)
    k = len(starts_deg)
    x = torch.randn(B, 8, 8, 8, generator=g)
    true = [_random_rot(g) for _ in range(B)]
    rel = torch.zeros(B, k, 6)
    for b in range(B):
        for j, deg in enumerate(starts_deg):
            ax = torch.randn(3, generator=g, dtype=torch.float64).numpy()
            rel[b, j] = torch.from_numpy((expm(math.radians(deg) * ax / np.linalg.norm(ax)) @ true[b])[:2].reshape(6)).float()
    true6 = torch.stack([torch.from_numpy(t[:2].reshape(6)).float() for t in true])
    xd = x.to(dev)
    first = model.u_net.forward_hypotheses(xd, torch.cat((true6[:, None], rel), 1).to(dev))      # one pass: the query and the starts' maps
    q = first[:, 0].contiguous()                                                # realizable: the device network's own output
    sim = hip.similarity(q, first[:, 1:].contiguous())                          # (B, k): the retrieval scores of the starts
    idx = torch.arange(k).expand(B, k).contiguous().to(dev)
    r = model.refine_from_feat(q, xd, rel.to(dev), idx, sim, iters=iters, fd_step=H_FD, max_step_deg=CLAMP_DEG, damping=DAMPING)
    traj = r.trajectory.cpu().numpy()
    assert traj.shape == (iters + 1, B, k, 3, 3) and tuple(r.costs.shape) == (iters, B, k)
    worst_traj = worst_final = 0.0
    for b in range(B):
        if forward64 is not None:
            q64 = forward64(x[b:b + 1].double(), torch.from_numpy(true[b][:2].reshape(1, 6).astype(np.float32)).double())[0].numpy()
        for j in range(k):
            start = gs(rel[b, j].numpy())
            assert np.abs(traj[0, b, j] - start).max() <= 1e-12
            if forward64 is not None:
                want = _oracle_refine(forward64, x[b:b + 1].double(), q64, start, iters)
                for it in range(iters):
                    worst_traj = max(worst_traj, angle_deg(traj[it + 1, b, j], want[it]))
            worst_final = max(worst_final, angle_deg(traj[iters, b, j], true[b]))
    print(f"planted[{tag}] seed {seed} starts {starts_deg} iters {iters}: device vs f64 oracle <= {worst_traj:.2e} deg, final error <= {worst_final:.2e} deg, "
          f"costs {r.costs.cpu().numpy().max(axis=(1, 2))}")
    assert worst_traj <= traj_tol and worst_final <= final_tol
    assert bool(r.accepted.all()) and bool((r.score > r.score_init).all())
    # the result is the last trajectory entry in the final order, and that order is descending
    order = r.order.cpu()
    for b in range(B):
        assert torch.equal(r.relR[b].cpu(), torch.from_numpy(traj[iters, b])[order[b]])
    assert bool((r.score[:, :-1] >= r.score[:, 1:]).all())
    return r


def test_planted_convergence(be):
    from nope_amd.model import PoseConditional
    hip, dev, name = be
    for seed in ((3, 4, 5) if name == "gpu" else (3,)):
        u = _tiny_unet(seed)
        sd64 = {k_: v.double() for k_, v in u.own_state_dict().items()}
        forward64 = lambda x, p: R.unet_forward(sd64, x, p)
        model = PoseConditional(u, None, {"similarity_metric": "l2"}, None).to(dev)
        if name == "gpu":
            _planted_case(hip, dev, model, forward64, 2, (4.0, 8.0, 10.0), 3, seed, 0.02, 0.005, name)
            _planted_case(hip, dev, model, forward64, 1, (20.0,), 4, seed, 0.02, 0.005, name)
        else:       # the CPU suite: one candidate, two iterations (the interpreter needs ~15 s per U-Net pass whatever its size: four passes)
            _planted_case(hip, dev, model, forward64, 1, (4.0,), 2, seed, 0.02, 0.02, name)


@pytest.mark.gpu
def test_chunked_forwards_same_result(gpu):
    """max_hypotheses_per_launch below 7k and below B * 7k: the refinement chunks its forwards as generate_templates does -- same trajectory.
    (Host-side slicing only, the same code on both backends: on the device, where a U-Net pass costs microseconds and not 15 s.)"""
    from nope_amd.model import PoseConditional
    hip, dev = gpu, "cuda"
    u = _tiny_unet(3)
    g = torch.Generator().manual_seed(7)
    B, k = 2, 2
    x, q = torch.randn(B, 8, 8, 8, generator=g).to(dev), torch.randn(B, 8, 8, 8, generator=g).to(dev)
    rel = torch.randn(B, 4, 6, generator=g).to(dev)
    idx = torch.tensor([[3, 0], [1, 2]]).to(dev)
    sim = torch.randn(B, 4, generator=g).to(dev)
    outs = []
    for max_hyp in (512, 14, 5):
        m = PoseConditional(u, None, {"similarity_metric": "l2"}, None, max_hypotheses_per_launch=max_hyp).to(dev)
        outs.append(m.refine_from_feat(q, x, rel, idx, sim, iters=1))
    for o in outs[1:]:
        worst = max(angle_deg(a, b_) for a, b_ in zip(o.trajectory[1].cpu().numpy().reshape(-1, 3, 3), outs[0].trajectory[1].cpu().numpy().reshape(-1, 3, 3)))
        assert worst <= 0.02, worst      # (another GEMM row count takes another launch plan: equal to rounding, as the banks are)


# ---- 5. API ------------------------------------------------------------------------------------------------------------------------------------
def _planted_batch(model, dev, B, n_templates, off_deg, seed=5):
    """harness.synthetic_batch with embeddings for images (StubEncoder) and the query planted: the network's output at a pose off_deg away
    from template j0[b] of the grid."""
    from nope_amd import harness
    batch = harness.synthetic_batch(B, n_templates, 8, seed=seed, device="cpu")
    g = torch.Generator().manual_seed(seed)
    batch["reference"] = torch.randn(B, 8, 8, 8, generator=g)
    gt_rel, q_pose = [], []
    for b in range(B):
        j0 = (3 + 5 * b) % n_templates
        ax = torch.randn(3, generator=g, dtype=torch.float64).numpy()
        off = expm(math.radians(off_deg) * ax / np.linalg.norm(ax))
        gt_rel.append(torch.from_numpy((off @ gs(batch["all_relativeR"][b, j0].numpy()))[:2].reshape(6)).float())
        q_pose.append(torch.from_numpy(off @ batch["template_poses"][b, j0].numpy()))
    batch["gt_relativeR"], batch["query_pose"] = torch.stack(gt_rel), torch.stack(q_pose)
    batch = {k_: v.to(dev) for k_, v in batch.items()}
    batch["query"] = model.u_net(batch["reference"], batch["gt_relativeR"])
    return batch


def test_predict_pose_and_eval_geodesic(be, tmp_path):
    from nope_amd import harness
    from nope_amd.model import PoseConditional
    hip, dev, name = be
    model = PoseConditional(_tiny_unet(3), None, {"similarity_metric": "l2"}, None).to(dev)
    B = 2 if name == "gpu" else 1
    batch = _planted_batch(model, dev, B, 12 if name == "gpu" else 6, 6.0)
    # refine_iters = 0: template_poses[nearest_idx] and the retrieval scores, bit for bit
    sim, idx, res_a = harness.eval_geodesic(model, batch, save_path=str(tmp_path / "a"))
    pred, score = model.predict_pose(batch["query"], batch["reference"], batch["all_relativeR"], batch["template_poses"])
    rows = torch.arange(B)[:, None]
    assert pred.dtype == torch.float64 and torch.equal(pred.cpu(), batch["template_poses"].cpu()[rows, idx.cpu()])
    assert torch.equal(score.cpu(), torch.gather(sim, 1, idx).cpu())
    if name == "gpu":             # one grid shared by every query
        pred1, _ = model.predict_pose(batch["query"], batch["reference"], batch["all_relativeR"], batch["template_poses"][:1])
        assert torch.equal(pred1, pred)
    # eval_geodesic(refine_iters=0) is the call without the argument: same dict, same file
    _, _, res_b = harness.eval_geodesic(model, batch, save_path=str(tmp_path / "b"), refine_iters=0)
    assert res_a == res_b and not any(k_.startswith("refined/") for k_ in res_b)
    za, zb = np.load(str(tmp_path / "a.npz")), np.load(str(tmp_path / "b.npz"))
    assert za.files == zb.files and all(za[f].tobytes() == zb[f].tobytes() for f in za.files)
    # refined: the planted query lies 6 degrees off the grid; three iterations find it
    _, idx_c, res = harness.eval_geodesic(model, batch, save_path=str(tmp_path / "c"), refine_iters=3)
    assert torch.equal(idx_c, idx) and {k_: v for k_, v in res.items() if not k_.startswith("refined/")} == res_a
    assert sorted(k_[len("refined/"):] for k_ in res if k_.startswith("refined/")) == sorted(k_ for k_ in res_a if k_ != "loss")
    print(f"eval_geodesic[{name}]: grid top-1 median {res['top1, median']:.4f} deg, refined {res['refined/top1, median']:.4f} deg")
    assert res["refined/top1, median"] < res["top1, median"]
    zc = np.load(str(tmp_path / "c.npz"))
    assert zc["refined_relR"].shape == (B, 5, 3, 3) and zc["refined_relR"].dtype == np.float64
    if name != "gpu":
        return
    # predict_pose with refinement: the poses eval_geodesic scored, closer to the truth than the grid's best
    pred3, score3 = model.predict_pose(batch["query"], batch["reference"], batch["all_relativeR"], batch["template_poses"], refine_iters=3)
    for b in range(B):
        gt = batch["query_pose"][b].cpu().numpy()
        assert angle_deg(pred3[b, 0].cpu().numpy(), gt) < angle_deg(pred[b, 0].cpu().numpy(), gt)
    assert bool((score3[:, 0] >= score[:, 0]).all())


# ---- 6. the LDM variant --------------------------------------------------------------------------------------------------------------------
def test_planted_convergence_ldm(be):
    """nope_amd.ldm.UNetModelPose at its smallest golden configuration ("m32"), f32: the refinement goes through the shared
    forward_hypotheses, so this network is refined by the same code.  The CPU study with oracle.nope_ref.ldm_forward in f32 (three planted
    problems, starts 4 and 8 degrees, the loop of _oracle_refine) ends at <= 4.2e-4 degrees after 3 iterations (<= 6.8e-4 after 2, 0.34 after
    1; the f32 floor is ~2e-4); the bound is 10x that.  The oracle's LDM restatement computes its timestep embedding in f32, so there is no
    f64 trajectory to compare with: only the final error is bounded."""
    from nope_amd.model import PoseConditional
    from tests.test_oracle_golden import build_ldm
    hip, dev, name = be
    model = PoseConditional(build_ldm("m32"), None, {"similarity_metric": "l2"}, None).to(dev)
    _planted_case(hip, dev, model, None, 1, (4.0, 8.0) if name == "gpu" else (8.0,), 3, 0, float("inf"), 4.2e-3, name + " ldm")
