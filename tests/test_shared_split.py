"""NOPE_SHARED_SPLIT (nope_amd/csrc/unet_runtime.hip): two 3x3 convs of the U-Net convolve their pose-independent input once per reference
image instead of once per pose hypothesis, and the GroupNorm behind each forms the sum itself (kernels_norm.hip, the shared addend).

  bit 0, downs[0][0].block2:   conv(u + e_n 1) = S + E[n][cls(p)], S = conv(u) + bias per reference, E = e_n against the nine border-class
                               weights (nope_op_conv_class_weights), cls(p) = 3 cy + cx the border class of pixel p;
  bit 1, final_res_block.block1: conv(W, cat(cur, r)) = conv(W[:, :C], cur) + Sr, Sr = conv(W[:, C:], r) + bias per reference.

(1) the algebra in float64, on the library's class weights; (2) the GroupNorm form at operator level (hip.op_group_norm_shared) against
float64; (3) the tiny U-Net with the switch at 3 against 0 and against the oracle; (4) the f16x2 mode on the device; (5) nothing is written
outside nope_unet_workspace_bytes.  Every test runs on the interpreter (tests/hipemu) and on the device unless it says otherwise."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gn_fused import OP_TOL, _chunk_sums
from tests.util import MODE_BOUNDS, StubEncoder, rel

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
MAPS = [(4, 4), (2, 5)]          # 2 x 5: not square (a transposed class index shows), no interior row (H = 2: top and bottom only)


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, "cuda" if request.param == "gpu" else "cpu", request.param


def _cls_map(h, w):
    """[h][w] border class 3 cy + cx, c = 0 on the first row / column, 2 on the last, 1 between (include/nope_hip.h)."""
    cy = torch.tensor([0 if y == 0 else 2 if y == h - 1 else 1 for y in range(h)])
    cx = torch.tensor([0 if x == 0 else 2 if x == w - 1 else 1 for x in range(w)])
    return cy[:, None] * 3 + cx[None, :]


def _gather_e(E, h, w):
    """E (n, 9, C) -> (n, C, h, w): every pixel takes the row of its border class."""
    return E[:, _cls_map(h, w).reshape(-1), :].reshape(E.shape[0], h, w, E.shape[2]).permute(0, 3, 1, 2)


@pytest.mark.parametrize("hw", MAPS)
def test_class_weight_algebra(be, hw):
    """(1) F.conv2d(u + e[:, :, None, None], W, b, padding = 1) == S + E[cls] in float64, bound 1e-12 relative, with E built from the class
    weights the LIBRARY packs.  The weights are multiples of 1/64 below 1 in magnitude: the f32 sums of up to nine of them that
    pack_conv_classes_kernel forms are exact, so the float64 identity is what is measured, not an f32 rounding of the pack."""
    hip, dev, _ = be
    h, w = hw
    g = torch.Generator().manual_seed(3100 + h)
    C, n = 16, 3
    W = torch.randint(-63, 64, (C, C, 3, 3), generator=g).float() / 64
    wcls = hip.op_conv_class_weights(W.to(dev)).cpu().double()            # [9][Cout][Cin]
    u = torch.randn(1, C, h, w, generator=g, dtype=torch.float64)
    e, b = torch.randn(n, C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    want = F.conv2d(u + e[:, :, None, None], W.double(), b, padding=1)
    S = F.conv2d(u, W.double(), b, padding=1)
    E = torch.einsum("koi,ni->nko", wcls, e)
    got = S + _gather_e(E, h, w)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"class-weight algebra {h} x {w}: {err:.2e} (bound 1e-12)")
    assert err < 1e-12, err
    # the interior class is the plain tap sum, a corner keeps four taps
    assert torch.equal(wcls[4], W.double().sum((2, 3))) and torch.equal(wcls[0], W.double()[:, :, 1:, 1:].sum((2, 3)))


def _q(x, dt, hip):
    return x.to(hip.torch_dtype(dt)).float()


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_group_norm_shared_form(be, dt):
    """(2) hip.op_group_norm_shared against float64 group_norm + SiLU + emb + resid of x_eff, on operands rounded to the storage type (S and
    E are f32 in every mode).  C = 16, G = 8 (two channels per group: no 16-byte vector lies in one group), maps 4 x 4 and 2 x 5, six
    hypotheses on two shared samples (s_rep = 3: n / rep against n % rep).  Both forms -- S + E without x, x + S -- each plain, with the
    embedding, with a residual shared by three hypotheses, with out_stats; the libm and (f32) the hardware SiLU.  Bounds: OP_TOL of
    tests/test_gn_fused.py for y, its out_stats bound (1e-5 on f32 storage, OP_TOL on 16-bit storage) for the sums.  Inputs carry a DC
    offset like the other GroupNorm tests.  Refused: no SiLU, x together with E, E on a one-row map, an n_hyp that s_rep does not divide.
    The interpreter runs f32."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs every storage type)")
    g = torch.Generator().manual_seed(3200 + dt)
    rn = lambda *s: torch.randn(*s, generator=g)
    C, G, n, s_rep = 16, 8, 6, 3
    tol, os_tol = OP_TOL[dt], (1e-5 if dt == 0 else OP_TOL[dt])
    worst, worst_os = 0.0, 0.0
    for (h, w) in MAPS:
        for form in ("S+E", "X+S"):
            for use_emb, use_rs, out_stats, fast in ((False, False, False, False), (True, False, False, dt == 0), (False, True, False, False),
                                                     (True, True, True, dt == 0)):
                S, E = rn(n // s_rep, C, h, w) * 2 + 0.4, rn(n, 9, C)
                x = rn(n, C, h, w) + 0.3
                ga, be_, emb, rs = rn(C), rn(C), rn(n, C), rn(n // s_rep, C, h, w)
                xq = _q(x, dt, hip)
                x_eff = S.double().repeat_interleave(s_rep, 0) + (_gather_e(E.double(), h, w) if form == "S+E" else xq.double())
                ref = F.silu(F.group_norm(x_eff, G, ga.double(), be_.double(), 1e-5))
                if use_emb:
                    ref = ref + emb.double()[:, :, None, None]
                if use_rs:
                    ref = ref + _q(rs, dt, hip).double().repeat_interleave(s_rep, 0)
                got = hip.op_group_norm_shared(dt, hip.to_nhwc(x.to(dev), dt) if form == "X+S" else None, hip.to_nhwc(S.to(dev), 0),
                                               E.to(dev) if form == "S+E" else None, ga.to(dev), be_.to(dev), G, n,
                                               emb=emb.to(dev) if use_emb else None, resid=hip.to_nhwc(rs.to(dev), dt) if use_rs else None,
                                               resid_rep=s_rep, out_stats=out_stats, fast_silu=fast)
                tag = (dt, h, w, form, use_emb, use_rs, out_stats, fast)
                y, ex = got if out_stats else (got, None)
                yw = hip.to_nchw(y, dt).cpu().double()
                err = float((yw - ref).abs().max() / ref.abs().max())
                worst = max(worst, err)
                assert err < tol, (tag, err)
                if out_stats:
                    blocks = hip.op_gn_apply_blocks(dt, h * w, C, n)
                    st = ex["out_stats"].double().cpu()
                    assert st.shape == (n, blocks, 2)
                    want, mag = _chunk_sums(yw if dt == 0 else ref, blocks)      # 16-bit storage: the sums are taken before the rounding
                    e1 = float(((st[..., 0] - want[..., 0]).abs() / mag).max())
                    e2 = float(((st[..., 1] - want[..., 1]).abs() / want[..., 1]).max())
                    worst_os = max(worst_os, e1, e2)
                    assert max(e1, e2) < os_tol, (tag, e1, e2)
    print(f"shared GroupNorm dt {dt} [{name}]: worst {worst:.2e} (bound {tol:.1e}), out_stats {worst_os:.2e} (bound {os_tol:.1e})")
    S, E, ga, be_ = hip.to_nhwc(rn(2, C, 4, 4).to(dev), 0), rn(n, 9, C).to(dev), rn(C).to(dev), rn(C).to(dev)
    x = hip.to_nhwc(rn(n, C, 4, 4).to(dev), dt)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_shared(dt, None, S, E, ga, be_, G, n, act_silu=False)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_shared(dt, x, S, E, ga, be_, G, n)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_shared(dt, None, hip.to_nhwc(rn(2, C, 1, 16).to(dev), 0), E, ga, be_, G, n)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_shared(dt, None, S, None, ga, be_, G, n)


def _tiny(golden, dim, cdt, dev):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    m = UNet(u_net_dim=dim, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
    synth_init_(m, 2022)
    sd = {k: v.clone() for k, v in m.own_state_dict().items()}
    return m.to(dev), sd


def _d8_inputs(golden):
    """The d8 fixture's three samples and poses, and a fourth pose (the fixture has three)."""
    g = golden("unet_tiny.npz")
    pose4 = torch.cat((g["d8/pose"], torch.randn(1, 6, generator=torch.Generator().manual_seed(3300))))
    return g["d8/x"], pose4


def _forward(h, x, pose, rep, split, monkeypatch, dev):
    monkeypatch.setenv("NOPE_SHARED_SPLIT", str(split))
    y = h.forward(x.to(dev), pose.to(dev), x_rep=rep)
    if dev == "cuda":
        torch.cuda.synchronize()
    monkeypatch.delenv("NOPE_SHARED_SPLIT")
    return y.cpu()


@pytest.fixture(scope="module")
def d8_oracle(golden):
    """Oracle outputs of the d8 network for the two sharing patterns, computed once."""
    from oracle import nope_ref as R
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    m = UNet(u_net_dim=8, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer")
    synth_init_(m, 2022)
    sd = {k: v.clone() for k, v in m.own_state_dict().items()}
    x, pose = _d8_inputs(golden)
    return {(n_src, rep): R.unet_forward(sd, x[:n_src].repeat_interleave(rep, 0), pose) for n_src, rep in ((1, 4), (2, 2))}


@pytest.mark.parametrize("cdt", ["f32", "bf16x3"])
def test_unet_shared_split(be, golden, d8_oracle, cdt, monkeypatch):
    """(3) The d8 fixture's network, one reference with x_rep = 4 and two references with x_rep = 2: NOPE_SHARED_SPLIT=3 against =0 and
    against the oracle within MODE_BOUNDS[mode][0]; the outputs differ in some bit (the new schedule ran).  What profile_launches() shows
    per bit: bit 0 -- one 9-tap launch over n_hyp samples fewer and one over n_src more (block2 of downs[0][0]); bit 1 -- the 9-tap launch
    over n_hyp samples with 2 dim input channels gone, one with dim input channels over n_hyp and one over n_src in its place (so the number
    of per-hypothesis 9-tap launches falls with bit 0 and stays with bit 1: its per-hypothesis launch has half the K).  With x_rep = 1 the
    two settings are bit-identical."""
    hip, dev, name = be
    dim = 8
    m, _ = _tiny(golden, dim, cdt, dev)
    h = m._get_handle(torch.device(dev))
    x, pose = _d8_inputs(golden)
    bound = MODE_BOUNDS[cdt][0]
    n_hyp = 4
    taps9 = {}

    def run(n_src, rep, split):
        h.profile(True)
        y = _forward(h, x[:n_src], pose, rep, split, monkeypatch, dev)
        taps9[(n_src, split)] = [(l["n_hyp"], l["Cin"], l["Cout"]) for l in h.profile_launches() if l["ntaps"] == 9]
        h.profile(False)
        return y

    for n_src, rep in ((1, 4), (2, 2)):
        y0, y3 = run(n_src, rep, 0), run(n_src, rep, 3)
        e03, e3o, e0o = rel(y3, y0), rel(y3, d8_oracle[(n_src, rep)]), rel(y0, d8_oracle[(n_src, rep)])
        print(f"shared split {cdt} [{name}] {n_src} x {rep}: 3 against 0 {e03:.2e}, against the oracle {e3o:.2e} (0: {e0o:.2e}); bound {bound:.1e}")
        assert e03 < bound and e3o < bound, (cdt, n_src, rep, e03, e3o)
        assert not torch.equal(y3, y0), "NOPE_SHARED_SPLIT=3 computed the same bits as 0: the new schedule did not run"
    y0, y3 = (_forward(h, x[:1], pose[:1], 1, s, monkeypatch, dev) for s in (0, 3))
    assert torch.equal(y0, y3), "x_rep = 1 must run the same schedule under either setting"
    n_src = 2
    splits = (0, 3) if cdt != "bf16x3" else (0, 1, 2, 3)       # (each bit by itself: one mode only, the schedule does not depend on it)
    for split in splits[1:-1]:
        run(n_src, 2, split)
    per_hyp = {s: sum(1 for l in taps9[(n_src, s)] if l[0] == n_hyp) for s in splits}
    per_ref = {s: sum(1 for l in taps9[(n_src, s)] if l[0] == n_src) for s in splits}
    wide = {s: sum(1 for l in taps9[(n_src, s)] if l == (n_hyp, 2 * dim, dim)) for s in splits}      # (ups[3]'s two blocks and final_res_block)
    assert wide[0] == 3 and wide[3] == 2, wide
    assert per_hyp[3] == per_hyp[0] - 1 and per_ref[3] == per_ref[0] + 2, (per_hyp, per_ref)
    if cdt == "bf16x3":
        assert per_hyp[1] == per_hyp[0] - 1 and per_ref[1] == per_ref[0] + 1 and wide[1] == 3, (per_hyp, per_ref, wide)
        assert per_hyp[2] == per_hyp[0] and per_ref[2] == per_ref[0] + 1 and wide[2] == 2, (per_hyp, per_ref, wide)


@pytest.mark.gpu
def test_unet_shared_split_f16x2(gpu, monkeypatch):
    """(4) f16x2 on the device: u_net_dim = 32, a 16 x 16 latent, 8 hypotheses of 2 references, the ping-pong kernels opened to small shapes
    (NOPE_CONV_PP=11).  The output is finite and within MODE_BOUNDS["f16x2"][0] of the f32 mode's; the two new per-reference launches run on the
    three-pass kernels; after the forward the range tracking reports nothing out of range, and the layer whose two-pass launch no longer
    exists (block2 of downs[0][0], the second layer that registered a second pack) was never judged: its shift has not moved."""
    hip, dev = gpu, "cuda"
    g = torch.Generator().manual_seed(3400)
    x, pose = torch.randn(2, 8, 16, 16, generator=g), torch.randn(8, 6, generator=g)
    m32, _ = _tiny(None, 32, "f32", dev)
    want = _forward(m32._get_handle(torch.device(dev)), x, pose, 4, 3, monkeypatch, dev)
    monkeypatch.setenv("NOPE_CONV_PP", "11")
    m, _ = _tiny(None, 32, "f16x2", dev)
    h = m._get_handle(torch.device(dev))
    y = _forward(h, x, pose, 4, 3, monkeypatch, dev)
    e = rel(y, want)
    print(f"shared split f16x2: against f32 {e:.2e} (bound {MODE_BOUNDS['f16x2'][0]:.1e})")
    assert torch.isfinite(y).all() and e < MODE_BOUNDS["f16x2"][0], e
    h.profile(True)
    y2 = _forward(h, x, pose, 4, 3, monkeypatch, dev)
    launches = h.profile_launches()
    h.profile(False)
    assert torch.isfinite(y2).all()
    assert any(l["mfma_passes"] == 2 for l in launches if l["n_hyp"] == 8), "no per-hypothesis launch took the two-pass tile"
    # the per-reference 3x3 launches in issue order: init_conv, block1 of downs[0][0] (as before: with its second pack), then the two new ones
    per_ref = [l for l in launches if l["n_hyp"] == 2 and l["ntaps"] == 9]
    assert [(l["Cin"], l["Cout"]) for l in per_ref] == [(8, 32), (32, 32), (32, 32), (32, 32)], per_ref
    assert per_ref[2]["mfma_passes"] == 3 and per_ref[3]["mfma_passes"] == 3, "a new per-reference launch left the three-pass kernels"
    code, bad, moved, _ = h.x2_range_check(torch.cuda.current_stream().cuda_stream)
    assert (code, bad) == (0, 0), (code, bad, moved)
    assert h.x2_shifts()[1] == 0, h.x2_shifts()


def test_workspace_canary_shared_split(be, golden):
    """(5) The pattern of tests/test_kernels_parity.py::test_workspace_canary_odd_hypotheses at x_rep = 2 with the switch at its default: a
    canary behind exactly nope_unet_workspace_bytes stays untouched and the output matches the oracle.  u_net_dim 64 on the device (the
    column statistics are the arena's last allocation at its peak there), 8 under the interpreter."""
    from oracle import nope_ref as R
    hip, dev, name = be
    dim, n_src, rep = (8 if name == "emu" else 64), 2, 2
    n_hyp = n_src * rep
    m, sd = _tiny(golden, dim, "f32", dev)
    g = torch.Generator().manual_seed(3500)
    x, pose = torch.randn(n_src, 8, 8, 8, generator=g), torch.randn(n_hyp, 6, generator=g)
    h = m._get_handle(torch.device(dev))
    need = h.workspace_bytes(n_hyp, n_src, 8, 8)
    ws = torch.full((need + 8192,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.empty((n_hyp, 8, 8, 8), device=dev)
    l = hip.lib()
    xd, pd = x.to(dev), pose.to(dev)
    l.check(l.dll.nope_unet_forward(h._h, xd.data_ptr(), n_src, rep, pd.data_ptr(), n_hyp, 8, 8, out.data_ptr(), hip.F32,
                                    ws.data_ptr(), need, None if dev == "cpu" else torch.cuda.current_stream().cuda_stream), "fwd")
    if dev != "cpu":
        torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()), "write beyond the reported workspace size"
    assert rel(out.cpu(), R.unet_forward(sd, x.repeat_interleave(rep, 0), pose)) < MODE_BOUNDS["f32"][0]
