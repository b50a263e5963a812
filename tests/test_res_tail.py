"""The end of a ResnetBlock with a res_conv in one pass (NOPE_RES_TAIL, nope_amd/csrc/unet_runtime.hip: Fwd::res_tail): res_conv reads the raw
output of block2's conv as its residual, and the lean epilogue of the per-tap ping-pong kernel (epilogue_wide, LEANM = 2) turns each residual
vector r into SiLU(GN(r)) on its way in -- gn_apply_kernel's arithmetic -- adds, and stores the block's output over it.

(1) operator level: hip.op_conv_gn_tail against conv + GroupNorm apply as two launches on the same inputs, bit for bit, with the range maximum;
(2) the GroupNorm(1) partials the epilogue emits, against float64 sums, and the (mean, rstd) they finalise to against the two-launch form's;
(3) a 32-dim U-Net at 16 x 16: NOPE_RES_TAIL=1 against 0 bit-equal, 3 against 0 through the f32 mode of the library;
(4) where the one-pass form must NOT be taken: launches, trace and bytes equal NOPE_RES_TAIL=0, and the operator refuses;
(5) nope_unet_workspace_bytes does not depend on the switch, and a forward that takes the one-pass form writes nothing behind it.
(1), (2), the operator's refusals and the workspace query of (5) run on the interpreter (tests/hipemu) and on the device.  The query is the
dry pass of the forward: Fwd::res_tail's conditions, its launch arguments and conv_plan's verdict on them, without a launch.
The whole-network forwards of (3), (4) and (5) run on the device only.  The lean epilogue needs whole 32-column passes and whole 256-row
tiles, so the smallest network whose res_conv reaches it is u_net_dim 32 on an 8 x 8 latent under 4 hypotheses (level 0: one tile), with the
ping-pong kernels forced onto every launch.  One interpreter forward of it takes 72 s in bf16x3 (measured; 85 s at 16 x 16, 225 s in f32):
the cost is the emulated 256-row tiles of the 3x3 convs, whatever the map.  Narrower networks are cheaper (u_net_dim 16: 42 s, 8: 23 s) but
never plan a lean launch.  The tests need three to a dozen forwards each."""
import pytest
import torch

from tests.util import MODE_BOUNDS, StubEncoder, rel

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
PP = {"NOPE_CONV_PP": "11", "NOPE_CONV_SMALL": "0", "NOPE_CONV_STREAM": "0"}      # bit 3: the ping-pong kernels at any tile count (tests/test_conv_pingpong.py)
U = 2.0 ** -24                                                                      # unit roundoff of f32, round to nearest

# (samples, H = W, Cin a | b, Cout, G): what each row exercises is in the issue's table and repeated at the assertion messages
SHAPES = [(4, 8, 64, 32, 96, 8),      # a wave tile is exactly one sample; only one of the two 96-column halves exists
          (2, 16, 64, 64, 192, 8),    # a sample spans four wave tiles
          (1, 32, 32, 32, 64, 8),     # a sample spans several 256-row tiles; absent 32-column passes are skipped
          (4, 8, 64, 0, 32, 1)]       # one group; cpg = one pass
MODES = [("bf16x3", 0), ("f16x2", 0), ("f16x2", 3)]      # (mode, range shift t of the packed layer): t != 0 runs the scaled accumulator path


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, "cuda" if request.param == "gpu" else "cpu", request.param


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _colstats(raw):
    """[n][HW / 64][C][2] f32 (sum, sum of squares) of raw NHWC (n, h, w, C) over blocks of 64 rows: what the producing conv's epilogue emits."""
    n, h, w, C = raw.shape
    r = raw.reshape(n, h * w // 64, 64, C)
    return torch.stack((r.sum(2), (r * r).sum(2)), -1).contiguous()


_CASES = {}


def _case(hip, dev, name, shape, mode, shift):
    """Inputs, the two-launch reference and the one-launch result of one (shape, mode): computed once, shared by tests (1) and (2).
    Inputs carry a DC offset and per-sample / per-group scales: a wrong sample or group index cannot pass."""
    key = (name, shape, mode, shift)
    if key in _CASES:
        return _CASES[key]
    n, hw, ca, cb, cout, G = shape
    dt = {"bf16x3": hip.BF16X3, "f16x2": hip.F16X2}[mode]
    g = torch.Generator().manual_seed(7100 + 10 * SHAPES.index(shape) + shift)
    rn = lambda *s: torch.randn(*s, generator=g)
    scale = (1.0 + 1.5 * torch.arange(n).float())[:, None, None, None]
    x1 = (rn(n, hw, hw, ca) * scale + 0.3).to(dev)
    x2 = (rn(n, hw, hw, cb) * scale - 0.2).to(dev) if cb else None
    grp = (0.5 + torch.arange(G).float()).repeat_interleave(cout // G)
    raw = ((rn(n, hw, hw, cout) * grp + 0.7 * grp) * scale).contiguous().to(dev)
    w, b = (rn(cout, ca + cb, 1, 1) / (ca + cb) ** 0.5).to(dev), rn(cout).to(dev)
    ga, bt = (1.0 + 0.3 * rn(cout)).to(dev), (0.5 * rn(cout)).to(dev)
    cs = _colstats(raw)
    t3 = hip.op_conv(dt, x1, w, b, src2=x2, x2_shift=shift)
    two, ex_two = hip.op_group_norm_ex(dt, raw, ga, bt, G, act_silu=True, resid=t3, colstats=cs, fast_silu=True, out_stats=True, want_amax=True)
    one, ex_one = hip.op_conv_gn_tail(dt, x1, w, b, raw, cs, ga, bt, G, src2=x2, in_place=True, tail_stats=True, want_amax=True, x2_shift=shift)
    sep, _ = hip.op_conv_gn_tail(dt, x1, w, b, raw, cs, ga, bt, G, src2=x2, in_place=False, want_amax=True, x2_shift=shift)
    _CASES[key] = dict(n=n, hw=hw, cout=cout, G=G, dt=dt, t3=t3.cpu(), two=two.cpu(), ex_two=ex_two, one=one.cpu(), ex_one=ex_one, sep=sep.cpu())
    return _CASES[key]


@pytest.mark.parametrize("mode,shift", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_op_bit_identical_to_two_launches(be, shape, mode, shift, monkeypatch, capfd):
    """(1) conv + SiLU(GN(resid)) in one launch == the conv, then hip.op_group_norm_ex (colstats, hardware SiLU) with the conv's output as its
    residual: every bit of the output, in place (resid == out, as the runtime launches it) and with a separate residual, and the range maximum
    both record for that tensor: the out_amax slot's content is compared through the one float the entry decodes it to (hip._amax_scratch), not
    word by word.  The launch is the per-tap ping-pong kernel's lean epilogue with the tail (trace line)."""
    hip, dev, name = be
    _setenv(monkeypatch, dict(PP, NOPE_CONV_TRACE="1"))
    capfd.readouterr()
    c = _case(hip, dev, name, shape, mode, shift)
    trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    if trace:      # (the case was computed in this test, not taken from the cache)
        assert len(trace) == 3 and all(" pp256 " in ln and " lean" in ln for ln in trace), trace
        assert "gn-tail" not in trace[0] and trace[1].endswith(" lean gn-tail") and trace[2].endswith(" lean gn-tail"), trace
    assert torch.isfinite(c["two"]).all() and not torch.equal(c["two"], c["t3"])
    assert torch.equal(c["one"], c["two"]), (shape, mode, shift, "in place", float((c["one"] - c["two"]).abs().max()))
    assert torch.equal(c["sep"], c["two"]), (shape, mode, shift, "separate residual")
    assert c["ex_one"]["amax"] == c["ex_two"]["amax"] == float(c["two"].abs().max()), (c["ex_one"]["amax"], c["ex_two"]["amax"])


@pytest.mark.parametrize("mode,shift", MODES[:2])
@pytest.mark.parametrize("shape", SHAPES)
def test_groupnorm1_partials(be, shape, mode, shift, monkeypatch):
    """(2) tail_stats [n][(HW / 64) ceil(Cout / 96)][2], finalised by nope_op_gn_finalize as the attention's PreNorm does.
    Bound.  An entry is a wave tile's sum: a lane adds its 4 x 8 values per 32-column pass as two chains (16 adds each, 3 passes: 48), the two
    chains (1), the 64 lanes by a butterfly (6); gn_finalize adds a sample's `blocks` entries in order.  Every addend passes through at most
    k = 48 + 1 + 6 + blocks f32 additions, so |S - sum y| <= k u sum |y| and, with one more rounding for the square, |Q - sum y^2| <= (k + 1) u
    sum y^2 (u = 2^-24; first order, Higham's gamma_k).  The two-launch form (gn_apply's out_stats) sums a thread's pixels in sequence: at most
    k2 = HW + 6 + 4 + blocks2 additions per addend.  (mean, rstd): mean = S / N (+ one rounding), var = Q / N - mean^2, rstd = (var + eps)^-1/2,
    so two results whose sums are within dS, dQ of the exact ones differ by at most dmean = dS / N + u |mean| and
    drstd / rstd = (dQ / N + 2 |mean| dmean + 3 u (Q / N + mean^2)) / (2 (var + eps)) + 2 u each, added for the pair."""
    hip, dev, name = be
    _setenv(monkeypatch, PP)
    c = _case(hip, dev, name, shape, mode, shift)
    n, HW, C = c["n"], c["hw"] ** 2, c["cout"]
    N = HW * C
    y = c["one"].double().reshape(n, -1)
    ts = c["ex_one"]["tail_stats"]
    blocks = HW // 64 * -(-C // 96)
    assert ts.shape == (n, blocks, 2) and blocks <= 64
    # per entry: the tile's own sums (k without the finalise)
    tiles = c["one"].double().reshape(n, HW // 64, 64, C)
    for j in range(-(-C // 96)):
        t = tiles[..., 96 * j:96 * (j + 1)]
        S, A, Q = t.sum((2, 3)), t.abs().sum((2, 3)), (t * t).sum((2, 3))
        got = ts.cpu().double().reshape(n, HW // 64, -1, 2)[:, :, j]
        assert bool(((got[..., 0] - S).abs() <= 55 * U * A).all()) and bool(((got[..., 1] - Q).abs() <= 56 * U * Q).all()), (shape, mode, j)
    k, k2 = 48 + 1 + 6 + blocks, HW + 6 + 4 + hip.op_gn_apply_blocks(c["dt"], HW, C, n)
    S, A, Q = y.sum(1), y.abs().sum(1), (y * y).sum(1)
    st = ts.cpu().double().sum(1)
    e1, e2 = float(((st[:, 0] - S).abs() / (k * U * A)).max()), float(((st[:, 1] - Q).abs() / ((k + 1) * U * Q)).max())
    print(f"tail_stats {shape} {mode} [{name}]: |S - sum| / (k u sum|y|) = {e1:.3f}, |Q - sum| / ((k + 1) u sum y^2) = {e2:.3f}, k = {k}")
    assert e1 <= 1.0 and e2 <= 1.0, (shape, mode, e1, e2)
    ms1 = hip.op_gn_finalize(ts, float(N)).cpu().double()
    ms2 = hip.op_gn_finalize(c["ex_two"]["out_stats"], float(N)).cpu().double()
    mean, var = S / N, Q / N - (S / N) ** 2
    rstd = (var + 1e-5) ** -0.5
    lim_mean, lim_rstd = 0.0, 0.0
    for kk in (k, k2):
        dmean = kk * U * A / N + U * mean.abs()
        lim_mean = lim_mean + dmean
        lim_rstd = lim_rstd + rstd * (((kk + 1) * U * Q / N + 2 * mean.abs() * dmean + 3 * U * (Q / N + mean ** 2)) / (2 * (var + 1e-5)) + 2 * U)
    for ms in (ms1, ms2):      # each within its own share of the exact values, hence the pair within the sum
        assert bool(((ms[:, 0] - mean).abs() <= lim_mean).all()) and bool(((ms[:, 1] - rstd).abs() <= lim_rstd).all()), (shape, mode)
    d_mean, d_rstd = float(((ms1[:, 0] - ms2[:, 0]).abs() / lim_mean).max()), float(((ms1[:, 1] - ms2[:, 1]).abs() / lim_rstd).max())
    print(f"  (mean, rstd) one launch against two: {d_mean:.3f}, {d_rstd:.3f} of the bound")
    assert d_mean <= 1.0 and d_rstd <= 1.0, (shape, mode, d_mean, d_rstd)


# ---- block level ------------------------------------------------------------------------------------------------------------------------
def _unet(dim, cdt, dev, groups=8):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    m = UNet(u_net_dim=dim, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", resnet_block_groups=groups, compute_dtype=cdt)
    synth_init_(m, 2022)
    return m.to(dev)._get_handle(torch.device(dev))


def _inputs(n_src, n_hyp, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_src, 8, hw, hw, generator=g), torch.randn(n_hyp, 6, generator=g)


def _forward(h, x, pose, tail, dev, monkeypatch, capfd):
    """(output, trace lines, profiled launches) of one forward under NOPE_RES_TAIL = tail."""
    monkeypatch.setenv("NOPE_RES_TAIL", str(tail))
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    h.profile(True)
    capfd.readouterr()
    y = h.forward(x.to(dev), pose.to(dev), x_rep=pose.shape[0] // x.shape[0])
    if dev == "cuda":
        torch.cuda.synchronize()
    trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    launches = [(l["kernel"], l["ntaps"], l["Cin"], l["Cout"], l["Hs"], l["n_hyp"], l["flops"], l["bytes"]) for l in h.profile_launches()]
    h.profile(False)
    monkeypatch.delenv("NOPE_CONV_TRACE")
    return y.cpu(), trace, launches


_F32_REF = {}


@pytest.fixture
def dev_be(gpu):
    return gpu, "cuda", "gpu"


@pytest.mark.gpu
@pytest.mark.parametrize("cdt", ["bf16x3", "f16x2"])
def test_unet_block_level(dev_be, cdt, monkeypatch, capfd):
    """(3) u_net_dim 32 at 16 x 16, four hypotheses of two references (M = 1024 and 256 rows at levels 0 and 1: whole 256-row tiles), the ping-pong
    kernels opened to small shapes: the res_convs of levels 0 and 1 plan as per-tap + lean.  Blocks with a res_conv on maps of >= 64 pixels:
    ups[2] and ups[3] (two each, the second followed by attention) and final_res_block -- 3 one-pass launches under bit 0, 5 under 3, none
    under 0, each in place of a lean launch (the conv launches and their order do not change).
    NOPE_RES_TAIL=1 against 0: bit-equal.  3 against 0: err(s) = max |y_s - y_f32| / max |y_f32| against the library's f32 mode, a reference
    that runs none of the code under test; |err(3) - err(0)| <= MODE_BOUNDS[mode][0], the spread tests/test_shared_split.py accepts for a
    change of summation order (its line `assert e03 < bound and e3o < bound`, bound = MODE_BOUNDS[cdt][0]); err(3), err(0) inside it too."""
    hip, dev, name = dev_be
    _setenv(monkeypatch, PP)
    x, pose = _inputs(2, 4, 16, 7300)
    if name not in _F32_REF:
        h32 = _unet(32, "f32", dev)
        monkeypatch.setenv("NOPE_RES_TAIL", "0")
        _F32_REF[name] = h32.forward(x.to(dev), pose.to(dev), x_rep=2).cpu()
    ref = _F32_REF[name]
    h = _unet(32, cdt, dev)
    if cdt == "f16x2":      # the range shifts of the two-pass layers settle on this input first (x2_range.h): later forwards then differ by the setting alone
        for _ in range(2):
            _forward(h, x, pose, 0, dev, monkeypatch, capfd)
            h.x2_range_check(torch.cuda.current_stream().cuda_stream)
    (y0, t0, l0), (y1, t1, l1), (y3, t3, l3) = (_forward(h, x, pose, s, dev, monkeypatch, capfd) for s in (0, 1, 3))
    assert torch.equal(_forward(h, x, pose, 0, dev, monkeypatch, capfd)[0], y0), "the forward must be reproducible before two settings are compared"
    tails = [sum(ln.endswith(" lean gn-tail") for ln in t) for t in (t0, t1, t3)]
    assert tails == [0, 3, 5], tails
    strip = lambda t: [ln.replace(" gn-tail", "") for ln in t]
    assert strip(t1) == t0 and strip(t3) == t0, "the conv launches, their kernels and their order must not change"
    assert [l[:7] for l in l1] == [l[:7] for l in l0] and [l[:7] for l in l3] == [l[:7] for l in l0]
    extra = [(b[7] - a[7], 4.0 * a[5] * a[4] * a[4] * a[3]) for a, b in zip(l0, l3) if a[7] != b[7]]
    assert len(extra) == 5 and all(d == r for d, r in extra), ("algorithmic bytes: + the residual read, on the one-pass launches only", extra)
    assert torch.equal(y1, y0), ("NOPE_RES_TAIL=1 must be bit-identical to 0", float((y1 - y0).abs().max()))
    e0, e3 = rel(y0, ref), rel(y3, ref)
    bound = MODE_BOUNDS[cdt][0]
    print(f"res tail {cdt} [{name}]: err(0) {e0:.3e}, err(3) {e3:.3e}, difference {abs(e3 - e0):.2e} (bound {bound:.1e}); 3 against 0 directly {rel(y3, y0):.2e}")
    assert e0 < bound and e3 < bound and abs(e3 - e0) <= bound, (cdt, e0, e3)
    assert torch.isfinite(y3).all()


def _same_as_off(h, x, pose, dev, monkeypatch, capfd, keep=lambda ln: True, keep_launch=lambda l: True):
    (y0, t0, l0), (y3, t3, l3) = (_forward(h, x, pose, s, dev, monkeypatch, capfd) for s in (0, 3))
    f0, f3 = [ln for ln in t0 if keep(ln)], [ln for ln in t3 if keep(ln)]
    assert f0 and f3 == f0, ("trace differs from NOPE_RES_TAIL=0", f3, f0)
    assert not any("gn-tail" in ln for ln in f3)
    assert [l for l in l3 if keep_launch(l)] == [l for l in l0 if keep_launch(l)], "launches / bytes differ from NOPE_RES_TAIL=0"
    return (y0, t0), (y3, t3)


@pytest.mark.gpu
def test_fallbacks_f32_and_other_kernel(dev_be, monkeypatch, capfd):
    """(4) The f32 parity mode (libm SiLU: no tail exists for it) with the ping-pong kernels forced, and a split-precision forward whose res_convs
    the plan puts on another kernel (the default policy at this size): trace, launches, bytes and output bits of NOPE_RES_TAIL=3 equal 0."""
    hip, dev, name = dev_be
    x, pose = _inputs(2, 4, 16, 7400)
    with monkeypatch.context() as mp:
        _setenv(mp, PP)
        (y0, t0), (y3, _) = _same_as_off(_unet(32, "f32", dev), x, pose, dev, mp, capfd)
        assert any(" pp256 " in ln for ln in t0) and torch.equal(y0, y3)
    (y0, t0), (y3, _) = _same_as_off(_unet(32, "bf16x3", dev), x, pose, dev, monkeypatch, capfd)
    assert not any(" pp256 " in ln for ln in t0) and torch.equal(y0, y3)


@pytest.mark.gpu
def test_fallbacks_small_maps_and_narrow_groups(dev_be, monkeypatch, capfd):
    """(4) 4 x 4 maps (a 64-row wave tile holds four samples): an 8 x 8 latent under 16 hypotheses puts level 1 at 4 x 4 with M = 256, whole
    tiles -- its res_convs are lean per-tap launches WITHOUT the tail (level 0, 8 x 8, takes it: the setting is on).  Channels per group not a
    multiple of 4: GroupNorm(16) on u_net_dim 32 leaves level 0 (32 channels, 2 per group) on the three passes while level 1 (64, 4 per
    group) takes the one-pass form.  The launches of the level that stays are the ones NOPE_RES_TAIL=0 makes."""
    hip, dev, name = dev_be
    _setenv(monkeypatch, PP)
    x, pose = _inputs(4, 16, 8, 7500)
    level1 = lambda ln: " taps 1 " in ln and " M 256 " in ln
    (_, t0), (_, t3) = _same_as_off(_unet(32, "bf16x3", dev), x, pose, dev, monkeypatch, capfd, keep=level1, keep_launch=lambda l: l[4] == 4)
    assert any(ln.endswith(" lean") for ln in t3 if level1(ln)), "level 1's 1x1 launches should be lean per-tap launches"
    assert any(ln.endswith(" gn-tail") and " M 1024 " in ln for ln in t3), "level 0 (8 x 8) should take the one-pass form"
    x, pose = _inputs(2, 4, 16, 7600)
    level0 = lambda ln: " taps 1 " in ln and " Cout 32 " in ln
    (_, t0), (_, t3) = _same_as_off(_unet(32, "bf16x3", dev, groups=16), x, pose, dev, monkeypatch, capfd, keep=level0, keep_launch=lambda l: l[3] == 32 and l[1] == 1)
    assert any(ln.endswith(" gn-tail") and " Cout 64 " in ln for ln in t3), "level 1 (4 channels per group) should take the one-pass form"


def test_operator_refuses_what_has_no_tail(be, monkeypatch):
    """(4) hip.op_conv_gn_tail never launches without the tail: a 4 x 4 map, 2 channels per group, the f32 mode and a launch the policy puts on
    another kernel are refused (NopeError): conv_plan rejects the launch before anything is enqueued."""
    hip, dev, name = be
    g = torch.Generator().manual_seed(7700)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)

    def refused(dt, n, hw, cin, cout, G, env):
        with monkeypatch.context() as mp:
            _setenv(mp, env)
            raw = rn(n, hw, hw, cout)
            cs = torch.zeros((n, max(1, hw * hw // 64), cout, 2), device=dev)
            with pytest.raises(hip.NopeError):
                hip.op_conv_gn_tail(dt, rn(n, hw, hw, cin), rn(cout, cin, 1, 1), rn(cout), raw, cs, rn(cout), rn(cout), G)

    refused(hip.BF16X3, 16, 4, 64, 64, 8, PP)            # 4 x 4: four samples per wave tile
    refused(hip.BF16X3, 4, 8, 64, 32, 16, PP)            # 2 channels per group: a 4-channel chunk straddles groups
    refused(hip.F32, 4, 8, 64, 64, 8, PP)                # the parity mode
    refused(hip.BF16X3, 4, 8, 64, 64, 8, {})             # default policy: 2 K steps, 2 tiles -- not a ping-pong launch
    refused(hip.BF16X3, 3, 8, 64, 64, 8, PP)             # 192 rows: no whole 256-row tile, not lean


# ---- workspace ---------------------------------------------------------------------------------------------------------------------------
def test_workspace_query_does_not_depend_on_the_switch(be, monkeypatch):
    """(5) nope_unet_workspace_bytes under NOPE_RES_TAIL = 0, 1, 3 at the shapes of (3) and (4), ping-pong kernels forced (the one-pass form is
    planned) and at the default policy (it is not): equal.  t3 stays allocated under the one-pass form, so a workspace sized under one
    setting serves a forward under another (the switch is read per forward)."""
    hip, dev, name = be
    h = _unet(32, "bf16x3", dev)
    for env in (PP, {}):
        with monkeypatch.context() as mp:
            _setenv(mp, env)
            for n_hyp, n_src, hw in ((4, 2, 16), (16, 4, 8), (4, 2, 8)):
                need = []
                for tail in (0, 1, 3):
                    mp.setenv("NOPE_RES_TAIL", str(tail))
                    hip.lib()      # (notices the changed NOPE_* variables)
                    need.append(h.workspace_bytes(n_hyp, n_src, hw, hw))
                assert need[0] > 0 and need[1] == need[0] and need[2] == need[0], (env, n_hyp, hw, need)


@pytest.mark.gpu
def test_workspace_canary_res_tail(dev_be, monkeypatch, capfd):
    """(5) The pattern of tests/test_shared_split.py::test_workspace_canary_shared_split with the switch at 3 and the one-pass form taken (trace):
    a canary behind exactly nope_unet_workspace_bytes stays untouched, and the output is the one the handle's own forward gives."""
    hip, dev, name = dev_be
    _setenv(monkeypatch, dict(PP, NOPE_RES_TAIL="3"))
    n_src, rep, hw = 2, 2, 16
    n_hyp = n_src * rep
    x, pose = _inputs(n_src, n_hyp, hw, 7800)
    h = _unet(32, "bf16x3", dev)
    want, trace, _ = _forward(h, x, pose, 3, dev, monkeypatch, capfd)
    assert sum(ln.endswith(" lean gn-tail") for ln in trace) == 5, trace
    l = hip.lib()
    need = h.workspace_bytes(n_hyp, n_src, hw, hw)
    ws = torch.full((need + 8192,), 0xAB, dtype=torch.uint8, device=dev)
    out = torch.empty((n_hyp, 8, hw, hw), device=dev)
    xd, pd = x.to(dev), pose.to(dev)
    l.check(l.dll.nope_unet_forward(h._h, xd.data_ptr(), n_src, rep, pd.data_ptr(), n_hyp, hw, hw, out.data_ptr(), hip.F32,
                                    ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "fwd")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xAB).all()), "write beyond the reported workspace size"
    assert torch.equal(out.cpu(), want)


@pytest.mark.gpu
def test_graph_replay_follows_the_switch(dev_be, monkeypatch):
    """With hipGraph replay on (nope_unet_graph_limit), a changed NOPE_RES_TAIL drops the cached graphs as a changed NOPE_SHARED_SPLIT does: the
    forward of a shape captured under 0 gives, under 3, what direct launches give under 3 -- not the stale graph's output."""
    hip, dev, name = dev_be
    _setenv(monkeypatch, PP)
    x, pose = _inputs(2, 4, 16, 7900)
    xd, pd = x.to(dev), pose.to(dev)
    h = _unet(32, "bf16x3", dev)
    direct = {}
    for tail in (0, 3):
        monkeypatch.setenv("NOPE_RES_TAIL", str(tail))
        direct[tail] = h.forward(xd, pd, x_rep=2).cpu()
    assert not torch.equal(direct[0], direct[3]), "the two settings must differ somewhere for this test to tell a stale graph"
    h.graph_limit(1 << 20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = {}
    with torch.cuda.stream(side):
        for tail in (0, 3, 0):
            monkeypatch.setenv("NOPE_RES_TAIL", str(tail))
            got[tail] = h.forward(xd, pd, x_rep=2)
            side.synchronize()
            assert torch.equal(got[tail].cpu(), direct[tail]), tail
    assert h.graph_replays() == 3, h.graph_replays()
    h.graph_limit(0)


@pytest.mark.parametrize("n,hw,ca,cb,cout", [(4, 8, 32, 32, 32), (4, 16, 32, 32, 32), (4, 8, 64, 64, 64)])
def test_network_res_conv_shapes_plan_the_tail(be, n, hw, ca, cb, cout, monkeypatch, capfd):
    """The res_convs of the 32-dim network of tests (3) to (5), as Fwd::res_tail hands them to conv_plan (GroupNorm(8), ping-pong kernels forced):
    level 0 of an 8 x 8 latent under 4 hypotheses (one 256-row tile: the conv trace of an interpreter forward shows `Cin 64 Cout 32 M 256 ...
    lean gn-tail`), level 0 of a 16 x 16 latent, and a 64-channel launch on level 1's 8 x 8 map.  conv_plan accepts the tail's arguments and the launch is the lean one with the
    tail -- so the equal byte counts of test_workspace_query_does_not_depend_on_the_switch are those of a dry pass that does take the form."""
    hip, dev, name = be
    _setenv(monkeypatch, dict(PP, NOPE_CONV_TRACE="1"))
    g = torch.Generator().manual_seed(8000 + hw + cout)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    raw = rn(n, hw, hw, cout)
    capfd.readouterr()
    y = hip.op_conv_gn_tail(hip.BF16X3, rn(n, hw, hw, ca), rn(cout, ca + cb, 1, 1) / (ca + cb) ** 0.5, rn(cout), raw, _colstats(raw), 1.0 + 0.3 * rn(cout), rn(cout), 8,
                            src2=rn(n, hw, hw, cb), in_place=True)
    trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    assert len(trace) == 1 and f" Cin {ca + cb} Cout {cout} M {n * hw * hw} " in trace[0] and trace[0].endswith(" lean gn-tail"), trace
    assert torch.isfinite(y).all()
