"""GroupNorm + SiLU in the tap-resident 3x3 kernel's own lean epilogue (NOPE_GN_EPI, nope_amd/csrc/unet_runtime.hip: Fwd::conv_gn_self; epilogue_wide,
LEANM = 3; nope_conv_op's gn_self): at the 16 x 16, 8 x 8 and 4 x 4 levels a 256-row tile holds whole samples and a 192-column tile whole groups, so
the conv normalises its own output and the GroupNorm pass over the tensor is not launched.

(1) operator level, interpreter and device: the one launch against conv + GroupNorm apply as two launches, torch.equal on the output and equality
    of the recorded range maximum (tests/gn_epi_emu_case.py: the maps, group widths and forms are listed there);
(2) refusals: NOPE_ERR_UNSUPPORTED, nothing launched, the output buffer untouched;
(3) network level, device: a 32-dim U-Net under 16 hypotheses at a 16 x 16 latent, NOPE_GN_EPI 0 against 3 (and 1, 2): outputs bit-equal, range
    events equal, ` gn-self` on launches at all three map sizes; once more at input scale x 1e3."""
import pytest
import torch

from tests import gn_epi_emu_case as case
from tests.util import StubEncoder, switches

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
PP = case.PP


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, "cuda" if request.param == "gpu" else "cpu", request.param


# ---- (1) operator level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("form", case.FORMS, ids=lambda f: f"cout{f[0]}_G{f[1]}_emb{int(f[2])}_res{int(f[3])}")
@pytest.mark.parametrize("nmap", case.MAPS, ids=lambda m: f"{m[0]}x{m[1]}x{m[1]}")
def test_op_bit_identical_to_two_launches(be, nmap, form, mode, capfd):
    hip, dev, name = be
    dt = {"bf16x3": hip.BF16X3, "f16x2": hip.F16X2}[mode]
    with switches(NOPE_CONV_TRACE=1):
        capfd.readouterr()
        case.one_case(hip, dev, dt, nmap, form)
        trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    assert len(trace) == 2 and all(" halo256 " in ln for ln in trace), trace
    assert trace[0].endswith(" lean") and trace[1].endswith(" lean gn-self"), trace
    assert trace[1].replace(" gn-self", "") == trace[0], "the same launch but for the epilogue form"


# ---- (2) refusals ------------------------------------------------------------------------------------------------------------------------
REFUSED = [("32x32", dict(n=1, hw=32, cout=192, G=8), {}),
           ("M240", dict(n=15, hw=4, cout=192, G=8), {}),
           ("cout320_width40", dict(n=1, hw=16, cout=320, G=8), {}),
           ("split_k", dict(n=1, hw=16, cout=192, G=8, cin=512, split_k=True), dict(NOPE_CONV_PP=3)),
           ("lean_off", dict(n=1, hw=16, cout=192, G=8), dict(NOPE_EPILOGUE_LEAN=0))]


@pytest.mark.parametrize("what,shape,env", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_unsupported_nothing_launched(be, what, shape, env, capfd):
    """Each combination conv_plan does not grant: the unsupported code, no conv launch in the trace, the output buffer as it was."""
    hip, dev, name = be
    n, hw, cout, G, cin = shape["n"], shape["hw"], shape["cout"], shape["G"], shape.get("cin", case.CIN)
    g = torch.Generator().manual_seed(9300)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    x, w, b, ga, bt = rn(n, hw, hw, cin), rn(cout, cin, 3, 3) / (9 * cin) ** 0.5, rn(cout), rn(cout), rn(cout)
    out = torch.full((n, hw, hw, cout), -7.5, dtype=torch.float32, device=dev)
    with switches(**dict(PP, NOPE_CONV_TRACE=1, **env)):
        if what == "split_k":      # the plan really is a split-K one: the launcher asks for a scratch at this shape
            assert int(hip._conv_query(**hip._conv_setup(hip.BF16X3, x, w, b, None, hip.CONV_PLAIN, 1, None, False, hip.F32, False).op).splitk_bytes) > 0
        capfd.readouterr()
        with pytest.raises(hip.NopeError) as ei:
            hip.op_conv_gn_self(hip.BF16X3, x, w, b, ga, bt, G, out=out, split_k=shape.get("split_k", False))
        trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    assert str(ei.value).endswith("(-6)"), str(ei.value)      # NOPE_ERR_UNSUPPORTED (include/nope_hip.h)
    assert not trace, trace
    assert bool((out == -7.5).all()), "a refused launch must not touch its output"


# ---- (3) network level -------------------------------------------------------------------------------------------------------------------
def _unet(cdt, dev):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    m = UNet(u_net_dim=32, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
    synth_init_(m, 2022)
    return m.to(dev)._get_handle(torch.device(dev))


def _forward(h, x, pose, epi, capfd):
    """(output, conv trace, range events) of one forward under NOPE_GN_EPI = epi"""
    with switches(NOPE_GN_EPI=epi, NOPE_CONV_TRACE=1):
        capfd.readouterr()
        y = h.forward(x, pose, x_rep=pose.shape[0] // x.shape[0])
        torch.cuda.synchronize()
        trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    ev = h.x2_range_check(torch.cuda.current_stream().cuda_stream)      # (code, layers out of range, layers whose shift moved, largest |activation|)
    return y.cpu(), trace, ev


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("cdt", ["bf16x3", "f16x2"])
def test_unet_bit_identical_and_path_taken(gpu, cdt, scale, capfd):
    g = torch.Generator().manual_seed(9400)
    x = (torch.randn(2, 8, 16, 16, generator=g) * scale).cuda()
    pose = torch.randn(16, 6, generator=g).cuda()
    with switches(**PP):
        h = _unet(cdt, "cuda")
        h.range_mode = "off"      # the handle does not look at the verdicts itself: _forward reads each forward's (x2_range_check) and compares them
        for _ in range(4):        # the range shifts of the two-pass layers settle on this input first (x2_range.h: a check re-centres them)
            _forward(h, x, pose, 0, capfd)
        y0, t0, e0 = _forward(h, x, pose, 0, capfd)
        runs = {epi: _forward(h, x, pose, epi, capfd) for epi in (3, 1, 2)}
        assert torch.equal(_forward(h, x, pose, 0, capfd)[0], y0), "the forward must be reproducible"
    assert torch.isfinite(y0).all() and e0[:3] == (0, 0, 0) and (e0[3] > 0) == (cdt == "f16x2"), e0
    assert not h.range_events
    for epi, (y, t, e) in runs.items():
        assert torch.equal(y, y0), (cdt, scale, epi, float((y - y0).abs().max()))
        assert e == e0, (cdt, scale, epi, "range events differ", e, e0)
        assert [ln.replace(" gn-self", "") for ln in t] == t0, "the conv launches, their kernels and their order must not change"
    t3 = runs[3][1]
    for m in (16 * 256, 16 * 64, 16 * 16):      # the 16 x 16, 8 x 8 and 4 x 4 levels
        assert any(ln.endswith(" gn-self") and f" M {m} " in ln for ln in t3), (m, "the form was never taken at this map size")
    assert not any("gn-self" in ln for ln in t0)
    n1, n2, n3 = (sum(ln.endswith(" gn-self") for ln in runs[k][1]) for k in (1, 2, 3))
    assert n1 > 0 and n2 > 0 and n3 == n1 + n2, (n1, n2, n3)


def test_workspace_query_does_not_depend_on_the_switch(be):
    hip, dev, name = be
    with switches(**PP):
        h = _unet("bf16x3", dev)
        sizes = []
        for epi in (0, 1, 3):
            with switches(NOPE_GN_EPI=epi):
                sizes.append(h.workspace_bytes(16, 2, 16, 16))
    assert sizes[0] > 0 and sizes[0] == sizes[1] == sizes[2], sizes
