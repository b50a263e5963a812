"""The tap-resident 3x3 kernel's padding-skipping form for 4 x 4 maps (conv3x3_halo_kernel, PADSKIP; NOPE_HALO_PADSKIP): a 256-row tile of 16
whole samples is staged in (position, sample) order, the 12 of 72 MFMA block-taps per channel chunk that lie wholly in the zero padding are not
executed, and the waves exchange accumulators through LDS in front of the unchanged lean epilogue.

(1) operator level, interpreter and device (tests/halo_padskip_emu_case.py: shapes, forms and inputs are listed there): NOPE_HALO_PADSKIP=1 against 0,
    torch.equal on the output and on the column statistics / the recorded range maximum; an impulse case against F.conv2d in f64;
(2) the same cases once more on the interpreter under its adversarial DMA and shuffle settings (a subprocess: the settings are read at load time);
(3) launches the planner does not grant the form to: marker absent, results equal to the switch-off run;
(4) network level, device: a 32-dim U-Net under 16 hypotheses at a 16 x 16 latent, switch 1 against 0: outputs bit-equal, range events equal, the
    marker on the 4 x 4 launches only; the workspace query does not depend on the switch."""
import os
import subprocess
import sys

import pytest
import torch

from tests import halo_padskip_emu_case as case
from tests.util import StubEncoder, switches

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
MODES = ["bf16x3", "f16x2"]


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, "cuda" if request.param == "gpu" else "cpu", request.param


def _dt(hip, mode):
    return {"bf16x3": hip.BF16X3, "f16x2": hip.F16X2}[mode]


# ---- (1) operator level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", case.FORMS)
@pytest.mark.parametrize("shape", case.SHAPES, ids=lambda s: f"n{s[0]}_c{s[1]}+{s[2]}_cout{s[3]}")
def test_op_equal_to_the_sample_major_form(be, shape, form, mode):
    hip, dev, name = be
    case.one_case(hip, dev, _dt(hip, mode), shape, form)


@pytest.mark.parametrize("mode", MODES)
def test_impulses_land_where_conv2d_puts_them(be, mode):
    hip, dev, name = be
    case.impulse_case(hip, dev, _dt(hip, mode), mode)


# ---- (2) the interpreter's adversarial settings ------------------------------------------------------------------------------------------
def test_interpreter_late_dma_and_shuffled_waves(emu):
    """DMA pieces that land as late as the waits allow, waves scheduled in a shuffled order: a missing wait or barrier in the form (the stage
    loads, the in-place rewrite, the accumulator exchange) shows as a wrong value."""
    env = dict(os.environ, HIPEMU_DMA="late", HIPEMU_SHUFFLE="1", HIPEMU_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(case.ROOT, "tests", "halo_padskip_emu_case.py"), "--light"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=3000)
    assert r.returncode == 0 and "halo_padskip_emu_case OK" in r.stdout, r.stdout[-3000:]


# ---- (3) not taken -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(case.NOT_TAKEN))
def test_not_taken_and_unchanged(be, what):
    hip, dev, name = be
    case.not_taken_case(hip, dev, what)


# ---- (4) network level -------------------------------------------------------------------------------------------------------------------
def _unet(cdt, dev):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    m = UNet(u_net_dim=32, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
    synth_init_(m, 2022)
    return m.to(dev)._get_handle(torch.device(dev))


def _forward(h, x, pose, sw, capfd):
    """(output, conv trace, range events) of one forward under NOPE_HALO_PADSKIP = sw"""
    with switches(NOPE_HALO_PADSKIP=sw, NOPE_CONV_TRACE=1):
        capfd.readouterr()
        y = h.forward(x, pose, x_rep=pose.shape[0] // x.shape[0])
        torch.cuda.synchronize()
        trace = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("conv ")]
    ev = h.x2_range_check(torch.cuda.current_stream().cuda_stream)
    return y.cpu(), trace, ev


@pytest.mark.gpu
@pytest.mark.parametrize("cdt", MODES)
def test_unet_bit_identical_and_path_taken(gpu, cdt, capfd):
    g = torch.Generator().manual_seed(9700)
    x = torch.randn(2, 8, 16, 16, generator=g).cuda()
    pose = torch.randn(16, 6, generator=g).cuda()
    with switches(**case.PP):
        h = _unet(cdt, "cuda")
        h.range_mode = "off"      # the handle does not look at the verdicts itself: _forward reads each forward's and compares them
        for _ in range(4):        # the range shifts of the two-pass layers settle on this input first
            _forward(h, x, pose, 0, capfd)
        y0, t0, e0 = _forward(h, x, pose, 0, capfd)
        y1, t1, e1 = _forward(h, x, pose, 1, capfd)
        assert torch.equal(_forward(h, x, pose, 0, capfd)[0], y0), "the forward must be reproducible"
    assert torch.isfinite(y0).all() and e0[:3] == (0, 0, 0), e0
    assert torch.equal(y1, y0), (cdt, float((y1 - y0).abs().max()))
    assert e1 == e0, (cdt, "range events differ", e1, e0)
    assert [ln.replace(" padskip", "") for ln in t1] == t0, "the conv launches, their kernels and their order must not change"
    assert not any("padskip" in ln for ln in t0)
    marked = [ln for ln in t1 if " padskip" in ln]
    assert marked and all(" halo256 " in ln and " taps 9 " in ln and f" M {16 * 16} " in ln for ln in marked), marked      # the 4 x 4 level only
    assert any(ln.endswith(" lean gn-self") for ln in marked), marked      # (the kernel's own GroupNorm is granted at this level: test_gn_epilogue.py)
    assert all(" padskip" in ln for ln in t1 if " halo256 " in ln and " taps 9 " in ln and f" M {16 * 16} " in ln and " lean" in ln), "a 4 x 4 lean launch without the form"


def test_workspace_query_does_not_depend_on_the_switch(be):
    hip, dev, name = be
    with switches(**case.PP):
        h = _unet("bf16x3", dev)
        sizes = []
        for sw in (0, 1):
            with switches(NOPE_HALO_PADSKIP=sw):
                sizes.append(h.workspace_bytes(16, 2, 16, 16))
    assert sizes[0] > 0 and sizes[0] == sizes[1], sizes
