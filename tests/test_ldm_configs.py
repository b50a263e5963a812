"""The LDM variant beyond its shipped configuration: attention heads 64 / 128 channels wide (num_head_channels, num_heads), ResBlocks
with down / up (resblock_updown), parameter-free resampling (conv_resample=False), and the variant inside PoseConditional.

Operator checks run on the device and, for the f32 and bf16 kernels, on the interpreter (tests/hipemu); whole networks are compared
with outputs recorded from the reference class itself (tests/golden/make_golden_ldm_configs.py: ldm_configs.npz)."""
import os

import pytest
import torch

from tests.golden.make_golden_ldm_configs import CASES, inputs, kwargs
from tests.util import StubEncoder, rel

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
F32_TOL = 1e-5
BF16_TOL = 4e-2
OP_TOL = {0: 2e-5, 1: BF16_TOL, 2: 5e-3, 3: 3e-5, 4: 3e-5}     # per dtype code (f32, bf16, f16, bf16x3, f16x2), as test_kernels_parity.py


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def _attention_f64(qkv, d):
    n, N, c3 = qkv.shape
    C = c3 // 3
    qq, kk, vv = (t.reshape(n, N, C // d, d).permute(0, 2, 1, 3) for t in qkv.double().chunk(3, dim=-1))
    return ((qq @ kk.transpose(-1, -2) * d ** -0.5).softmax(-1) @ vv).permute(0, 2, 1, 3).reshape(n, N, C)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dt", [0, 1, 2, 3, 4])
def test_token_attention_wide_heads(be, dt, d):
    """Softmax self-attention with heads of 64 / 128 channels in every kernel (f32: VALU, the head split across 2 / 4 lanes; bf16 / f16:
    v_mfma_f32_32x32x16; bf16x3 / f16x2: three bf16 passes over (hi, lo) splits) against torch in f64 on the storage-rounded inputs:
    ragged token counts, several heads, more keys than one block; the VALU kernel of the 16-bit modes too (NOPE_LDM_ATTN=0)."""
    hip, dev, name = be
    if name == "emu" and dt not in (0, 1):
        pytest.skip("interpreter: the f32 and bf16 kernels (the others share their schedules; all of them run on the device)")
    g = torch.Generator().manual_seed(70 + d)
    tdt = hip.torch_dtype(hip.storage_code(dt))
    shapes = [(2, 37, 2 * d), (1, 300, 2 * d), (1, 1025, 256)] if name == "gpu" else [(2, 37, 2 * d), (1, 130, d)]
    for (n, N, C) in shapes:
        qkv = torch.randn(n, N, 3 * C, generator=g).to(tdt)
        want = _attention_f64(qkv.float(), d).float()
        got = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).float().cpu()
        assert torch.isfinite(got).all() and rel(got, want) < OP_TOL[dt], (dt, d, n, N, C, rel(got, want))
        if name == "gpu" and dt in (1, 2):
            os.environ["NOPE_LDM_ATTN"] = "0"
            try:
                valu = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).float().cpu()
            finally:
                os.environ.pop("NOPE_LDM_ATTN", None)
            assert rel(valu, want) < OP_TOL[dt], (dt, d, N, "valu")


@pytest.mark.parametrize("d", [64, 128])
def test_token_attention_wide_heads_large_scores(be, d):
    """Scores of +-50 (softmax close to one-hot) in the split-precision kernel: within 2e-4 of f64 (the bound of the 32-wide kernel)."""
    hip, dev, name = be
    g = torch.Generator().manual_seed(80 + d)
    for (n, N, C) in ((1, 130, 2 * d),) if name == "emu" else ((1, 130, 2 * d), (2, 300, 256)):
        qkv = torch.randn(n, N, 3 * C, generator=g) * 4.0
        want = _attention_f64(qkv, d).float()
        assert rel(hip.op_token_attention(0, qkv.to(dev), dim_head=d).cpu(), want) < OP_TOL[0]
        for dt in (3, 4):
            got = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).cpu()
            assert rel(got, want) < 2e-4, (dt, d, N, rel(got, want))


def test_token_attention_rejects_other_widths(emu):
    """dim_head outside {32, 64, 128}, or not dividing the channels: NOPE_ERR_ARG (no kernel for it)."""
    hip = emu
    qkv = torch.randn(1, 16, 3 * 96)
    for d in (48, 16, 256, 64):          # (64: 96 channels are not whole 64-wide heads)
        with pytest.raises(hip.NopeError, match="nope_op_token_attention"):
            hip.op_token_attention(0, qkv, dim_head=d)


def _build(tag, cdt="f32", **over):
    from nope_amd.ldm import UNetModelPose
    from nope_amd.weights import synth_init_
    kw = kwargs(tag)
    kw.update(over)
    m = UNetModelPose(encoder=StubEncoder(8), compute_dtype=cdt, **kw)
    synth_init_(m, 2022)
    return m


def _case(golden, tag):
    from nope_amd.weights import sha256_of
    g = golden("ldm_configs.npz")
    x, pose = inputs(tag)
    assert sha256_of(torch.cat([x.flatten(), pose.flatten()])) == str(g[f"{tag}/sha_x"])        # the generator still gives the recorded inputs
    return x, pose, g[f"{tag}/out"]


def test_ldm_configs_parameter_tree(golden):
    """Head widths per level as the reference derives them; the weights are the recorded ones (digest); the resampling slots carry the
    reference's keys (ResBlocks under resblock_updown, nothing under conv_resample=False)."""
    from nope_amd.weights import sha256_of
    g = golden("ldm_configs.npz")
    want = {"h64": (64, 64), "heads2": (32, 64, 128), "updown": (32, 32), "noconv": (32, 32, 32), "combo": (64, 128), "full": (32, 64, 128)}
    for tag in CASES:
        m = _build(tag)
        assert m.head_channels == want[tag], tag
        sd = m.own_state_dict()
        assert sha256_of(sd["input_blocks.0.0.weight"]) == str(g[f"{tag}/sha_in"])
        if tag == "updown":
            assert "input_blocks.2.0.in_layers.2.weight" in sd and "output_blocks.1.2.out_layers.3.weight" in sd
            assert not any(k.endswith(".op.weight") or k.endswith(".conv.weight") for k in sd)
        if tag == "noconv":
            assert not any(k.startswith("input_blocks.2.") or k.endswith(".op.weight") or k.endswith(".conv.weight") for k in sd)


def test_ldm_configs_rejected():
    """What still raises: head widths outside 32 / 64 / 128, widths that do not divide a level's channels (the reference's inner_dim
    would differ from them), no spatial transformer."""
    base = kwargs("h64")
    from nope_amd.ldm import UNetModelPose
    for over in (dict(num_head_channels=48, legacy=False), dict(num_head_channels=16), dict(num_head_channels=-1, num_heads=1, model_channels=32, channel_mult=(1, 8)),
                 dict(num_head_channels=64, legacy=False, model_channels=96, channel_mult=(1, 2)), dict(use_spatial_transformer=False)):
        kw = dict(base)
        kw.update(over)
        with pytest.raises(NotImplementedError):
            UNetModelPose(encoder=StubEncoder(8), **kw)
    # legacy: 128 channels with num_head_channels = 96 are ONE head of 128 (openaimodel.py:570-576), as in the reference
    kw = dict(base, num_head_channels=96, model_channels=128, channel_mult=(1,), attention_resolutions=[1])
    assert UNetModelPose(encoder=StubEncoder(8), **kw).head_channels == (128,)


@pytest.mark.parametrize("tag", ["h64", "heads2", "updown", "noconv", "combo"])
def test_ldm_configs_vs_reference(be, golden, tag):
    """Whole network through nope_ldm_* against the reference class's recorded output: f32, bf16, bf16x3 and f16x2 (the 3x3 convs forced
    onto the two-pass tile, range mode "repeat", as test_ldm_unet_vs_reference_golden); the interpreter runs f32 of two of the cases."""
    hip, dev, name = be
    if name == "emu" and tag not in ("updown", "h64"):
        pytest.skip("interpreter: two cases (the device runs all of them)")
    x, pose, ref = _case(golden, tag)
    for cdt, tol in (("f32", F32_TOL), ("bf16", 8e-2), ("bf16x3", 1e-4), ("f16x2", 1e-4)):
        if name == "emu" and cdt != "f32":
            continue
        if cdt == "f16x2":
            os.environ["NOPE_CONV_PP"] = "11"
            os.environ["NOPE_X2_RANGE_CHECK"] = "2"
        try:
            m = _build(tag, cdt).to(dev)
            y = m(x.to(dev), pose.to(dev)).cpu()
        finally:
            os.environ.pop("NOPE_CONV_PP", None)
            os.environ.pop("NOPE_X2_RANGE_CHECK", None)
        print(f"LDM {tag} {cdt}: {rel(y, ref):.2e}")
        assert rel(y, ref) < tol, (tag, cdt, rel(y, ref))
        if cdt == "f32" and name == "gpu":       # the batched form = one forward per hypothesis
            bank = m.forward_hypotheses(x[:1].to(dev), pose.unsqueeze(0).to(dev))[0].cpu()
            one = torch.cat([m(x[:1].to(dev), pose[i:i + 1].to(dev)).cpu() for i in range(pose.shape[0])])
            assert torch.equal(bank, one)


@pytest.mark.gpu
def test_ldm_full_size_heads_updown(gpu, golden):
    """The shipped size with num_heads = 8 (widths 32 / 64 / 128) and resblock_updown: f32 within 1e-4 of the reference's recorded
    output; bf16x3 and f16x2 over 128 hypotheses within 1e-4 of the f32 mode, on the plain inputs and on inputs x 1e4 (range mode
    "repeat": a resampling producer that left the range tracking uninformed would leave f16x2 silently inaccurate there)."""
    x, pose, ref = _case(golden, "full")
    m = _build("full").cuda()
    y = m(x.cuda(), pose.cuda()).cpu()
    print(f"LDM full f32: {rel(y, ref):.2e}")
    assert rel(y, ref) < 1e-4
    g = torch.Generator().manual_seed(91)
    poses = torch.randn(1, 128, 6, generator=g).cuda()
    for scale in (1.0, 1e4):
        xs = (x[:1] * scale).cuda()
        want = m.forward_hypotheses(xs, poses).cpu()
        for cdt in ("bf16x3", "f16x2"):
            os.environ["NOPE_X2_RANGE_CHECK"] = "2"
            try:
                mm = _build("full", cdt).cuda()
                got = mm.forward_hypotheses(xs, poses).cpu()
            finally:
                os.environ.pop("NOPE_X2_RANGE_CHECK", None)
            print(f"LDM full x{scale:g} {cdt}: {rel(got, want):.2e}")
            assert torch.isfinite(got).all() and rel(got, want) < 1e-4, (scale, cdt, rel(got, want))


@pytest.mark.gpu
def test_pose_conditional_drives_ldm(gpu):
    """PoseConditional around the LDM variant (num_heads + resblock_updown): generate_and_retrieve in f16x2 ranks the same top-5 as in
    f32 with scores within 1e-4, and its bank is forward_hypotheses'."""
    from nope_amd.model import PoseConditional
    g = torch.Generator().manual_seed(92)
    ref_lat, query = torch.randn(2, 8, 16, 16, generator=g).cuda(), torch.randn(2, 8, 16, 16, generator=g).cuda()
    poses = torch.randn(2, 40, 6, generator=g).cuda()
    res = {}
    for cdt in ("f32", "f16x2"):
        if cdt == "f16x2":           # (the 3x3 convs on the two-pass tile: a bank this small would not reach it)
            os.environ["NOPE_CONV_PP"] = "11"
        try:
            u = _build("combo", cdt, image_size=16)
            pc = PoseConditional(u, None, {"similarity_metric": "l2"}, None).cuda()
            sim, idx, bank = pc.generate_and_retrieve(query, ref_lat, poses)
            again = u.forward_hypotheses(ref_lat, poses)
            templates = pc.generate_templates(ref_lat, poses)[0]
        finally:
            os.environ.pop("NOPE_CONV_PP", None)
        if cdt == "f32":
            assert torch.equal(bank, again) and torch.equal(bank, templates)
        else:                        # (the range shifts may have been re-centred between the calls: same values to the mode's accuracy)
            assert rel(again.cpu(), bank.cpu()) < 1e-4 and rel(templates.cpu(), bank.cpu()) < 1e-4
        res[cdt] = (sim.cpu(), idx.cpu(), bank.cpu())
    assert torch.equal(res["f32"][1], res["f16x2"][1])
    assert rel(res["f16x2"][0], res["f32"][0]) < 1e-4 and rel(res["f16x2"][2], res["f32"][2]) < 1e-4
