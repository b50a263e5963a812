"""The Stable Diffusion VAE (nope_amd.vae, csrc/vae_runtime.hip): the asymmetric stride-2 conv geometry of its Downsample, the one-head
attention of width 256 / 512, the whole encoder / decoder against outputs recorded from the reference's CompVis Encoder / Decoder
(tests/golden/make_golden_vae.py: vae.npz), loading from a diffusers directory, chunked decoding and PoseConditional with the VAE.

Operator and network checks run on the device and, for the f32 and bf16 kernels, on the interpreter (tests/hipemu)."""
import json

import pytest
import torch
import torch.nn.functional as F

from tests.golden.make_golden_vae import CASES, SEED, config, inputs, make_vae
from tests.util import MODE_BOUNDS, rel

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
OP_TOL = {0: 2e-5, 1: 4e-2, 2: 5e-3, 3: 3e-5, 4: 3e-5}     # per dtype code (f32, bf16, f16, bf16x3, f16x2), as test_ldm_configs.py
ENC_TOL, DEC_TOL = 1.5e-5, 1.5e-5   # f32 against the reference (max-relative): ~3x the 4.8e-6 / 5.2e-6 an MI355X shows at SD-1.5 (tiny / mid: 1-2.3e-6)


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


# ---- NOPE_CONV_STRIDE2_PAD01 ------------------------------------------------------------------------------------------------------
def _kernel_of(err):
    """The conv kernel a launch took, from the launcher's NOPE_CONV_TRACE line ("conv <kernel> mode ...")."""
    kinds = [ln.split()[1] for ln in err.splitlines() if ln.startswith("conv ") and " mode 4 taps 9 " in ln]
    assert len(kinds) == 1, err
    return "small" if kinds[0].startswith("small") else kinds[0]


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_stride2_pad01_conv(be, dt, monkeypatch, capfd):
    """pad (0, 1, 0, 1) + 3x3 stride 2 (Downsample, u_net/ldm/model.py:57-74) as one launch against F.conv2d(F.pad(x, (0, 1, 0, 1)), w,
    stride=2): odd and even output sizes, on each of the three loaders that implement the geometry -- the generic kernel (Cin not a
    whole K step), the small-tile kernel (few 128 x 192 tiles) and the LDS-DMA 128 x 192 kernel (>= 320 tiles on the device: a batched
    256^2 encode; on the interpreter the small-tile policy is switched off, NOPE_CONV_SMALL=0).  The launcher's trace says which ran."""
    hip, dev, name = be
    if name == "emu" and dt not in (0, 1):
        pytest.skip("interpreter: the f32 and bf16 kernels")
    g = torch.Generator().manual_seed(300 + dt)
    # (n, Cin, Cout, source side, NOPE_CONV_SMALL override)
    shapes = [(2, 32, 32, 14, None), (1, 64, 40, 8, None), (1, 128, 256, 16, None), (2, 24, 16, 10, None)]
    if name == "gpu":
        shapes += [(4, 128, 128, 64, None), (2, 256, 256, 34, None), (8, 128, 192, 32, None), (3, 64, 64, 256, None), (2, 128, 40, 30, None)]
    else:
        shapes += [(1, 128, 256, 16, "0"), (2, 64, 40, 10, "0")]
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    seen = set()
    for (n, cin, cout, hs, small) in shapes:
        if small is None:
            monkeypatch.delenv("NOPE_CONV_SMALL", raising=False)
        else:
            monkeypatch.setenv("NOPE_CONV_SMALL", small)
        x = torch.randn(n, cin, hs, hs, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        xs = hip.to_nhwc(x.to(dev), dt)
        xr = hip.to_nchw(xs, dt).cpu()            # (the storage-rounded input)
        want = F.conv2d(F.pad(xr.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2)
        capfd.readouterr()
        got = hip.op_conv(dt, xs, w.to(dev), b.to(dev), mode=hip.CONV_STRIDE2_PAD01, out_nchw=True).cpu()
        kind = _kernel_of(capfd.readouterr().err)
        seen.add(kind)
        assert got.shape == want.shape == (n, cout, hs // 2, hs // 2)
        assert rel(got, want) < OP_TOL[dt], (dt, kind, n, cin, cout, hs, rel(got, want))
        if dt == 0:      # not the STRIDE2 geometry (centre tap at (2 oy, 2 ox))
            other = hip.op_conv(dt, xs, w.to(dev), b.to(dev), mode=hip.CONV_STRIDE2, out_nchw=True).cpu()
            assert rel(other, want) > 1e-2
    assert {"generic", "small", "dma128"} <= seen, seen


def test_stride2_pad01_rejects_other_taps(emu):
    hip = emu
    xs = hip.to_nhwc(torch.randn(1, 16, 8, 8), 0)
    with pytest.raises(hip.NopeError, match="nope_op_conv"):
        hip.op_conv(0, xs, torch.randn(16, 16, 1, 1), mode=hip.CONV_STRIDE2_PAD01)
    with pytest.raises(hip.NopeError, match="nope_op_conv"):
        hip.op_conv(0, hip.to_nhwc(torch.randn(1, 16, 7, 7), 0), torch.randn(16, 16, 3, 3), mode=hip.CONV_STRIDE2_PAD01)


# ---- nope_op_wide_attention ---------------------------------------------------------------------------------------------------------
def _attention_f64(qkv):
    q, k, v = qkv.double().chunk(3, dim=-1)
    return ((q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5).softmax(-1) @ v


@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("dt", [0, 1, 2, 3, 4])
def test_wide_attention(be, dt, C):
    """One head of C = 256 / 512 channels against torch in f64 on the storage-rounded inputs: ragged token counts, several samples,
    4 096 tokens on the device."""
    hip, dev, name = be
    if name == "emu" and dt not in (0, 1):
        pytest.skip("interpreter: the f32 and bf16 kernels")
    g = torch.Generator().manual_seed(400 + C + dt)
    tdt = hip.torch_dtype(hip.storage_code(dt))
    shapes = [(2, 37), (1, 300)] if name == "emu" else [(2, 37), (1, 300), (3, 1025), (1, 4096)]
    for (n, N) in shapes:
        qkv = torch.randn(n, N, 3 * C, generator=g).to(tdt)
        want = _attention_f64(qkv.float()).float()
        got = hip.op_wide_attention(dt, qkv.to(dev)).float().cpu()
        assert torch.isfinite(got).all() and rel(got, want) < OP_TOL[dt], (dt, C, n, N, rel(got, want))


@pytest.mark.parametrize("C", [256, 512])
def test_wide_attention_large_scores(be, C):
    """Scores of +-50 (softmax close to one-hot) in every f32-storage mode."""
    hip, dev, name = be
    g = torch.Generator().manual_seed(500 + C)
    q = torch.randn(2, 130, C, generator=g)
    q = q / q.norm(dim=-1, keepdim=True) * (50.0 * C ** 0.5) ** 0.5
    qkv = torch.cat([q, q, torch.randn(2, 130, C, generator=g)], dim=-1)
    want = _attention_f64(qkv).float()
    for dt in ((0,) if name == "emu" else (0, 3, 4)):
        got = hip.op_wide_attention(dt, qkv.to(dev)).cpu()
        assert rel(got, want) < 2e-4, (dt, C, rel(got, want))


def test_wide_attention_rejects_other_widths(emu):
    hip = emu
    for C in (128, 384, 1024):
        with pytest.raises(hip.NopeError, match="nope_op_wide_attention"):
            hip.op_wide_attention(0, torch.randn(1, 16, 3 * C))


# ---- the whole network in f32 against the reference ---------------------------------------------------------------------------------
def _golden(golden, tag):
    from nope_amd.weights import sha256_of
    z = golden("vae.npz")
    image, latent = inputs(tag)
    assert sha256_of(torch.cat([image.flatten(), latent.flatten()])) == str(z[f"{tag}/sha_in"])
    return image, latent, z[f"{tag}/enc"], z[f"{tag}/dec"]


@pytest.mark.parametrize("tag", list(CASES))
def test_vae_matches_reference(be, golden, tag):
    """encode_image / decode_latent in f32 against the CompVis Encoder / Decoder + quant_conv / post_quant_conv and the 0.18215 scale.
    tiny: mid width 64 (the token-attention kernels); mid: 256 and sd15: 512 (the wide-attention kernel)."""
    hip, dev, name = be
    if name == "emu" and tag == "sd15":
        pytest.skip("interpreter: the SD-1.5 shapes run on the device")
    image, latent, want_e, want_d = _golden(golden, tag)
    vae = make_vae(tag)
    got_e = vae.encode_image(image.to(dev)).cpu()
    got_d = vae.decode_latent(latent.to(dev)).cpu()
    print(f"{tag}: encode {rel(got_e, want_e):.2e} decode {rel(got_d, want_d):.2e}")
    assert got_e.shape == want_e.shape and rel(got_e, want_e) < ENC_TOL
    assert got_d.shape == want_d.shape and rel(got_d, want_d) < DEC_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["mid", "sd15"])
def test_vae_modes(gpu, golden, tag):
    """bf16x3 / f16 / bf16 against the f32 mode within MODE_BOUNDS; f16x2 runs as bf16x3 (bit-identical)."""
    image, latent, _, _ = _golden(golden, tag)
    res = {}
    for mode in ("f32", "bf16x3", "f16x2", "f16", "bf16"):
        vae = make_vae(tag, compute_dtype=mode)
        res[mode] = (vae.encode_image(image.cuda()).cpu(), vae.decode_latent(latent.cuda()).cpu())
    for mode in ("bf16x3", "f16", "bf16"):
        for i in (0, 1):
            r = rel(res[mode][i], res["f32"][i])
            print(f"{tag} {mode} {'dec' if i else 'enc'} {r:.2e}")
            assert torch.isfinite(res[mode][i]).all() and r < MODE_BOUNDS[mode][0], (tag, mode, i, r)
    assert torch.equal(res["f16x2"][0], res["bf16x3"][0]) and torch.equal(res["f16x2"][1], res["bf16x3"][1])


# ---- loading, configuration ---------------------------------------------------------------------------------------------------------
def test_load_from_diffusers_directory(tmp_path, golden):
    """config.json + diffusion_pytorch_model.bin build the config path's module; the to_q / to_k / to_v / to_out.0 spelling loads to the same
    weights; the key / shape tree is the recorded one (the diffusers keys the CompVis map took, tests/golden/make_golden_vae.py)."""
    from nope_amd.vae import VAE_StableDiffusion
    ref = make_vae("tiny")
    sd = ref.encoder.state_dict()
    d = tmp_path / "vae"
    d.mkdir()
    cfg = dict(config("tiny"), _class_name="AutoencoderKL", _diffusers_version="0.14.0", sample_size=32, scaling_factor=0.18215)
    (d / "config.json").write_text(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in cfg.items()}))
    torch.save(sd, d / "diffusion_pytorch_model.bin")
    a = VAE_StableDiffusion(str(d))
    new = {}
    for k, v in sd.items():
        for o, n in ((".query.", ".to_q."), (".key.", ".to_k."), (".value.", ".to_v."), (".proj_attn.", ".to_out.0.")):
            k = k.replace(".attentions.0" + o, ".attentions.0" + n)
        new[k] = v
    assert any(".to_out.0." in k for k in new)
    torch.save(new, d / "diffusion_pytorch_model.bin")
    b = VAE_StableDiffusion(str(d))
    for m in (a, b):
        got = m.state_dict()
        assert list(got) == list(ref.state_dict())
        assert all(torch.equal(got[k], v) for k, v in ref.state_dict().items())
    assert (a.latent_dim, a.name, a.using_KL, a.encode_mode) == (4, "vae", False, "mode")
    recorded = sorted(str(s) for s in golden("vae.npz")["tiny/keys"])
    assert sorted("%s:%s" % (k, ",".join(str(s) for s in v.shape)) for k, v in sd.items()) == recorded
    assert all(k.startswith("encoder.") for k in a.state_dict())        # the wrapper's keys: encoder.encoder.*, encoder.quant_conv.*, ...
    assert "encoder.encoder.mid_block.attentions.0.query.weight" in a.state_dict()


def test_unsupported_config_and_modes():
    from nope_amd.vae import VAE_StableDiffusion
    for bad in ({"act_fn": "relu"}, {"down_block_types": ("AttnDownEncoderBlock2D",) * 4}, {"force_upcast": True}, {"mid_block_add_attention": False}):
        with pytest.raises(NotImplementedError, match=list(bad)[0]):
            VAE_StableDiffusion(None, config=dict(config("tiny"), **bad))
    vae = VAE_StableDiffusion(None, config=config("tiny"), using_KL=True)
    assert vae.encode_mode is None
    with pytest.raises(NotImplementedError):
        vae.encode_image(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        VAE_StableDiffusion(None)


# ---- chunked decode -----------------------------------------------------------------------------------------------------------------
def test_chunked_decode_equals_one_at_a_time(be):
    """40 latents under a workspace cap that forces several chunks: bit-identical to decoding them one at a time; load_state_dict drops the
    packed weights."""
    hip, dev, name = be
    vae = make_vae("tiny")
    g = torch.Generator().manual_seed(77)
    n = 40 if name == "gpu" else 12
    lat = torch.randn(n, 4, 8, 8, generator=g).to(dev)
    one = int(hip.lib().dll.nope_vae_workspace_bytes(vae._get_handle(lat.device)._h, 1, 1, 8, 8))
    vae.max_workspace_bytes = 5 * one            # (several samples per chunk, several chunks)
    whole = vae.decode_latent(lat)
    h = vae._handle
    assert h._ws[(str(lat.device), hip._stream(lat))].numel() <= 5 * one
    singles = torch.cat([vae.decode_latent(lat[i:i + 1]) for i in range(n)])
    assert torch.equal(whole, singles)
    sd = vae.state_dict()
    sd["encoder.decoder.conv_out.bias"] = sd["encoder.decoder.conv_out.bias"] + 1.0
    vae.load_state_dict(sd)
    assert vae._handle is None
    assert torch.allclose(vae.decode_latent(lat[:2]), whole[:2] + 1.0, atol=1e-5)


# ---- PoseConditional with the VAE ---------------------------------------------------------------------------------------------------
def _unet(cdt, vae):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_tensor
    u = UNet(u_net_dim=32, rot_representation_dim=6, encoder=vae, pose_mlp_name="single_layer", compute_dtype=cdt)
    with torch.no_grad():
        for k, v in u.state_dict().items():
            if not k.startswith("encoder."):
                v.copy_(synth_tensor(2022, k, tuple(v.shape)))
    return u


def _ldm(cdt, vae):
    from nope_amd.ldm import UNetModelPose
    from nope_amd.weights import synth_tensor
    from tests.golden.make_golden_ldm_configs import kwargs
    kw = kwargs("h64")
    kw.update(in_channels=4, out_channels=4, image_size=16)
    u = UNetModelPose(encoder=vae, compute_dtype=cdt, **kw)
    with torch.no_grad():
        for k, v in u.state_dict().items():
            if not k.startswith("encoder."):
                v.copy_(synth_tensor(2022, k, tuple(v.shape)))
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["unet", "ldm"])
def test_pose_conditional_with_vae(gpu, variant):
    """vae_base (UNet) and vae_cin_ldm (UNetModelPose) around the VAE, from images: generate_and_retrieve in f16x2 ranks the same top-5
    as in f32 with scores within 1e-4; sample()[1] = (decode_latent(pred) + 1) / 2; generate_templates' decoded templates are
    decode_latent of its bank."""
    from nope_amd.model import PoseConditional
    g = torch.Generator().manual_seed(93)
    ref, query = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda(), (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).cuda()
    poses = torch.randn(2, 24, 6, generator=g).cuda()
    res = {}
    for cdt in ("f32", "f16x2"):
        vae = make_vae("tiny", compute_dtype=cdt)
        u = (_unet if variant == "unet" else _ldm)(cdt, vae)
        vae.synth_init_(SEED)
        pc = PoseConditional(u, None, {"similarity_metric": "l2"}, None).cuda()
        sim, idx, bank = pc.generate_and_retrieve(query, ref, poses)
        res[cdt] = (sim.cpu(), idx.cpu())
        if cdt == "f32":
            pred, rgb = pc.sample(ref, poses[:, 0])
            assert rgb.shape == (2, 3, 32, 32)
            assert torch.allclose(rgb, (vae.decode_latent(pred) + 1) / 2, atol=1e-6, rtol=0)
            lat, tpl, none = pc.generate_templates(ref, poses)
            assert none is None and tpl.shape == (2, 24, 3, 32, 32)
            assert torch.equal(lat, bank)
            assert torch.equal(tpl, vae.decode_latent(lat.reshape(48, 4, 16, 16)).reshape(2, 24, 3, 32, 32))
    assert torch.equal(res["f32"][1], res["f16x2"][1])
    assert rel(res["f16x2"][0], res["f32"][0]) < 1e-4


def test_template_encoder_keeps_none(emu):
    """With the template encoder (no decode_latent) sample and generate_templates still return None in the decoded slots."""
    from nope_amd.model import PoseConditional
    from tests.util import StubEncoder

    class _U(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = StubEncoder(8)

        def forward(self, x, pose):
            return x

    pc = PoseConditional(_U(), None, {"similarity_metric": "l2"}, None)
    assert pc._decoder() is None
    x = torch.zeros(1, 8, 4, 4)
    out = pc.sample(x, torch.zeros(1, 6))
    assert out[1] is None and out[0] is x


def test_sample_with_a_foreign_decoder(emu):
    """An encoder whose decode_latent takes no `unnormalize` (another VAE wrapper): sample() applies (x + 1) / 2 to its output, as
    model.py:117-123 does."""
    from nope_amd.model import PoseConditional

    class _Enc(torch.nn.Module):
        latent_dim, name = 4, "vae"

        def encode_image(self, image, mode=None):
            return image

        def decode_latent(self, latent):
            return latent * 2

    class _U(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = _Enc()

        def forward(self, x, pose):
            return x

    pc = PoseConditional(_U(), None, {"similarity_metric": "l2"}, None)
    x = torch.randn(2, 4, 4, 4)
    pred, rgb = pc.sample(x, torch.zeros(2, 6))
    assert pred is x and torch.equal(rgb, (x * 2 + 1) / 2)


def test_generate_templates_empty_bank_shape(emu):
    """No templates: the decoded templates are (B, 0, 3, S, S), the documented shape."""
    from nope_amd.model import PoseConditional
    vae = make_vae("tiny")
    pc = PoseConditional(_unet("f32", vae), None, {"similarity_metric": "l2"}, None)
    bank, tpl, none = pc.generate_templates(torch.rand(1, 3, 32, 32) * 2 - 1, torch.zeros(1, 0, 6))
    assert bank.shape == (1, 0, 4, 16, 16) and tpl.shape == (1, 0, 3, 32, 32) and none is None
