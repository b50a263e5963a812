"""The guided-diffusion U-Net variant (nope_amd.guided, csrc/gd_runtime.hip): the parameter tree against the reference's, whole networks
against outputs recorded from the reference class itself with its forward call corrected (tests/golden/make_golden_guided.py:
guided.npz), the conv geometries of its 2x2 and 1x1 levels on every loader the launcher picks there, the shipped size in every
split-precision mode, and the variant inside PoseConditional with the Stable Diffusion VAE.

Network checks run on the device and, in f32 for two of the tiny cases, on the interpreter (tests/hipemu)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.golden.make_golden_guided import CASES, inputs, kwargs
from tests.util import StubEncoder, rel

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
OP_TOL = {0: 2e-5, 1: 4e-2, 2: 5e-3, 3: 3e-5}     # per dtype code (f32, bf16, f16, bf16x3), as test_ldm_configs.py
TINY = [t for t in CASES if t != "full"]
NPARAM_FULL = 552_818_948      # parameters of configs/model/vae_guidedDiffusion.yaml (the reference class counts the same: strict load)


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def _build(tag, cdt="f32", encoder=None, **over):
    from nope_amd.guided import UNetModelPose
    from nope_amd.weights import synth_init_
    kw = kwargs(tag)
    kw.update(over)
    m = UNetModelPose(encoder=encoder if encoder is not None else StubEncoder(4), compute_dtype=cdt, **kw)
    synth_init_(m, 2022)
    return m


def _case(golden, tag):
    from nope_amd.weights import sha256_of
    g = golden("guided.npz")
    x, pose = inputs(tag)
    assert sha256_of(torch.cat([x.flatten(), pose.flatten()])) == str(g[f"{tag}/sha_x"])        # the generator still gives the recorded inputs
    return x, pose, g[f"{tag}/out"]


def test_guided_parameter_tree(golden):
    """Keys and shapes equal the reference class's (conv1d qkv / proj_out, time_embed.* present); the weights are the recorded ones."""
    from nope_amd.weights import sha256_of
    g = golden("guided.npz")
    heads = {"neworder": ((32, 64), (64, 128), 64), "full": ((32, 32, 32, 64, 64, 64), (32, 32, 32, 64, 64, 64), 64)}
    for tag in CASES:
        m = _build(tag)
        sd = m.own_state_dict()
        assert sorted(f"{k}:{'x'.join(map(str, v.shape))}" for k, v in sd.items()) == [str(k) for k in g[f"{tag}/keys"]], tag
        assert sha256_of(sd["input_blocks.0.0.weight"]) == str(g[f"{tag}/sha_in"])
        if tag in heads:
            assert (m.head_channels_in, m.head_channels_out, m.head_channels_mid) == heads[tag], tag
    sd = _build("full").own_state_dict()
    assert tuple(sd["input_blocks.10.1.qkv.weight"].shape) == (3 * 512, 512, 1) and tuple(sd["middle_block.1.proj_out.weight"].shape) == (1024, 1024, 1)
    assert "time_embed.2.weight" in sd and "label_emb.weight" not in sd
    assert sum(v.numel() for v in sd.values()) == NPARAM_FULL


def test_guided_rejected():
    """What raises NotImplementedError: 3-d, class conditioning, an unknown pose MLP, posEncoding where the reference cannot build it,
    head widths other than 32 / 64 / 128 or widths that do not divide the channels (num_heads=4 alone: 256-wide heads at 1024 channels)."""
    from nope_amd.guided import UNetModelPose
    base = kwargs("legacy")
    full = kwargs("full")
    for kw in (dict(base, dims=3), dict(base, num_classes=10), dict(base, pose_mlp_name="three_layers"), dict(base, pose_mlp_name="posEncoding"),
               dict(base, pose_mlp_name="posEncoding", model_channels=96, rot_representation_dim=4), dict(base, num_head_channels=16),
               dict(base, num_head_channels=48), dict(base, num_head_channels=-1, num_heads=3), dict(full, num_head_channels=-1),
               dict(base, num_head_channels=-1, num_heads=1, num_heads_upsample=4)):
        with pytest.raises(NotImplementedError):
            UNetModelPose(encoder=StubEncoder(4), **kw)


@pytest.mark.parametrize("tag", TINY)
def test_guided_vs_reference(be, golden, tag):
    """Whole network through nope_gd_* against the reference class's recorded output: f32, bf16, bf16x3 and f16x2 (the 3x3 convs forced
    onto the two-pass tile, range mode "repeat"); the batched form equals one forward per hypothesis bit for bit (f32); the interpreter
    runs f32 of two of the cases."""
    hip, dev, name = be
    if name == "emu" and tag not in ("legacy", "bottom1"):
        pytest.skip("interpreter: two cases (the device runs all of them)")
    x, pose, ref = _case(golden, tag)
    for cdt, tol in (("f32", 1e-5), ("bf16", 8e-2), ("bf16x3", 1e-4), ("f16x2", 1e-4)):
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
        print(f"guided {tag} {cdt}: {rel(y, ref):.2e}")
        assert rel(y, ref) < tol, (tag, cdt, rel(y, ref))
        if cdt == "f32":       # the batched form = one forward per hypothesis
            bank = m.forward_hypotheses(x[:1].to(dev), pose.unsqueeze(0).to(dev))[0].cpu()
            one = torch.cat([m(x[:1].to(dev), pose[i:i + 1].to(dev)).cpu() for i in range(pose.shape[0])])
            assert torch.equal(bank, one)


def _kernel_of(err):
    kinds = [ln.split()[1] for ln in err.splitlines() if ln.startswith("conv ")]
    assert len(kinds) == 1, err
    return "small" if kinds[0].startswith("small") else kinds[0]


def _conv_ref(x, w, b, mode, hip):
    x, w, b = x.double(), w.double(), b.double()
    if mode == hip.CONV_STRIDE2:
        return F.conv2d(x, w, b, stride=2, padding=1)
    if mode == hip.CONV_UP2P:
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_small_level_convs(be, dt, monkeypatch, capfd):
    """The conv launches of the 2x2 and 1x1 levels -- 3x3 stride 1 at 2x2 and 1x1, the stride-2 Downsample conv 2x2 -> 1x1, the nearest-x2
    Upsample phase conv 1x1 -> 2x2, skip 1x1s -- against F.conv2d in f64, from 1 to 512 hypotheses, under each launch policy that changes
    the loader (default, small-tile off, small-tile whenever it applies, ping-pong at any tile count) and with channel counts that are not
    a whole K step (the generic kernel).  The launcher's trace says which loaders ran."""
    hip, dev, name = be
    if name == "emu" and dt not in (0, 1):
        pytest.skip("interpreter: the f32 and bf16 kernels")
    g = torch.Generator().manual_seed(500 + dt)
    P, S2, UP = hip.CONV_PLAIN, hip.CONV_STRIDE2, hip.CONV_UP2P
    # (mode, k, n, Cin, Cout, source side)
    shapes = [(P, 3, 3, 64, 64, 2), (P, 3, 2, 64, 32, 1), (S2, 3, 3, 64, 64, 2), (UP, 3, 2, 64, 64, 1), (P, 1, 3, 96, 64, 1), (P, 3, 2, 40, 32, 1),
              (UP, 3, 1, 40, 32, 1)]
    policies = [{}, {"NOPE_CONV_SMALL": "0"}, {"NOPE_CONV_SMALL": "2"}]
    if name == "gpu":
        shapes += [(P, 3, 512, 512, 512, 2), (P, 3, 512, 1024, 1024, 1), (P, 3, 1, 2048, 1024, 1), (S2, 3, 256, 1024, 1024, 2),
                   (UP, 3, 512, 1024, 1024, 1), (P, 1, 128, 2048, 1024, 1), (P, 3, 64, 1536, 1024, 2), (S2, 3, 1, 512, 512, 2),
                   (UP, 3, 7, 1024, 1024, 1), (P, 3, 96, 40, 64, 2)]
        policies += [{"NOPE_CONV_PP": "11"}]
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    seen = set()
    for pol in policies:
        for k in ("NOPE_CONV_SMALL", "NOPE_CONV_PP"):
            if k in pol:
                monkeypatch.setenv(k, pol[k])
            else:
                monkeypatch.delenv(k, raising=False)
        for (mode, k, n, cin, cout, hs) in shapes:
            x = torch.randn(n, cin, hs, hs, generator=g)
            w = torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5
            b = torch.randn(cout, generator=g) * 0.1
            xs = hip.to_nhwc(x.to(dev), dt)
            xr = hip.to_nchw(xs, dt).cpu()
            want = _conv_ref(xr, w, b, mode, hip)
            capfd.readouterr()
            if mode == UP:          # (the phase conv writes NHWC only)
                got = hip.to_nchw(hip.op_conv(dt, xs, w.to(dev), b.to(dev), mode=mode), dt).cpu()
            else:
                got = hip.op_conv(dt, xs, w.to(dev), b.to(dev), mode=mode, out_nchw=True).cpu()
            kind = _kernel_of(capfd.readouterr().err)
            seen.add(kind)
            assert got.shape == want.shape
            assert torch.isfinite(got).all() and rel(got, want) < OP_TOL[dt], (pol, dt, kind, mode, n, cin, cout, hs, rel(got, want))
    print(f"dt {dt}: loaders {sorted(seen)}")
    assert {"generic", "small"} <= seen, seen
    if name == "gpu":
        assert "dma128" in seen or "pp256" in seen, seen


@pytest.mark.gpu
def test_guided_full_size(gpu, golden):
    """configs/model/vae_guidedDiffusion.yaml at a 32x32 latent: f32 within 1e-4 of the reference's recorded output; bf16x3 and f16x2 over
    128 hypotheses within 1e-4 of the f32 mode, on the plain inputs and on inputs x 1e4 (range mode "repeat")."""
    x, pose, ref = _case(golden, "full")
    m = _build("full").cuda()
    y = m(x.cuda(), pose.cuda()).cpu()
    print(f"guided full f32: {rel(y, ref):.2e}")
    assert rel(y, ref) < 1e-4
    g = torch.Generator().manual_seed(95)
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
            print(f"guided full x{scale:g} {cdt}: {rel(got, want):.2e}")
            assert torch.isfinite(got).all() and rel(got, want) < 1e-4, (scale, cdt, rel(got, want))
            del mm
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_pose_conditional_drives_guided(gpu):
    """PoseConditional around the variant with a small VAE_StableDiffusion as its encoder, from images: generate_and_retrieve in f16x2
    ranks the same top-5 as in f32 with scores within 1e-4; its bank is forward_hypotheses'; sample()[1] = (decode_latent(pred) + 1) / 2."""
    from nope_amd.model import PoseConditional
    from tests.golden.make_golden_vae import SEED, make_vae
    g = torch.Generator().manual_seed(96)
    ref, query = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda(), (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
    poses = torch.randn(2, 40, 6, generator=g).cuda()
    res = {}
    for cdt in ("f32", "f16x2"):
        if cdt == "f16x2":           # (the 3x3 convs on the two-pass tile: a bank this small would not reach it)
            os.environ["NOPE_CONV_PP"] = "11"
        try:
            vae = make_vae("tiny", compute_dtype=cdt)
            u = _build("bottom1", cdt, encoder=vae, image_size=64)
            vae.synth_init_(SEED)
            pc = PoseConditional(u, None, {"similarity_metric": "l2"}, None).cuda()
            sim, idx, bank = pc.generate_and_retrieve(query, ref, poses)
            lat = vae.encode_image(ref)
            again = u.forward_hypotheses(lat, poses)
            if cdt == "f32":
                pred, rgb = pc.sample(ref, poses[:, 0])
                assert rgb.shape == (2, 3, 64, 64)
                assert torch.allclose(rgb, (vae.decode_latent(pred) + 1) / 2, atol=1e-6, rtol=0)
        finally:
            os.environ.pop("NOPE_CONV_PP", None)
        if cdt == "f32":
            assert torch.equal(bank, again)
        else:
            assert rel(again.cpu(), bank.cpu()) < 1e-4
        res[cdt] = (sim.cpu(), idx.cpu(), bank.cpu())
    assert torch.equal(res["f32"][1], res["f16x2"][1])
    assert rel(res["f16x2"][0], res["f32"][0]) < 1e-4 and rel(res["f16x2"][2], res["f32"][2]) < 1e-4
