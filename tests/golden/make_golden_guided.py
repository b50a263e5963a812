"""Fixtures of the guided-diffusion U-Net variant, recorded from THE REFERENCE CLASS ITSELF
(src/model/u_net/guided_diffusion/adapt_u_net.py: UNetModelPose):

    python tests/golden/make_golden_guided.py        # build container only (needs the reference sources)

The reference's forward calls `module(h, emb, emb)`, which guided-diffusion's TimestepEmbedSequential.forward(x, emb) does not accept:
every forward raises TypeError.  This script corrects that one call at run time -- a TimestepEmbedSequential.forward of our own that
accepts and ignores a third argument -- so emb = pose_mlp(pose) drives every ResBlock (nope_amd/guided.py runs the same reading).

Tiny networks cover both attention orders, num_heads vs num_head_channels, num_heads_upsample != num_heads, resblock_updown,
conv_resample and FiLM on and off, the three pose MLPs ("posEncoding" at model_channels = 96, where the reference can build it),
attention at ds = 1 (64 tokens) and a 1x1 bottom level; "full" is configs/model/vae_guidedDiffusion.yaml, 2 hypotheses at a 32x32 latent.
Weights are `synth_init_(mine, 2022)`, loaded STRICTLY into the reference class (key / shape parity); only outputs, input digests, a
weight digest and the reference's key / shape list are stored; the inputs are regenerated from a seeded generator (`inputs(tag)`, pinned by their digest).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from nope_amd.weights import sha256_of, synth_init_  # noqa: E402

SEED = 2022

TINY = dict(rot_representation_dim=6, image_size=8, in_channels=4, out_channels=4, num_res_blocks=1)
# tag: (constructor arguments over TINY, latent size, samples)
CASES = {
    # legacy order, num_head_channels, FiLM, Downsample / Upsample convs, attention at ds = 1 (64 tokens) and 2
    "legacy": (dict(model_channels=32, channel_mult=(1, 2), attention_resolutions=[1, 2], num_head_channels=32,
                    pose_mlp_name="single_layer", use_scale_shift_norm=True), 8, 3),
    # new order, num_heads = 2 (widths 32 / 64) with num_heads_upsample = 1 (64 / 128), two-layer MLP, no FiLM, resblock_updown
    "neworder": (dict(model_channels=64, channel_mult=(1, 2), attention_resolutions=[1, 2], num_heads=2, num_heads_upsample=1,
                      use_new_attention_order=True, pose_mlp_name="two_layers", resblock_updown=True), 8, 3),
    # posEncoding (model_channels = 96: 3 / 6 heads of 32), conv_resample = False (avg_pool / nearest alone), FiLM
    "posenc": (dict(model_channels=96, channel_mult=(1, 2), attention_resolutions=[2], num_head_channels=32,
                    pose_mlp_name="posEncoding", conv_resample=False, use_scale_shift_norm=True), 8, 3),
    # a 1x1 bottom level: channel_mult (1, 2, 2, 2) at 8x8, attention at 2x2 and 1x1, resblock_updown, FiLM, two ResBlocks a level
    "bottom1": (dict(model_channels=32, channel_mult=(1, 2, 2, 2), attention_resolutions=[4, 8], num_head_channels=32, num_res_blocks=2,
                     pose_mlp_name="single_layer", resblock_updown=True, use_scale_shift_norm=True), 8, 3),
    # the same with Downsample / Upsample convs at 2x2 -> 1x1 -> 2x2, legacy heads from num_heads
    "bottom1conv": (dict(model_channels=32, channel_mult=(1, 2, 2, 2), attention_resolutions=[2, 4, 8], num_heads=2,
                         pose_mlp_name="two_layers"), 8, 3),
    # configs/model/vae_guidedDiffusion.yaml
    "full": (dict(model_channels=256, channel_mult=(1, 1, 2, 2, 4, 4), attention_resolutions=[32, 16, 8], num_head_channels=64, num_heads=4,
                  num_heads_upsample=-1, num_res_blocks=2, resblock_updown=True, use_scale_shift_norm=True, num_classes=None,
                  pose_mlp_name="single_layer", image_size=256), 32, 2),
}


def inputs(tag):
    """x (n, 4, hw, hw), pose (n, 6) of a case: torch's CPU generator, seeded per case."""
    _, hw, n = CASES[tag]
    g = torch.Generator().manual_seed(SEED + 31 + list(CASES).index(tag))
    return torch.randn(n, 4, hw, hw, generator=g), torch.randn(n, 6, generator=g)


def kwargs(tag):
    kw = dict(TINY)
    kw.update(CASES[tag][0])
    return kw


def _correct_forward_call():
    """TimestepEmbedSequential.forward accepting (and ignoring) the third argument adapt_u_net.py passes."""
    from src.model.u_net.guided_diffusion import u_net as gd
    two_args = gd.TimestepEmbedSequential.forward

    def forward(self, x, emb, _ignored=None):
        return two_args(self, x, emb)
    gd.TimestepEmbedSequential.forward = forward


@torch.no_grad()
def main():
    import _ref_import as RI          # (here, not at the top: the tests import CASES / inputs / kwargs from this file)
    RI.install()
    from src.model.u_net.guided_diffusion.adapt_u_net import UNetModelPose as RefGd
    from nope_amd.guided import UNetModelPose
    _correct_forward_call()
    out = {}
    for tag in CASES:
        kw = kwargs(tag)
        mine = UNetModelPose(encoder=RI.StubEncoder(4), **kw)
        synth_init_(mine, SEED)
        ref = RefGd(encoder=RI.StubEncoder(4), **kw)
        ref.load_state_dict(mine.state_dict(), strict=True)       # proves key / shape parity
        ref.eval()
        x, pose = inputs(tag)
        y = ref(x, pose)
        assert float(y.abs().max()) > 1e-3
        out[f"{tag}/out"] = y.numpy()
        out[f"{tag}/sha_x"] = np.array(sha256_of(torch.cat([x.flatten(), pose.flatten()])))
        out[f"{tag}/sha_in"] = np.array(sha256_of(mine.state_dict()["input_blocks.0.0.weight"]))
        out[f"{tag}/keys"] = np.array(sorted(f"{k}:{'x'.join(map(str, v.shape))}" for k, v in ref.state_dict().items() if not k.startswith("encoder.")))
        print(tag, tuple(y.shape), mine.head_channels_in, mine.head_channels_out, mine.head_channels_mid)
    path = os.path.join(HERE, "guided.npz")
    np.savez_compressed(path, **out)
    print(f"guided.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
