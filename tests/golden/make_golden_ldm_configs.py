"""Fixtures of the LDM variant's wider configuration space, recorded from THE REFERENCE CLASS ITSELF (as make_golden.py ldm()):

    python tests/golden/make_golden_ldm_configs.py        # build container only (needs the reference sources)

Attention head widths 64 / 128 (`num_head_channels`, `num_heads` -- one network with 32 / 64 / 128), `resblock_updown` (ResBlocks
with down / up, openaimodel.py:177-288), `conv_resample=False` (avg_pool 2x2 / nearest x2 alone, :94-175), and one full-size case: the
shipped configuration (configs/model/vae_cin_ldm.yaml) with `num_heads=8` and `resblock_updown`, 2 hypotheses at a 32x32 latent.
Weights are `synth_init_(mine, 2022)`, loaded STRICTLY into the reference class (key / shape parity); only inputs, outputs and a weight
digest are stored; the inputs are regenerated from a seeded generator (`inputs(tag)`, pinned by their digest), which keeps the
fixture to the outputs.
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

TINY = dict(rot_representation_dim=6, image_size=8, in_channels=8, out_channels=8, use_spatial_transformer=True, transformer_depth=1)
# tag: (constructor arguments over TINY, latent size, samples)
CASES = {
    "h64": (dict(model_channels=64, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=[1, 2], context_dim=24, num_head_channels=64,
                 pose_mlp_name="single_layer", injecting_condition_twice=False), 8, 3),
    "heads2": (dict(model_channels=64, channel_mult=(1, 2, 4), num_res_blocks=1, attention_resolutions=[1, 2, 4], context_dim=24, num_heads=2,
                    pose_mlp_name="single_layer", injecting_condition_twice=False), 8, 3),
    "updown": (dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=[1, 2], context_dim=24, num_head_channels=32,
                    pose_mlp_name="two_layers", injecting_condition_twice=True, use_scale_shift_norm=True, resblock_updown=True), 8, 3),
    "noconv": (dict(model_channels=32, channel_mult=(1, 2, 2), num_res_blocks=1, attention_resolutions=[2], context_dim=24, num_head_channels=32,
                    pose_mlp_name="single_layer", injecting_condition_twice=False, conv_resample=False), 8, 3),
    "combo": (dict(model_channels=64, channel_mult=(1, 2), num_res_blocks=1, attention_resolutions=[1, 2], context_dim=24, num_heads=1,
                   pose_mlp_name="single_layer", injecting_condition_twice=True, resblock_updown=True, transformer_depth=2), 8, 3),
    # vae_cin_ldm.yaml with num_heads = 8 (widths 32 / 64 / 128) and resblock_updown
    "full": (dict(model_channels=256, channel_mult=(1, 2, 4), num_res_blocks=2, attention_resolutions=[4, 2, 1], context_dim=512, num_heads=8,
                  pose_mlp_name="single_layer", injecting_condition_twice=False, resblock_updown=True, image_size=32), 32, 2),
}


def inputs(tag):
    """x (n, 8, hw, hw), pose (n, 6) of a case: torch's CPU generator, seeded per case."""
    _, hw, n = CASES[tag]
    g = torch.Generator().manual_seed(SEED + 11 + list(CASES).index(tag))
    return torch.randn(n, 8, hw, hw, generator=g), torch.randn(n, 6, generator=g)


def kwargs(tag):
    kw = dict(TINY)
    kw.update(CASES[tag][0])
    return kw


@torch.no_grad()
def main():
    import _ref_import as RI          # (here, not at the top: the tests import CASES / inputs / kwargs from this file)
    RI.install()
    from src.model.u_net.ldm.adapt_openaimodel import UNetModelPose as RefLdm
    from nope_amd.ldm import UNetModelPose
    out = {}
    for tag in CASES:
        kw = kwargs(tag)
        mine = UNetModelPose(encoder=RI.StubEncoder(8), **kw)
        synth_init_(mine, SEED)
        ref = RefLdm(encoder=RI.StubEncoder(8), **kw)
        ref.load_state_dict(mine.state_dict(), strict=True)       # proves key / shape parity
        ref.eval()
        x, pose = inputs(tag)
        y = ref(x, pose)
        assert float(y.abs().max()) > 1e-3
        out[f"{tag}/out"] = y.numpy()
        out[f"{tag}/sha_x"] = np.array(sha256_of(torch.cat([x.flatten(), pose.flatten()])))
        out[f"{tag}/sha_in"] = np.array(sha256_of(mine.state_dict()["input_blocks.0.0.weight"]))
        print(tag, tuple(y.shape), mine.head_channels)
    path = os.path.join(HERE, "ldm_configs.npz")
    np.savez_compressed(path, **out)
    print(f"ldm_configs.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
