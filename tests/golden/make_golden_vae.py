"""Fixtures of the Stable Diffusion VAE (nope_amd.vae), recorded from THE REFERENCE'S CompVis Encoder / Decoder (src/model/u_net/ldm/model.py):

    python tests/golden/make_golden_vae.py        # build container only (needs the reference sources)

diffusers' AutoencoderKL is converted key for key from that network; the map below is the standard diffusers <-> CompVis one.  Weights are
`VAE_StableDiffusion(...).synth_init_(SEED)` under the diffusers keys, mapped onto the reference classes and loaded STRICTLY (key / shape
parity).  quant_conv, post_quant_conv, taking the first latent_channels moments and the 0.18215 scale are diffusers' and the wrapper's lines
(AutoencoderKL.py:33-34,44-47), restated here with F.conv2d.  Inputs are regenerated from a seeded generator (`inputs(tag)`, pinned by their
digest); only outputs, digests and the diffusers key / shape list are stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from nope_amd.vae import SD15_CONFIG, VAE_StableDiffusion  # noqa: E402
from nope_amd.weights import sha256_of  # noqa: E402

SEED = 2023
SCALE = 0.18215
# tag: (config over SD15_CONFIG, encode input (n, H), decode input (n, h))
CASES = {
    "tiny": (dict(block_out_channels=(32, 64), layers_per_block=1, down_block_types=("DownEncoderBlock2D",) * 2,
                  up_block_types=("UpDecoderBlock2D",) * 2), (2, 32), (2, 8)),
    "mid": (dict(block_out_channels=(64, 128, 256), layers_per_block=1, down_block_types=("DownEncoderBlock2D",) * 3,
                 up_block_types=("UpDecoderBlock2D",) * 3), (1, 64), (1, 8)),
    "sd15": (dict(), (1, 256), (1, 16)),
}


def config(tag):
    c = dict(SD15_CONFIG)
    c.update(CASES[tag][0])
    return c


def make_vae(tag, **kw):
    return VAE_StableDiffusion(None, config=config(tag), **kw).synth_init_(SEED)


def inputs(tag):
    """image (n, 3, H, H) uniform in [-1, 1] and latent (n, 4, h, h) ~ N(0, 1): torch's CPU generator, seeded per case."""
    _, (ne, H), (nd, h) = CASES[tag]
    g = torch.Generator().manual_seed(SEED + 7 + list(CASES).index(tag))
    image = torch.rand(ne, 3, H, H, generator=g) * 2 - 1
    latent = torch.randn(nd, config(tag)["latent_channels"], h, h, generator=g)
    return image, latent


def to_compvis(sd, part, n_levels):
    """diffusers AutoencoderKL keys of `part` ("encoder" / "decoder") -> CompVis Encoder / Decoder keys (attention Linear -> 1x1 conv)."""
    out = {}
    ren = {"group_norm": "norm", "query": "q", "key": "k", "value": "v", "proj_attn": "proj_out"}
    for k, v in sd.items():
        if not k.startswith(part + "."):
            continue
        p = k[len(part) + 1:].split(".")
        if p[0] == "conv_norm_out":
            p[0] = "norm_out"
        elif p[0] in ("down_blocks", "up_blocks"):
            lvl = int(p[1]) if p[0] == "down_blocks" else n_levels - 1 - int(p[1])
            if p[2] == "resnets":
                p = ["down" if p[0] == "down_blocks" else "up", str(lvl), "block", p[3]] + p[4:]
                if p[4] == "conv_shortcut":
                    p[4] = "nin_shortcut"
            else:                                      # downsamplers.0.conv / upsamplers.0.conv
                p = ["down" if p[0] == "down_blocks" else "up", str(lvl), "downsample" if p[2] == "downsamplers" else "upsample"] + p[4:]
        elif p[0] == "mid_block":
            if p[1] == "resnets":
                p = ["mid", "block_%d" % (int(p[2]) + 1)] + p[3:]
            else:
                p = ["mid", "attn_1", ren[p[3]]] + p[4:]
                if v.dim() == 2:
                    v = v[:, :, None, None]
        out[".".join(p)] = v
    return out


@torch.no_grad()
def main():
    import _ref_import as RI
    RI.install()
    from src.model.u_net.ldm.model import Decoder, Encoder
    out = {}
    for tag in CASES:
        cfg = config(tag)
        vae = make_vae(tag)
        sd = vae.encoder.state_dict()
        boc = cfg["block_out_channels"]
        mult = tuple(c // boc[0] for c in boc)
        z = cfg["latent_channels"]
        kw = dict(ch=boc[0], ch_mult=mult, num_res_blocks=cfg["layers_per_block"], attn_resolutions=[], in_channels=cfg["in_channels"],
                  resolution=256, z_channels=z, dropout=0.0)
        enc = Encoder(out_ch=cfg["out_channels"], double_z=True, **kw)
        dec = Decoder(out_ch=cfg["out_channels"], **kw)
        enc.load_state_dict(to_compvis(sd, "encoder", len(boc)), strict=True)
        dec.load_state_dict(to_compvis(sd, "decoder", len(boc)), strict=True)
        enc.eval(); dec.eval()
        image, latent = inputs(tag)
        moments = F.conv2d(enc(image), sd["quant_conv.weight"], sd["quant_conv.bias"])
        lat = moments[:, :z] * SCALE                                  # latent_dist.mode() * 0.18215
        img = dec(F.conv2d(latent / SCALE, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"]))
        assert float(lat.abs().max()) > 1e-3 and float(img.abs().max()) > 1e-3
        out[f"{tag}/enc"] = lat.numpy()
        out[f"{tag}/dec"] = img.numpy()
        out[f"{tag}/sha_in"] = np.array(sha256_of(torch.cat([image.flatten(), latent.flatten()])))
        out[f"{tag}/keys"] = np.array(["%s:%s" % (k, ",".join(str(s) for s in v.shape)) for k, v in sd.items()])
        print(tag, tuple(lat.shape), tuple(img.shape), float(lat.abs().max()), float(img.abs().max()))
    path = os.path.join(HERE, "vae.npz")
    np.savez_compressed(path, **out)
    print(f"vae.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
