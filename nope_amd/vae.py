"""`VAE_StableDiffusion` -- the Stable Diffusion VAE encoder of the `vae_*` model configs (src/model/encoder/AutoencoderKL.py:6-47),
over diffusers' `AutoencoderKL` (the CompVis Encoder / Decoder of src/model/u_net/ldm/model.py:77-448).

Same constructor arguments and attributes as the reference (`latent_dim`, `name`, `using_KL`, `encode_mode`, `encoder`); `encoder` holds the
parameters under diffusers 0.14's AutoencoderKL key tree (`encoder.*`, `quant_conv.*`, `decoder.*`, `post_quant_conv.*`; the mid-block
attention as `group_norm` / `query` / `key` / `value` / `proj_attn`, Linear [C, C]), so the wrapper's state-dict keys are the reference
wrapper's.  `pretrained_path` names a diffusers model directory (`config.json` + `diffusion_pytorch_model.bin`); `pretrained_path=None,
config={...}` builds the same module from a config alone (synthetic weights: tests, the harness).

Execution: device tensors go through the C ABI (`nope_vae_*`, csrc/vae_runtime.hip) -- every convolution, GroupNorm, SiLU and the attention
on hand-written gfx950 kernels, 0.18215 and its inverse folded into quant_conv / post_quant_conv at pack time, and (x + 1) / 2 of
`PoseConditional.sample` folded into the output conv.  There is no torch forward and no fallback: the module tree only holds parameters.
"""
from __future__ import annotations

import json
import os
from typing import Optional

import torch
from torch import nn

from . import hip
from .handle_cache import HandleCache
from .weights import synth_tensor

SD15_CONFIG = dict(in_channels=3, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4,
                   norm_num_groups=32, act_fn="silu", down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4)

_ACCEPTED = {"in_channels", "out_channels", "block_out_channels", "layers_per_block", "latent_channels", "norm_num_groups", "act_fn",
             "down_block_types", "up_block_types"}
# diffusers' bookkeeping and fields whose value does not change the network this runtime evaluates
_IGNORED = {"_class_name", "_diffusers_version", "_name_or_path", "sample_size", "scaling_factor"}
_NEW_ATTN_NAMES = {"to_q.": "query.", "to_k.": "key.", "to_v.": "value.", "to_out.0.": "proj_attn."}


def check_config(config: dict) -> dict:
    """The fields of a diffusers AutoencoderKL config this runtime implements; anything else raises NotImplementedError naming the field."""
    cfg = dict(SD15_CONFIG)
    for k, v in config.items():
        if k in _IGNORED:
            continue
        if k not in _ACCEPTED:
            raise NotImplementedError(f"AutoencoderKL config field {k!r} is not supported")
        cfg[k] = v
    n = len(cfg["block_out_channels"])
    if cfg["act_fn"] != "silu":
        raise NotImplementedError(f"AutoencoderKL config field 'act_fn' = {cfg['act_fn']!r} is not supported (silu only)")
    if tuple(cfg["down_block_types"]) != ("DownEncoderBlock2D",) * n:
        raise NotImplementedError(f"AutoencoderKL config field 'down_block_types' = {cfg['down_block_types']!r} is not supported")
    if tuple(cfg["up_block_types"]) != ("UpDecoderBlock2D",) * n:
        raise NotImplementedError(f"AutoencoderKL config field 'up_block_types' = {cfg['up_block_types']!r} is not supported")
    cfg["block_out_channels"] = tuple(int(c) for c in cfg["block_out_channels"])
    return cfg


class _Holder(nn.Module):
    """Parameter container: never called."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder; the VAE runs in libnope_hip.so (VAE_StableDiffusion.encode_image / decode_latent)")


class _Resnet(_Holder):      # diffusers ResnetBlock2D, temb_channels=None
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-6)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=1e-6)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)


class _Attention(_Holder):   # diffusers 0.14 AttentionBlock, one head
    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=1e-6)
        self.query, self.key, self.value, self.proj_attn = (nn.Linear(c, c) for _ in range(4))


class _Mid(_Holder):
    def __init__(self, c, groups):
        super().__init__()
        self.attentions = nn.ModuleList([_Attention(c, groups)])
        self.resnets = nn.ModuleList([_Resnet(c, c, groups), _Resnet(c, c, groups)])


class _Sampler(_Holder):     # Downsample2D / Upsample2D: the conv only
    def __init__(self, c, stride):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=stride, padding=0 if stride == 2 else 1)


class _Block(_Holder):
    def __init__(self, cins, cout, groups, sampler):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(ci, cout, groups) for ci in cins])
        if sampler == "down":
            self.downsamplers = nn.ModuleList([_Sampler(cout, 2)])
        elif sampler == "up":
            self.upsamplers = nn.ModuleList([_Sampler(cout, 1)])


class _Encoder(_Holder):
    def __init__(self, cfg):
        super().__init__()
        boc, g, lpb = cfg["block_out_channels"], cfg["norm_num_groups"], cfg["layers_per_block"]
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, padding=1)
        blocks, ch = [], boc[0]
        for i, c in enumerate(boc):
            blocks.append(_Block([ch] + [c] * (lpb - 1), c, g, "down" if i < len(boc) - 1 else None))
            ch = c
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = _Mid(ch, g)
        self.conv_norm_out = nn.GroupNorm(g, ch, eps=1e-6)
        self.conv_out = nn.Conv2d(ch, 2 * cfg["latent_channels"], 3, padding=1)


class _Decoder(_Holder):
    def __init__(self, cfg):
        super().__init__()
        boc, g, lpb = cfg["block_out_channels"], cfg["norm_num_groups"], cfg["layers_per_block"]
        rev = tuple(reversed(boc))
        self.conv_in = nn.Conv2d(cfg["latent_channels"], rev[0], 3, padding=1)
        blocks, ch = [], rev[0]
        for i, c in enumerate(rev):
            blocks.append(_Block([ch] + [c] * lpb, c, g, "up" if i < len(rev) - 1 else None))
            ch = c
        self.up_blocks = nn.ModuleList(blocks)
        self.mid_block = _Mid(rev[0], g)
        self.conv_norm_out = nn.GroupNorm(g, ch, eps=1e-6)
        self.conv_out = nn.Conv2d(ch, cfg["out_channels"], 3, padding=1)


class AutoencoderKLParams(_Holder):
    """diffusers 0.14 AutoencoderKL's parameter tree (encoder, decoder, quant_conv, post_quant_conv)."""

    def __init__(self, cfg):
        super().__init__()
        z = cfg["latent_channels"]
        self.encoder = _Encoder(cfg)
        self.decoder = _Decoder(cfg)
        self.quant_conv = nn.Conv2d(2 * z, 2 * z, 1)
        self.post_quant_conv = nn.Conv2d(z, z, 1)


def synth_vae_tensor(seed: int, key: str, shape) -> torch.Tensor:
    """`weights.synth_tensor` under the diffusers key; GroupNorm scales are moved to 1 +- 0.1 (diffusers' norm names carry no `.norm.`,
    so synth_tensor draws them as biases, +-0.05: a network of near-zero GroupNorm gains)."""
    t = synth_tensor(seed, key, tuple(shape))
    leaf = key.rsplit(".", 2)
    if len(shape) == 1 and leaf[-1] == "weight" and leaf[-2] in ("norm1", "norm2", "group_norm", "conv_norm_out"):
        t = 1.0 + 2.0 * t
    return t


def convert_state_dict(sd: dict) -> dict:
    """Newer diffusers spellings of the mid-block attention (to_q / to_k / to_v / to_out.0) onto the 0.14 names; [C, C, 1, 1] -> [C, C]."""
    out = {}
    for k, v in sd.items():
        if ".attentions." in k:
            for new, old in _NEW_ATTN_NAMES.items():
                k = k.replace(".attentions.0." + new, ".attentions.0." + old)
            if v.dim() == 4 and v.shape[2:] == (1, 1):
                v = v[:, :, 0, 0]
        out[k] = v
    return out


class VAE_StableDiffusion(HandleCache, nn.Module):
    _cache_versioned_tensors = False     # (the parameters of `encoder` are walked at every call)

    def __init__(self, pretrained_path, latent_dim=4, name="vae", using_KL=False, compute_dtype="f32", config: Optional[dict] = None,
                 max_workspace_bytes: int = 4 << 30, **kwargs):
        super().__init__()
        if pretrained_path is not None:
            with open(os.path.join(pretrained_path, "config.json")) as f:
                config = json.load(f)
        elif config is None:
            raise ValueError("VAE_StableDiffusion: pass pretrained_path, or pretrained_path=None with config={...}")
        self.config = check_config(config)
        self.compute_dtype = compute_dtype
        self.max_workspace_bytes = int(max_workspace_bytes)
        self.encoder = AutoencoderKLParams(self.config)
        if pretrained_path is not None:
            sd = torch.load(os.path.join(pretrained_path, "diffusion_pytorch_model.bin"), map_location="cpu")
            self.encoder.load_state_dict(convert_state_dict(sd), strict=True)
        self.latent_dim = latent_dim
        self.name = name
        self.using_KL = using_KL
        self.encode_mode = None if using_KL else "mode"
        self.eval()
        self._init_handle_cache()

    @torch.no_grad()
    def synth_init_(self, seed: int):
        """Every parameter from `synth_vae_tensor(seed, diffusers key, shape)`."""
        for k, v in self.encoder.state_dict().items():
            v.copy_(synth_vae_tensor(seed, k, tuple(v.shape)))
        self.invalidate()
        return self

    def _versioned_tensors(self):
        return self.encoder.parameters()

    def _handle_key_extra(self):
        return (self.max_workspace_bytes,)

    def _make_handle(self, device):
        sd = {k: v.to(device) for k, v in self.encoder.state_dict().items()}
        return hip.VaeHandle(self.config, sd, hip.dtype_code(self.compute_dtype), max_workspace_bytes=self.max_workspace_bytes)

    @torch.no_grad()
    def encode_image(self, image, mode=None):
        """AutoencoderKL.py:28-41: the mode of the latent distribution x 0.18215, (B, latent_channels, H/8, W/8) f32, on the device."""
        mode = self.encode_mode if mode is None else mode
        if mode is None:
            raise NotImplementedError("VAE_StableDiffusion.encode_image with using_KL=True and mode=None (the DiagonalGaussianDistribution of KL training)")
        if mode != "mode":
            raise NotImplementedError(f"encode_image mode {mode!r}")
        hip.require_device(image)
        return self._get_handle(image.device).encode(image)

    @torch.no_grad()
    def decode_latent(self, latent, unnormalize: bool = False, out: Optional[torch.Tensor] = None):
        """AutoencoderKL.py:43-47: Decoder(post_quant_conv(latent / 0.18215)), (B, 3, 8h, 8w) f32, on the device, in chunks of at most
        max_workspace_bytes of workspace.  unnormalize: (x + 1) / 2 (unnormalize_to_zero_to_one) in the output conv."""
        hip.require_device(latent)
        return self._get_handle(latent.device).decode(latent, unnormalize=unnormalize, out=out)
