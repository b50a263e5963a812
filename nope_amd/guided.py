"""`UNetModelPose` -- drop-in for the reference's guided-diffusion U-Net variant
(src/model/u_net/guided_diffusion/adapt_u_net.py:13-97 over guided_diffusion/u_net.py:141-253 ResBlock, :255-300 AttentionBlock,
:323-386 QKVAttentionLegacy / QKVAttention, :389- UNetModel and nn.py), the variant whose pose conditioning is `emb = pose_mlp(pose)`
used as the timestep embedding; executed by libnope_hip.so (`nope_gd_*`, csrc/gd_runtime.hip).

One correction to the reference: its forward calls `module(h, emb, emb)` (adapt_u_net.py:90,92,95), but
`TimestepEmbedSequential.forward(self, x, emb)` (u_net.py:72) takes two arguments, so every forward of the reference raises
TypeError.  The only reading that type-checks is `module(h, emb)`: emb = pose_mlp(pose) (width 4 * model_channels) drives every
ResBlock's emb_layers (SiLU -> Linear), added to h or, with use_scale_shift_norm, as out_norm(h) * (1 + scale) + shift.  That is what
runs here.  GroupNorm(32, eps 1e-5) in f32, dropout the identity (eval); `use_checkpoint` and `use_fp16` are accepted and ignored (the
reference never calls convert_to_fp16: it computes in f32).

Same constructor arguments as the reference class (the ones configs/model/vae_guidedDiffusion.yaml passes), same attributes (`encoder`,
`channels`, `name`), same `state_dict()` keys and shapes (conv1d `qkv.weight` [3C, C, 1] and `proj_out.weight` [C, C, 1]; `time_embed.*`
is present and never evaluated, as there) and the same call `u_net(x, pose) -> pred`, so it plugs into `nope_amd.PoseConditional` as
`nope_amd.ldm.UNetModelPose` does (`forward_hypotheses` is the batched form `generate_templates` uses).  The module tree only holds
parameters.

Supported configuration: `dims=2`, `num_classes=None`; `pose_mlp_name` "single_layer", "two_layers" (GELU, exact erf) and
"posEncoding" where the reference can build it (4 * model_channels divisible by 6 -- else the reference's warning branch raises
NameError -- and rot_representation_dim = 6); attention heads from `num_head_channels`, or `num_heads` on the input / middle side and
`num_heads_upsample` on the output side (u_net.py:444-445, 580), as long as every AttentionBlock's heads are 32, 64 or 128 channels wide
and divide its channels; `use_new_attention_order`, `resblock_updown`, `conv_resample` and `use_scale_shift_norm` on or off; a latent
whose H and W are multiples of 2^(levels-1).  Anything else raises NotImplementedError naming the option.
"""
from __future__ import annotations

from torch import nn

from . import hip
from .handle_cache import HypothesisNetwork
from .u_net import _Params, _slot

POSE_MLP = {"single_layer": 1, "two_layers": 2, "posEncoding": 3}          # NOPE_GD_POSE_*


def _res_params(cin, cout, emb_dim, film=False):
    m = _Params()
    m.in_layers = _slot(nn.GroupNorm(32, cin), None, nn.Conv2d(cin, cout, 3, padding=1))            # u_net.py:179-183
    m.emb_layers = _slot(None, nn.Linear(emb_dim, 2 * cout if film else cout))                        # :196-202 (FiLM: scale | shift)
    m.out_layers = _slot(nn.GroupNorm(32, cout), None, None, nn.Conv2d(cout, cout, 3, padding=1))     # :203-210
    if cin != cout:
        m.skip_connection = nn.Conv2d(cin, cout, 1)                                                   # :212-219
    return m


def _attention_params(ch):
    m = _Params()                                                                                     # u_net.py:262-289
    m.norm = nn.GroupNorm(32, ch)
    m.qkv = nn.Conv1d(ch, 3 * ch, 1)
    m.proj_out = nn.Conv1d(ch, ch, 1)
    return m


def head_channels(ch, num_heads, num_head_channels):
    """Head width of an AttentionBlock of `ch` channels, as u_net.py:270-278 derives it; NotImplementedError unless it is 32, 64 or 128
    and the heads divide the channels."""
    if num_head_channels == -1:
        if num_heads < 1 or ch % num_heads:
            raise NotImplementedError(f"num_heads={num_heads} at {ch} channels: the heads must divide the channels")
        heads, dh = num_heads, ch // num_heads
    else:
        if num_head_channels < 1 or ch % num_head_channels:
            raise NotImplementedError(f"num_head_channels={num_head_channels} does not divide {ch} channels")
        heads, dh = ch // num_head_channels, num_head_channels
    if dh not in (32, 64, 128):
        raise NotImplementedError(f"{ch} channels as {heads} attention heads of {dh}: head widths 32 / 64 / 128 only "
                                  "(num_heads / num_head_channels / num_heads_upsample)")
    return dh


class UNetModelPose(HypothesisNetwork, nn.Module):
    """adapt_u_net.py:13-97; `forward(x, pose)` is adapt_u_net.py:78-97 with module(h, emb) (-> (B,out_channels,h,w) f32),
    `forward_hypotheses` the template loop model.py:212-222 (both, the device handle behind them and `invalidate()` in
    handle_cache.HypothesisNetwork)."""

    def __init__(self, pose_mlp_name, rot_representation_dim, encoder, image_size, in_channels, model_channels, out_channels,
                 num_res_blocks, attention_resolutions, dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2,
                 num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False, compute_dtype="f32", **kwargs):
        super().__init__()
        if dims != 2:
            raise NotImplementedError(f"dims={dims}: 2-d only")
        if num_classes is not None:
            raise NotImplementedError(f"num_classes={num_classes}: no class conditioning (label_emb)")
        if pose_mlp_name not in POSE_MLP:
            raise NotImplementedError(f"pose_mlp_name={pose_mlp_name!r}")
        emb = model_channels * 4
        if model_channels % 32:
            raise NotImplementedError(f"model_channels={model_channels}: GroupNorm(32) needs a multiple of 32")
        if pose_mlp_name == "posEncoding" and (emb % 6 or rot_representation_dim != 6):
            # (emb % 6: the reference's warning branch calls an unimported `logging` -- NameError at construction)
            raise NotImplementedError(f"pose_mlp_name='posEncoding' with model_channels={model_channels}, rot_representation_dim="
                                      f"{rot_representation_dim}: the reference builds it only for 4 * model_channels % 6 == 0 and 6-d poses")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        self.encoder = encoder
        self.channels = encoder.latent_dim
        self.name = encoder.name
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.channel_mult = num_res_blocks, tuple(int(m) for m in channel_mult)
        self.attention_resolutions = tuple(attention_resolutions)
        self.rot_representation_dim, self.pose_mlp_name = rot_representation_dim, pose_mlp_name
        self.use_scale_shift_norm = film = bool(use_scale_shift_norm)
        self.resblock_updown, self.conv_resample = bool(resblock_updown), bool(conv_resample)
        self.use_new_attention_order = bool(use_new_attention_order)
        self.compute_dtype = compute_dtype
        levels = len(self.channel_mult)
        attn = tuple(int((1 << l) in self.attention_resolutions) for l in range(levels))
        self.attn_levels = attn
        # per level (levels without attention: 32, a placeholder the library does not read)
        self.head_channels_in = tuple(head_channels(m * model_channels, num_heads, num_head_channels) if a else 32
                                      for m, a in zip(self.channel_mult, attn))
        self.head_channels_out = tuple(head_channels(m * model_channels, num_heads_upsample, num_head_channels) if a else 32
                                       for m, a in zip(self.channel_mult, attn))
        self.head_channels_mid = head_channels(self.channel_mult[-1] * model_channels, num_heads, num_head_channels)
        self.time_embed_dim = emb
        self.time_embed = _slot(nn.Linear(model_channels, emb), None, nn.Linear(emb, emb))           # present, never evaluated
        ch = input_ch = self.channel_mult[0] * model_channels
        self.input_blocks = nn.ModuleList([_slot(nn.Conv2d(in_channels, ch, 3, padding=1))])
        chans, ds = [ch], 1
        for level, mult in enumerate(self.channel_mult):                                              # u_net.py:480-530
            for _ in range(num_res_blocks):
                layers = [_res_params(ch, mult * model_channels, emb, film)]
                ch = mult * model_channels
                if ds in self.attention_resolutions:
                    layers.append(_attention_params(ch))
                self.input_blocks.append(_slot(*layers))
                chans.append(ch)
            if level != levels - 1:
                down = _Params()                                                                      # Downsample :112-138
                if self.resblock_updown:
                    down = _res_params(ch, ch, emb, film)
                elif self.conv_resample:
                    down.op = nn.Conv2d(ch, ch, 3, stride=2, padding=1)
                self.input_blocks.append(_slot(down))
                chans.append(ch)
                ds *= 2
        self.middle_block = _slot(_res_params(ch, ch, emb, film), _attention_params(ch), _res_params(ch, ch, emb, film))
        self.output_blocks = nn.ModuleList()
        for level, mult in list(enumerate(self.channel_mult))[::-1]:                                  # :560-603
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [_res_params(ch + ich, model_channels * mult, emb, film)]
                ch = model_channels * mult
                if ds in self.attention_resolutions:
                    layers.append(_attention_params(ch))
                if level and i == num_res_blocks:
                    up = _Params()                                                                    # Upsample :81-109
                    if self.resblock_updown:
                        up = _res_params(ch, ch, emb, film)
                    elif self.conv_resample:
                        up.conv = nn.Conv2d(ch, ch, 3, padding=1)
                    layers.append(up)
                    ds //= 2
                self.output_blocks.append(_slot(*layers))
        self.out = _slot(nn.GroupNorm(32, ch), None, nn.Conv2d(input_ch, out_channels, 3, padding=1))
        if pose_mlp_name == "single_layer":                                                            # adapt_u_net.py:62-78
            self.pose_mlp = _slot(nn.Linear(rot_representation_dim, emb))
        elif pose_mlp_name == "two_layers":
            self.pose_mlp = _slot(nn.Linear(rot_representation_dim, emb), None, nn.Linear(emb, emb))
        self._init_handle_cache()

    def _make_handle(self, device):
        sd = {k: v.to(device) for k, v in self.own_state_dict().items() if not k.startswith("time_embed.")}
        cfg = dict(in_channels=self.in_channels, model_channels=self.model_channels, out_channels=self.out_channels,
                   num_res_blocks=self.num_res_blocks, channel_mult=self.channel_mult, attn_levels=self.attn_levels,
                   head_channels_in=self.head_channels_in, head_channels_out=self.head_channels_out,
                   head_channels_mid=self.head_channels_mid, pose_dim=self.rot_representation_dim, pose_mlp=POSE_MLP[self.pose_mlp_name],
                   new_attention_order=int(self.use_new_attention_order), resblock_updown=int(self.resblock_updown),
                   conv_resample=int(self.conv_resample), use_scale_shift_norm=int(self.use_scale_shift_norm))
        return hip.GdHandle(cfg, sd, hip.dtype_code(self.compute_dtype))
