"""`UNetModelPose` -- drop-in for the reference's LDM cross-attention U-Net variant
(src/model/u_net/ldm/adapt_openaimodel.py:14-158 over ldm/openaimodel.py:428-760 and ldm/attention.py:149-277), the
variant whose pose conditioning is cross-attention against `context = pose_mlp(pose).unsqueeze(1)`; executed by
libnope_hip.so (`nope_ldm_*`, csrc/ldm_runtime.hip).

Same constructor arguments as the reference class (the ones configs/model/vae_cin_ldm.yaml passes), same attributes
(`encoder`, `channels`, `name`), same `state_dict()` keys and shapes -- an LDM checkpoint loads with `load_state_dict`
-- and the same call `u_net(x, pose) -> pred`, so it plugs into `nope_amd.PoseConditional` exactly as `nope_amd.UNet` does
(`forward_hypotheses` is the batched form `generate_templates` uses).  The module tree only holds parameters.

Supported configuration: `use_spatial_transformer=True` with any `transformer_depth`; attention heads set by
`num_head_channels` or `num_heads` (and `legacy`) exactly as the reference derives them per level (openaimodel.py:560-580,
622-630, 666-690), as long as every level's head width is 32, 64 or 128 channels and divides the level's channels (else the
reference's `inner_dim = heads * dim_head` differs from the channels); `conv_resample` and `resblock_updown` on or off;
`use_scale_shift_norm` (FiLM ResBlocks) on or off; `pose_mlp_name` "single_layer" / "two_layers";
`injecting_condition_twice` on or off.  `num_heads_upsample` and `use_new_attention_order` only reach the reference's
`AttentionBlock`, which the spatial transformer replaces: accepted and ignored, as there.  Anything else raises
NotImplementedError -- among it `use_spatial_transformer=False`, which the reference class cannot be built with either
(openaimodel.py:491-495 asserts it whenever `context_dim` is set, and `pose_mlp` needs `context_dim`).
"""
from __future__ import annotations

from torch import nn

from . import hip
from .handle_cache import HypothesisNetwork
from .u_net import _Params, _slot


def _res_params(cin, cout, emb_dim, film=False):
    m = _Params()
    m.in_layers = _slot(nn.GroupNorm(32, cin), None, nn.Conv2d(cin, cout, 3, padding=1))            # openaimodel.py:214-218
    m.emb_layers = _slot(None, nn.Linear(emb_dim, 2 * cout if film else cout))                        # :233-239 (FiLM: scale | shift)
    m.out_layers = _slot(nn.GroupNorm(32, cout), None, None, nn.Conv2d(cout, cout, 3, padding=1))     # :248-255
    if cin != cout:
        m.skip_connection = nn.Conv2d(cin, cout, 1)                                                   # :257-264
    return m


def _cross_attention_params(query_dim, context_dim):
    m = _Params()                                                                                     # attention.py:149-166
    m.to_q = nn.Linear(query_dim, query_dim, bias=False)
    m.to_k = nn.Linear(context_dim, query_dim, bias=False)
    m.to_v = nn.Linear(context_dim, query_dim, bias=False)
    m.to_out = _slot(nn.Linear(query_dim, query_dim), None)
    return m


def _transformer_params(ch, context_dim, depth=1):
    def block():
        blk = _Params()                                                                               # attention.py:192-212
        blk.attn1 = _cross_attention_params(ch, ch)
        ff = _Params()
        geglu = _Params()
        geglu.proj = nn.Linear(ch, 8 * ch)                                                            # GEGLU(dim, 4*dim): proj to 2 x inner
        ff.net = _slot(geglu, None, nn.Linear(4 * ch, ch))
        blk.ff = ff
        blk.attn2 = _cross_attention_params(ch, context_dim)
        blk.norm1, blk.norm2, blk.norm3 = nn.LayerNorm(ch), nn.LayerNorm(ch), nn.LayerNorm(ch)
        return blk
    m = _Params()                                                                                     # attention.py:232-262
    m.norm = nn.GroupNorm(32, ch, eps=1e-6)
    m.proj_in = nn.Conv2d(ch, ch, 1)
    m.transformer_blocks = nn.ModuleList([block() for _ in range(depth)])
    m.proj_out = nn.Conv2d(ch, ch, 1)
    return m


def level_head_channels(ch, num_heads, num_head_channels, legacy):
    """The attention head width of a level with `ch` channels, as openaimodel.py:566-576 derives it under use_spatial_transformer;
    NotImplementedError unless it is 32, 64 or 128 and heads * width = ch (attention.py:152: inner_dim = heads * dim_head)."""
    if num_head_channels == -1:
        if num_heads == -1:
            raise ValueError("either num_heads or num_head_channels has to be set")
        heads, dim_head = num_heads, ch // num_heads
    else:
        heads, dim_head = ch // num_head_channels, num_head_channels
    if legacy:
        if heads < 1:
            raise NotImplementedError(f"num_head_channels={num_head_channels} > {ch} channels: no attention head")
        dim_head = ch // heads
    if dim_head not in (32, 64, 128) or heads * dim_head != ch:
        raise NotImplementedError(f"{ch} channels as {heads} attention heads of {dim_head}: head widths 32 / 64 / 128 dividing the channels only")
    return dim_head


class UNetModelPose(HypothesisNetwork, nn.Module):
    """adapt_openaimodel.py:14-158; `forward(x, pose)` is adapt_openaimodel.py:130-158 (-> (B,out_channels,h,w) f32), `forward_hypotheses`
    the template loop model.py:212-222 (both, the device handle behind them and `invalidate()` in handle_cache.HypothesisNetwork)."""

    def __init__(self, injecting_condition_twice, pose_mlp_name, rot_representation_dim, encoder, image_size, in_channels,
                 model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0, channel_mult=(1, 2, 4, 8),
                 conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None,
                 n_embed=None, legacy=True, compute_dtype="f32", **kwargs):
        super().__init__()
        if not use_spatial_transformer or transformer_depth < 1 or context_dim is None:
            raise NotImplementedError("only use_spatial_transformer=True (configs/model/vae_cin_ldm.yaml), transformer_depth >= 1")
        self.transformer_depth = int(transformer_depth)
        if dims != 2 or num_classes is not None or n_embed is not None:
            raise NotImplementedError("unsupported UNetModel option (see module docstring)")
        if pose_mlp_name not in ("single_layer", "two_layers"):
            raise NotImplementedError(f"pose_mlp_name={pose_mlp_name!r}")
        self.encoder = encoder
        self.channels = encoder.latent_dim
        self.name = encoder.name
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.channel_mult = num_res_blocks, tuple(channel_mult)
        self.attention_resolutions = tuple(attention_resolutions)
        self.context_dim, self.rot_representation_dim = context_dim, rot_representation_dim
        self.injecting_condition_twice = bool(injecting_condition_twice)
        self.use_scale_shift_norm = film = bool(use_scale_shift_norm)
        self.compute_dtype = compute_dtype
        self.resblock_updown, self.conv_resample = bool(resblock_updown), bool(conv_resample)
        # per level (the middle block: the last level's); num_heads_upsample only reaches AttentionBlock (not built here, nor there)
        # (levels without attention: no width -- 32 is a placeholder the library does not read)
        last = len(self.channel_mult) - 1
        self.head_channels = tuple(level_head_channels(mult * model_channels, num_heads, num_head_channels, legacy)
                                   if (1 << l) in self.attention_resolutions or l == last else 32 for l, mult in enumerate(self.channel_mult))
        emb = model_channels * 4
        self.time_embed_dim = emb
        self.time_embed = _slot(nn.Linear(model_channels, emb), None, nn.Linear(emb, emb))           # present, never evaluated (timesteps skipped)
        self.input_blocks = nn.ModuleList([_slot(nn.Conv2d(in_channels, model_channels, 3, padding=1))])
        chans, ch, ds = [model_channels], model_channels, 1
        for level, mult in enumerate(self.channel_mult):                                              # openaimodel.py:523-612
            for _ in range(num_res_blocks):
                layers = [_res_params(ch, mult * model_channels, emb, film)]
                ch = mult * model_channels
                if ds in self.attention_resolutions:
                    layers.append(_transformer_params(ch, context_dim, transformer_depth))
                self.input_blocks.append(_slot(*layers))
                chans.append(ch)
            if level != len(self.channel_mult) - 1:
                down = _Params()                                                                      # :597-609 (Downsample :143-174)
                if self.resblock_updown:
                    down = _res_params(ch, ch, emb, film)
                elif self.conv_resample:
                    down.op = nn.Conv2d(ch, ch, 3, stride=2, padding=1)
                self.input_blocks.append(_slot(down))
                chans.append(ch)
                ds *= 2
        self.middle_block = _slot(_res_params(ch, ch, emb, film), _transformer_params(ch, context_dim, transformer_depth), _res_params(ch, ch, emb, film))
        self.output_blocks = nn.ModuleList()
        for level, mult in list(enumerate(self.channel_mult))[::-1]:                                  # :651-731
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [_res_params(ch + ich, model_channels * mult, emb, film)]
                ch = model_channels * mult
                if ds in self.attention_resolutions:
                    layers.append(_transformer_params(ch, context_dim, transformer_depth))
                if level and i == num_res_blocks:
                    up = _Params()                                                                    # :711-727 (Upsample :94-124)
                    if self.resblock_updown:
                        up = _res_params(ch, ch, emb, film)
                    elif self.conv_resample:
                        up.conv = nn.Conv2d(ch, ch, 3, padding=1)
                    layers.append(up)
                    ds //= 2
                self.output_blocks.append(_slot(*layers))
        self.out = _slot(nn.GroupNorm(32, ch), None, nn.Conv2d(model_channels, out_channels, 3, padding=1))
        if pose_mlp_name == "single_layer":                                                            # adapt_openaimodel.py:105-116
            self.pose_mlp = _slot(nn.Linear(rot_representation_dim, context_dim))
            self._pose_layers = 1
        else:
            self.pose_mlp = _slot(nn.Linear(rot_representation_dim, context_dim), None, nn.Linear(context_dim, context_dim))
            self._pose_layers = 2
        if self.injecting_condition_twice:                                                             # :119-123
            self.pose_mlp_timesteps = _slot(nn.Linear(rot_representation_dim, emb))
        self._init_handle_cache()

    def _make_handle(self, device):
        sd = {k: v.to(device) for k, v in self.own_state_dict().items() if not k.startswith("time_embed.")}
        levels = len(self.channel_mult)
        cfg = dict(in_channels=self.in_channels, model_channels=self.model_channels, out_channels=self.out_channels,
                   num_res_blocks=self.num_res_blocks, channel_mult=self.channel_mult,
                   attn_levels=tuple(int((1 << l) in self.attention_resolutions) for l in range(levels)),
                   num_head_channels=0, head_channels=self.head_channels, resblock_updown=int(self.resblock_updown),
                   conv_resample=int(self.conv_resample), context_dim=self.context_dim, pose_dim=self.rot_representation_dim,
                   pose_mlp_layers=self._pose_layers, injecting_condition_twice=int(self.injecting_condition_twice),
                   use_scale_shift_norm=int(self.use_scale_shift_norm), transformer_depth=self.transformer_depth)
        return hip.LdmHandle(cfg, sd, hip.dtype_code(self.compute_dtype))
