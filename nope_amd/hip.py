"""ctypes binding of libnope_hip.so (include/nope_hip.h) for torch tensors.

PyTorch is plumbing here: it owns device memory and the stream; every computation below is
a hand-written gfx950 kernel behind the C ABI.  There is NO fallback: if the library is
missing (not built) the import of anything that computes fails with a clear error.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

F32, BF16, F16, BF16X3 = 0, 1, 2, 3      # BF16X3: compute mode only (f32 storage, three bf16 MFMA passes per product)
F16X2 = 4                                # compute mode only: BF16X3, but the ping-pong launches (tap-resident 3x3, per-tap 1x1 / up / down) run one f16 + one MX-fp8 MFMA pass (include/nope_hip.h)
ABI_VERSION = 25                         # NOPE_ABI_VERSION of include/nope_hip.h these ctypes structs mirror
CONV_PLAIN, CONV_UP2, CONV_DOWN2, CONV_UP2P, CONV_STRIDE2, CONV_STRIDE2_PAD01 = 0, 1, 2, 3, 4, 5
ERR_RANGE, ERR_RANGE_F16 = -7, -8        # nope_unet_x2_range_check (include/nope_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NOPE_HIP_LIB: load another build of the SAME gfx950 library (A/B timing of kernel variants); default = in-tree build
LIB_PATH = os.environ.get("NOPE_HIP_LIB") or os.path.join(_HERE, "csrc", "libnope_hip.so")

_vp, _i, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", _vp), ("ndim", _i), ("shape", _i64 * 4)]


class UNetConfig(C.Structure):
    _fields_ = [("u_net_dim", _i), ("channels", _i), ("out_dim", _i), ("pose_dim", _i), ("n_levels", _i),
                ("dim_mults", _i * 8), ("groups", _i), ("heads", _i), ("dim_head", _i), ("pose_mlp_layers", _i),
                ("compute_dtype", _i), ("soft_up_down", _i)]


class LdmConfig(C.Structure):
    _fields_ = [("in_channels", _i), ("model_channels", _i), ("out_channels", _i), ("num_res_blocks", _i), ("n_levels", _i),
                ("channel_mult", _i * 8), ("attn_levels", _i * 8), ("num_head_channels", _i), ("context_dim", _i), ("pose_dim", _i),
                ("pose_mlp_layers", _i), ("injecting_condition_twice", _i), ("compute_dtype", _i), ("use_scale_shift_norm", _i),
                ("transformer_depth", _i), ("head_channels", _i * 8), ("resblock_updown", _i), ("conv_resample", _i)]


class GdConfig(C.Structure):
    _fields_ = [("in_channels", _i), ("model_channels", _i), ("out_channels", _i), ("num_res_blocks", _i), ("n_levels", _i),
                ("channel_mult", _i * 8), ("attn_levels", _i * 8), ("head_channels_in", _i * 8), ("head_channels_out", _i * 8),
                ("head_channels_mid", _i), ("pose_dim", _i), ("pose_mlp", _i), ("new_attention_order", _i), ("resblock_updown", _i),
                ("conv_resample", _i), ("use_scale_shift_norm", _i), ("compute_dtype", _i)]


class VaeConfig(C.Structure):
    _fields_ = [("in_channels", _i), ("out_channels", _i), ("n_levels", _i), ("block_out_channels", _i * 8), ("layers_per_block", _i),
                ("latent_channels", _i), ("norm_num_groups", _i), ("compute_dtype", _i), ("gn_eps", C.c_float)]


class ConvLaunchInfo(C.Structure):
    _fields_ = [("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double), ("kernel", _i), ("mode", _i), ("ntaps", _i), ("Cin", _i),
                ("Cout", _i), ("Hs", _i), ("Ws", _i), ("n_hyp", _i), ("mfma_passes", _i), ("posmajor", _i)]


CONV_KERNEL_NAMES = ("conv_gemm_kernel", "conv_gemm_dma_kernel", "conv_gemm_pp_kernel", "conv3x3_halo_kernel", "conv_gemm_small_kernel", "conv1x1_stream_kernel")


class EncoderConfig(C.Structure):
    _fields_ = [("descriptor_size", _i), ("compute_dtype", _i), ("bn_eps", C.c_float)]


class VisColumn(C.Structure):
    """nope_vis_column: one column of a picture, a stack of f32 NCHW images read in place."""
    _fields_ = [("data", _vp), ("stride_b", _i64), ("stride_f", _i64), ("index", _vp), ("index_stride", _i64), ("index_limit", _i64), ("flags", _i)]


VIS_UNNORMALIZE, VIS_CLAMP, VIS_MAX_COLS = 1, 2, 8


# The arguments of the conv / GroupNorm operator entries, by name.  tests/test_host_logic.py holds the field names to the header's, in order;
# the entries refuse a struct_size that is not their sizeof.
class ConvOp(C.Structure):
    """nope_conv_op"""
    _fields_ = [("struct_size", C.c_uint32), ("dtype", _i), ("src1", _vp), ("C1", _i), ("rep1", _i), ("src2", _vp), ("C2", _i), ("rep2", _i),
                ("Hs", _i), ("Ws", _i), ("mode", _i), ("ntaps", _i), ("w_packed", _vp), ("bias", _vp), ("resid", _vp), ("out", _vp),
                ("Cout", _i), ("n_hyp", _i), ("out_nchw", _i), ("out_dtype", _i), ("act_relu", _i), ("splitk_ws", _vp), ("splitk_bytes", _sz),
                ("colstats", _vp), ("stat_rows", _i), ("pn_ms", _vp), ("pn_c0", _vp), ("pn_c1", _vp),
                ("tail_colstats", _vp), ("tail_stat_blocks", _i), ("gn_gamma", _vp), ("gn_beta", _vp), ("gn_G", _i), ("gn_eps", C.c_float),
                ("gn_ms", _vp), ("tail_stats", _vp), ("amax_slot", _vp), ("amax_out", _vp),
                ("gn_emb", _vp), ("gn_emb_stride", _i), ("gn_self", _i), ("gn_resid_rep", _i)]


class ConvOpInfo(C.Structure):
    """nope_conv_op_info"""
    _fields_ = [("splitk_bytes", _sz), ("stat_rows", _i), ("tail_stat_blocks", _i), ("records_out_amax", _i), ("err", _i)]


class GnOp(C.Structure):
    """nope_gn_op"""
    _fields_ = [("struct_size", C.c_uint32), ("dtype", _i), ("x", _vp), ("y", _vp), ("partial", _vp), ("colstats", _vp), ("stat_blocks", _i),
                ("fold_launch", _i), ("gamma", _vp), ("beta", _vp), ("n_hyp", _i), ("H", _i), ("W", _i), ("C", _i), ("G", _i), ("act_silu", _i),
                ("emb", _vp), ("emb_stride", _i), ("film", _vp), ("film_stride", _i), ("resid", _vp), ("x_rep", _i), ("resid_rep", _i),
                ("out_stats", _vp), ("eps", C.c_float), ("fast_silu", _i), ("sh_s", _vp), ("sh_rep", _i), ("sh_e", _vp), ("amax_slot", _vp),
                ("amax_out", _vp)]


_PROTOS = {
    "nope_strerror": (C.c_char_p, [_i]),
    "nope_abi_version": (_i, []),
    "nope_tuning_reload": (None, []),
    "nope_similarity": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i64, _i, _vp]),
    "nope_topk": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_gather_topk": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp]),
    "nope_topk_merge": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "nope_op_geodesic": (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "nope_op_pose_modes": (_i, [_vp, _i64, _vp, _i64, _i, _vp, C.c_double, C.c_double, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "nope_op_c2f_expand": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, C.c_double, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "nope_op_c2f_commit": (_i, [_vp, _vp, _i, _i, _vp, _i64, _i, _vp]),
    "nope_op_multiref_prepare": (_i, [_vp, _i64, _i, _vp, _i, _vp, _i, C.c_double, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "nope_multiref_similarity": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "nope_op_multiref_fuse_scores": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp]),
    "nope_op_multiref_select": (_i, [_vp, _i64, _i, _vp, _i, _vp, _vp, _i, _i, _i, C.c_double, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "nope_op_multiref_gather": (_i, [_vp, _vp, _vp, _i, _i, _i, _i64, _vp]),
    "nope_robust_similarity": (_i, [_vp, _vp, _i, _vp, C.c_float, _vp, _i, _i, _i, _i, _i, _i64, _i, _vp]),
    "nope_op_residual_maps": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i64, _vp]),
    "nope_op_pool_mask": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i64, C.c_float, _vp, _vp]),
    "nope_op_refine_init": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, _vp]),
    "nope_op_refine_normal_eq_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "nope_op_refine_normal_eq": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, C.c_double, _vp, _sz, _vp]),
    "nope_op_refine_step": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, C.c_double, _vp]),
    "nope_op_refine_select": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "nope_op_render_depth_workspace_bytes": (_sz, [_i, _i]),
    "nope_op_render_depth": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "nope_op_vsd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "nope_op_vsd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, C.c_double, C.c_double, _i, _i, _vp, _vp, _sz, _vp]),
    "nope_op_pose_errors_workspace_bytes": (_sz, [_i, _i, _i]),
    "nope_op_pose_errors": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nope_op_mesh_diameter_workspace_bytes": (_sz, [_i, _i]),
    "nope_op_mesh_diameter": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "nope_op_fit_translation": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "nope_op_mask_boxes": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "nope_op_depth_shift_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "nope_op_depth_shift": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, C.c_double, _vp, _vp, _vp, _sz, _vp]),
    "nope_op_vis_grid": (_i, [C.POINTER(VisColumn), _i, _i, _i, _i, _i, _vp, _vp]),
    "nope_op_vis_sheet": (_i, [C.POINTER(VisColumn), _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "nope_unet_graph_limit": (_i, [_vp, C.c_longlong]),
    "nope_unet_graph_replays": (_i, [_vp]),
    "nope_unet_x2_shifts": (_i, [_vp, C.POINTER(_i), _i, C.POINTER(_i)]),
    "nope_unet_profile": (_i, [_vp, _i]),
    "nope_unet_profile_read": (_i, [_vp, C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nope_unet_profile_launches": (_i, [_vp, C.POINTER(ConvLaunchInfo), _i, C.POINTER(_i)]),
    "nope_op_nchw_to_nhwc": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
    "nope_op_nhwc_to_nchw": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
    "nope_op_pack_conv_weight": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_encoder_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "nope_op_conv": (_i, [C.POINTER(ConvOp), C.POINTER(_i), _vp]),
    "nope_op_conv_query": (_i, [C.POINTER(ConvOp), C.POINTER(ConvOpInfo)]),
    "nope_op_stem_conv": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "nope_op_gn_chunks": (_i, [_i, _i, _i]),
    "nope_op_group_norm": (_i, [C.POINTER(GnOp), _vp]),
    "nope_op_amax_slot_words": (_i, []),
    "nope_op_gn_apply_blocks": (_i, [_i, _i, _i, _i]),
    "nope_op_gn_finalize": (_i, [_vp, _vp, _i, _i, C.c_float, C.c_float, _vp]),
    "nope_op_conv_class_weights": (_i, [_vp, _vp, _i, _i, _vp]),
    "nope_op_absmax_f32": (_i, [_vp, _sz, _vp, _vp, _vp]),
    "nope_op_linear_attention": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_op_attention": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_op_linear": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_op_warp_perspective": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_float), _vp, _i, _i, C.c_float, C.c_float, _vp]),
    "nope_op_crop_frames": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, C.c_float, C.c_float, _i, _vp]),
    "nope_op_layer_norm": (_i, [_i, _vp, _vp, _vp, _vp, _i64, _i, C.c_float, _vp]),
    "nope_op_geglu": (_i, [_i, _vp, _vp, _i64, _i, _vp]),
    "nope_op_token_attention": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "nope_op_wide_attention": (_i, [_i, _vp, _vp, _i, _i, _i, _vp]),
    "nope_vae_encode": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "nope_vae_decode": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp]),
}
# the entries every network runtime exports under its own stem, nope_{stem}_{entry}; the hypothesis networks (forward(x, pose) with the
# NOPE_F16X2 range tracking) share their whole call surface
_NETWORKS = {"unet": (UNetConfig, 4, True), "ldm": (LdmConfig, 4, True), "gd": (GdConfig, 4, True),       # stem: (config struct, size arguments
             "encoder": (EncoderConfig, 3, False), "vae": (VaeConfig, 4, False)}                           #  of workspace_bytes, hypothesis network)
_X2_VERDICT = (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_float)])
for _stem, (_cfg, _nsize, _hyp) in _NETWORKS.items():
    _PROTOS[f"nope_{_stem}_create"] = (_i, [C.POINTER(_cfg), C.POINTER(TensorDesc), _i, _vp, C.POINTER(_vp)])
    _PROTOS[f"nope_{_stem}_destroy"] = (None, [_vp])
    _PROTOS[f"nope_{_stem}_workspace_bytes"] = (_sz, [_vp] + [_i] * _nsize)
    if _hyp:
        _PROTOS[f"nope_{_stem}_forward"] = (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp])
        _PROTOS[f"nope_{_stem}_x2_range_check"] = _PROTOS[f"nope_{_stem}_x2_poll"] = _X2_VERDICT
        _PROTOS[f"nope_{_stem}_x2_enable"] = (_i, [_vp, _i])
EXPORTED_SYMBOLS = tuple(_PROTOS)


class NopeError(RuntimeError):
    pass


class NopeLib:
    """A loaded C-ABI library with typed prototypes."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise NopeError(
                f"{path} not found: the gfx950 library is not built. Run `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (needs hipcc). nope_amd has no CPU fallback.")
        self.path = path
        self.dll = C.CDLL(path)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
        got = self.dll.nope_abi_version()
        if got != ABI_VERSION:     # a stale build would read the config structs below past their end
            raise NopeError(f"{path} has ABI version {got}, this binding was written for {ABI_VERSION}: rebuild the library")

    def check(self, code: int, what: str):
        if code != 0:
            raise NopeError(f"{what}: {self.dll.nope_strerror(code).decode()} ({code})")


_lib: Optional[NopeLib] = None
_tuning_seen: Optional[tuple] = None


def lib() -> NopeLib:
    """The loaded library.  Every binding comes through here, so this is also where a change of the NOPE_* tuning variables since the last call
    is noticed: the library caches them per call site (nope_tuning_reload, include/nope_hip.h)."""
    global _lib, _tuning_seen
    if _lib is None:
        _lib = NopeLib(LIB_PATH)
    cur = tuple(sorted(kv for kv in os.environ.items() if kv[0].startswith("NOPE_")))
    if cur != _tuning_seen:
        _tuning_seen = cur
        _lib.dll.nope_tuning_reload()
    return _lib


def _set_library_for_testing(l: Optional[NopeLib]):
    """tests/ only: lets the CPU test-suite run the same host code over tests/hipemu (a build of the same C ABI
    that takes host pointers)."""
    global _lib, _tuning_seen
    if l is not None:
        l.host_pointers = True
    _lib = l
    _tuning_seen = None


def require_device(t: torch.Tensor):
    """The product library takes device pointers only: a host tensor is an error, never a detour through torch CPU ops."""
    l = lib()      # (always: every binding starts here, and lib() is where a changed NOPE_* tuning variable is noticed)
    if not t.is_cuda and not getattr(l, "host_pointers", False):
        raise NopeError("nope_amd computes on the GPU only: pass CUDA (ROCm) tensors; there is no CPU path")


def compute_device() -> torch.device:
    """Where data that arrives from the host (decoded frames, maps) is put before a launch: the GPU -- or the host itself under the
    interpreter build of tests/, which takes host pointers."""
    return torch.device("cpu" if getattr(lib(), "host_pointers", False) else "cuda")


class overlap_stream:
    """`with overlap_stream(t) as ov: y = f(t)` issues f on a second HIP stream ordered after the current one;
    `ov.join(y)` makes the current stream wait for it.  (Host tensors -- the interpreter build of the tests -- have no
    streams: the body simply runs in place.)"""
    _streams: Dict[str, "torch.cuda.Stream"] = {}

    def __init__(self, t: torch.Tensor, wait_current: bool = True):
        """wait_current=False: the side work does NOT wait for what the current stream has queued -- the caller vouches that the inputs of the
        body are complete (PoseConditional.pipeline_encoders: the encoder passes of the next query may then run under the previous query's
        U-Net); the side stream itself stays in order."""
        self.dev = t.device if t.is_cuda else None
        self.wait_current = wait_current

    def __enter__(self):
        if self.dev is None:
            return self
        self.cur = torch.cuda.current_stream(self.dev)
        side = self._streams.get(str(self.dev))
        if side is None:
            side = self._streams[str(self.dev)] = torch.cuda.Stream(device=self.dev)
        self.side = side
        if self.wait_current:
            side.wait_stream(self.cur)              # whatever produced the inputs is ordered before the side work
        self._ctx = torch.cuda.stream(side)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.dev is not None:
            self._ctx.__exit__(*exc)
        return False

    def mark(self):
        """An event on the side stream at this point of the body (for join_at: the current stream then waits only for the work before it)."""
        return self.side.record_event() if self.dev is not None else None

    def join_at(self, event, *tensors):
        if self.dev is not None:
            self.cur.wait_event(event)
            for t in tensors:
                t.record_stream(self.cur)
                t.record_stream(self.side)

    def join(self, *tensors):
        if self.dev is not None:
            self.cur.wait_stream(self.side)
            for t in tensors:          # used on both streams, whichever of them it was allocated on
                t.record_stream(self.cur)
                t.record_stream(self.side)


def _stream(t: torch.Tensor) -> int:
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return 0


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def torch_dtype(dt: int) -> torch.dtype:
    """torch dtype of tensors STORED under dtype code dt (BF16X3 keeps f32 activations)."""
    return {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, BF16X3: torch.float32, F16X2: torch.float32}[dt]


def storage_code(dt: int) -> int:
    """dtype code the non-conv operators see for tensors of compute mode dt."""
    return F32 if dt in (BF16X3, F16X2) else dt


def dtype_code(dt) -> int:
    if dt in (F32, "f32", "fp32", "float32", torch.float32):
        return F32
    if dt in (BF16, "bf16", "bfloat16", torch.bfloat16):
        return BF16
    if dt in (F16, "f16", "fp16", "float16", "half", torch.float16):
        return F16
    if dt in (BF16X3, "bf16x3"):
        return BF16X3
    if dt in (F16X2, "f16x2"):
        return F16X2
    raise NopeError(f"unsupported dtype {dt!r}")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# --------------------------------------------------------------------------------------------
# scoring
# --------------------------------------------------------------------------------------------
def similarity(q: torch.Tensor, bank: torch.Tensor, out: Optional[torch.Tensor] = None,
               col_offset: int = 0) -> torch.Tensor:
    """score[b,n] of model.py:257-262.  q (B,C,H,W) f32; bank (B|1,N,C,H,W) f32|bf16|fp16.
    With `out` (B, Ntotal) given, writes columns [col_offset, col_offset+N)."""
    require_device(q)
    q = _f32c(q)
    B, Cc, H, W = q.shape
    if bank.dim() != 5 or tuple(bank.shape[2:]) != (Cc, H, W) or bank.shape[0] not in (1, B):
        raise NopeError(f"bank shape {tuple(bank.shape)} does not match query {tuple(q.shape)}")
    if bank.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        bank = bank.float()
    bank = bank.contiguous()
    N = bank.shape[1]
    if N == 0:
        return torch.empty((B, 0), dtype=torch.float32, device=q.device) if out is None else out
    stride_b = 0 if (bank.shape[0] == 1 and B > 1) else N * Cc * H * W
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=q.device)
        col_offset = 0
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B
    ld = out.shape[1]
    assert col_offset + N <= ld
    l = lib()
    l.check(l.dll.nope_similarity(_ptr(q), _ptr(bank), dtype_code(bank.dtype), out.data_ptr() + 4 * col_offset, B, N, Cc,
                                  H, W, stride_b, ld, _stream(q)), "nope_similarity")
    return out


def topk(scores: torch.Tensor, k: int = 5) -> Tuple[torch.Tensor, torch.Tensor]:
    require_device(scores)
    scores = _f32c(scores)
    B, N = scores.shape
    idx = torch.empty((B, k), dtype=torch.int64, device=scores.device)
    vals = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    l = lib()
    l.check(l.dll.nope_topk(_ptr(scores), _ptr(idx), _ptr(vals), B, N, k, N, _stream(scores)), "nope_topk")
    return vals, idx


def gather_topk(gathered: torch.Tensor, n_total: int, k: int = 5) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """gathered (G, B, nmax) f32 = the all-gathered padded score slices of a template-sharded step -> (similarity (B, n_total) owned,
    nearest_idx (B, k) or None for k = 0), one launch (nope_gather_topk)."""
    require_device(gathered)
    G, B, nmax = gathered.shape
    assert gathered.is_contiguous() and gathered.dtype == torch.float32 and nmax == (n_total + G - 1) // G
    sim = torch.empty((B, n_total), dtype=torch.float32, device=gathered.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=gathered.device) if k > 0 else None
    l = lib()
    l.check(l.dll.nope_gather_topk(_ptr(gathered), G, B, n_total, _ptr(sim), _ptr(idx), None, k, _stream(gathered)), "nope_gather_topk")
    return sim, idx


def topk_merge(cand_vals: torch.Tensor, cand_idx: torch.Tensor, k: int = 5) -> Tuple[torch.Tensor, torch.Tensor]:
    """cand_vals / cand_idx (B, M): per-shard top-k lists with global template indices, shards in rank order -> global (vals, idx) (B, k)."""
    require_device(cand_vals)
    cand_vals, cand_idx = _f32c(cand_vals), cand_idx.to(torch.int64).contiguous()
    B, M = cand_vals.shape
    idx = torch.empty((B, k), dtype=torch.int64, device=cand_vals.device)
    vals = torch.empty((B, k), dtype=torch.float32, device=cand_vals.device)
    l = lib()
    l.check(l.dll.nope_topk_merge(_ptr(cand_vals), _ptr(cand_idx), _ptr(idx), _ptr(vals), B, M, k, _stream(cand_vals)), "nope_topk_merge")
    return vals, idx


def op_geodesic(poses: torch.Tensor, gt: torch.Tensor, symmetry: Optional[torch.Tensor] = None,
                idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Geodesic error (radians, f64) of poses[b, idx[b, j]] (or poses[b, j] without `idx`) against gt[b], with the reference's
    symmetry handling (loss.py:14-75).  poses (B|1, N, 3, 3), gt (B, 3, 3), symmetry (B,) / (B, 1) in {0, 1, 2}, idx (B, k) int64.
    Raises ValueError where pytorch3d's so3_rotation_angle does (trace outside [-1 - eps, 3 + eps])."""
    require_device(poses)
    # everything follows the PREDICTIONS' device (a ground-truth pose / symmetry flag / index tensor left on the host is moved, not dereferenced)
    poses = poses.to(torch.float64).contiguous()
    gt = gt.to(device=poses.device, dtype=torch.float64).contiguous()
    B = gt.shape[0]
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 3) or poses.shape[0] not in (1, B) or tuple(gt.shape[1:]) != (3, 3):
        raise NopeError(f"poses {tuple(poses.shape)} / gt {tuple(gt.shape)}: expected (B|1, N, 3, 3) and (B, 3, 3)")
    N = poses.shape[1]
    if idx is not None:
        if idx.dim() != 2 or idx.shape[0] != B:
            raise NopeError(f"idx {tuple(idx.shape)}: expected ({B}, k)")
        idx = idx.to(device=gt.device, dtype=torch.int64).contiguous()
        k = idx.shape[1]
    else:
        k = N
    sym = None if symmetry is None else symmetry.reshape(-1).to(device=gt.device, dtype=torch.int32).contiguous()
    if sym is not None and sym.numel() != B:
        raise NopeError(f"symmetry has {sym.numel()} entries for {B} samples")
    err = torch.empty((B, k), dtype=torch.float64, device=gt.device)
    if B == 0 or k == 0:
        return err
    status = torch.empty(1, dtype=torch.int32, device=gt.device)
    stride_b = 0 if (poses.shape[0] == 1 and B > 1) else N * 9
    l = lib()
    l.check(l.dll.nope_op_geodesic(_ptr(poses), stride_b, N, _ptr(idx), _ptr(gt), _ptr(sym), _ptr(err), _ptr(status), B, k, _stream(gt)),
            "nope_op_geodesic")
    st = int(status.item())
    if st & 2:
        raise NopeError("nope_op_geodesic: an index lies outside the pose grid")
    if st & 1:
        raise ValueError("A matrix has trace outside valid range [-1-eps,3+eps].")      # pytorch3d so3_rotation_angle's message
    return err


class PoseModes(NamedTuple):
    """op_pose_modes: prob (B, N) f32 or None, entropy (B,) f32 (nats), idx (B, max_modes) int64, score, mass (B, max_modes) f32,
    count (B, max_modes) int32, n_modes (B,) int32.  An undefined row (NaN / +inf score, or all -inf) has n_modes 0 and a NaN entropy."""
    prob: Optional[torch.Tensor]
    entropy: torch.Tensor
    idx: torch.Tensor
    score: torch.Tensor
    mass: torch.Tensor
    count: torch.Tensor
    n_modes: torch.Tensor


def op_pose_modes(similarity: torch.Tensor, template_poses: torch.Tensor, symmetry: Optional[torch.Tensor] = None, *, temperature: float,
                  radius_deg: float, max_modes: int = 5, fill: bool = False, want_prob: bool = True) -> PoseModes:
    """The pose distribution of each score row -- softmax at `temperature` (score units) and its entropy -- and its distinct modes: greedy
    suppression on the template grid within `radius_deg` under the sample's symmetry class (include/nope_hip.h: nope_op_pose_modes).
    similarity (B, N) f32 (a view with inner stride 1 is read in place through its row stride), template_poses (B|1, N, 3, 3) of any float
    dtype, symmetry (B,) / (B, 1) in {0, 1, 2}.  Everything follows the scores' device.  fill: left-over slots take the best templates not
    yet listed (mass 0, count 0) instead of idx -1; needs max_modes <= N.  Nothing is read by the host."""
    require_device(similarity)
    if similarity.dim() != 2:
        raise NopeError(f"similarity {tuple(similarity.shape)}: expected (B, N)")
    if similarity.dtype != torch.float32 or (similarity.shape[1] > 1 and similarity.stride(1) != 1) or \
            (similarity.shape[0] > 1 and similarity.stride(0) < similarity.shape[1]):
        similarity = _f32c(similarity)
    B, N = similarity.shape
    ld = similarity.stride(0) if B > 1 else N
    dev = similarity.device
    poses = template_poses.to(device=dev, dtype=torch.float64).contiguous()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 3) or poses.shape[0] not in (1, B) or poses.shape[1] != N:
        raise NopeError(f"template_poses {tuple(poses.shape)}: expected (B|1, N, 3, 3) for similarity {(B, N)}")
    sym = None if symmetry is None else symmetry.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if sym is not None and sym.numel() != B:
        raise NopeError(f"symmetry has {sym.numel()} entries for {B} samples")
    max_modes = int(max_modes)
    prob = torch.empty((B, N), dtype=torch.float32, device=dev) if want_prob else None
    out = PoseModes(prob, torch.empty(B, dtype=torch.float32, device=dev), torch.empty((B, max(max_modes, 0)), dtype=torch.int64, device=dev),
                    torch.empty((B, max(max_modes, 0)), dtype=torch.float32, device=dev), torch.empty((B, max(max_modes, 0)), dtype=torch.float32, device=dev),
                    torch.empty((B, max(max_modes, 0)), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    status = torch.empty(1, dtype=torch.int32, device=dev)
    stride_b = 0 if (poses.shape[0] == 1 and B > 1) else N * 9
    return _pose_modes_call(similarity, ld, poses, stride_b, N, sym, temperature, math.radians(radius_deg), max_modes, fill, out, status)


def _pose_modes_call(similarity, ld, poses, stride_b, N, sym, temperature, radius_rad, max_modes, fill, out: PoseModes, status) -> PoseModes:
    """The launch of op_pose_modes into given outputs (the argument tests pre-fill them)."""
    l = lib()
    l.check(l.dll.nope_op_pose_modes(_ptr(similarity), ld, _ptr(poses), stride_b, N, _ptr(sym), float(temperature), float(radius_rad),
                                     int(max_modes), int(bool(fill)), _ptr(out.prob), N, _ptr(out.entropy), _ptr(out.idx), _ptr(out.score),
                                     _ptr(out.mass), _ptr(out.count), _ptr(out.n_modes), _ptr(status), similarity.shape[0],
                                     _stream(similarity)), "nope_op_pose_modes")
    return out


# --------------------------------------------------------------------------------------------
# coarse-to-fine retrieval over nested grids (csrc/kernels_search.hip; the loop is nope_amd/search.py)
# --------------------------------------------------------------------------------------------
C2F_OVERFLOW, C2F_BAD_SEED = 1, 2            # bits of op_c2f_expand's status
C2F_ROTATION, C2F_VIEWPOINT = 0, 1           # dist_kind
C2F_MAX_SEEDS = 16


class C2FExpand(NamedTuple):
    """op_c2f_expand: cand (B, M) int32 (the candidates in emission order, then -1), n_cand, n_dropped (B,) int32, rows (B, M, 6) f32 (the bits
    of all_relativeR[b, cand]; a padded slot: the first valid seed's row), status (1,) int32 (C2F_OVERFLOW | C2F_BAD_SEED), left on the device."""
    cand: torch.Tensor
    n_cand: torch.Tensor
    n_dropped: torch.Tensor
    rows: torch.Tensor
    status: torch.Tensor


def op_c2f_expand(template_poses: torch.Tensor, stage_of: torch.Tensor, max_stage: int, state: torch.Tensor, seeds: Optional[torch.Tensor],
                  all_relativeR: torch.Tensor, *, radius_rad: float = 0.0, dist_kind: int = C2F_VIEWPOINT, capacity: int) -> C2FExpand:
    """This stage's candidates of a coarse-to-fine search and their pose rows (include/nope_hip.h: nope_op_c2f_expand).  template_poses
    (B|1, N, 3, 3) of any float dtype, stage_of (N,), state (B, N) uint8 contiguous -- UPDATED IN PLACE --, seeds (B, n_seeds) int64 as
    hip.topk returns them or None (stage 0: every eligible pose), all_relativeR (B, N, 6).  Everything follows the state's device.
    Nothing is read by the host."""
    require_device(state)
    if state.dim() != 2 or state.dtype != torch.uint8 or not state.is_contiguous():
        raise NopeError(f"state {tuple(state.shape)} {state.dtype}: expected a contiguous (B, N) uint8 tensor (it is updated in place)")
    B, N = state.shape
    dev = state.device
    poses = template_poses.to(device=dev, dtype=torch.float64).contiguous()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 3) or poses.shape[0] not in (1, B) or poses.shape[1] != N:
        raise NopeError(f"template_poses {tuple(poses.shape)}: expected (B|1, N, 3, 3) for state {(B, N)}")
    stage_of = stage_of.to(device=dev, dtype=torch.int32).contiguous()
    rel = all_relativeR.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(stage_of.shape) != (N,) or tuple(rel.shape) != (B, N, 6):
        raise NopeError(f"stage_of {tuple(stage_of.shape)} / all_relativeR {tuple(rel.shape)}: expected ({N},) and ({B}, {N}, 6)")
    if seeds is not None:
        if seeds.dim() != 2 or seeds.shape[0] != B:
            raise NopeError(f"seeds {tuple(seeds.shape)}: expected ({B}, n_seeds)")
        seeds = seeds.to(device=dev, dtype=torch.int64).contiguous()
    M = max(int(capacity), 1)
    out = C2FExpand(torch.empty((B, M), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                    torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, M, 6), dtype=torch.float32, device=dev),
                    torch.empty(1, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    stride_b = 0 if (poses.shape[0] == 1 and B > 1) else N * 9
    return _c2f_expand_call(poses, stride_b, N, stage_of, max_stage, state, seeds, 0 if seeds is None else seeds.shape[1], radius_rad,
                            dist_kind, rel, capacity, out)


def _c2f_expand_call(poses, stride_b, N, stage_of, max_stage, state, seeds, n_seeds, radius_rad, dist_kind, rel, capacity, out: C2FExpand) -> C2FExpand:
    """The launch of op_c2f_expand into given outputs (the argument tests pre-fill them)."""
    l = lib()
    l.check(l.dll.nope_op_c2f_expand(_ptr(poses), stride_b, N, _ptr(stage_of), int(max_stage), _ptr(state), _ptr(seeds), int(n_seeds),
                                     float(radius_rad), int(dist_kind), _ptr(rel), int(capacity), _ptr(out.cand), _ptr(out.n_cand),
                                     _ptr(out.n_dropped), _ptr(out.rows), _ptr(out.status), state.shape[0], _stream(state)), "nope_op_c2f_expand")
    return out


def op_c2f_commit(scores: torch.Tensor, cand: torch.Tensor, similarity: torch.Tensor) -> torch.Tensor:
    """similarity[b, cand[b, j]] = scores[b, j] for every cand >= 0, bit for bit, IN PLACE (nope_op_c2f_commit).  scores (B, M) f32, cand
    (B, M) int32, similarity (B, N) f32 with inner stride 1 (a view is written through its row stride: columns >= N stay untouched)."""
    require_device(similarity)
    if similarity.dim() != 2 or similarity.dtype != torch.float32 or (similarity.shape[1] > 1 and similarity.stride(1) != 1) or \
            (similarity.shape[0] > 1 and similarity.stride(0) < similarity.shape[1]):
        raise NopeError(f"similarity {tuple(similarity.shape)} {similarity.dtype} strides {similarity.stride()}: expected (B, N) f32 rows (it is written in place)")
    B, N = similarity.shape
    if scores.dim() != 2 or scores.shape[0] != B or tuple(cand.shape) != tuple(scores.shape):
        raise NopeError(f"scores {tuple(scores.shape)} / cand {tuple(cand.shape)}: expected two ({B}, M) tensors")
    scores = scores.to(device=similarity.device, dtype=torch.float32).contiguous()
    cand = cand.to(device=similarity.device, dtype=torch.int32).contiguous()
    if B == 0 or scores.shape[1] == 0:
        return similarity
    ld = similarity.stride(0) if B > 1 else max(N, 1)
    l = lib()
    l.check(l.dll.nope_op_c2f_commit(_ptr(scores), _ptr(cand), scores.shape[1], N, _ptr(similarity), ld, B, _stream(similarity)), "nope_op_c2f_commit")
    return similarity


# --------------------------------------------------------------------------------------------
# multi-reference retrieval (csrc/kernels_multiref.hip; the drivers are PoseConditional.retrieve_multi*)
# --------------------------------------------------------------------------------------------
MULTIREF_BAD_POSE, MULTIREF_BAD_COUNT = 1, 2            # bits of op_multiref_prepare's status
MULTIREF_MAX_REFS = 8
MULTIREF_WEIGHTINGS = {"uniform": 0, "softmax": 1, "nearest": 2}


class MultiRefPrep(NamedTuple):
    """op_multiref_prepare: all_relativeR (B, R, N, 6) f32 or None, weights (B, R, N) f32, dist (B, R, N) f64 radians or None (+inf at a
    padded reference), status (1,) int32 (MULTIREF_BAD_POSE | MULTIREF_BAD_COUNT; every weight of such a sample is NaN), left on the device."""
    all_relativeR: Optional[torch.Tensor]
    weights: torch.Tensor
    dist: Optional[torch.Tensor]
    status: torch.Tensor


def op_multiref_prepare(template_poses: torch.Tensor, ref_poses: torch.Tensor, n_refs: Optional[torch.Tensor] = None, *, weighting="softmax",
                        tau_deg: float = 30.0, dist_kind: int = C2F_ROTATION, want_rel: bool = True, want_dist: bool = False) -> MultiRefPrep:
    """The relative poses T[n] P[b, r]^T (6-D rows for the U-Net) and the blend weights of R posed reference views per sample
    (include/nope_hip.h: nope_op_multiref_prepare).  template_poses (B|1, N, 3, 3) and ref_poses (B, R, 3, 3) of any float dtype, n_refs (B,)
    or None (all R valid; references r >= n_refs[b] are padding: weight 0, the pose rows of reference 0).  weighting "uniform" | "softmax"
    (over -d / tau_deg, d the distance of `dist_kind` between grid pose and reference pose) | "nearest".  Everything follows the reference
    poses' device.  Nothing is read by the host."""
    require_device(ref_poses)
    if ref_poses.dim() != 4 or tuple(ref_poses.shape[2:]) != (3, 3):
        raise NopeError(f"ref_poses {tuple(ref_poses.shape)}: expected (B, R, 3, 3)")
    B, R = ref_poses.shape[:2]
    dev = ref_poses.device
    refs = ref_poses.to(torch.float64).contiguous()
    poses = template_poses.to(device=dev, dtype=torch.float64).contiguous()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 3) or poses.shape[0] not in (1, B):
        raise NopeError(f"template_poses {tuple(poses.shape)}: expected (B|1, N, 3, 3) for ref_poses {tuple(ref_poses.shape)}")
    N = poses.shape[1]
    nr = None if n_refs is None else n_refs.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if nr is not None and nr.numel() != B:
        raise NopeError(f"n_refs has {nr.numel()} entries for {B} samples")
    if not isinstance(weighting, int):
        if weighting not in MULTIREF_WEIGHTINGS:
            raise NopeError(f"weighting {weighting!r}: one of {sorted(MULTIREF_WEIGHTINGS)}")
        weighting = MULTIREF_WEIGHTINGS[weighting]
    out = MultiRefPrep(torch.empty((B, R, N, 6), dtype=torch.float32, device=dev) if want_rel else None,
                       torch.empty((B, R, N), dtype=torch.float32, device=dev),
                       torch.empty((B, R, N), dtype=torch.float64, device=dev) if want_dist else None,
                       torch.empty(1, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    stride_b = 0 if (poses.shape[0] == 1 and B > 1) else N * 9
    return _multiref_prepare_call(poses, stride_b, N, refs, R, nr, weighting, math.radians(tau_deg), dist_kind, out)


def _multiref_prepare_call(poses, stride_b, N, refs, R, n_refs, weighting, tau_rad, dist_kind, out: MultiRefPrep) -> MultiRefPrep:
    """The launch of op_multiref_prepare into given outputs (the argument tests pre-fill them)."""
    l = lib()
    l.check(l.dll.nope_op_multiref_prepare(_ptr(poses), stride_b, int(N), _ptr(refs), int(R), _ptr(n_refs), int(weighting), float(tau_rad),
                                           int(dist_kind), _ptr(out.all_relativeR), _ptr(out.weights), _ptr(out.dist), _ptr(out.status),
                                           refs.shape[0], _stream(refs)), "nope_op_multiref_prepare")
    return out


def multiref_similarity(q: torch.Tensor, bank: torch.Tensor, weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """score[b, n] of model.py:257-262 against the blend sum_r weights[b, r, n] bank[b, r, n] of R banks, in one pass that never writes the
    blend (include/nope_hip.h: nope_multiref_similarity).  q (B,C,H,W) f32; bank (B,R,N,C,H,W) f32|bf16|fp16; weights (B,R,N) f32.  With
    `out` (B, ld >= N) given, writes its columns [0, N)."""
    require_device(q)
    q = _f32c(q)
    B, Cc, H, W = q.shape
    if bank.dim() != 6 or bank.shape[0] != B or tuple(bank.shape[3:]) != (Cc, H, W):
        raise NopeError(f"bank shape {tuple(bank.shape)} does not match query {tuple(q.shape)}: expected (B, R, N, C, H, W)")
    R, N = bank.shape[1:3]
    if tuple(weights.shape) != (B, R, N):
        raise NopeError(f"weights {tuple(weights.shape)}: expected {(B, R, N)} for bank {tuple(bank.shape)}")
    if bank.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        bank = bank.float()
    bank = bank.contiguous()
    weights = weights.to(device=q.device, dtype=torch.float32).contiguous()
    if N == 0:
        return torch.empty((B, 0), dtype=torch.float32, device=q.device) if out is None else out
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B and out.shape[1] >= N
    l = lib()
    l.check(l.dll.nope_multiref_similarity(_ptr(q), _ptr(bank), dtype_code(bank.dtype), _ptr(weights), _ptr(out), B, R, N, Cc, H, W, out.shape[1],
                                           _stream(q)), "nope_multiref_similarity")
    return out


def op_multiref_fuse_scores(per_ref: torch.Tensor, weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Late fusion: scores[b, n] = f32(sum_r f64(weights[b, r, n]) f64(per_ref[b, r, n])), terms with a zero weight skipped
    (nope_op_multiref_fuse_scores).  per_ref, weights (B, R, N) f32.  With `out` (B, ld >= N) given, writes its columns [0, N)."""
    require_device(per_ref)
    if per_ref.dim() != 3 or tuple(weights.shape) != tuple(per_ref.shape):
        raise NopeError(f"per_ref {tuple(per_ref.shape)} / weights {tuple(weights.shape)}: expected two (B, R, N) tensors")
    per_ref = _f32c(per_ref)
    weights = weights.to(device=per_ref.device, dtype=torch.float32).contiguous()
    B, R, N = per_ref.shape
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=per_ref.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B and out.shape[1] >= N
    if B == 0 or N == 0:
        return out
    l = lib()
    l.check(l.dll.nope_op_multiref_fuse_scores(_ptr(per_ref), _ptr(weights), _ptr(out), B, R, N, out.shape[1], _stream(per_ref)),
            "nope_op_multiref_fuse_scores")
    return out


# --------------------------------------------------------------------------------------------
# occlusion-robust scoring (csrc/kernels_robust.hip; the drivers are PoseConditional.retrieval*(robust=...) / retrieve_robust)
# --------------------------------------------------------------------------------------------
def _robust_mask(mask: Optional[torch.Tensor], B: int, H: int, W: int, device) -> Optional[torch.Tensor]:
    """mask (B, H, W) uint8 | bool -> contiguous uint8 on `device` (bool is reinterpreted, not converted: True is the byte 1)."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
        raise NopeError(f"mask must be a uint8 or bool tensor, got {getattr(mask, 'dtype', type(mask))}")
    if tuple(mask.shape) != (B, H, W):
        raise NopeError(f"mask {tuple(mask.shape)}: expected {(B, H, W)}")
    require_device(mask)
    mask = mask.to(device).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def check_trim(trim) -> float:
    trim = float(trim)
    if not (0.0 <= trim < 1.0):         # (a NaN fails both comparisons)
        raise NopeError(f"trim {trim!r}: a fraction in [0, 1)")
    return trim


def robust_similarity(q: torch.Tensor, bank: torch.Tensor, mask: Optional[torch.Tensor] = None, trim: float = 0.0,
                      out: Optional[torch.Tensor] = None, col_offset: int = 0) -> torch.Tensor:
    """Masked, trimmed template scores (include/nope_hip.h: nope_robust_similarity): minus the sum of the m smallest per-pixel terms of
    `similarity` over the pixels of `mask`, m = a - min(a - 1, floor(trim a)).  q (B,C,H,W) f32; bank (B|1,N,C,H,W) f32|bf16|fp16; mask
    (B,H,W) uint8|bool or None (every pixel); trim in [0, 1).  With `out` (B, Ntotal) given, writes columns [col_offset, col_offset+N)."""
    require_device(q)
    trim = check_trim(trim)
    q = _f32c(q)
    B, Cc, H, W = q.shape
    if bank.dim() != 5 or tuple(bank.shape[2:]) != (Cc, H, W) or bank.shape[0] not in (1, B):
        raise NopeError(f"bank shape {tuple(bank.shape)} does not match query {tuple(q.shape)}")
    require_device(bank)
    mask = _robust_mask(mask, B, H, W, q.device)
    if bank.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        bank = bank.float()
    bank = bank.contiguous()
    N = bank.shape[1]
    if N == 0:
        return torch.empty((B, 0), dtype=torch.float32, device=q.device) if out is None else out
    stride_b = 0 if (bank.shape[0] == 1 and B > 1) else N * Cc * H * W
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=q.device)
        col_offset = 0
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B
    ld = out.shape[1]
    assert 0 <= col_offset and col_offset + N <= ld
    l = lib()
    l.check(l.dll.nope_robust_similarity(_ptr(q), _ptr(bank), dtype_code(bank.dtype), _ptr(mask), trim, out.data_ptr() + 4 * col_offset, B, N, Cc,
                                         H, W, stride_b, ld, _stream(q)), "nope_robust_similarity")
    return out


def op_residual_maps(q: torch.Tensor, bank: torch.Tensor, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-pixel terms d[b, idx[b, j], p] = sqrt(sum_c (q - t)^4) of chosen hypotheses -- where a match disagrees -- (B, k, H, W) f32
    (nope_op_residual_maps).  q (B,C,H,W) f32; bank (B|1,N,C,H,W) f32|bf16|fp16; idx (B, k) int64 as hip.topk returns it, or None: every
    template.  An index outside [0, N) gives a NaN plane."""
    require_device(q)
    q = _f32c(q)
    B, Cc, H, W = q.shape
    if bank.dim() != 5 or tuple(bank.shape[2:]) != (Cc, H, W) or bank.shape[0] not in (1, B):
        raise NopeError(f"bank shape {tuple(bank.shape)} does not match query {tuple(q.shape)}")
    require_device(bank)
    if bank.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        bank = bank.float()
    bank = bank.contiguous()
    N = bank.shape[1]
    if idx is not None:
        if idx.dim() != 2 or idx.shape[0] != B:
            raise NopeError(f"idx {tuple(idx.shape)}: expected ({B}, k)")
        idx = idx.to(device=q.device, dtype=torch.int64).contiguous()
        k = idx.shape[1]
    else:
        k = N
    out = torch.empty((B, k, H, W), dtype=torch.float32, device=q.device)
    if B == 0 or k == 0:
        return out
    if N == 0:
        return out.fill_(float("nan"))
    stride_b = 0 if (bank.shape[0] == 1 and B > 1) else N * Cc * H * W
    l = lib()
    l.check(l.dll.nope_op_residual_maps(_ptr(q), _ptr(bank), dtype_code(bank.dtype), _ptr(idx), _ptr(out), B, N, k, Cc, H, W, stride_b, _stream(q)),
            "nope_op_residual_maps")
    return out


def op_pool_mask(cover: torch.Tensor, hw, threshold: float = 0.5) -> torch.Tensor:
    """An image-resolution coverage plane -> the latent mask robust_similarity takes (nope_op_pool_mask).  cover (B, S_h, S_w) uint8 alpha
    or f32 visibility in [0, 1]; hw = (H, W) with S_h % H == 0 and S_w % W == 0.  A latent pixel is scored where the mean coverage of its
    cell reaches `threshold`: uint8, exactly, byte sum >= ceil(threshold 255 area); f32, f32 sum / area >= f32(threshold).  -> (B, H, W) uint8."""
    from fractions import Fraction
    require_device(cover)
    H, W = int(hw[0]), int(hw[1])
    if cover.dim() != 3 or cover.dtype not in (torch.uint8, torch.float32):
        raise NopeError(f"cover {tuple(cover.shape)} {cover.dtype}: expected a (B, S_h, S_w) uint8 or float32 tensor")
    B, Sh, Sw = cover.shape
    if H < 1 or W < 1 or Sh % H or Sw % W:
        raise NopeError(f"cover {tuple(cover.shape)}: its size must be a multiple of the latent size {(H, W)}")
    threshold = float(threshold)
    if not (0.0 <= threshold <= 1.0):
        raise NopeError(f"threshold {threshold!r}: a coverage in [0, 1]")
    cover = cover.contiguous()
    area = (Sh // H) * (Sw // W)
    min_sum = math.ceil(Fraction(threshold) * 255 * area)          # exact: Fraction(float) is the float's value
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=cover.device)
    if B == 0:
        return mask
    l = lib()
    l.check(l.dll.nope_op_pool_mask(_ptr(cover), int(cover.dtype == torch.uint8), B, Sh, Sw, H, W, int(min_sum), threshold, _ptr(mask),
                                    _stream(cover)), "nope_op_pool_mask")
    return mask


MULTIREF_BAD_CAND = 4                                   # bit 2 of op_multiref_select's status: a cand entry below -1 or >= N


class MultiRefSelect(NamedTuple):
    """op_multiref_select: all_relativeR (B, M, S, 6) f32 or None, weights (B, M, S) f32, dist (B, M, S) f64 radians or None (+inf at a slot
    m >= min(M, n_refs[b]) and at a padded candidate), status (1,) int32 (MULTIREF_BAD_POSE | MULTIREF_BAD_COUNT | MULTIREF_BAD_CAND), src
    (B, M, S) int32: the reference each slot is generated from.  Left on the device."""
    all_relativeR: Optional[torch.Tensor]
    weights: torch.Tensor
    dist: Optional[torch.Tensor]
    status: torch.Tensor
    src: torch.Tensor


def op_multiref_select(template_poses: torch.Tensor, ref_poses: torch.Tensor, n_refs: Optional[torch.Tensor] = None, *, max_refs: int,
                       cand: Optional[torch.Tensor] = None, weighting="softmax", tau_deg: float = 30.0, dist_kind: int = C2F_ROTATION,
                       want_rel: bool = True, want_dist: bool = False) -> MultiRefSelect:
    """The max_refs = M nearest of R posed references per (sample, slot), their relative poses and their blend weights (include/nope_hip.h:
    nope_op_multiref_select).  Arguments as op_multiref_prepare; cand (B, S) integers or None: the grid poses the slots stand for (-1:
    padding, as op_c2f_expand writes them; hip.topk's indices do as well); None: slot s is pose s, S = N.  Nothing is read by the host."""
    require_device(ref_poses)
    if ref_poses.dim() != 4 or tuple(ref_poses.shape[2:]) != (3, 3):
        raise NopeError(f"ref_poses {tuple(ref_poses.shape)}: expected (B, R, 3, 3)")
    B, R = ref_poses.shape[:2]
    dev = ref_poses.device
    refs = ref_poses.to(torch.float64).contiguous()
    poses = template_poses.to(device=dev, dtype=torch.float64).contiguous()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 3) or poses.shape[0] not in (1, B):
        raise NopeError(f"template_poses {tuple(poses.shape)}: expected (B|1, N, 3, 3) for ref_poses {tuple(ref_poses.shape)}")
    N = poses.shape[1]
    nr = None if n_refs is None else n_refs.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    if nr is not None and nr.numel() != B:
        raise NopeError(f"n_refs has {nr.numel()} entries for {B} samples")
    if not isinstance(weighting, int):
        if weighting not in MULTIREF_WEIGHTINGS:
            raise NopeError(f"weighting {weighting!r}: one of {sorted(MULTIREF_WEIGHTINGS)}")
        weighting = MULTIREF_WEIGHTINGS[weighting]
    S = N
    if cand is not None:
        if cand.dim() != 2 or cand.shape[0] != B:
            raise NopeError(f"cand {tuple(cand.shape)}: expected ({B}, S)")
        cand = cand.to(device=dev, dtype=torch.int32).contiguous()
        S = cand.shape[1]
    M = int(max_refs)
    Mo = max(M, 0)
    out = MultiRefSelect(torch.empty((B, Mo, S, 6), dtype=torch.float32, device=dev) if want_rel else None,
                         torch.empty((B, Mo, S), dtype=torch.float32, device=dev),
                         torch.empty((B, Mo, S), dtype=torch.float64, device=dev) if want_dist else None,
                         torch.empty(1, dtype=torch.int32, device=dev), torch.empty((B, Mo, S), dtype=torch.int32, device=dev))
    if B == 0:
        return out
    stride_b = 0 if (poses.shape[0] == 1 and B > 1) else N * 9
    return _multiref_select_call(poses, stride_b, N, refs, R, nr, cand, S, M, weighting, math.radians(tau_deg), dist_kind, out)


def _multiref_select_call(poses, stride_b, N, refs, R, n_refs, cand, S, M, weighting, tau_rad, dist_kind, out: MultiRefSelect) -> MultiRefSelect:
    """The launch of op_multiref_select into given outputs (the argument tests pre-fill them)."""
    l = lib()
    l.check(l.dll.nope_op_multiref_select(_ptr(poses), stride_b, int(N), _ptr(refs), int(R), _ptr(n_refs), _ptr(cand), int(S), int(M), int(weighting),
                                          float(tau_rad), int(dist_kind), _ptr(out.src), _ptr(out.all_relativeR), _ptr(out.weights), _ptr(out.dist),
                                          _ptr(out.status), refs.shape[0], _stream(refs)), "nope_op_multiref_select")
    return out


def op_multiref_gather(reference_feats: torch.Tensor, src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, j] = reference_feats[b, src[b, j]], bit for bit (nope_op_multiref_gather).  reference_feats (B, R, ...) f32 with rows of a
    multiple of 4 elements; src (B, ...) int32, J entries per sample (op_multiref_select's (B, M, S)); -> (B, J, ...) f32.  A src entry outside
    [0, R) gives a NaN row."""
    require_device(reference_feats)
    if reference_feats.dim() < 3 or src.dim() < 2 or src.shape[0] != reference_feats.shape[0]:
        raise NopeError(f"reference_feats {tuple(reference_feats.shape)} / src {tuple(src.shape)}: expected (B, R, ...) and (B, ...)")
    feats = _f32c(reference_feats)
    B, R = feats.shape[:2]
    src = src.to(device=feats.device, dtype=torch.int32).contiguous()
    J = src.numel() // B if B else 0
    L = feats[0, 0].numel() if B and R else 0
    if out is None:
        out = torch.empty((B, J, *feats.shape[2:]), dtype=torch.float32, device=feats.device)
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != feats.device or out.numel() != B * J * L:
        raise NopeError(f"out {tuple(out.shape)} {out.dtype}: expected a contiguous f32 tensor of {B * J * L} elements ({B}, {J}, ...) on {feats.device}")
    if B == 0 or J == 0:
        return out
    l = lib()
    l.check(l.dll.nope_op_multiref_gather(_ptr(feats), _ptr(src), _ptr(out), B, R, J, L, _stream(feats)), "nope_op_multiref_gather")
    return out


# --------------------------------------------------------------------------------------------
# sub-grid pose refinement (csrc/kernels_refine.hip; the loop is PoseConditional.refine_from_feat)
# --------------------------------------------------------------------------------------------
REFINE_NONFINITE, REFINE_SINGULAR, REFINE_ZERO_STEP, REFINE_CLAMPED, REFINE_BAD_INDEX = 1, 2, 3, 4, 5


def op_refine_init(all_relativeR: torch.Tensor, idx: torch.Tensor, fd_step: float = 1e-2):
    """all_relativeR (B,N,6), idx (B,k) int64 -> (dR (B,k,3,3) f64, dR_init (its copy), poses (B,7k,6) f32, status (B,k) int32): the
    Gram-Schmidt matrix of all_relativeR[b, idx[b, j]] and the seven poses [dR, exp(+-h e_x) dR, exp(+-h e_y) dR, exp(+-h e_z) dR]."""
    require_device(all_relativeR)
    rel = _f32c(all_relativeR)
    idx = idx.to(device=rel.device, dtype=torch.int64).contiguous()
    if rel.dim() != 3 or rel.shape[2] != 6 or idx.dim() != 2 or idx.shape[0] != rel.shape[0]:
        raise NopeError(f"all_relativeR {tuple(rel.shape)} / idx {tuple(idx.shape)}: expected (B, N, 6) and (B, k)")
    B, N, k = rel.shape[0], rel.shape[1], idx.shape[1]
    dR = torch.empty((B, k, 3, 3), dtype=torch.float64, device=rel.device)
    dR0 = torch.empty_like(dR)
    poses = torch.empty((B, 7 * k, 6), dtype=torch.float32, device=rel.device)
    status = torch.empty((B, k), dtype=torch.int32, device=rel.device)
    l = lib()
    l.check(l.dll.nope_op_refine_init(_ptr(rel), N, _ptr(idx), _ptr(dR), _ptr(dR0), _ptr(poses), _ptr(status), B, k, float(fd_step), _stream(rel)),
            "nope_op_refine_init")
    return dR, dR0, poses, status


def op_refine_normal_eq(q: torch.Tensor, maps: torch.Tensor, fd_step: float = 1e-2, out: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q (B,C,h,w) f32, maps (B,k,7,C,h,w) or (B,7k,C,h,w) f32 -> (B,k,10) f64: A00 A01 A02 A11 A12 A22 | g0 g1 g2 | cost."""
    require_device(q)
    if q.dtype != torch.float32 or maps.dtype != torch.float32:
        raise NopeError("refinement reads f32 maps")
    q, maps = q.contiguous(), maps.contiguous()
    B, Cc, H, W = q.shape
    if maps.dim() == 5:
        maps = maps.view(B, -1, 7, Cc, H, W) if maps.shape[0] == B and maps.shape[1] % 7 == 0 and tuple(maps.shape[2:]) == (Cc, H, W) else maps
    if maps.dim() != 6 or maps.shape[0] != B or maps.shape[2] != 7 or tuple(maps.shape[3:]) != (Cc, H, W):
        raise NopeError(f"maps {tuple(maps.shape)} do not match the query {tuple(q.shape)}: expected (B, k, 7, C, h, w)")
    k = maps.shape[1]
    if out is None:
        out = torch.empty((B, k, 10), dtype=torch.float64, device=q.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (B, k, 10)
    l = lib()
    need = int(l.dll.nope_op_refine_normal_eq_workspace_bytes(B, k, H, W))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=q.device)
    l.check(l.dll.nope_op_refine_normal_eq(_ptr(q), _ptr(maps), _ptr(out), B, k, Cc, H, W, float(fd_step), _ptr(workspace),
                                           workspace.numel() * workspace.element_size(), _stream(q)), "nope_op_refine_normal_eq")
    return out


def op_refine_step(normal_eq: torch.Tensor, dR: torch.Tensor, poses: torch.Tensor, fd_step: float = 1e-2, max_step_rad: float = 0.17453292519943295,
                   damping: float = 1e-6, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One damped Gauss-Newton step IN PLACE on dR (B,k,3,3) f64 and poses (B,7k,6) f32 from normal_eq (B,k,10) f64; returns the
    per-candidate status (B,k) int32 (REFINE_*; 0 and REFINE_CLAMPED are steps taken)."""
    require_device(dR)
    B, k = dR.shape[:2]
    if (dR.dtype != torch.float64 or not dR.is_contiguous() or tuple(dR.shape[2:]) != (3, 3) or poses.dtype != torch.float32 or not poses.is_contiguous()
            or poses.numel() != B * k * 42 or normal_eq.dtype != torch.float64 or not normal_eq.is_contiguous() or tuple(normal_eq.shape) != (B, k, 10)):
        raise NopeError(f"refine step: dR {tuple(dR.shape)}, poses {tuple(poses.shape)}, normal_eq {tuple(normal_eq.shape)}")
    if status is None:
        status = torch.empty((B, k), dtype=torch.int32, device=dR.device)
    assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == B * k
    l = lib()
    l.check(l.dll.nope_op_refine_step(_ptr(normal_eq), _ptr(dR), _ptr(poses), _ptr(status), B, k, float(fd_step), float(max_step_rad), float(damping),
                                      _stream(dR)), "nope_op_refine_step")
    return status


def op_refine_select(dR: torch.Tensor, dR_init: torch.Tensor, score_refined: torch.Tensor, similarity: torch.Tensor, idx: torch.Tensor,
                     template_poses: Optional[torch.Tensor] = None) -> SimpleNamespace:
    """Accept / revert against similarity[b, idx[b, j]] and order by final score (include/nope_hip.h).  Returns a namespace of tensors in the
    final order: dR (B,k,3,3) f64, rot6d (B,k,6) f32, score, score_init (B,k) f32, accepted (B,k) bool, order (B,k) int64, and pred_R (B,k,3,3)
    f64 = (dR dR_init^T) template_poses[b, idx] when template_poses (B|1,N,3,3) is given (None otherwise)."""
    require_device(dR)
    B, k = dR.shape[:2]
    dev = dR.device
    score_refined, similarity = _f32c(score_refined), _f32c(similarity)
    idx = idx.to(device=dev, dtype=torch.int64).contiguous()
    if (tuple(score_refined.shape) != (B, k) or tuple(idx.shape) != (B, k) or similarity.dim() != 2 or similarity.shape[0] != B
            or dR.dtype != torch.float64 or dR_init.dtype != torch.float64 or dR_init.shape != dR.shape):
        raise NopeError(f"refine select: dR {tuple(dR.shape)}, scores {tuple(score_refined.shape)}, similarity {tuple(similarity.shape)}, idx {tuple(idx.shape)}")
    dR, dR_init = dR.contiguous(), dR_init.contiguous()
    tpl, stride_b, n_tpl, pred = None, 0, 0, None
    if template_poses is not None:
        tpl = template_poses.to(device=dev, dtype=torch.float64).contiguous()
        if tpl.dim() != 4 or tuple(tpl.shape[2:]) != (3, 3) or tpl.shape[0] not in (1, B):
            raise NopeError(f"template_poses {tuple(tpl.shape)}: expected (B|1, N, 3, 3)")
        n_tpl = tpl.shape[1]
        stride_b = 0 if (tpl.shape[0] == 1 and B > 1) else n_tpl * 9
        pred = torch.empty((B, k, 3, 3), dtype=torch.float64, device=dev)
    r = SimpleNamespace(dR=torch.empty_like(dR), rot6d=torch.empty((B, k, 6), dtype=torch.float32, device=dev),
                        score=torch.empty((B, k), dtype=torch.float32, device=dev), score_init=torch.empty((B, k), dtype=torch.float32, device=dev),
                        order=torch.empty((B, k), dtype=torch.int64, device=dev), pred_R=pred)
    accepted = torch.empty((B, k), dtype=torch.int32, device=dev)
    l = lib()
    l.check(l.dll.nope_op_refine_select(_ptr(dR), _ptr(dR_init), _ptr(score_refined), _ptr(similarity), similarity.shape[1], similarity.shape[1],
                                        _ptr(idx), _ptr(tpl), stride_b, n_tpl, _ptr(r.dR), _ptr(r.rot6d), _ptr(r.score), _ptr(r.score_init),
                                        _ptr(accepted), _ptr(r.order), _ptr(pred), B, k, _stream(dR)), "nope_op_refine_select")
    r.accepted = accepted != 0
    return r


# --------------------------------------------------------------------------------------------
# visualisation pictures (nope_amd/vis.py)
# --------------------------------------------------------------------------------------------
class VisCol:
    """One column of a picture for op_vis_grid / op_vis_sheet: `tensor` (B, 3, H, W) -- the same images in every frame -- or (B, F, 3, H, W)
    f32, any strides over B and F (a slice of the template axis is read in place; the (3, H, W) planes are contiguous); `unnormalize`:
    (x + 1) * 0.5 first; `clamp`: clamp to [0, 1]; `index` (B,) int64 on the tensor's device, any stride (nearest_idx[:, 0]): sample b of
    every frame shows tensor[b, index[b]], the index clamped into the tensor's frame axis on the device."""

    def __init__(self, tensor: torch.Tensor, unnormalize: bool = False, clamp: bool = False, index: Optional[torch.Tensor] = None):
        if tensor.dim() not in (4, 5) or tensor.shape[-3] != 3:
            raise NopeError(f"picture column {tuple(tensor.shape)}: expected (B, 3, H, W) or (B, F, 3, H, W)")
        if index is not None and (tensor.dim() != 5 or index.dim() != 1 or index.shape[0] != tensor.shape[0] or index.dtype != torch.int64
                                  or index.device != tensor.device):
            raise NopeError("picture column index: expected (B,) int64 on the device of a (B, N, 3, H, W) tensor")
        if tensor.dtype != torch.float32:
            tensor = tensor.float()
        H, W = tensor.shape[-2:]
        if tensor.numel() and tuple(tensor.stride()[-3:]) != (H * W, W, 1):
            tensor = tensor.contiguous()
        self.tensor, self.index = tensor, index
        self.flags = (VIS_UNNORMALIZE if unnormalize else 0) | (VIS_CLAMP if clamp else 0)
        self.frames = tensor.shape[1] if tensor.dim() == 5 and index is None else None      # None: the same images in every frame

    def desc(self, frame0: int = 0) -> VisColumn:
        t = self.tensor
        c = VisColumn(data=t.data_ptr(), stride_b=t.stride(0), stride_f=0, index=None, index_stride=0, index_limit=0, flags=self.flags)
        if t.dim() == 5:
            c.stride_f = t.stride(1)
            if self.index is not None:
                c.index, c.index_stride, c.index_limit = self.index.data_ptr(), self.index.stride(0), t.shape[1]
            else:
                c.data = t.data_ptr() + 4 * frame0 * t.stride(1)
        return c


def _vis_setup(columns, frame0, n_frames):
    if not columns:
        raise NopeError("a picture needs at least one column")
    columns = [c if isinstance(c, VisCol) else VisCol(*c) if isinstance(c, (tuple, list)) else VisCol(c) for c in columns]
    t0 = columns[0].tensor
    require_device(t0)
    B, (H, W) = t0.shape[0], t0.shape[-2:]
    counts = {c.frames for c in columns if c.frames is not None}
    if len(counts) > 1:
        raise NopeError(f"picture columns disagree on the number of frames: {sorted(counts)}")
    if counts:
        F = counts.pop()
    else:           # no column has a frame axis: every frame shows the same images, as many as the caller asks for
        F = 1 if n_frames is None else frame0 + n_frames
    for c in columns:
        if c.tensor.shape[0] != B or tuple(c.tensor.shape[-2:]) != (H, W) or c.tensor.device != t0.device:
            raise NopeError(f"picture columns disagree: {tuple(c.tensor.shape)} against {tuple(t0.shape)}")
    if n_frames is None:
        n_frames = F - frame0
    if frame0 < 0 or n_frames < 0 or frame0 + n_frames > F:
        raise NopeError(f"frames [{frame0}, {frame0 + n_frames}) of {F}")
    descs = (VisColumn * len(columns))(*[c.desc(frame0) for c in columns])
    return columns, descs, B, n_frames, H, W, t0


def op_vis_grid(columns, frame0: int = 0, n_frames: Optional[int] = None) -> torch.Tensor:
    """put_image_to_grid (visualization_utils.py:43-57) of n_frames pictures: (n_frames, B * (n_cols + 1), 3, H, W) f16 with the zero margin
    column.  columns: VisCol, or (tensor, unnormalize, clamp, index) tuples, or plain tensors."""
    columns, descs, B, nf, H, W, t0 = _vis_setup(columns, frame0, n_frames)
    out = torch.empty((nf, B * (len(columns) + 1), 3, H, W), dtype=torch.float16, device=t0.device)
    l = lib()
    l.check(l.dll.nope_op_vis_grid(descs, len(columns), B, nf, H, W, _ptr(out), _stream(t0)), "nope_op_vis_grid")
    return out


def vis_sheet_shape(n_cols: int, B: int, tile: int, nrow: int, padding: int) -> Tuple[int, int]:
    """(Hs, Ws) of make_grid(nrow, padding) over B * (n_cols + 1) images of tile x tile."""
    n_img = B * (n_cols + 1)
    xmaps = max(1, min(nrow, n_img))
    ymaps = -(-n_img // xmaps)
    return (tile + padding) * ymaps + padding, (tile + padding) * xmaps + padding


def op_vis_sheet(columns, tile: int = 64, nrow: int = 16, padding: int = 2, frame0: int = 0, n_frames: Optional[int] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The PNG bytes of n_frames pictures, (n_frames, Hs, Ws, 3) u8 (nope_op_vis_sheet); `out`: a contiguous u8 tensor of that shape to
    write into (a slice of a larger sheet stack: any byte offset)."""
    columns, descs, B, nf, H, W, t0 = _vis_setup(columns, frame0, n_frames)
    Hs, Ws = vis_sheet_shape(len(columns), B, max(int(tile), 0), int(nrow), max(int(padding), 0))
    if out is None:
        out = torch.empty((nf, Hs, Ws, 3), dtype=torch.uint8, device=t0.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (nf, Hs, Ws, 3) or not out.is_contiguous() or out.device != t0.device:
        raise NopeError(f"sheet output {tuple(out.shape)} {out.dtype}: expected contiguous uint8 {(nf, Hs, Ws, 3)}")
    l = lib()
    l.check(l.dll.nope_op_vis_sheet(descs, len(columns), B, nf, H, W, tile, nrow, padding, _ptr(out), _stream(t0)), "nope_op_vis_sheet")
    return out


def _tensor_descs(state_dict: Dict[str, torch.Tensor]):
    keep, dev = [], None
    descs = (TensorDesc * max(1, len(state_dict)))()
    for i, (k, v) in enumerate(state_dict.items()):
        t = _f32c(v.detach())
        keep.append(t)
        dev = t.device
        descs[i].name = k.encode()
        descs[i].data = t.data_ptr()
        descs[i].ndim = t.dim()
        for j, s in enumerate(t.shape[:4]):
            descs[i].shape[j] = s
    return descs, keep, dev


# --------------------------------------------------------------------------------------------
# Network handles: what the five of them share
# --------------------------------------------------------------------------------------------
def _fill(c, cfg: dict, ints=(), arrays=(), **defaults):
    """Config struct c from the cfg dict: the int fields `ints` (required) and `defaults` (name=value when absent), and the fixed-length int
    arrays `arrays`, of which the first gives c.n_levels and each is read up to that length."""
    for k in ints:
        setattr(c, k, int(cfg[k]))
    for k, d in defaults.items():
        setattr(c, k, int(cfg.get(k, d)))
    for k in arrays:
        if k == arrays[0]:
            c.n_levels = len(tuple(cfg[k]))
        for i in range(c.n_levels):
            getattr(c, k)[i] = int(cfg[k][i])
    return c


class _Handle:
    """Owns one `nope_{_stem}*` of the library: create / destroy by symbol stem, and one workspace arena per (device, stream)."""
    _stem = ""

    def _fn(self, entry: str):
        return getattr(self._l.dll, f"nope_{self._stem}_{entry}")

    def _create(self, c, state_dict: Dict[str, torch.Tensor]):
        self._l = l = lib()
        self.compute_dtype = c.compute_dtype
        descs, keep, dev = _tensor_descs(state_dict)
        self.device = dev
        h = _vp()
        stream = torch.cuda.current_stream(dev).cuda_stream if dev is not None and dev.type == "cuda" else 0
        l.check(self._fn("create")(C.byref(c), descs, len(state_dict), stream, C.byref(h)), f"nope_{self._stem}_create")
        self._h = h
        self._ws: Dict[tuple, torch.Tensor] = {}     # one arena per (device, stream): forwards on different streams never share one

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._fn("destroy")(h)
            self._h = None

    def _arena(self, t: torch.Tensor, need: int) -> torch.Tensor:
        """The workspace of t's (device, stream), grown to at least `need` bytes."""
        key = (str(t.device), _stream(t))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._ws.pop(key, None)          # release the smaller arena before taking a bigger one
            ws = None
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=t.device)
        return ws


# --------------------------------------------------------------------------------------------
# Template-encoder handle
# --------------------------------------------------------------------------------------------
class EncoderHandle(_Handle):
    """Owns a `nope_encoder*` built from the FeatureExtractor's state dict (BatchNorm folded at create time)."""
    _stem = "encoder"

    def __init__(self, descriptor_size: int, state_dict: Dict[str, torch.Tensor], compute_dtype=F32, bn_eps: float = 1e-5):
        c = EncoderConfig()
        c.descriptor_size = int(descriptor_size)
        c.compute_dtype = dtype_code(compute_dtype)
        c.bn_eps = float(bn_eps)
        self.descriptor_size = c.descriptor_size
        self._create(c, {k: v for k, v in state_dict.items() if k.startswith(("backbone.", "projector.")) and v.dtype.is_floating_point})

    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """image (B,3,H,W) f32 -> (B,descriptor_size,H/8,W/8) f32."""
        require_device(image)
        image = _f32c(image)
        B, Cc, H, W = image.shape
        if Cc != 3:
            raise NopeError(f"encoder expects 3-channel images, got {tuple(image.shape)}")
        need = int(self._l.dll.nope_encoder_workspace_bytes(self._h, B, H, W))
        if need == 0:
            raise NopeError(f"unsupported encoder input size {H}x{W} (must be multiples of 8)")
        ws = self._arena(image, need)      # (per stream: two encoder passes may be in flight on different streams, model.generate_and_retrieve)
        out = torch.empty((B, self.descriptor_size, H // 8, W // 8), dtype=torch.float32, device=image.device)
        self._l.check(self._l.dll.nope_encoder_forward(self._h, _ptr(image), B, H, W, _ptr(out), _ptr(ws), need, _stream(image)),
                      "nope_encoder_forward")
        return out


def op_stem_conv(dt: int, image: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """conv1 7x7/2 pad 3 + per-channel affine + ReLU: image (B,3,H,W) f32 NCHW -> NHWC (B,H/2,W/2,64) of dtype dt."""
    image = _f32c(image)
    B, _, H, W = image.shape
    out = torch.empty((B, H // 2, W // 2, 64), dtype=torch_dtype(dt), device=image.device)
    scratch = torch.empty(147 * 64, dtype=torch.float32, device=image.device)
    l = lib()
    l.check(l.dll.nope_op_stem_conv(dt, _ptr(image), _ptr(_f32c(w)), _ptr(_f32c(scale)), _ptr(_f32c(shift)), _ptr(scratch),
                                    _ptr(out), B, H, W, _stream(image)), "nope_op_stem_conv")
    return out


# --------------------------------------------------------------------------------------------
# The hypothesis networks (U-Net, LDM, guided diffusion): one forward(x, pose) and the NOPE_F16X2 activation ranges
# (include/nope_hip.h: nope_unet_x2_poll; the three runtimes export the same entries under their stems)
# --------------------------------------------------------------------------------------------
class _HypothesisHandle(_Handle):
    _label = ""          # the network's name in the "unsupported ... problem size" message

    def _create(self, c, state_dict, cin: int, cout: int):
        self._cin, self._cout, self.pose_dim = cin, cout, c.pose_dim
        super()._create(c, state_dict)
        # NOPE_F16X2 activation ranges.  The library judges every forward on the device and overwrites the output of one whose layers left
        # their accurate windows with NaNs (include/nope_hip.h: nope_unet_x2_poll) -- no synchronisation in the step.  range_mode:
        #   "poison"            nothing more: the verdicts that have arrived are read at the start of the next forward (shifts re-centred,
        #                       an event recorded, one warning); a caller that finds NaNs in a bank repeats its call;
        #   "repeat"            after a forward (or, deferred, at the end of the caller's step) synchronise, read the verdict and issue
        #                       the forward again until it is inside its windows: never a NaN, one host synchronisation per step;
        #   "auto" (default)    "repeat" until three forwards in a row were inside their windows without any shift moving -- a network's
        #                       first calls settle its shifts without a NaN -- then "poison"; back to "repeat" when a verdict says so;
        #   "off"               do not look (the device still judges and poisons).
        # NOPE_X2_RANGE_CHECK = 0 / 1 / 2 / 3 selects off / auto / repeat / poison.
        self.range_mode = {"0": "off", "1": "auto", "2": "repeat", "3": "poison"}.get(os.environ.get("NOPE_X2_RANGE_CHECK", "1"), "auto") \
            if self.compute_dtype == F16X2 else "off"
        self._settled = 0                            # "auto": forwards in a row that needed nothing
        self.range_events: List[dict] = []           # one record per forward that had to be repeated
        self._pending: List[tuple] = []              # forwards issued with defer_range_check: (re-launch closure, stream)
        self._warned = False
        self.x2_enabled = self.compute_dtype == F16X2

    def forward(self, x: torch.Tensor, pose: torch.Tensor, x_rep: int = 1, out: Optional[torch.Tensor] = None,
                out_dtype=F32, defer_range_check: bool = False) -> torch.Tensor:
        """out[j] = net(x[j // x_rep], pose[j]); x (n_src,C,H,W) f32, pose (n_src*x_rep, pose_dim).  defer_range_check (NOPE_F16X2): the
        caller will call finish_range_check() itself before it hands results out."""
        require_device(x)
        x = _f32c(x)
        pose = _f32c(pose)
        n_src, Cc, H, W = x.shape
        n_hyp = pose.shape[0]
        if Cc != self._cin or pose.shape[1] != self.pose_dim or n_src * x_rep != n_hyp:
            raise NopeError(f"shape mismatch: x {tuple(x.shape)}, pose {tuple(pose.shape)}, x_rep {x_rep}")
        odt = dtype_code(out_dtype)
        if out is None:
            out = torch.empty((n_hyp, self._cout, H, W), dtype=torch_dtype(odt), device=x.device)
        assert out.is_contiguous() and out.numel() == n_hyp * self._cout * H * W and out.dtype == torch_dtype(odt)
        need = int(self._fn("workspace_bytes")(self._h, n_hyp, n_src, H, W))
        if need == 0:
            raise NopeError(f"unsupported {self._label} problem size n_hyp={n_hyp} H={H} W={W}")
        ws = self._arena(x, need)
        fn, what = self._fn("forward"), f"nope_{self._stem}_forward"
        def launch():
            self._l.check(fn(self._h, _ptr(x), n_src, x_rep, _ptr(pose), n_hyp, H, W, _ptr(out), odt, _ptr(ws), ws.numel(), _stream(x)), what)
        self._x2_before_forward(_stream(x))
        launch()
        if self._x2_mode() == "repeat" and self.x2_enabled:
            # the check needs the forward to have finished: callers that go on issuing work on the stream (PoseConditional: scoring,
            # top-k) call finish_range_check() at the END of their step -- one synchronisation where the results are read anyway --
            # and repeat their own tail when it says the forward was repeated
            self._pending.append((launch, _stream(x)))
            if not defer_range_check:
                self.finish_range_check()
        return out

    def _x2_mode(self) -> str:
        if self.range_mode == "auto":
            return "repeat" if self._settled < 3 else "poison"
        return self.range_mode

    def _x2_before_forward(self, stream):
        if self.range_mode != "off" and self.x2_enabled:
            # verdicts of EARLIER forwards that have reached the host (no waiting): their outputs were NaN; the shifts are re-centred now
            code, bad, moved, amax = self.x2_range_check(stream, sync=False)
            if code != 0 or moved:
                self._settled = 0
            if code != 0:
                self.range_events.append({"code": code, "layers_out_of_range": bad, "layers_adjusted": moved, "max_abs": amax, "attempt": -1})
                if self._x2_mode() == "poison" and not self._warned:
                    import warnings
                    self._warned = True
                    warnings.warn(f"nope_amd f16x2: an earlier U-Net forward saw activations up to {amax:.3g}, outside the accurate range of "
                                  f"{bad} layer(s): its output was overwritten with NaNs (never silently inaccurate); the layers' range shifts "
                                  "are re-centred now -- repeat that call (or use range_mode = 'repeat' / NOPE_X2_RANGE_CHECK=2)", RuntimeWarning)
                if code == ERR_RANGE_F16:
                    self.x2_enable(False)

    def x2_range_check(self, stream, sync: bool = True) -> Tuple[int, int, int, float]:
        """(code, layers out of range, layers whose shift moved, largest |activation|) of the forwards judged since the last look; sync:
        synchronise `stream` first (every forward issued on it is judged), else only the verdicts that have already arrived."""
        bad, moved, amax = _i(0), _i(0), C.c_float(0)
        code = int(self._fn("x2_range_check" if sync else "x2_poll")(self._h, stream, C.byref(bad), C.byref(moved), C.byref(amax)))
        if code not in (0, ERR_RANGE, ERR_RANGE_F16):
            self._l.check(code, f"nope_{self._stem}_x2_range_check")
        return code, bad.value, moved.value, float(amax.value)

    def x2_enable(self, on: bool):
        self._l.check(self._fn("x2_enable")(self._h, int(bool(on))), f"nope_{self._stem}_x2_enable")
        self.x2_enabled = bool(on) and self.compute_dtype == F16X2

    def finish_range_check(self) -> bool:
        """Check the forwards issued since the last check (nope_unet_x2_range_check: synchronises their stream); every forward whose layers
        left their accurate window is issued again -- same arguments, re-centred shifts -- until it is inside.  Returns True when anything
        was repeated: work the caller derived from the outputs has to be repeated too."""
        pending, self._pending = self._pending, []
        repeated = False
        for attempt in range(8):        # (a repeated forward can move the maxima of layers downstream of the repaired ones: a few rounds at most)
            if not pending or not (self._x2_mode() == "repeat" and self.x2_enabled):
                break
            code, bad, moved, amax = self.x2_range_check(pending[-1][1])
            if code == 0:
                self._settled = 0 if (moved or repeated) else self._settled + 1
                break
            # a two-pass layer saw activations outside its accurate window: those forwards have plain-f16 accuracy there -- repeat them
            self.range_events.append({"code": code, "layers_out_of_range": bad, "layers_adjusted": moved, "max_abs": amax, "attempt": attempt})
            if code == ERR_RANGE_F16 or attempt == 6:
                import warnings
                warnings.warn(f"nope_amd f16x2: activations up to {amax:.3g} " + ("are not finite" if code == ERR_RANGE_F16 else
                              "keep leaving the layers' windows") + ": this U-Net runs as bf16x3 (three MFMA passes) from now on", RuntimeWarning)
                self.x2_enable(False)
            for launch, _ in pending:
                launch()
            repeated = True
        return repeated


class UNetHandle(_HypothesisHandle):
    """Owns a `nope_unet*` built from a reference-keyed state dict."""
    _stem, _label = "unet", "U-Net"

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], compute_dtype=F32):
        c = _fill(UNetConfig(), {"dim_mults": (1, 2, 4, 8), **cfg}, ints=("u_net_dim", "channels"), arrays=("dim_mults",),
                  out_dim=cfg["channels"], pose_dim=6, groups=8, pose_mlp_layers=1, soft_up_down=0)
        c.heads, c.dim_head = 4, 32
        c.compute_dtype = dtype_code(compute_dtype)
        self.cfg = dict(cfg)
        self.channels, self.out_dim = c.channels, c.out_dim
        self._create(c, state_dict, c.channels, c.out_dim)

    def x2_shifts(self) -> List[int]:
        n = _i(0)
        self._l.check(self._l.dll.nope_unet_x2_shifts(self._h, None, 0, C.byref(n)), "nope_unet_x2_shifts")
        buf = (_i * max(1, n.value))()
        self._l.check(self._l.dll.nope_unet_x2_shifts(self._h, buf, n.value, C.byref(n)), "nope_unet_x2_shifts")
        return list(buf[:n.value])

    def profile(self, enable: bool):
        self._l.check(self._l.dll.nope_unet_profile(self._h, int(enable)), "nope_unet_profile")

    def graph_limit(self, max_hyp_pixels: int):
        """Opt in to hipGraph replay for forwards of at most this many n_hyp * H * W (0 = off, the default)."""
        self._l.check(self._l.dll.nope_unet_graph_limit(self._h, int(max_hyp_pixels)), "nope_unet_graph_limit")

    def graph_replays(self) -> int:
        return int(self._l.dll.nope_unet_graph_replays(self._h))

    def profile_read(self):
        """(n_launches, total_ms, total_flops, total_bytes) of the conv-GEMM launches since profile(True)."""
        n, ms, fl, by = _i(0), C.c_double(0), C.c_double(0), C.c_double(0)
        self._l.check(self._l.dll.nope_unet_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "profile_read")
        return n.value, ms.value, fl.value, by.value

    def profile_launches(self):
        """One dict per conv launch since profile(True), in issue order: kernel name, shape, ms, flops, bytes."""
        n = _i(0)
        self._l.check(self._l.dll.nope_unet_profile_launches(self._h, None, 0, C.byref(n)), "profile_launches")
        buf = (ConvLaunchInfo * max(1, n.value))()
        self._l.check(self._l.dll.nope_unet_profile_launches(self._h, buf, n.value, C.byref(n)), "profile_launches")
        out = []
        for r in buf[:n.value]:
            d = {k: getattr(r, k) for k, _ in ConvLaunchInfo._fields_}
            d["kernel"] = CONV_KERNEL_NAMES[r.kernel]
            out.append(d)
        return out

    def workspace_bytes(self, n_hyp: int, n_src: int, H: int, W: int) -> int:
        return int(self._l.dll.nope_unet_workspace_bytes(self._h, n_hyp, n_src, H, W))


class LdmHandle(_HypothesisHandle):
    """Owns a `nope_ldm*` built from a UNetModelPose state dict (reference keys)."""
    _stem, _label = "ldm", "LDM U-Net"

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], compute_dtype=F32):
        c = _fill(LdmConfig(), cfg, ints=("in_channels", "model_channels", "out_channels", "num_res_blocks", "num_head_channels", "context_dim",
                                          "pose_dim", "pose_mlp_layers", "injecting_condition_twice"), arrays=("channel_mult", "attn_levels"),
                  use_scale_shift_norm=0, transformer_depth=1, resblock_updown=0, conv_resample=1)
        for i, d in enumerate(cfg.get("head_channels", ())):      # per level (num_head_channels = 0); else num_head_channels everywhere
            c.head_channels[i] = int(d)
        c.compute_dtype = dtype_code(compute_dtype)
        self.in_channels, self.out_channels = c.in_channels, c.out_channels
        self._create(c, state_dict, c.in_channels, c.out_channels)


class GdHandle(_HypothesisHandle):
    """Owns a `nope_gd*` built from a guided-diffusion UNetModelPose state dict (reference keys)."""
    _stem, _label = "gd", "GD U-Net"

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], compute_dtype=F32):
        c = _fill(GdConfig(), cfg, ints=("in_channels", "model_channels", "out_channels", "num_res_blocks", "head_channels_mid", "pose_dim", "pose_mlp",
                                         "new_attention_order", "resblock_updown", "conv_resample", "use_scale_shift_norm"),
                  arrays=("channel_mult", "attn_levels", "head_channels_in", "head_channels_out"))
        c.compute_dtype = dtype_code(compute_dtype)
        self.in_channels, self.out_channels = c.in_channels, c.out_channels
        self._create(c, state_dict, c.in_channels, c.out_channels)


def op_warp_perspective(img: torch.Tensor, minv, size: int, scale: float = 1.0, shift: float = 0.0, round_u8: bool = False) -> torch.Tensor:
    """img (H,W,C) uint8 or f32 on the device, minv 3x3 (host) mapping output pixels to source pixels -> (C,size,size) f32.
    round_u8 (uint8 sources): round + clamp the interpolated value to [0, 255] before scale / shift (a uint8 destination image)."""
    require_device(img)
    img = img.contiguous()
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    H, W, Cc = img.shape
    out = torch.empty((Cc, size, size), dtype=torch.float32, device=img.device)
    m = (C.c_float * 9)(*[float(v) for v in list(minv.reshape(-1))])
    l = lib()
    l.check(l.dll.nope_op_warp_perspective(_ptr(img), (2 if round_u8 else 1) if img.dtype == torch.uint8 else 0, H, W, Cc, m, _ptr(out), size, size, scale, shift,
                                           _stream(img)), "nope_op_warp_perspective")
    return out


def op_crop_frames(frames: torch.Tensor, minv: torch.Tensor, size: int, scale: float = 1.0, shift: float = 0.0, round_u8: bool = False) -> torch.Tensor:
    """frames (F,H,W,Cs) uint8 on the device, Cs = 3 (RGB) or 4 (RGBA: each tap is pasted on black through its alpha first); minv (F,3,3) or (F,9)
    f32 on the device, one inverse map per frame -> (F,3,size,size) f32 in one launch; scale / shift / round_u8 as op_warp_perspective."""
    require_device(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise NopeError(f"op_crop_frames: frames must be (F, H, W, Cs) uint8, got {tuple(frames.shape)} {frames.dtype}")
    frames = frames.contiguous()
    F, H, W, Cs = frames.shape
    minv = minv.to(device=frames.device, dtype=torch.float32).reshape(-1, 9).contiguous()
    if minv.shape[0] != F:
        raise NopeError(f"op_crop_frames: {F} frames but {minv.shape[0]} maps")
    out = torch.empty((F, 3, size, size), dtype=torch.float32, device=frames.device)
    l = lib()
    l.check(l.dll.nope_op_crop_frames(_ptr(frames), F, H, W, Cs, _ptr(minv), _ptr(out), size, size, scale, shift, int(bool(round_u8)), _stream(frames)),
            "nope_op_crop_frames")
    return out


def op_layer_norm(dt: int, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """x (..., C) of dtype dt: LayerNorm over the last axis."""
    y = torch.empty_like(x)
    l = lib()
    l.check(l.dll.nope_op_layer_norm(dt, _ptr(x), _ptr(y), _ptr(_f32c(gamma)), _ptr(_f32c(beta)), x.numel() // x.shape[-1], x.shape[-1], eps,
                                     _stream(x)), "nope_op_layer_norm")
    return y


def op_geglu(dt: int, x: torch.Tensor) -> torch.Tensor:
    """x (..., 2D) = [a | gate] -> a * gelu(gate), (..., D)."""
    D = x.shape[-1] // 2
    y = torch.empty((*x.shape[:-1], D), dtype=x.dtype, device=x.device)
    l = lib()
    l.check(l.dll.nope_op_geglu(dt, _ptr(x), _ptr(y), x.numel() // x.shape[-1], D, _stream(x)), "nope_op_geglu")
    return y


def op_token_attention(dt: int, qkv: torch.Tensor, dim_head: int = 32) -> torch.Tensor:
    """qkv (n, N, 3C) -> softmax(q k^T / sqrt(d)) v per head of `dim_head` channels, (n, N, C)."""
    n, N, c3 = qkv.shape
    out = torch.empty((n, N, c3 // 3), dtype=qkv.dtype, device=qkv.device)
    l = lib()
    l.check(l.dll.nope_op_token_attention(dt, _ptr(qkv), _ptr(out), n, N, c3 // 3, dim_head, _stream(qkv)), "nope_op_token_attention")
    return out


def op_wide_attention(dt: int, qkv: torch.Tensor) -> torch.Tensor:
    """qkv (n, N, 3C), C = 256 / 512 -> softmax(q k^T / sqrt(C)) v with ONE head of all C channels, (n, N, C)."""
    n, N, c3 = qkv.shape
    out = torch.empty((n, N, c3 // 3), dtype=qkv.dtype, device=qkv.device)
    l = lib()
    l.check(l.dll.nope_op_wide_attention(dt, _ptr(qkv), _ptr(out), n, N, c3 // 3, _stream(qkv)), "nope_op_wide_attention")
    return out


# --------------------------------------------------------------------------------------------
# Stable Diffusion VAE handle
# --------------------------------------------------------------------------------------------
class VaeHandle(_Handle):
    """Owns a `nope_vae*` built from an AutoencoderKL state dict (diffusers 0.14 keys, without the wrapper's `encoder.` prefix)."""
    _stem = "vae"

    def __init__(self, cfg: dict, state_dict: Dict[str, torch.Tensor], compute_dtype=F32, max_workspace_bytes: int = 4 << 30):
        c = _fill(VaeConfig(), cfg, ints=("in_channels", "out_channels", "layers_per_block", "latent_channels", "norm_num_groups"),
                  arrays=("block_out_channels",))
        c.compute_dtype = dtype_code(compute_dtype)
        c.gn_eps = 1e-6
        self.in_channels, self.out_channels, self.latent_channels = c.in_channels, c.out_channels, c.latent_channels
        self.factor = 2 ** (c.n_levels - 1)
        self.max_workspace_bytes = int(max_workspace_bytes)
        self._create(c, state_dict)

    def _workspace(self, x: torch.Tensor, decode: int, n: int, H: int, W: int) -> torch.Tensor:
        """The workspace of the largest chunk of at most n samples within max_workspace_bytes (the library runs the batch chunk by chunk)."""
        one = int(self._l.dll.nope_vae_workspace_bytes(self._h, decode, 1, H, W))
        if one == 0:
            raise NopeError(f"unsupported VAE {'latent' if decode else 'image'} size {H}x{W}")
        need = one
        lo, hi = 1, n
        while lo < hi:          # (the library picks the same chunk from the bytes it is given)
            mid = (lo + hi + 1) // 2
            b = int(self._l.dll.nope_vae_workspace_bytes(self._h, decode, mid, H, W))
            if b and b <= self.max_workspace_bytes:
                lo, need = mid, b
            else:
                hi = mid - 1
        if lo == 1:
            need = one
        return self._arena(x, need)

    def encode(self, image: torch.Tensor) -> torch.Tensor:
        """image (B, in_channels, H, W) f32 -> latent (B, latent_channels, H/f, W/f) f32 (x 0.18215)."""
        require_device(image)
        image = _f32c(image)
        B, Cc, H, W = image.shape
        if Cc != self.in_channels or H % self.factor or W % self.factor:
            raise NopeError(f"VAE encode: image {tuple(image.shape)} (needs {self.in_channels} channels, sides multiples of {self.factor})")
        out = torch.empty((B, self.latent_channels, H // self.factor, W // self.factor), dtype=torch.float32, device=image.device)
        if B == 0:
            return out
        ws = self._workspace(image, 0, B, H, W)
        self._l.check(self._l.dll.nope_vae_encode(self._h, _ptr(image), B, H, W, _ptr(out), _ptr(ws), ws.numel(), _stream(image)), "nope_vae_encode")
        return out

    def decode(self, latent: torch.Tensor, unnormalize: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """latent (B, latent_channels, h, w) f32 -> image (B, out_channels, f h, f w) f32; unnormalize: (image + 1) / 2."""
        require_device(latent)
        latent = _f32c(latent)
        B, Cc, h, w = latent.shape
        if Cc != self.latent_channels:
            raise NopeError(f"VAE decode: latent {tuple(latent.shape)} (needs {self.latent_channels} channels)")
        shape = (B, self.out_channels, h * self.factor, w * self.factor)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=latent.device)
        assert out.is_contiguous() and tuple(out.shape) == shape and out.dtype == torch.float32
        if B == 0:
            return out
        ws = self._workspace(latent, 1, B, h, w)
        self._l.check(self._l.dll.nope_vae_decode(self._h, _ptr(latent), B, h, w, _ptr(out), int(unnormalize), _ptr(ws), ws.numel(),
                                                  _stream(latent)), "nope_vae_decode")
        return out


# --------------------------------------------------------------------------------------------
# operator-level wrappers (parity tests of single blocks; NCHW f32 in/out at the boundary)
# --------------------------------------------------------------------------------------------
def to_nhwc(x: torch.Tensor, dt: int) -> torch.Tensor:
    x = _f32c(x)
    n, c, h, w = x.shape
    y = torch.empty((n, h, w, c), dtype=torch_dtype(dt), device=x.device)
    l = lib()
    l.check(l.dll.nope_op_nchw_to_nhwc(storage_code(dt), _ptr(x), _ptr(y), n, c, h * w, _stream(x)), "nchw_to_nhwc")
    return y


def to_nchw(y: torch.Tensor, dt: int) -> torch.Tensor:
    n, h, w, c = y.shape
    x = torch.empty((n, c, h, w), dtype=torch.float32, device=y.device)
    l = lib()
    l.check(l.dll.nope_op_nhwc_to_nchw(storage_code(dt), _ptr(y), _ptr(x), n, c, h * w, _stream(y)), "nhwc_to_nchw")
    return x


def pack_conv_weight(w: torch.Tensor, dt: int, mode: int = CONV_PLAIN) -> Tuple[torch.Tensor, int, int]:
    w = _f32c(w)
    cout = w.shape[0]
    if mode == CONV_DOWN2:
        cin, ntaps = w.shape[1] // 4, 4
    elif mode == CONV_UP2P:
        cin, ntaps = w.shape[1], 4
    else:
        cin, ntaps = w.shape[1], w.shape[2] * w.shape[3]
    if dt == F16X2:      # the f16 + MX-fp8 tile's layout (ping-pong kernels): 4 bytes per weight + a 16-byte tail with the layer's block scale
        out = torch.empty((4 if mode == CONV_UP2P else 1) * cout * ntaps * cin + 4, dtype=torch.float32, device=w.device)
    else:
        out = torch.empty((4 if mode == CONV_UP2P else 1, cout, ntaps, cin), dtype=torch_dtype(dt), device=w.device)
    l = lib()
    l.check(l.dll.nope_op_pack_conv_weight(dt, _ptr(w), _ptr(out), cout, cin, ntaps, mode, _stream(w)), "pack_conv_weight")
    return out, cin, ntaps


def _op_struct(cls, fields):
    """A zeroed ConvOp / GnOp with struct_size and the named fields set; a tensor goes in as its data pointer, None as NULL."""
    op = cls(struct_size=C.sizeof(cls))
    for k, v in fields.items():
        setattr(op, k, _ptr(v) if isinstance(v, torch.Tensor) else v)
    return op


def _conv_call(stream: int, **fields) -> bool:
    """nope_op_conv on these fields of nope_conv_op; whether the launch recorded its range maximum."""
    l, rec = lib(), _i(0)
    l.check(l.dll.nope_op_conv(C.byref(_op_struct(ConvOp, fields)), C.byref(rec), stream), "nope_op_conv")
    return bool(rec.value)


def _conv_query(**fields) -> ConvOpInfo:
    """nope_op_conv_query: a pure host call, pointers count as NULL / non-NULL only."""
    l, info = lib(), ConvOpInfo()
    l.check(l.dll.nope_op_conv_query(C.byref(_op_struct(ConvOp, fields)), C.byref(info)), "nope_op_conv_query")
    return info


def _conv_setup(dt, src1, w, bias, src2, mode, rep1, n_hyp, out_nchw, out_dtype, split_k, x2_shift=0):
    """What the conv wrappers set up alike: the packed weight (x2_shift poked into it), the shapes, the output tensor, the f32 bias and -- split_k
    -- the scratch the launcher asks for; `op` holds them under the names of nope_conv_op's fields."""
    pw, cin, ntaps = pack_conv_weight(w, dt, mode)
    if x2_shift:
        assert dt == F16X2
        pw.view(torch.int32)[-1] = int(x2_shift)
    n1, hs, ws, c1 = src1.shape
    c2 = 0 if src2 is None else src2.shape[3]
    assert c1 + c2 == cin
    n_hyp = n_hyp if n_hyp is not None else n1 * rep1
    ho, wo = (2 * hs, 2 * ws) if mode in (CONV_UP2, CONV_UP2P) else ((hs // 2, ws // 2) if mode in (CONV_DOWN2, CONV_STRIDE2, CONV_STRIDE2_PAD01) else (hs, ws))
    cout = w.shape[0]
    if out_nchw:
        out = torch.empty((n_hyp, cout, ho, wo), dtype=torch_dtype(out_dtype), device=src1.device)
    else:
        out = torch.empty((n_hyp, ho, wo, cout), dtype=torch_dtype(dt), device=src1.device)
    op = dict(dtype=dt, src1=src1, C1=c1, rep1=rep1, src2=src2, C2=c2, Hs=hs, Ws=ws, mode=mode, ntaps=ntaps, w_packed=pw, out=out, Cout=cout,
              n_hyp=n_hyp)
    scratch, sk = None, 0
    if split_k:      # (asked of the shape alone; a scratch the launch with all its arguments finds too small means no split)
        sk = int(_conv_query(**op).splitk_bytes)
        if sk:
            scratch = torch.empty(sk, dtype=torch.uint8, device=src1.device)
    op.update(bias=None if bias is None else _f32c(bias), out_nchw=int(out_nchw), out_dtype=out_dtype, splitk_ws=scratch, splitk_bytes=sk)
    return SimpleNamespace(op=op, ntaps=ntaps, hs=hs, ws=ws, ho=ho, wo=wo, cout=cout, n_hyp=n_hyp, out=out)


def _amax_scratch(dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(range slot, one float) for an entry that reports max |.| of what it wrote (include/nope_hip.h: RANGE SLOTS; the entry clears the slot)."""
    return (torch.empty(lib().dll.nope_op_amax_slot_words(), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))


def op_conv(dt: int, src1: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
            src2: Optional[torch.Tensor] = None, mode: int = CONV_PLAIN, rep1: int = 1, rep2: int = 1,
            resid: Optional[torch.Tensor] = None, n_hyp: Optional[int] = None, out_nchw: bool = False,
            out_dtype: int = F32, act_relu: bool = False, split_k: bool = False, x2_shift: int = 0) -> torch.Tensor:
    """src* NHWC tensors of dtype dt; w torch Conv2d weight (f32).  Returns NHWC (or NCHW).  split_k: hand the launcher the scratch it
    asks for (as the U-Net / encoder runtimes do), so shapes it would split along K (few tiles, long K) are.  x2_shift (F16X2 only): the
    activation range shift t of the packed layer (word 3 of the pack's tail; include/nope_hip.h: full accuracy for 2^(t-4) <= |a| <= 1792 2^t)."""
    s = _conv_setup(dt, src1, w, bias, src2, mode, rep1, n_hyp, out_nchw, out_dtype, split_k, x2_shift)
    _conv_call(_stream(src1), rep2=rep2, resid=resid, act_relu=int(act_relu), **s.op)
    return s.out


_ANY = C.c_int(0)      # a query's stand-in for a tensor that exists: its address, never read


def op_conv_stat_rows(dt: int, c1: int, c2: int, rep1: int, hs: int, ws: int, mode: int, ntaps: int, cout: int, n_hyp: int,
                      resid: bool = False, out_nchw: bool = False, act_relu: bool = False) -> int:
    """Rows per block of the fused column statistics a conv of this shape emits under the launch policy in force (0: none)."""
    some = C.addressof(_ANY)
    return int(_conv_query(dtype=dt, src1=some, C1=c1, rep1=rep1, src2=some if c2 else None, C2=c2, Hs=hs, Ws=ws, mode=mode, ntaps=ntaps,
                           w_packed=some, resid=some if resid else None, out=some, Cout=cout, n_hyp=n_hyp, out_nchw=int(out_nchw),
                           act_relu=int(act_relu)).stat_rows)


def prenorm_fold(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, dt: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """A GroupNorm(1, C) in front of a 1x1 conv, folded for ConvArgs::pn_*: (W', c0, c1) with W'[n, c] = W[n, c] gamma[c], c0[n] =
    sum_c W[n, c] beta[c], c1[n] = sum_c W'[n, c], in float64, then cast to f32.  This is what unet_runtime.hip builds at create time
    (prenorm_qkv: gamma as the packer's per-input-channel scale, c0 = W beta by nope_op_linear's kernel, c1 = launch_rowsum over the PACKED
    rows): c1 is the row sum of W' AS STORED -- rounded to bf16 / f16, or the bf16 (hi, lo) pair of the split-precision modes -- so that the
    mean of a sample cancels against the very weights the matrix cores multiply; the sum here runs over the same rounded values."""
    w64 = w.double().reshape(w.shape[0], w.shape[1], -1)         # (a k x k weight folds the same way; the launcher takes 1x1 only)
    wg = (w64 * gamma.double()[None, :, None]).float().reshape(w.shape[0], -1)
    c0 = (w64 * beta.double()[None, :, None]).sum((1, 2)).float()
    if dt in (BF16, F16):
        stored = wg.to(torch_dtype(dt)).double()
    elif dt in (BF16X3, F16X2):
        hi = wg.to(torch.bfloat16)
        stored = hi.double() + (wg - hi.float()).to(torch.bfloat16).double()
    else:
        stored = wg.double()
    return wg.reshape(w.shape).contiguous(), c0.contiguous(), stored.sum(1).float().contiguous()


def op_conv_ex(dt: int, src1: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
               src2: Optional[torch.Tensor] = None, mode: int = CONV_PLAIN, rep1: int = 1, rep2: int = 1,
               resid: Optional[torch.Tensor] = None, n_hyp: Optional[int] = None, out_nchw: bool = False,
               out_dtype: int = F32, act_relu: bool = False, split_k: bool = False, colstats: Optional[torch.Tensor] = None,
               stat_rows: int = 0, prenorm: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, want_amax: bool = False):
    """op_conv with the fusion plumbing of nope_conv_op: `colstats` (an f32 tensor of at least [M / stat_rows][Cout][2] values, written in place) with
    `stat_rows` as op_conv_stat_rows answered; prenorm = (ms [n_hyp][2], gamma, beta): the conv reads the UN-normalised tensor and applies
    GroupNorm(1) in its epilogue (prenorm_fold); want_amax: returns (out, max |out| as the launch recorded it, whether it did record).
    A combination the launcher refuses raises NopeError."""
    pn = (None, None, None)
    if prenorm is not None:
        ms, gamma, beta = prenorm
        w, c0, c1 = prenorm_fold(w.cpu(), gamma.cpu(), beta.cpu(), dt)
        pn = (_f32c(ms), c0.to(src1.device), c1.to(src1.device))
        w = w.to(src1.device)
    s = _conv_setup(dt, src1, w, bias, src2, mode, rep1, n_hyp, out_nchw, out_dtype, split_k)
    if colstats is not None:
        assert colstats.dtype == torch.float32 and colstats.is_contiguous()
        assert stat_rows <= 0 or colstats.numel() >= (s.n_hyp * s.ho * s.wo // stat_rows) * s.cout * 2
    slot, amax = _amax_scratch(src1.device) if want_amax else (None, None)
    rec = _conv_call(_stream(src1), rep2=rep2, resid=resid, act_relu=int(act_relu), colstats=colstats, stat_rows=int(stat_rows),
                     pn_ms=pn[0], pn_c0=pn[1], pn_c1=pn[2], amax_slot=slot, amax_out=amax, **s.op)
    if want_amax:
        return s.out, float(amax.item()), rec
    return s.out


def op_conv_gn_tail(dt: int, src1: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], resid: torch.Tensor, colstats: torch.Tensor,
                    gamma: torch.Tensor, beta: torch.Tensor, groups: int, src2: Optional[torch.Tensor] = None, eps: float = 1e-5,
                    in_place: bool = False, tail_stats: bool = False, want_amax: bool = False, x2_shift: int = 0):
    """conv1x1(src1 [cat src2]) + bias + SiLU(GroupNorm(groups)(resid)) in the conv's epilogue (nope_conv_op's GroupNorm tail, include/nope_hip.h);
    colstats [n][blocks][Cout][2]: resid's column statistics over blocks of 64 rows.  in_place: resid (a copy of it) is also the output buffer,
    as the U-Net runtime launches it.  Returns out, or (out, extras) with extras["tail_stats"] [n][op_conv_tail_stat_blocks][2] / extras["amax"]."""
    s = _conv_setup(dt, src1, w, bias, src2, CONV_PLAIN, 1, None, False, F32, False, x2_shift)
    assert s.ntaps == 1 and tuple(resid.shape) == tuple(s.out.shape) and resid.dtype == torch.float32 and resid.is_contiguous()
    assert colstats.dtype == torch.float32 and colstats.is_contiguous() and tuple(colstats.shape[::3]) == (s.n_hyp, 2) and colstats.shape[2] == s.cout
    if in_place:
        s.out.copy_(resid)
        resid = s.out
    ms = torch.empty((s.n_hyp, groups, 2), dtype=torch.float32, device=src1.device)
    ts = None
    if tail_stats:
        ts = torch.zeros((s.n_hyp, int(_conv_query(**s.op).tail_stat_blocks), 2), dtype=torch.float32, device=src1.device)
    slot, amax = _amax_scratch(src1.device) if want_amax else (None, None)
    _conv_call(_stream(src1), resid=resid, tail_colstats=colstats, tail_stat_blocks=colstats.shape[1], gn_gamma=_f32c(gamma), gn_beta=_f32c(beta),
               gn_G=groups, gn_eps=float(eps), gn_ms=ms, tail_stats=ts, amax_slot=slot, amax_out=amax, **s.op)
    if not (tail_stats or want_amax):
        return s.out
    extras = {"ms": ms}
    if tail_stats:
        extras["tail_stats"] = ts
    if want_amax:
        extras["amax"] = float(amax.item())
    return s.out, extras


def op_conv_gn_self(dt: int, src1: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                    emb: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, src2: Optional[torch.Tensor] = None, eps: float = 1e-5,
                    split_k: bool = False, want_amax: bool = False, x2_shift: int = 0, out: Optional[torch.Tensor] = None):
    """SiLU(GroupNorm(groups)(conv3x3(src1 [cat src2]) + bias)) [+ emb[sample]] [+ resid] in ONE launch (nope_conv_op's gn_self, include/nope_hip.h):
    the conv forms the statistics of its own output.  A combination the launcher refuses raises NopeError (NOPE_ERR_UNSUPPORTED) with nothing
    launched; `out` (optional) is the buffer to write, so a caller can see that a refusal left it alone.  Returns out, or (out, max |out|)."""
    s = _conv_setup(dt, src1, w, bias, src2, CONV_PLAIN, 1, None, False, F32, split_k, x2_shift)
    if out is not None:
        assert tuple(out.shape) == tuple(s.out.shape) and out.dtype == s.out.dtype and out.is_contiguous()
        s.op["out"] = out
    e = None if emb is None else _f32c(emb)
    slot, amax = _amax_scratch(src1.device) if want_amax else (None, None)
    _conv_call(_stream(src1), resid=resid, gn_gamma=_f32c(gamma), gn_beta=_f32c(beta), gn_G=groups, gn_eps=float(eps), gn_self=1, gn_emb=e,
               gn_emb_stride=0 if e is None else e.shape[1], amax_slot=slot, amax_out=amax, **s.op)
    res = s.op["out"]
    return (res, float(amax.item())) if want_amax else res


def op_gn_apply_blocks(dt: int, hw: int, c: int, n_hyp: int) -> int:
    """Workgroups per hypothesis of a GroupNorm apply launch = chunks per hypothesis of its out_stats."""
    return int(lib().dll.nope_op_gn_apply_blocks(storage_code(dt), hw, c, n_hyp))


def _gn_run(dt, y, partial_rows, groups, gamma, beta, act_silu, emb, out_stats, want_amax, **fields):
    """What the GroupNorm wrappers do alike around nope_op_group_norm, into y NHWC [n_hyp][h][w][C]: the `partial` scratch (partial_rows x groups
    (sum, sum of squares) pairs; 0: none), out_stats and the range slot when asked for, the call, and the return value: y, or (y, extras)."""
    n, h, w, c = y.shape
    g, b = _f32c(gamma), _f32c(beta)
    e = None if emb is None else _f32c(emb)
    partial = torch.empty((partial_rows, groups, 2), dtype=torch.float32, device=y.device) if partial_rows else None
    os_ = torch.empty((n, op_gn_apply_blocks(dt, h * w, c, n), 2), dtype=torch.float32, device=y.device) if out_stats else None
    slot, amax = _amax_scratch(y.device) if want_amax else (None, None)
    op = _op_struct(GnOp, dict(fields, dtype=dt, y=y, partial=partial, gamma=g, beta=b, n_hyp=n, H=h, W=w, C=c, G=groups, act_silu=int(act_silu), emb=e,
                               emb_stride=0 if e is None else e.shape[1], out_stats=os_, amax_slot=slot, amax_out=amax))
    l = lib()
    l.check(l.dll.nope_op_group_norm(C.byref(op), _stream(y)), "nope_op_group_norm")
    if not (out_stats or want_amax):
        return y
    extras = {}
    if out_stats:
        extras["out_stats"] = os_
    if want_amax:
        extras["amax"] = float(amax.item())
    return y, extras


def op_group_norm(dt: int, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, act_silu: bool = False,
                  emb: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None) -> torch.Tensor:
    n, h, w, c = x.shape
    dt = storage_code(dt)
    return _gn_run(dt, torch.empty_like(x), n * lib().dll.nope_op_gn_chunks(dt, h * w, c), groups, gamma, beta, act_silu, emb, False, False,
                   x=x, resid=resid, eps=1e-5)


def op_group_norm_ex(dt: int, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, act_silu: bool = False,
                     emb: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, film: Optional[torch.Tensor] = None,
                     colstats: Optional[torch.Tensor] = None, fold_launch: bool = False, x_rep: int = 1, resid_rep: int = 1,
                     out_stats: bool = False, eps: float = 1e-5, fast_silu: bool = False, want_amax: bool = False):
    """op_group_norm with the fusion plumbing of nope_gn_op (include/nope_hip.h).  x NHWC [n_x][h][w][C], n_hyp = n_x * x_rep; emb (n_hyp, C);
    resid NHWC of n_hyp / resid_rep samples; film (n_hyp, 2 C) = one [scale | shift] row per hypothesis, or (2 C,) = one row for all;
    colstats [n_x][blocks][C][2] f32 column statistics instead of a statistics pass (fold_launch: folded by its own launch).
    Returns y, or (y, extras) with extras["out_stats"] [n_hyp][op_gn_apply_blocks][2] / extras["amax"] when asked for."""
    nx, h, w, c = x.shape
    dt = storage_code(dt)
    f = None if film is None else _f32c(film)
    if colstats is not None:
        assert colstats.dtype == torch.float32 and colstats.is_contiguous() and tuple(colstats.shape[::3]) == (nx, 2) and colstats.shape[2] == c
        rows = nx if fold_launch else 0      # (`partial`: the fold launch's output; none when every workgroup folds for itself)
    else:
        rows = nx * lib().dll.nope_op_gn_chunks(dt, h * w, c)
    y = torch.empty((nx * x_rep, h, w, c), dtype=x.dtype, device=x.device)
    return _gn_run(dt, y, rows, groups, gamma, beta, act_silu, emb, out_stats, want_amax, x=x, colstats=colstats,
                   stat_blocks=0 if colstats is None else colstats.shape[1], fold_launch=int(fold_launch), film=f,
                   film_stride=0 if f is None or f.dim() == 1 else f.shape[1], resid=resid, x_rep=x_rep, resid_rep=resid_rep, eps=float(eps),
                   fast_silu=int(fast_silu))


def op_group_norm_shared(dt: int, x: Optional[torch.Tensor], sh_s: torch.Tensor, sh_e: Optional[torch.Tensor], gamma: torch.Tensor,
                         beta: torch.Tensor, groups: int, n_hyp: int, act_silu: bool = True, emb: Optional[torch.Tensor] = None,
                         resid: Optional[torch.Tensor] = None, resid_rep: int = 1, out_stats: bool = False, eps: float = 1e-5,
                         fast_silu: bool = False, want_amax: bool = False):
    """GroupNorm of x_eff = x + sh_s[j / sh_rep] + sh_e[j][border class of the pixel]: nope_gn_op's shared addend (include/nope_hip.h).
    sh_s f32 NHWC [n_s][h][w][C] shared by n_hyp / n_s consecutive hypotheses; sh_e f32 (n_hyp, 9, C) or None; x NHWC [n_hyp][h][w][C] of
    the storage type, or None.  Returns y (storage type), or (y, extras) as op_group_norm_ex."""
    ns, h, w, c = sh_s.shape
    assert sh_s.dtype == torch.float32 and sh_s.is_contiguous() and n_hyp % ns == 0
    assert sh_e is None or (sh_e.dtype == torch.float32 and sh_e.is_contiguous() and tuple(sh_e.shape) == (n_hyp, 9, c))
    assert x is None or (tuple(x.shape) == (n_hyp, h, w, c) and x.is_contiguous())
    dt = storage_code(dt)
    y = torch.empty((n_hyp, h, w, c), dtype=torch_dtype(dt), device=sh_s.device)
    return _gn_run(dt, y, n_hyp * lib().dll.nope_op_gn_chunks(dt, h * w, c), groups, gamma, beta, act_silu, emb, out_stats, want_amax, x=x,
                   sh_s=sh_s, sh_rep=n_hyp // ns, sh_e=sh_e, resid=resid, resid_rep=resid_rep, eps=float(eps), fast_silu=int(fast_silu))


def op_conv_class_weights(w: torch.Tensor) -> torch.Tensor:
    """The nine border-class weights [9][Cout][Cin] f32 of a 3x3 conv weight [Cout][Cin][3][3] (nope_op_conv_class_weights)."""
    require_device(w)
    w = _f32c(w)
    cout, cin = w.shape[:2]
    assert tuple(w.shape[2:]) == (3, 3)
    out = torch.empty((9, cout, cin), dtype=torch.float32, device=w.device)
    l = lib()
    l.check(l.dll.nope_op_conv_class_weights(_ptr(w), _ptr(out), cout, cin, _stream(w)), "nope_op_conv_class_weights")
    return out


def op_gn_finalize(partial: torch.Tensor, count: float, eps: float = 1e-5) -> torch.Tensor:
    """partial [n][chunks][2] (sum, sum of squares) pairs of whole samples -> [n][2] (mean, rstd) of GroupNorm(1) over `count` values."""
    partial = _f32c(partial)
    n, nch, _ = partial.shape
    ms = torch.empty((n, 2), dtype=torch.float32, device=partial.device)
    l = lib()
    l.check(l.dll.nope_op_gn_finalize(_ptr(partial), _ptr(ms), n, nch, float(count), float(eps), _stream(partial)), "nope_op_gn_finalize")
    return ms


def op_absmax(x: torch.Tensor) -> float:
    """max |x| of an f32 tensor as the range tracking computes it (NaNs ignored)."""
    require_device(x)
    x = _f32c(x).reshape(-1)
    slot, amax = _amax_scratch(x.device)
    l = lib()
    l.check(l.dll.nope_op_absmax_f32(_ptr(x), x.numel(), _ptr(slot), _ptr(amax), _stream(x)), "nope_op_absmax_f32")
    return float(amax.item())


def op_linear_attention(dt: int, qkv: torch.Tensor, heads: int = 4, dim_head: int = 32, full: bool = False) -> torch.Tensor:
    n, h, w, c3 = qkv.shape
    out = torch.empty((n, h, w, heads * dim_head), dtype=qkv.dtype, device=qkv.device)
    l = lib()
    fn = l.dll.nope_op_attention if full else l.dll.nope_op_linear_attention
    l.check(fn(storage_code(dt), _ptr(qkv), _ptr(out), n, h * w, heads, dim_head, _stream(qkv)), "nope_op_attention")
    return out


def op_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act_in: int = 0) -> torch.Tensor:
    x, w = _f32c(x), _f32c(w)
    b = None if bias is None else _f32c(bias)
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    l = lib()
    l.check(l.dll.nope_op_linear(_ptr(x), _ptr(w), _ptr(b), _ptr(out), x.shape[0], w.shape[0], x.shape[1], act_in,
                                 _stream(x)), "nope_op_linear")
    return out
