"""The module side of the device handles: what the five `nn.Module` wrappers (FeatureExtractor, VAE_StableDiffusion, UNet and the two
UNetModelPose) do alike around their `hip.*Handle` -- build it on first use, key it on the weights, drop it when they change.

Mixins only: no parameter, no buffer, no state-dict key.
"""
from __future__ import annotations

import torch

from . import hip


class HandleCache:
    """The cached device handle of a module.  The class supplies `_versioned_tensors()` (which tensors the handle was built from),
    `_make_handle(device)` and, if more than device / compute_dtype / weights decides, `_handle_key_extra()`; its __init__ calls
    `_init_handle_cache()`."""
    _cache_versioned_tensors = True      # the module tree is fixed after __init__: walk it once per invalidate(), not once per forward

    def _init_handle_cache(self):
        self._handle = None
        self._handle_key = None
        # nn.Module.load_state_dict on a PARENT (UNet, PoseConditional, a Lightning module) never calls a child's load_state_dict (it
        # recurses through _load_from_state_dict), but it does run every sub-module's post hooks: drop the repacked device copy there.
        self.register_load_state_dict_post_hook(lambda mod, _keys: mod.invalidate())

    def invalidate(self):
        """Drop the folded / repacked device weights; the next device call rebuilds them.  Called automatically after any load_state_dict
        that reaches this module and when a tensor was modified in place."""
        self._handle = None
        self.__dict__.pop("_own_tensors", None)      # the cached tensor list: parameters may have been re-assigned (load_state_dict(assign=True))

    def _handle_key_extra(self) -> tuple:
        return ()

    def _weights_version(self):
        """Key of the repacked device copy: (storage address, version counter) of every versioned tensor.  In-place writes through the
        tensor itself (optimizer steps, `p.copy_`, `p.mul_`) bump `_version`, re-assigned storage moves `data_ptr`; writes through `p.data`
        have their own counter and are NOT seen -- call `invalidate()` after those (EMA swaps, hand-written checkpoint loaders);
        `load_state_dict` on the module or any parent invalidates by itself.  With the list cached a forward pays ~40 us for the ~420
        tensors of the U-Net, not a named_parameters walk."""
        ts = self.__dict__.get("_own_tensors")
        if ts is None:
            ts = self._versioned_tensors()
            if self._cache_versioned_tensors:
                self.__dict__["_own_tensors"] = ts
        return hash(tuple((t.data_ptr(), t._version) for t in ts))

    def _get_handle(self, device):
        key = (str(device), self.compute_dtype, *self._handle_key_extra(), self._weights_version())
        if self._handle is None or self._handle_key != key:
            self._handle = self._make_handle(device)
            self._handle_key = key
        return self._handle


class HypothesisNetwork(HandleCache):
    """The call surface of the pose-conditioned networks `PoseConditional` drives (`self.encoder` is not theirs: its keys are left out and
    it is invalidated with them)."""

    def own_state_dict(self):
        """The network's own tensors (no `encoder.*`), keyed as in the reference."""
        return {k: v for k, v in self.state_dict().items() if not k.startswith("encoder.")}

    def invalidate(self):
        """As HandleCache.invalidate; also the encoder's."""
        super().invalidate()
        inv = getattr(self.encoder, "invalidate", None)
        if callable(inv):
            inv()

    def _versioned_tensors(self):
        return [p for n, p in self.named_parameters(recurse=True) if not n.startswith("encoder.")]

    @torch.no_grad()
    def forward(self, x, pose):
        """x (B,C,h,w), pose (B,rot_dim) -> (B,C_out,h,w) f32."""
        return self._get_handle(x.device).forward(x, pose, x_rep=1)

    @torch.no_grad()
    def forward_hypotheses(self, x, poses, out=None, out_dtype="f32", defer_range_check=False):
        """x (B,C,h,w) reference embeddings, poses (B,N,rot_dim) -> (B,N,C,h,w): net(x[b], poses[b,n]) for every (b,n) -- the body of the
        template loop model.py:212-222 -- as one batched launch sequence.  defer_range_check (f16x2): the caller calls
        finish_range_check() before it reads the output."""
        B, N = poses.shape[:2]
        flat = poses.reshape(B * N, poses.shape[-1])
        o = None if out is None else out.view(B * N, *out.shape[2:])
        y = self._get_handle(x.device).forward(x, flat, x_rep=N, out=o, out_dtype=hip.dtype_code(out_dtype), defer_range_check=defer_range_check)
        return y.view(B, N, *y.shape[1:])

    def finish_range_check(self) -> bool:
        """f16x2: check (and if needed repeat) the forwards issued with defer_range_check; True when any was repeated (hip: the handles'
        finish_range_check)."""
        return self._handle.finish_range_check() if self._handle is not None else False
