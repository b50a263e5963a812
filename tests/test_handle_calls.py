"""CPU: what the five network handles of nope_amd.hip hand to the C ABI, call by call, against a recording fake of the library.

No library and no interpreter: `hip._set_library_for_testing` gets a NopeLib whose `dll` answers every symbol with a recorder.  Each call is
recorded as (symbol, arguments): scalars as they are, config structs as dicts of their fields, pointers as None / "ptr", the stream as its
number and the handle as "h<n>" -- the n-th handle a `*_create` handed out (any other value there fails the comparison).  The expected
lists are literal; they were recorded on the commit before the handle classes were put on one base and must not change with it.
"""
import ctypes as C
import warnings

import pytest
import torch

from nope_amd import hip

ERR_RANGE, ERR_RANGE_F16 = hip.ERR_RANGE, hip.ERR_RANGE_F16
_STREAM_ARG = {"create": 3, "forward": -1, "encode": -1, "decode": -1, "x2_range_check": 1, "x2_poll": 1}     # by entry: the stream's position
_QUIET = ("nope_tuning_reload", "nope_strerror")      # bookkeeping of hip.lib() / NopeLib.check: not part of a handle's calls


class _Fake:
    def __init__(self):
        self.calls, self.handles = [], []
        self.verdicts = {"x2_range_check": [], "x2_poll": []}      # scripted (code, bad, moved, amax); (0, 0, 0, 0.0) when empty
        self.forced = {}                                            # entry -> what it returns instead of doing anything

    def __getattr__(self, name):
        if not name.startswith("nope_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _reduce(self, name, args):
        types = hip._PROTOS[name][1]
        assert len(args) == len(types), (name, len(args), len(types))
        entry = name.split("_", 2)[2]
        at = _STREAM_ARG.get(entry)
        at = at if at is None or at >= 0 else len(args) + at
        out = []
        for i, (a, ty) in enumerate(zip(args, types)):
            pointer = ty is C.c_void_p or issubclass(ty, C._Pointer)
            if isinstance(a, C.c_void_p):
                out.append(f"h{self.handles.index(a.value)}" if a.value in self.handles else f"?{a.value}")
            elif i == at:
                out.append(int(a))
            elif type(a).__name__ == "CArgObject" and isinstance(a._obj, C.Structure):
                out.append({f: (list(v) if hasattr(v, "__len__") else v) for f, _ in a._obj._fields_ for v in [getattr(a._obj, f)]})
            elif pointer:
                out.append(None if a is None else "ptr")
            else:
                out.append(a)
        return tuple(out)

    def _call(self, name, args):
        if name == "nope_strerror":
            return b"scripted"
        if name not in _QUIET:
            self.calls.append((name,) + self._reduce(name, args))
        entry = name.split("_", 2)[2]
        if entry in self.forced:
            return self.forced[entry]
        if entry == "create":
            self.handles.append(0x1000 + 16 * len(self.handles))
            args[-1]._obj.value = self.handles[-1]
        elif entry == "workspace_bytes":
            return 256 + 16 * sum(int(a) for a in args[1:])
        elif entry in self.verdicts:
            code, bad, moved, amax = self.verdicts[entry].pop(0) if self.verdicts[entry] else (0, 0, 0, 0.0)
            args[2]._obj.value, args[3]._obj.value, args[4]._obj.value = bad, moved, amax
            return code
        return 0

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def fake():
    before = (hip._lib, hip._tuning_seen)
    f = _Fake()
    l = hip.NopeLib.__new__(hip.NopeLib)
    l.path, l.dll = "<recording fake>", f
    hip._set_library_for_testing(l)
    yield f
    hip._lib, hip._tuning_seen = before


UNET_CFG = dict(u_net_dim=32, channels=4, pose_dim=6, dim_mults=(1, 2), pose_mlp_layers=2, soft_up_down=1)
LDM_CFG = dict(in_channels=4, model_channels=32, out_channels=5, num_res_blocks=1, num_head_channels=0, context_dim=24, pose_dim=6, pose_mlp_layers=1,
               injecting_condition_twice=1, channel_mult=(1, 2), attn_levels=(1, 0), head_channels=(32, 64), resblock_updown=1, conv_resample=0)
GD_CFG = dict(in_channels=4, model_channels=32, out_channels=5, num_res_blocks=2, head_channels_mid=64, pose_dim=6, pose_mlp=2, new_attention_order=1,
              resblock_updown=0, conv_resample=1, use_scale_shift_norm=1, channel_mult=(1, 2, 2), attn_levels=(0, 1, 1), head_channels_in=(32, 64, 64),
              head_channels_out=(32, 32, 64))
VAE_CFG = dict(in_channels=3, out_channels=3, block_out_channels=(32, 64), layers_per_block=1, latent_channels=4, norm_num_groups=32)
SD = {"backbone.w": torch.zeros(2, 3), "projector.b": torch.zeros(3), "other.w": torch.zeros(1)}      # (the encoder keeps two of the three)


def _pad8(*v):
    return list(v) + [0] * (8 - len(v))


UNET_STRUCT = dict(u_net_dim=32, channels=4, out_dim=4, pose_dim=6, n_levels=2, dim_mults=_pad8(1, 2), groups=8, heads=4, dim_head=32,
                   pose_mlp_layers=2, compute_dtype=hip.F32, soft_up_down=1)
LDM_STRUCT = dict(in_channels=4, model_channels=32, out_channels=5, num_res_blocks=1, n_levels=2, channel_mult=_pad8(1, 2), attn_levels=_pad8(1, 0),
                  num_head_channels=0, context_dim=24, pose_dim=6, pose_mlp_layers=1, injecting_condition_twice=1, compute_dtype=hip.F32,
                  use_scale_shift_norm=0, transformer_depth=1, head_channels=_pad8(32, 64), resblock_updown=1, conv_resample=0)
GD_STRUCT = dict(in_channels=4, model_channels=32, out_channels=5, num_res_blocks=2, n_levels=3, channel_mult=_pad8(1, 2, 2), attn_levels=_pad8(0, 1, 1),
                 head_channels_in=_pad8(32, 64, 64), head_channels_out=_pad8(32, 32, 64), head_channels_mid=64, pose_dim=6, pose_mlp=2,
                 new_attention_order=1, resblock_updown=0, conv_resample=1, use_scale_shift_norm=1, compute_dtype=hip.F32)
VAE_STRUCT = dict(in_channels=3, out_channels=3, n_levels=2, block_out_channels=_pad8(32, 64), layers_per_block=1, latent_channels=4, norm_num_groups=32,
                  compute_dtype=hip.BF16, gn_eps=C.c_float(1e-6).value)
ENCODER_STRUCT = dict(descriptor_size=16, compute_dtype=hip.F32, bn_eps=C.c_float(1e-3).value)

HYP = {   # stem: (handle class name, cfg, config struct as the library sees it, output channels)
    "unet": ("UNetHandle", UNET_CFG, UNET_STRUCT, 4),
    "ldm": ("LdmHandle", LDM_CFG, LDM_STRUCT, 5),
    "gd": ("GdHandle", GD_CFG, GD_STRUCT, 5),
}


def _hyp_handle(stem, dt=hip.F32):
    name, cfg, _, _ = HYP[stem]
    return getattr(hip, name)(cfg, SD, dt)


def _xp(side, n_hyp=2):
    return torch.zeros(1, 4, side, side), torch.zeros(n_hyp, 6)


def _arena_walk(monkeypatch, h, steps, second):
    """steps: three callables (small, large, small again); second: a handle of the same kind for the other stream.  Returns the arena sizes
    after each step; asserts one allocation per growth, reuse afterwards and an arena of its own per stream key."""
    key = ("cpu", 0)
    seen = []
    for step in steps:
        step(h)
        seen.append(h._ws[key])
    assert seen[0] is not seen[1] and seen[1] is seen[2] and list(h._ws) == [key]
    with monkeypatch.context() as m:
        m.setattr(hip, "_stream", lambda t: 7)
        steps[0](h)
        steps[0](second)
    assert list(h._ws) == [key, ("cpu", 7)] and h._ws[key] is seen[1] and list(second._ws) == [("cpu", 7)]
    assert second._ws[("cpu", 7)] is not h._ws[("cpu", 7)]
    return [t.numel() for t in seen] + [h._ws[("cpu", 7)].numel(), second._ws[("cpu", 7)].numel()]


# ---- (a) life cycle of each handle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", ["unet", "ldm", "gd"])
def test_hypothesis_handle_life_cycle(fake, monkeypatch, stem):
    _, _, struct, cout = HYP[stem]
    h, h2 = _hyp_handle(stem), _hyp_handle(stem)
    assert fake.take() == [(f"nope_{stem}_create", struct, "ptr", 3, 0, "ptr")] * 2
    assert (h.device, h.compute_dtype, h.pose_dim, h.range_mode, h.x2_enabled, h.range_events) == (torch.device("cpu"), hip.F32, 6, "off", False, [])
    if stem == "unet":
        assert (h.channels, h.out_dim, h.cfg) == (4, 4, UNET_CFG)
    else:
        assert (h.in_channels, h.out_channels) == (4, 5)

    def step(side):
        def run(hh):
            x, pose = _xp(side)
            y = hh.forward(x, pose, x_rep=2)
            assert tuple(y.shape) == (2, cout, side, side) and y.dtype == torch.float32
        return run
    sizes = _arena_walk(monkeypatch, h, [step(4), step(8), step(4)], h2)
    assert sizes == [432, 560, 560, 432, 432]

    def fwd(hn, side, nbytes, stream=0):
        return [(f"nope_{stem}_workspace_bytes", hn, 2, 1, side, side),
                (f"nope_{stem}_forward", hn, "ptr", 1, 2, "ptr", 2, side, side, "ptr", hip.F32, "ptr", nbytes, stream)]
    # (the small forward on the grown arena hands over the arena's size, not the need)
    assert fake.take() == fwd("h0", 4, 432) + fwd("h0", 8, 560) + fwd("h0", 4, 560) + fwd("h0", 4, 432, 7) + fwd("h1", 4, 432, 7)
    del h
    assert fake.take() == [(f"nope_{stem}_destroy", "h0")]
    del h2
    assert fake.take() == [(f"nope_{stem}_destroy", "h1")]


def test_hypothesis_handle_refusals(fake):
    for stem, label in (("unet", "U-Net"), ("ldm", "LDM U-Net"), ("gd", "GD U-Net")):
        h = _hyp_handle(stem)
        with pytest.raises(hip.NopeError, match="shape mismatch"):
            h.forward(*_xp(4, n_hyp=3), x_rep=2)
        fake.forced = {"workspace_bytes": 0}
        with pytest.raises(hip.NopeError, match=f"unsupported {label} problem size n_hyp=2 H=4 W=4"):
            h.forward(*_xp(4), x_rep=2)
        fake.forced = {}
        assert h._ws == {}


def test_create_failure_names_the_entry(fake):
    fake.forced = {"create": -2}
    for cls, args, stem in ((hip.UNetHandle, (UNET_CFG, SD), "unet"), (hip.LdmHandle, (LDM_CFG, SD), "ldm"), (hip.GdHandle, (GD_CFG, SD), "gd"),
                            (hip.VaeHandle, (VAE_CFG, SD), "vae"), (hip.EncoderHandle, (16, SD), "encoder")):
        with pytest.raises(hip.NopeError, match=rf"nope_{stem}_create: scripted \(-2\)"):
            cls(*args)
    # (no destroy of a handle that was never made, when the half-built objects go)
    assert [c[0] for c in fake.take()] == [f"nope_{s}_create" for s in ("unet", "ldm", "gd", "vae", "encoder")]


def test_encoder_handle_life_cycle(fake, monkeypatch):
    h, h2 = hip.EncoderHandle(16, SD, hip.F32, bn_eps=1e-3), hip.EncoderHandle(16, SD, hip.F32, bn_eps=1e-3)
    assert fake.take() == [("nope_encoder_create", ENCODER_STRUCT, "ptr", 2, 0, "ptr")] * 2
    assert (h.device, h.compute_dtype, h.descriptor_size) == (torch.device("cpu"), hip.F32, 16)

    def step(side):
        def run(hh):
            y = hh.forward(torch.zeros(1, 3, side, side))
            assert tuple(y.shape) == (1, 16, side // 8, side // 8) and y.dtype == torch.float32
        return run
    sizes = _arena_walk(monkeypatch, h, [step(8), step(16), step(8)], h2)
    assert sizes == [528, 784, 784, 528, 528]

    def fwd(hn, side, nbytes, stream=0):
        return [("nope_encoder_workspace_bytes", hn, 1, side, side), ("nope_encoder_forward", hn, "ptr", 1, side, side, "ptr", "ptr", nbytes, stream)]
    # (the encoder hands over the NEED, also on a larger arena)
    assert fake.take() == fwd("h0", 8, 528) + fwd("h0", 16, 784) + fwd("h0", 8, 528) + fwd("h0", 8, 528, 7) + fwd("h1", 8, 528, 7)
    del h
    assert fake.take() == [("nope_encoder_destroy", "h0")]
    del h2
    assert fake.take() == [("nope_encoder_destroy", "h1")]


def test_vae_handle_life_cycle(fake, monkeypatch):
    # workspace_bytes of the fake: 256 + 16 (decode + n + H + W): with 5 samples, the largest chunk within 600 bytes is bisected per call
    h, h2 = (hip.VaeHandle(VAE_CFG, SD, hip.BF16, max_workspace_bytes=600) for _ in range(2))
    assert fake.take() == [("nope_vae_create", VAE_STRUCT, "ptr", 3, 0, "ptr")] * 2
    assert (h.device, h.compute_dtype, h.in_channels, h.out_channels, h.latent_channels, h.factor, h.max_workspace_bytes) == \
        (torch.device("cpu"), hip.BF16, 3, 3, 4, 2, 600)

    def step(side):
        def run(hh):
            z = hh.encode(torch.zeros(5, 3, side, side))
            assert tuple(z.shape) == (5, 4, side // 2, side // 2)
            y = hh.decode(torch.zeros(5, 4, side // 2, side // 2), unnormalize=True)
            assert tuple(y.shape) == (5, 3, side, side)
        return run
    sizes = _arena_walk(monkeypatch, h, [step(8), step(16), step(8)], h2)
    assert sizes == [592, 784, 784, 592, 592]

    def ws(hn, decode, side, mids):
        return [("nope_vae_workspace_bytes", hn, decode, n, side, side) for n in [1] + mids]

    def both(hn, side, mids_e, enc_bytes, mids_d, dec_bytes, stream=0):
        return (ws(hn, 0, side, mids_e) + [("nope_vae_encode", hn, "ptr", 5, side, side, "ptr", "ptr", enc_bytes, stream)]
                + ws(hn, 1, side // 2, mids_d) + [("nope_vae_decode", hn, "ptr", 5, side // 2, side // 2, "ptr", 1, "ptr", dec_bytes, stream)])
    # side 8: encode fits all 5 (592 bytes), decode all 5 (480 bytes, on the 592-byte arena); side 16: one sample of the encode alone is over
    # the limit (784 bytes: taken anyway), the decode fits 4 (592 bytes)
    assert fake.take() == (both("h0", 8, [3, 4, 5], 592, [3, 4, 5], 592) + both("h0", 16, [3, 2], 784, [3, 4, 5], 784) + both("h0", 8, [3, 4, 5], 784, [3, 4, 5], 784)
                           + both("h0", 8, [3, 4, 5], 592, [3, 4, 5], 592, 7) + both("h1", 8, [3, 4, 5], 592, [3, 4, 5], 592, 7))
    assert h.encode(torch.zeros(0, 3, 8, 8)).shape[0] == 0 and h.decode(torch.zeros(0, 4, 4, 4)).shape[0] == 0 and fake.take() == []
    del h
    assert fake.take() == [("nope_vae_destroy", "h0")]
    del h2
    assert fake.take() == [("nope_vae_destroy", "h1")]


# ---- (b) f16x2 under NOPE_X2_RANGE_CHECK=2 ("repeat") ---------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", ["unet", "ldm", "gd"])
def test_x2_repeat_mode(fake, monkeypatch, stem):
    monkeypatch.setenv("NOPE_X2_RANGE_CHECK", "2")
    h = _hyp_handle(stem, hip.F16X2)
    fake.take()
    assert (h.range_mode, h.x2_enabled, h.compute_dtype) == ("repeat", True, hip.F16X2)
    x, pose = _xp(4)
    wsb = (f"nope_{stem}_workspace_bytes", "h0", 2, 1, 4, 4)
    fwd = (f"nope_{stem}_forward", "h0", "ptr", 1, 2, "ptr", 2, 4, 4, "ptr", hip.F32, "ptr", 432, 0)
    poll = (f"nope_{stem}_x2_poll", "h0", 0, "ptr", "ptr", "ptr")
    check = (f"nope_{stem}_x2_range_check", "h0", 0, "ptr", "ptr", "ptr")

    # out of range, then clean: the forward is issued twice with the same arguments
    fake.verdicts["x2_range_check"] = [(ERR_RANGE, 2, 1, 5.0), (0, 0, 0, 0.0)]
    h.forward(x, pose, x_rep=2)
    assert fake.take() == [wsb, poll, fwd, check, fwd, check]
    assert h.range_events == [{"code": ERR_RANGE, "layers_out_of_range": 2, "layers_adjusted": 1, "max_abs": 5.0, "attempt": 0}]

    # two deferred forwards, one finish: both are relaunched
    fake.verdicts["x2_range_check"] = [(ERR_RANGE, 1, 1, 9.0), (0, 0, 0, 0.0)]
    h.forward(x, pose, x_rep=2, defer_range_check=True)
    h.forward(x, pose, x_rep=2, defer_range_check=True)
    assert fake.take() == [wsb, poll, fwd, wsb, poll, fwd]
    assert h.finish_range_check() is True
    assert fake.take() == [check, fwd, fwd, check]
    assert h.finish_range_check() is False and fake.take() == []
    assert [e["attempt"] for e in h.range_events] == [0, 0]

    # an earlier forward's verdict arrives with the poll: recorded as attempt -1
    fake.verdicts["x2_poll"] = [(ERR_RANGE, 3, 2, 7.0)]
    h.forward(x, pose, x_rep=2)
    assert fake.take() == [wsb, poll, fwd, check]
    assert h.range_events[-1] == {"code": ERR_RANGE, "layers_out_of_range": 3, "layers_adjusted": 2, "max_abs": 7.0, "attempt": -1}

    # not finite: the two-pass mode is switched off, the forward repeated once, and later forwards make no x2 call
    fake.verdicts["x2_range_check"] = [(ERR_RANGE_F16, 1, 0, float("inf"))]
    with pytest.warns(RuntimeWarning, match="are not finite: this U-Net runs as bf16x3"):
        h.forward(x, pose, x_rep=2)
    assert fake.take() == [wsb, poll, fwd, check, (f"nope_{stem}_x2_enable", "h0", 0), fwd]
    assert h.x2_enabled is False and h.range_events[-1]["code"] == ERR_RANGE_F16 and h.range_events[-1]["attempt"] == 0
    h.forward(x, pose, x_rep=2)
    assert fake.take() == [wsb, fwd]


def test_x2_range_check_error_names_the_entry(fake, monkeypatch):
    monkeypatch.setenv("NOPE_X2_RANGE_CHECK", "2")
    for stem in ("unet", "ldm", "gd"):
        h = _hyp_handle(stem, hip.F16X2)
        fake.verdicts["x2_range_check"] = [(-1, 0, 0, 0.0)]
        with pytest.raises(hip.NopeError, match=rf"nope_{stem}_x2_range_check: scripted \(-1\)"):
            h.x2_range_check(0)


# ---- (c) "auto" ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem,env", [("unet", None), ("ldm", "1"), ("gd", "junk")])
def test_x2_auto_mode(fake, monkeypatch, stem, env):
    if env is None:
        monkeypatch.delenv("NOPE_X2_RANGE_CHECK", raising=False)
    else:
        monkeypatch.setenv("NOPE_X2_RANGE_CHECK", env)
    h = _hyp_handle(stem, hip.F16X2)
    fake.take()
    assert h.range_mode == "auto"
    x, pose = _xp(4)
    wsb = (f"nope_{stem}_workspace_bytes", "h0", 2, 1, 4, 4)
    fwd = (f"nope_{stem}_forward", "h0", "ptr", 1, 2, "ptr", 2, 4, 4, "ptr", hip.F32, "ptr", 432, 0)
    poll = (f"nope_{stem}_x2_poll", "h0", 0, "ptr", "ptr", "ptr")
    check = (f"nope_{stem}_x2_range_check", "h0", 0, "ptr", "ptr", "ptr")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(3):          # settling: one synchronising check each
            h.forward(x, pose, x_rep=2)
            assert fake.take() == [wsb, poll, fwd, check]
        for _ in range(3):          # settled: the poll only
            h.forward(x, pose, x_rep=2)
            assert fake.take() == [wsb, poll, fwd]
        fake.verdicts["x2_poll"] = [(ERR_RANGE, 1, 1, 3.0)]
        h.forward(x, pose, x_rep=2)         # a verdict arrives: the checks are back
        assert fake.take() == [wsb, poll, fwd, check]
        fake.verdicts["x2_range_check"] = [(0, 0, 1, 0.0)]      # clean, but a shift moved: counts as unsettled
        h.forward(x, pose, x_rep=2)
        assert fake.take() == [wsb, poll, fwd, check]
        for _ in range(3):
            h.forward(x, pose, x_rep=2)
            assert fake.take() == [wsb, poll, fwd, check]
        h.forward(x, pose, x_rep=2)
        assert fake.take() == [wsb, poll, fwd]
    assert h.range_events == [{"code": ERR_RANGE, "layers_out_of_range": 1, "layers_adjusted": 1, "max_abs": 3.0, "attempt": -1}]


@pytest.mark.parametrize("env,mode", [("0", "off"), ("3", "poison")])
def test_x2_modes_without_checks(fake, monkeypatch, env, mode):
    monkeypatch.setenv("NOPE_X2_RANGE_CHECK", env)
    h = _hyp_handle("ldm", hip.F16X2)
    fake.take()
    assert (h.range_mode, h.x2_enabled) == (mode, True)
    h.forward(*_xp(4), x_rep=2)
    names = [c[0] for c in fake.take()]
    assert names == ["nope_ldm_workspace_bytes"] + (["nope_ldm_x2_poll"] if mode == "poison" else []) + ["nope_ldm_forward"]


# ---- (d) f32: no x2 call at all -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem", ["unet", "ldm", "gd"])
def test_f32_handle_makes_no_x2_call(fake, monkeypatch, stem):
    monkeypatch.setenv("NOPE_X2_RANGE_CHECK", "2")
    h = _hyp_handle(stem, hip.F32)
    h.forward(*_xp(4), x_rep=2)
    h.forward(*_xp(4), x_rep=2, defer_range_check=True)
    assert h.finish_range_check() is False
    del h
    assert [c[0] for c in fake.take()] == [f"nope_{stem}_create"] + [f"nope_{stem}_workspace_bytes", f"nope_{stem}_forward"] * 2 + [f"nope_{stem}_destroy"]
