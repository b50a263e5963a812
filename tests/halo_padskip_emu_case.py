"""The tap-resident 3x3 kernel's padding-skipping form for 4 x 4 maps (conv3x3_halo_kernel, PADSKIP; ConvParams::padskip; NOPE_HALO_PADSKIP): a tile staged
in (position, sample) order, the MFMA block-taps that lie wholly in the zero padding not executed, the accumulators exchanged through LDS before the
unchanged lean epilogue -- against the sample-major form (NOPE_HALO_PADSKIP=0), torch.equal on everything a launch writes.
Shared by tests/test_halo_padskip.py (interpreter and device); `python tests/halo_padskip_emu_case.py` runs the interpreter cases alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
import torch
import torch.nn.functional as F

from tests.up2p_emu_case import launch_trace
from tests.util import MODE_BOUNDS, rel, switches

PP = dict(NOPE_CONV_PP=11, NOPE_CONV_SMALL=0, NOPE_CONV_STREAM=0)      # bit 3: small shapes reach the tap-resident kernel
# (samples, C1, C2, Cout): one tile / two tiles (m0 != 0); two and three channel chunks (both A stages, an odd chunk count); one and two weight
# panels; a concatenated second source whose boundary is a chunk boundary
SHAPES = [(16, 64, 0, 192), (32, 96, 0, 384), (16, 64, 32, 192)]
FORMS = ["colstats", "gn_self", "resid"]
G = 8


def inputs(n, c1, c2, cout, dev, seed):
    """The recipe of gn_epi_emu_case.inputs (a DC offset, per-sample and per-group scales: a wrong sample, position or group cannot pass) with the
    channel counts as parameters and an optional second source."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    cin = c1 + c2
    scale = (1.0 + 0.75 * torch.arange(n).float())[:, None, None, None]
    x = (rn(n, 4, 4, cin) * scale + 0.4)
    grp = (0.5 + torch.arange(G).float()).repeat_interleave(cout // G)
    w = (rn(cout, cin, 3, 3) / (9 * cin) ** 0.5 * grp[:, None, None, None]).to(dev)
    b = (0.6 * grp + 0.2 * rn(cout)).to(dev)
    ga, bt = (1.0 + 0.3 * rn(cout)).to(dev), (0.5 * rn(cout)).to(dev)
    e = rn(n, cout + 64).to(dev)
    r = (rn(n, 4, 4, cout) * scale).contiguous().to(dev)
    x1 = x[..., :c1].contiguous().to(dev)
    x2 = x[..., c1:].contiguous().to(dev) if c2 else None
    return x1, x2, w, b, ga, bt, e, r


def launch(hip, dt, form, x1, x2, w, b, ga, bt, e, r):
    """One launch of the form: everything it writes, as a tuple of CPU tensors / floats."""
    n, cout = x1.shape[0], w.shape[0]
    if form == "colstats":
        sr = hip.op_conv_stat_rows(dt, x1.shape[3], 0 if x2 is None else x2.shape[3], 1, 4, 4, hip.CONV_PLAIN, 9, cout, n)
        assert sr == 16, sr
        cs = torch.zeros((n, 1, cout, 2), dtype=torch.float32, device=x1.device)
        y = hip.op_conv_ex(dt, x1, w, b, src2=x2, colstats=cs, stat_rows=sr)
        return y.cpu(), cs.cpu()
    if form == "gn_self":
        y, amax = hip.op_conv_gn_self(dt, x1, w, b, ga, bt, G, emb=e, resid=r, src2=x2, want_amax=True)
        return y.cpu(), amax
    y, amax, rec = hip.op_conv_ex(dt, x1, w, b, src2=x2, resid=r, want_amax=True)
    assert rec
    return y.cpu(), amax


def same(a, b):
    return all(torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v for u, v in zip(a, b)) and len(a) == len(b)


def conv_lines(trace):
    return [ln for ln in trace.splitlines() if ln.startswith("conv ")]


def on_off(fn):
    """fn() under NOPE_HALO_PADSKIP = 1 and 0: (results, trace lines) of each"""
    out = []
    for sw in (1, 0):
        with switches(NOPE_HALO_PADSKIP=sw):
            y, tr = launch_trace(fn)
        out.append((y, conv_lines(tr)))
    return out


def one_case(hip, dev, dt, shape, form, seed=9500):
    n, c1, c2, cout = shape
    args = inputs(n, c1, c2, cout, dev, seed + 10 * SHAPES.index(shape) + FORMS.index(form))
    with switches(**PP):
        (y1, t1), (y0, t0) = on_off(lambda: launch(hip, dt, form, *args))
    assert torch.isfinite(y0[0]).all() and float(y0[0].abs().max()) > 0.1
    assert len(t1) == 1 and len(t0) == 1 and " halo256 " in t0[0], (t1, t0)
    assert " padskip" in t1[0] and " padskip" not in t0[0], (t1, t0)
    assert t1[0].replace(" padskip", "") == t0[0], "the same launch but for the form"
    assert t1[0].endswith(" lean gn-self" if form == "gn_self" else " lean"), t1
    assert " padskip" in t1[0].split(" xcd ")[1].split(" x2")[0].split(" lean")[0], "the marker stands in front of the existing suffixes"
    assert same(y1, y0), (shape, form, dt, float((y1[0] - y0[0]).abs().max()))


def impulse_case(hip, dev, dt, mode, n=32, cin=64, cout=192):
    """Sample s is zero except one pixel, at position s % 16, in one channel; the weights are distinct per tap, input channel and output channel.  Every
    output value is then ONE product, at a place that tells the tap, the position and the sample: a wrong tap offset, a wrong skip or a wrong
    un-permutation moves a value and fails.  Reference: F.conv2d in f64, within the mode's bound of tests/util.py."""
    x = torch.zeros(n, cin, 4, 4, dtype=torch.float64)
    for s in range(n):
        x[s, (5 * s + 3) % cin, (s % 16) // 4, (s % 16) % 4] = 1.0 + 0.125 * s
    tap = torch.arange(9, dtype=torch.float64).reshape(1, 1, 3, 3)
    w = (1.0 + tap) * (1.0 + 0.01 * torch.arange(cin, dtype=torch.float64))[None, :, None, None] * (0.5 + 0.003 * torch.arange(cout, dtype=torch.float64))[:, None, None, None]
    want = F.conv2d(x, w, None, padding=1)
    xs = x.float().permute(0, 2, 3, 1).contiguous().to(dev)
    with switches(**PP):
        (y1, t1), (y0, t0) = on_off(lambda: hip.op_conv_ex(dt, xs, w.float().to(dev), None, want_amax=True)[0].cpu())
    assert " padskip" in t1[0] and " padskip" not in t0[0], (t1, t0)
    for y in (y1, y0):
        got = y.permute(0, 3, 1, 2).double()
        err = rel(got, want)
        print(f"impulse[{mode}]: rel err {err:.2e} (bound {MODE_BOUNDS[mode][0]:.0e})")
        assert err < MODE_BOUNDS[mode][0], (mode, err)
        assert bool((got[want == 0] == 0).all()), "a product landed where the reference has none"
    assert torch.equal(y1, y0)


# Launches the planner does not grant the form to (the marker absent, results equal to the switch-off run all the same):
# name: (dtype name, samples, map, Cin, mode name, split_k, switches)
NOT_TAKEN = {"8x8": ("BF16X3", 4, 8, 32, "CONV_PLAIN", False, PP),
             "n15": ("BF16X3", 15, 4, 32, "CONV_PLAIN", False, PP),
             "f32": ("F32", 16, 4, 32, "CONV_PLAIN", False, PP),
             "bf16": ("BF16", 16, 4, 64, "CONV_PLAIN", False, PP),
             "split_k": ("BF16X3", 16, 4, 512, "CONV_PLAIN", True, dict(PP, NOPE_CONV_PP=3)),
             "up2p": ("F16X2", 16, 4, 32, "CONV_UP2P", False, dict(PP, NOPE_CONV_PP=13))}


def not_taken_case(hip, dev, name, cout=192):
    dtn, n, hw, cin, moden, split_k, env = NOT_TAKEN[name]
    dt, mode = getattr(hip, dtn), getattr(hip, moden)
    g = torch.Generator().manual_seed(9600 + sorted(NOT_TAKEN).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(n, hw, hw, cin) + 0.4).to(hip.torch_dtype(dt)).to(dev)
    w, b = (rn(cout, cin, 3, 3) / (9 * cin) ** 0.5).to(dev), rn(cout).to(dev)
    with switches(**env):
        if name == "split_k":      # the plan really is a split-K one: the launcher asks for a scratch at this shape
            assert int(hip._conv_query(**hip._conv_setup(dt, x, w, b, None, mode, 1, None, False, hip.F32, False).op).splitk_bytes) > 0
        (y1, t1), (y0, t0) = on_off(lambda: hip.op_conv(dt, x, w, b, mode=mode, split_k=split_k).cpu())
    assert t1 and t1 == t0 and not any("padskip" in ln for ln in t1), (name, t1, t0)
    if name in ("8x8", "split_k", "up2p", "f32", "bf16"):
        assert all(" halo256 " in ln for ln in t1), (name, t1)      # the tap-resident kernel, in the form it had
    assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0), name


def run(hip, dev, dts=None, light=False):
    dts = dts or (("bf16x3", hip.BF16X3), ("f16x2", hip.F16X2))
    k = 0
    for mode, dt in dts:
        for shape in (SHAPES[1:] if light else SHAPES):
            for form in FORMS:
                one_case(hip, dev, dt, shape, form)
                k += 1
        impulse_case(hip, dev, dt, mode)
        k += 1
    return k


if __name__ == "__main__":
    import build_emu
    from nope_amd import hip
    hip._set_library_for_testing(hip.NopeLib(build_emu.build()))
    print(f"halo_padskip_emu_case OK, {run(hip, 'cpu', light='--light' in sys.argv)} cases")
