"""The conv launcher's policy as a table, and one plan per launch.

nope::conv_plan (nope_amd/csrc/kernels_gemm.hip) decides everything about a conv launch: kernel, tile, grid, K splits, tile walk,
epilogue form.  A silent drift of that policy is a speed regression no numerical test sees, so tests/conv_plan_dump.cpp prints the plan
of a sweep of launches -- pure host arithmetic, no kernel runs -- and tests/conv_plan_table.txt records a thinned subset of it.

A DELIBERATE policy change changes the table.  Regenerate it with

    python tests/test_conv_plan.py --regenerate

and review the diff line by line: each changed line is a launch that now runs differently.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "tests", "conv_plan_dump.cpp")
TABLE = os.path.join(ROOT, "tests", "conv_plan_table.txt")
BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]


def build_dump():
    """tests/conv_plan_dump.cpp against the interpreter build of the library (host code only)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    lib = build_emu.build()
    exe = os.path.join(ROOT, "build", "emu", "conv_plan_dump")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(SRC), os.path.getmtime(lib))):
        subprocess.run([build_emu.CLANG, "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "tests", "hipemu", "include"),
                        "-I", os.path.join(ROOT, "nope_amd", "csrc"), "-Wno-unknown-attributes", "-Wno-ignored-attributes", "-Wno-unknown-pragmas",
                        SRC, "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return exe


def dump_table():
    env = {k: v for k, v in os.environ.items() if not k.startswith("NOPE_")}
    return subprocess.run([build_dump(), "table"], check=True, stdout=subprocess.PIPE, text=True, env=env).stdout


def _field(line, pattern):
    m = re.search(pattern, line)
    return tuple(int(v) for v in m.groups()) if m else None


def coverage_gaps(text):
    """What a plan table must contain so that it cannot degenerate; returns the names of the conditions no line meets."""
    seen = set()
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        case, plan, ans = line.split(" | ")
        err, splitk = _field(ans, r"err (-?\d+) stat_rows \d+ splitk (\d+)")
        seen.add(f"err {err}")
        tail = re.search(r" gn \d+,\d$", case) is not None      # a launch with a GroupNorm tail (ConvArgs::gn_*)
        if err:
            if tail:
                seen.add("tail refused")
            continue
        kind, = _field(plan, r" kind (\d) ")
        xcd, = _field(plan, r" xcd (\d)/")
        persist, = _field(plan, r" persist (\d+),")
        splits, = _field(plan, r" splits (\d+) ")
        reduce_, = _field(plan, r" reduce (\d)(?: gn_G .*)?$")
        mode, = _field(plan, r" mode (\d) ")
        ws, = _field(case, r" ws (\d)(?: gn \d+,\d)?$")
        seen.update({f"kind {kind}", f"xcd_map {xcd}", "lean %d" % _field(plan, r" lean (\d)")})
        if " posmajor 1 " in plan:
            seen.add("posmajor")
        if persist > 1:
            seen.add(f"persist on kind {kind}")
        if splits > 1:
            seen.add(f"splits on kind {kind} reduce {reduce_}")
        if _field(plan, r" nchw \d,\d,(\d) ") == (1,):
            seen.add("nchw_staged")
        if " x2 1 " in plan:
            seen.add("x2 phase convs tap-resident" if (kind, mode) == (3, 3) else f"x2 on kind {kind}")
        if " geglu 1 " in plan:
            seen.add("geglu")
        if tail and " gn_G " in plan:
            seen.add("tail")
        if ws == 2 and splitk > 1 and splits == 1:
            seen.add("downgraded: split-K scratch short")
    want = ([f"kind {k}" for k in range(6)] + [f"xcd_map {m}" for m in range(5)] + ["posmajor", "lean 0", "lean 1", "nchw_staged", "geglu"] +
            ["persist on kind 1", "persist on kind 3", "persist on kind 5"] +       # 128 x 192, tap-resident, streaming
            # K splits of both origins: the tap-resident kernel's (its reduce with and without statistics) and the 128 x 192 kernel's
            # (conv_splitk_factor never splits a launch that emits statistics unless the tap-resident split applies: plain reduce only)
            ["splits on kind 3 reduce 1", "splits on kind 3 reduce 2", "splits on kind 1 reduce 1"] +
            ["x2 on kind 3", "x2 on kind 2", "x2 phase convs tap-resident"] +      # two-pass tile: tap-resident, per tap, the phase convs of an up-sampling
            ["tail", "tail refused"] +      # GroupNorm tail: one launch that carries it, one that is refused rather than run without it
            ["downgraded: split-K scratch short", "err 0", "err -1", "err -6"])     # (NOPE_ERR_ARG, NOPE_ERR_UNSUPPORTED: all conv_plan returns)
    return [w for w in want if w not in seen]


def test_conv_plan_table(emu):
    got = dump_table()
    with open(TABLE) as f:
        want = f.read()
    lines = [l for l in want.splitlines() if not l.startswith("#")]
    assert 300 <= len(lines) <= 4000 and len(want) <= 512 * 1024
    assert coverage_gaps(want) == []
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail(f"the conv plan differs from tests/conv_plan_table.txt ({len(g)} / {len(w)} lines), first at line {first + 1}:\n"
                    f"  table: {w[first] if first < len(w) else '(end)'}\n  now:   {g[first] if first < len(g) else '(end)'}\n"
                    "a deliberate policy change: python tests/test_conv_plan.py --regenerate, and review the diff")


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, "cuda" if request.param == "gpu" else "cpu", request.param


TRACE_KERNEL = {"generic": "conv_gemm_kernel", "dma128": "conv_gemm_dma_kernel", "pp256": "conv_gemm_pp_kernel", "halo256": "conv3x3_halo_kernel",
                "small": "conv_gemm_small_kernel", "stream128": "conv1x1_stream_kernel"}


def test_profile_reports_the_plan_that_ran(be, golden, monkeypatch, capfd):
    """One plan per launch: what profile_launches() reports of a forward -- kernel, posmajor, MFMA passes -- is, launch for launch, what the
    launcher's NOPE_CONV_TRACE lines say ran.  The d8 fixture at one hypothesis and its own 8 x 8 map (three halvings: the smallest it takes), the
    smallest forward of the fixture; it reaches two kernel kinds already: the 8-channel convs on the register-staged kernel, the rest on the
    small-tile kernel.  In the f16x2 mode with the ping-pong kernels opened to small shapes (NOPE_CONV_PP=11) the layers with a multiple of 32
    input channels run the two-pass tile; that leg runs on the GPU only (its forward, issued twice by the range tracking, was measured at
    133 s under the interpreter, against 7 s for the bf16x3 leg).  Position-major launches need 128 hypotheses and more than 128 tiles, which
    this fixture cannot reach: tests/test_gn_fused.py reads them from the trace, and the plan table records them."""
    hip, dev, name = be
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    from tests.util import StubEncoder
    g = golden("unet_tiny.npz")
    x, pose = g["d8/x"][:1], g["d8/pose"][:1]
    for cdt, env in [("bf16x3", {})] + ([("f16x2", {"NOPE_CONV_PP": "11"})] if name == "gpu" else []):
        m = UNet(u_net_dim=8, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name="single_layer", compute_dtype=cdt)
        synth_init_(m, 2022)
        m = m.to(dev)
        xd, pd = x.to(dev), pose.to(dev)
        h = m._get_handle(xd.device)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("NOPE_CONV_TRACE", "1")
        h.profile(True)
        capfd.readouterr()
        m(xd, pd)
        if dev == "cuda":
            torch.cuda.synchronize()
        trace = [l.split() for l in capfd.readouterr().err.splitlines() if l.startswith("conv ")]
        launches = h.profile_launches()
        h.profile(False)
        monkeypatch.delenv("NOPE_CONV_TRACE")
        for k in env:
            monkeypatch.delenv(k)
        # The pose embedding's GEMM ([n_hyp] rows, 1x1) opens every forward (the f16x2 mode may issue one twice); it is issued beside the
        # network's conv path: traced, not profiled.  Walk both lists together and set aside only trace lines that are such a GEMM and
        # do not describe the next profiled launch.
        shape = lambda t: tuple(int(t[t.index(k) + 1]) for k in ("taps", "Cin", "Cout"))
        kept, pose_gemms = [], 0
        for t in trace:
            l = launches[len(kept)] if len(kept) < len(launches) else None
            if l is not None and shape(t) == (l["ntaps"], l["Cin"], l["Cout"]):
                kept.append(t)
            else:
                assert shape(t)[0] == 1 and int(t[t.index("M") + 1]) == x.shape[0], (t, l)
                pose_gemms += 1
        trace = kept
        assert len(trace) == len(launches) > 10 and 1 <= pose_gemms <= 2, (len(trace), len(launches), pose_gemms)
        for t, l in zip(trace, launches):
            kind = "small" if t[1].startswith("small") else t[1]
            assert l["kernel"] == TRACE_KERNEL[kind], (t, l)
            assert l["posmajor"] == (int(t[t.index("posmajor") + 1]) if "posmajor" in t else 0), (t, l)
            assert (l["mfma_passes"] == 2) == ("x2" in t), (t, l)
            assert (l["ntaps"], l["Cout"]) == (int(t[t.index("taps") + 1]), int(t[t.index("Cout") + 1])), (t, l)
        assert len({l["kernel"] for l in launches}) >= 2, {l["kernel"] for l in launches}
        assert any(l["mfma_passes"] == 2 for l in launches) == (cdt == "f16x2")


if __name__ == "__main__":
    if sys.argv[1:] == ["--regenerate"]:
        text = dump_table()
        assert coverage_gaps(text) == [], coverage_gaps(text)
        with open(TABLE, "w") as f:
            f.write(text)
        print(f"{TABLE}: {len(text.splitlines())} lines, {len(text)} bytes")
    elif sys.argv[1:2] == ["--gaps"]:
        print(coverage_gaps(open(sys.argv[2]).read()))
    else:
        sys.exit("usage: python tests/test_conv_plan.py --regenerate | --gaps FILE")
