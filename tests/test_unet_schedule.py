"""The launch schedule of the network runtimes, pinned under the interpreter.

The U-Net's host runtime (nope_amd/csrc/unet_runtime.hip) and the core the other networks run on (runtime_common.h) decide which conv
launches a forward makes, in which order, over how many samples, with which scratch from the arena.  A host-side change that is meant to
leave all of that alone is checked here against tests/unet_schedule_table.txt, which records for every case below

  * the ordered conv launches of profile_launches(): kernel, mode, ntaps, Cin, Cout, Hs, n_hyp, mfma_passes, posmajor (U-Net handles);
  * the `conv ...` lines NOPE_CONV_TRACE=1 writes (kernel, tiles, grid): every launch_conv, the embedding GEMMs included;
  * workspace_bytes of the case's shape;
  * a SHA-1 of the output tensor's bytes: no kernel and no kernel argument changed, and the interpreter is reproducible.

The table is recorded from the commit a change STARTS from, never from the code under test:

    python tests/test_unet_schedule.py --record          # in a checkout of that commit; then copy the table over

A deliberate schedule change re-records it and reviews the diff line by line.  Only the public Python surface is used, so that this
file runs unchanged in the older checkout.  CPU only: the device's kernel choice depends on its CU count."""
import contextlib
import hashlib
import os
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, "tests", "unet_schedule_table.txt")
LAUNCH_FIELDS = ("kernel", "mode", "ntaps", "Cin", "Cout", "Hs", "n_hyp", "mfma_passes", "posmajor")

# U-Net cases: the network of tests/test_shared_split.py::_tiny (single_layer pose MLP, synth_init_ seed 2022, 8-channel input) unless a row
# says otherwise.  name: (mode, n_src, x_rep, (H, W), u_net_dim, pose MLP, environment)
UNET_CASES = {
    "1_no_sharing": ("f32", 2, 1, (8, 8), 8, "single_layer", {}),
    "2_prefix_only": ("f32", 2, 2, (8, 8), 8, "single_layer", {"NOPE_SHARED_SPLIT": "0"}),
    "3_both_splits": ("f32", 2, 2, (8, 8), 8, "single_layer", {}),
    "4_odd_count_8x16": ("f32", 1, 3, (8, 16), 8, "single_layer", {}),
    "5_bf16": ("bf16", 2, 2, (8, 8), 8, "single_layer", {}),
    "6_bf16x3_fused_tail": ("bf16x3", 1, 4, (8, 8), 8, "single_layer", {"NOPE_FINAL_FUSED": "1"}),
    "6_bf16x3_own_tail": ("bf16x3", 1, 4, (8, 8), 8, "single_layer", {"NOPE_FINAL_FUSED": "0"}),
    "7_f16x2_dim32": ("f16x2", 2, 2, (16, 16), 32, "single_layer", {}),
    "8_splitk_scratch": ("f32", 2, 2, (16, 16), 8, "single_layer", {"NOPE_CONV_SMALL": "0"}),
    "9_two_layer_mlp": ("f32", 2, 2, (8, 8), 8, "two_layers", {}),
}
# the networks on the shared core: the smallest configuration the golden tests of each build (tests/golden/make_golden_*.py)
CORE_CASES = {"10_ldm_updown": ("ldm", "updown"), "11_guided_legacy": ("guided", "legacy"), "12_vae_tiny": ("vae", "tiny")}
SWITCHES = ("NOPE_SHARED_SPLIT", "NOPE_FINAL_FUSED", "NOPE_CONV_SMALL", "NOPE_CONV_TRACE")


@contextlib.contextmanager
def _stderr_lines(into):
    """The lines the library writes to file descriptor 2 inside the block (fprintf of C code: below sys.stderr)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(keep, 2)
            os.close(keep)
            tmp.seek(0)
            into.extend(tmp.read().decode(errors="replace").splitlines())


def _sha1(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _unet_case(name):
    from nope_amd.u_net import UNet
    from nope_amd.weights import synth_init_
    from tests.util import StubEncoder
    cdt, n_src, rep, (H, W), dim, mlp, _ = UNET_CASES[name]
    m = UNet(u_net_dim=dim, rot_representation_dim=6, encoder=StubEncoder(8), pose_mlp_name=mlp, compute_dtype=cdt)
    synth_init_(m, 2022)
    h = m._get_handle(torch.device("cpu"))
    g = torch.Generator().manual_seed(4100 + list(UNET_CASES).index(name))
    x, pose = torch.randn(n_src, 8, H, W, generator=g), torch.randn(n_src * rep, 6, generator=g)
    err = []
    h.profile(True)
    with _stderr_lines(err):
        y = h.forward(x, pose, x_rep=rep)
    launches = h.profile_launches()
    h.profile(False)
    return launches, err, [h.workspace_bytes(n_src * rep, n_src, H, W)], _sha1(y)


def _core_case(name):
    kind, tag = CORE_CASES[name]
    err = []
    if kind == "vae":
        from tests.golden.make_golden_vae import inputs, make_vae
        vae = make_vae(tag)
        image, latent = inputs(tag)
        with _stderr_lines(err):
            enc, dec = vae.encode_image(image), vae.decode_latent(latent)
        h = vae._get_handle(torch.device("cpu"))
        ws = [int(h._l.dll.nope_vae_workspace_bytes(h._h, decode, t.shape[0], t.shape[2], t.shape[3])) for decode, t in ((0, image), (1, latent))]
        return None, err, ws, _sha1(enc, dec)
    from nope_amd.weights import synth_init_
    from tests.util import StubEncoder
    if kind == "ldm":
        from nope_amd.ldm import UNetModelPose
        from tests.golden.make_golden_ldm_configs import inputs, kwargs
        m = UNetModelPose(encoder=StubEncoder(8), compute_dtype="f32", **kwargs(tag))
    else:
        from nope_amd.guided import UNetModelPose
        from tests.golden.make_golden_guided import inputs, kwargs
        m = UNetModelPose(encoder=StubEncoder(4), compute_dtype="f32", **kwargs(tag))
    synth_init_(m, 2022)
    x, pose = inputs(tag)
    with _stderr_lines(err):      # one reference under every pose (x_rep = 3: conv_in reads a shared input), then one reference per pose
        y_rep, y_one = m.forward_hypotheses(x[:1], pose.unsqueeze(0)), m(x, pose)
    h = m._get_handle(torch.device("cpu"))
    n, (H, W) = pose.shape[0], x.shape[2:]
    ws = [int(h._fn("workspace_bytes")(h._h, n, n_src, H, W)) for n_src in (1, n)]
    return None, err, ws, _sha1(y_rep, y_one)


def run_case(name, setenv, delenv):
    """The table's lines for one case.  setenv / delenv: how the caller sets and clears an environment variable."""
    for k in SWITCHES:
        delenv(k)
    for k, v in (UNET_CASES[name][6] if name in UNET_CASES else {}).items():
        setenv(k, v)
    setenv("NOPE_CONV_TRACE", "1")
    launches, err, ws, sha = (_unet_case if name in UNET_CASES else _core_case)(name)
    lines = [f"case {name}"]
    for l in launches or []:
        lines.append("launch " + " ".join(f"{k} {l[k]}" for k in LAUNCH_FIELDS))
    lines += ["trace " + e for e in err if e.startswith("conv ")]
    lines.append("workspace " + " ".join(str(w) for w in ws))
    lines.append("sha1 " + sha)
    return lines


def _table():
    cases, cur = {}, None
    with open(TABLE) as f:
        for line in f.read().splitlines():
            if line.startswith("#") or not line:
                continue
            if line.startswith("case "):
                cur = cases.setdefault(line[5:], [line])
            else:
                cur.append(line)
    return cases


@pytest.mark.parametrize("name", list(UNET_CASES) + list(CORE_CASES))
def test_schedule_matches_the_table(emu, name, monkeypatch):
    want = _table()[name]
    got = run_case(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    if name in UNET_CASES:
        assert sum(l.startswith("launch ") for l in got) > 10, got
    else:
        assert sum(l.startswith("trace ") for l in got) > 10, got
    if name == "8_splitk_scratch":      # the case is here for the split-K scratch of the arena: it must keep launching K splits (grid.z > 1)
        assert any(int(l.split()[l.split().index("grid") + 1].split(",")[2]) > 1 for l in got if l.startswith("trace ")), "no split-K launch"
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"{name}: differs from tests/unet_schedule_table.txt ({len(got)} / {len(want)} lines), first at line {first} of the case:\n"
                    f"  table: {want[first] if first < len(want) else '(end)'}\n  now:   {got[first] if first < len(got) else '(end)'}")


def test_table_is_whole():
    t = _table()
    assert list(t) == list(UNET_CASES) + list(CORE_CASES)
    assert os.path.getsize(TABLE) <= 512 * 1024
    for name, lines in t.items():
        assert lines[-1].startswith("sha1 ") and lines[-2].startswith("workspace "), name
        assert all(int(w) > 0 for w in lines[-2].split()[1:]), (name, lines[-2])


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_unet_schedule.py --record [CASE ...]   (in a checkout of the commit the change starts from)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    from nope_amd import hip
    hip._set_library_for_testing(hip.NopeLib(build_emu.build()))
    out = ["# The launch schedule of the network runtimes under the interpreter (tests/test_unet_schedule.py --record).",
           "# Per case: the profiled conv launches, the NOPE_CONV_TRACE lines, workspace_bytes, the SHA-1 of the output bytes."]
    for case in sys.argv[2:] or list(UNET_CASES) + list(CORE_CASES):
        out += run_case(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        print(case, len(out), flush=True)
    with open(TABLE if not sys.argv[2:] else TABLE + ".part", "w") as f:
        f.write("\n".join(out) + "\n")
