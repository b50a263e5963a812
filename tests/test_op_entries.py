"""The operator-level conv / GroupNorm entries behind nope_amd.hip's public functions, pinned under the interpreter.

op_conv, op_conv_ex, op_conv_gn_tail, op_conv_stat_rows, op_group_norm, op_group_norm_ex, op_group_norm_shared and op_gn_apply_blocks are how
every kernel of the conv / GroupNorm family is parity-tested in isolation.  A change of the plumbing between those functions and the
launchers (the C entries of nope_amd/csrc/capi.hip, their ctypes mirrors) that is meant to leave every launch alone is checked here
against tests/op_entries_table.txt, which records for every case below

  * the `conv ...` lines NOPE_CONV_TRACE=1 writes (kernel, tiles, grid, epilogue form);
  * the answers of the queries the case asks (op_conv_stat_rows, op_gn_apply_blocks, the shape of tail_stats);
  * a SHA-1 of every tensor the function returns, `extras` tensors included, and the range maximum as the float's hex form;
  * for a refused combination, the error code of the NopeError.

The table is recorded from the commit a change STARTS from, never from the code under test:

    python tests/test_op_entries.py --record          # in a checkout of that commit; then copy the table over

Only the public Python surface is used, so that this file runs unchanged in the older checkout.  CPU only: the device's kernel choice
depends on its CU count (tests/test_unet_schedule.py)."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_unet_schedule import _sha1, _stderr_lines      # noqa: E402

TABLE = os.path.join(ROOT, "tests", "op_entries_table.txt")
PP = {"NOPE_CONV_PP": "11", "NOPE_CONV_SMALL": "0", "NOPE_CONV_STREAM": "0"}      # the ping-pong kernels at any tile count (tests/test_res_tail.py)
SWITCHES = ("NOPE_CONV_PP", "NOPE_CONV_SMALL", "NOPE_CONV_STREAM", "NOPE_CONV_TRACE")
CASES = {}      # name: (environment, function(hip, rn) -> (query answers, what the public function returned))


def case(name, env=None):
    def add(fn):
        CASES[name] = (env or {}, fn)
        return fn
    return add


def _nhwc(hip, rn, dt, n, c, h, w, scale=1.0, dc=0.3):
    """An NHWC tensor of dt's storage type with a DC offset (a wrong mean cannot pass)."""
    return hip.to_nhwc(rn(n, c, h, w) * scale + dc, dt)


# ---- op_conv ------------------------------------------------------------------------------------------------------------------------------
def _conv_4x4(hip, rn, **kw):
    x, w, b = _nhwc(hip, rn, hip.F32, 1, 32, 4, 4), rn(8, 32, 3, 3) / 17, rn(8)
    return [hip.op_conv_stat_rows(hip.F32, 32, 0, 1, 4, 4, hip.CONV_PLAIN, 9, 8, 1)], hip.op_conv(hip.F32, x, w, b, **kw)


@case("conv_f32_3x3")
def _(hip, rn):
    return _conv_4x4(hip, rn)


@case("conv_f32_3x3_split_k")
def _(hip, rn):
    return _conv_4x4(hip, rn, split_k=True)


@case("conv_f32_3x3_long_k_split_k", {"NOPE_CONV_SMALL": "0"})      # (a shape the launcher does split: grid.z > 1 in the trace)
def _(hip, rn):
    x, w = _nhwc(hip, rn, hip.F32, 1, 256, 4, 4), rn(8, 256, 3, 3) / 48
    return [], hip.op_conv(hip.F32, x, w, None, split_k=True)


@case("conv_bf16_two_sources_rep1")
def _(hip, rn):
    x1, x2 = _nhwc(hip, rn, hip.BF16, 1, 16, 8, 8), _nhwc(hip, rn, hip.BF16, 2, 16, 8, 8, dc=-0.2)
    q = [hip.op_conv_stat_rows(hip.BF16, 16, 16, 2, 8, 8, hip.CONV_PLAIN, 9, 32, 2)]
    return q, hip.op_conv(hip.BF16, x1, rn(32, 32, 3, 3) / 17, rn(32), src2=x2, rep1=2)


def _resample(hip, rn, mode, wshape):
    x = _nhwc(hip, rn, hip.F32, 1, 32, 8, 8)
    ntaps = 4 if mode in (hip.CONV_DOWN2, hip.CONV_UP2P) else 9
    q = [hip.op_conv_stat_rows(hip.F32, 32, 0, 1, 8, 8, mode, ntaps, 32, 1)]
    return q, hip.op_conv(hip.F32, x, rn(*wshape) / (wshape[1] * wshape[2] * wshape[3]) ** 0.5, rn(32), mode=mode)


@case("conv_down2")
def _(hip, rn):
    return _resample(hip, rn, hip.CONV_DOWN2, (32, 128, 1, 1))


@case("conv_up2p")
def _(hip, rn):
    return _resample(hip, rn, hip.CONV_UP2P, (32, 32, 3, 3))


@case("conv_stride2_pad01")
def _(hip, rn):
    return _resample(hip, rn, hip.CONV_STRIDE2_PAD01, (32, 32, 3, 3))


@case("conv_out_nchw_f16")
def _(hip, rn):
    x = _nhwc(hip, rn, hip.F32, 1, 32, 4, 4)
    q = [hip.op_conv_stat_rows(hip.F32, 32, 0, 1, 4, 4, hip.CONV_PLAIN, 9, 8, 1, out_nchw=True)]
    return q, hip.op_conv(hip.F32, x, rn(8, 32, 3, 3) / 17, rn(8), out_nchw=True, out_dtype=hip.F16)


@case("conv_relu_resid")
def _(hip, rn):
    x, r = _nhwc(hip, rn, hip.F32, 1, 32, 4, 4), _nhwc(hip, rn, hip.F32, 1, 8, 4, 4, dc=-0.5)
    q = [hip.op_conv_stat_rows(hip.F32, 32, 0, 1, 4, 4, hip.CONV_PLAIN, 9, 8, 1, resid=True, act_relu=True)]
    return q, hip.op_conv(hip.F32, x, rn(8, 32, 3, 3) / 17, rn(8), resid=r, act_relu=True)


# ---- op_conv_ex: (2, 8 x 8, 64 -> 96, 1x1) in bf16x3 on the per-tap ping-pong kernel ---------------------------------------------------------
def _ex_inputs(hip, rn):
    return _nhwc(hip, rn, hip.BF16X3, 2, 64, 8, 8, scale=2.0, dc=0.4), rn(96, 64, 1, 1) / 8, rn(96)


@case("conv_ex_colstats", PP)
def _(hip, rn):
    x, w, b = _ex_inputs(hip, rn)
    rows = hip.op_conv_stat_rows(hip.BF16X3, 64, 0, 1, 8, 8, hip.CONV_PLAIN, 1, 96, 2)
    cs = torch.zeros((128 // max(rows, 1)) * 96 * 2)
    return [rows], (hip.op_conv_ex(hip.BF16X3, x, w, b, colstats=cs, stat_rows=rows), cs)


@case("conv_ex_prenorm", PP)
def _(hip, rn):
    x, w, b = _ex_inputs(hip, rn)
    flat = x.reshape(2, -1)
    ms = torch.stack((flat.mean(1), (flat.var(1, unbiased=False) + 1e-5).rsqrt()), 1).contiguous()
    return [], hip.op_conv_ex(hip.BF16X3, x, w, b, prenorm=(ms, 1.0 + 0.3 * rn(64), 0.5 * rn(64)))


@case("conv_ex_want_amax", PP)
def _(hip, rn):
    x, w, b = _ex_inputs(hip, rn)
    return [], hip.op_conv_ex(hip.BF16X3, x, w, b, want_amax=True)


# ---- op_conv_gn_tail: the inputs of tests/test_res_tail.py::_case ----------------------------------------------------------------------------
def _tail(hip, rn, shape, dt, shift):
    n, hw, ca, cb, cout, G = shape
    scale = (1.0 + 1.5 * torch.arange(n).float())[:, None, None, None]
    x1 = rn(n, hw, hw, ca) * scale + 0.3
    x2 = rn(n, hw, hw, cb) * scale - 0.2 if cb else None
    grp = (0.5 + torch.arange(G).float()).repeat_interleave(cout // G)
    raw = ((rn(n, hw, hw, cout) * grp + 0.7 * grp) * scale).contiguous()
    w, b = rn(cout, ca + cb, 1, 1) / (ca + cb) ** 0.5, rn(cout)
    r = raw.reshape(n, hw * hw // 64, 64, cout)
    cs = torch.stack((r.sum(2), (r * r).sum(2)), -1).contiguous()
    out, ex = hip.op_conv_gn_tail(dt, x1, w, b, raw, cs, 1.0 + 0.3 * rn(cout), 0.5 * rn(cout), G, src2=x2, in_place=True, tail_stats=True,
                                  want_amax=True, x2_shift=shift)
    return [tuple(ex["tail_stats"].shape)], (out, ex)


for _shape in ((4, 8, 64, 32, 96, 8), (4, 8, 64, 0, 32, 1)):
    for _mode, _shift in (("BF16X3", 0), ("F16X2", 3)):
        case(f"gn_tail_{_mode.lower()}_cout{_shape[4]}", PP)(lambda hip, rn, s=_shape, m=_mode, t=_shift: _tail(hip, rn, s, getattr(hip, m), t))


# ---- op_group_norm / op_group_norm_ex on (2, 8 x 8, 32, G = 8) -------------------------------------------------------------------------------
def _gn_inputs(hip, rn, dt, n=2):
    return _nhwc(hip, rn, dt, n, 32, 8, 8, scale=2.0, dc=0.4), 1.0 + 0.3 * rn(32), 0.5 * rn(32)


def _gn_colstats(x, rows=16):
    """[n][HW / rows][C][2] f32 (sum, sum of squares) of NHWC x over blocks of `rows` pixels: what a producing conv's epilogue emits."""
    n, h, w, c = x.shape
    r = x.float().reshape(n, h * w // rows, rows, c)
    return torch.stack((r.sum(2), (r * r).sum(2)), -1).contiguous()


@case("gn_plain")
def _(hip, rn):
    x, ga, be = _gn_inputs(hip, rn, hip.F32)
    return [], (hip.op_group_norm(hip.F32, x, ga, be, 8), hip.op_group_norm(hip.F32, x, ga, be, 8, act_silu=True))


@case("gn_emb_resid")
def _(hip, rn):
    x, ga, be = _gn_inputs(hip, rn, hip.F32)
    return [], hip.op_group_norm(hip.F32, x, ga, be, 8, act_silu=True, emb=rn(2, 32), resid=_nhwc(hip, rn, hip.F32, 2, 32, 8, 8, dc=-0.5))


def _gn_ex(form):
    def run(hip, rn, dt):
        x, ga, be = _gn_inputs(hip, rn, dt)
        q = [hip.op_gn_apply_blocks(dt, 64, 32, 4 if form == "reps" else 2)]
        if form in ("colstats", "colstats_fold_launch"):
            kw = dict(colstats=_gn_colstats(x), fold_launch=form.endswith("fold_launch"))
        elif form == "film_1d":
            kw = dict(film=0.2 * rn(64))
        elif form == "film_2d":
            kw = dict(film=0.2 * rn(2, 64))
        elif form == "reps":
            kw = dict(x_rep=2, resid_rep=2, emb=rn(4, 32), resid=_nhwc(hip, rn, dt, 2, 32, 8, 8, dc=-0.5))
        elif form == "out_stats":
            kw = dict(out_stats=True)
        else:
            kw = dict(fast_silu=True, want_amax=True)
        return q, hip.op_group_norm_ex(dt, x, ga, be, 8, act_silu=True, **kw)
    return run


for _form in ("colstats", "colstats_fold_launch", "film_1d", "film_2d", "reps", "out_stats", "fast_silu_amax"):
    for _dt in ("F32", "BF16"):
        case(f"gn_ex_{_form}_{_dt.lower()}")(lambda hip, rn, f=_form, d=_dt: _gn_ex(f)(hip, rn, getattr(hip, d)))


# ---- op_group_norm_shared at 4 x 4 x 32, four hypotheses over two shared samples -------------------------------------------------------------
def _shared(hip, rn, form, **kw):
    S, ga, be = _nhwc(hip, rn, hip.F32, 2, 32, 4, 4, scale=2.0, dc=0.4), 1.0 + 0.3 * rn(32), 0.5 * rn(32)
    x = _nhwc(hip, rn, hip.F32, 4, 32, 4, 4) if form == "X+S" else None
    E = rn(4, 9, 32) if form == "S+E" else None
    return [hip.op_gn_apply_blocks(hip.F32, 16, 32, 4)], hip.op_group_norm_shared(hip.F32, x, S, E, ga, be, 8, 4, **kw)


@case("gn_shared_s_e")
def _(hip, rn):
    return _shared(hip, rn, "S+E", emb=rn(4, 32), out_stats=True, fast_silu=True, want_amax=True)


@case("gn_shared_x_s")
def _(hip, rn):
    return _shared(hip, rn, "X+S", resid=_nhwc(hip, rn, hip.F32, 2, 32, 4, 4, dc=-0.5), resid_rep=2)


# ---- one refused combination per entry -------------------------------------------------------------------------------------------------------
@case("refused_conv_down2_odd_map")
def _(hip, rn):
    return [], hip.op_conv(hip.F32, hip.to_nhwc(rn(1, 32, 6, 6), hip.F32)[:, :5, :5].contiguous(), rn(32, 128, 1, 1), None, mode=hip.CONV_DOWN2)


@case("refused_conv_ex_stat_rows_off_by_one", PP)
def _(hip, rn):
    x, w, b = _ex_inputs(hip, rn)
    rows = hip.op_conv_stat_rows(hip.BF16X3, 64, 0, 1, 8, 8, hip.CONV_PLAIN, 1, 96, 2)
    return [rows], hip.op_conv_ex(hip.BF16X3, x, w, b, colstats=torch.zeros(2 * 128 * 96), stat_rows=rows + 1)


@case("refused_gn_tail_f32", PP)
def _(hip, rn):
    return _tail(hip, rn, (4, 8, 64, 0, 32, 1), hip.F32, 0)


@case("refused_gn_shared_without_silu")
def _(hip, rn):
    return _shared(hip, rn, "S+E", act_silu=False)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _result_lines(ret, name="out"):
    """One line per value a public function returned: tensors by SHA-1, the range maximum by its hex form, flags as they are."""
    if isinstance(ret, torch.Tensor):
        return [f"{name} {ret.dtype} {tuple(ret.shape)} sha1 {_sha1(ret)}"]
    if isinstance(ret, dict):
        return [l for k in sorted(ret) for l in _result_lines(ret[k], f"{name}.{k}")]
    if isinstance(ret, (tuple, list)):
        return [l for i, v in enumerate(ret) for l in _result_lines(v, f"{name}.{i}")]
    return [f"{name} {float(ret).hex() if isinstance(ret, float) else ret!r}"]


def run_case(name, setenv, delenv):
    """The table's lines for one case.  setenv / delenv: how the caller sets and clears an environment variable."""
    from nope_amd import hip
    env, fn = CASES[name]
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    setenv("NOPE_CONV_TRACE", "1")
    g = torch.Generator().manual_seed(9100 + list(CASES).index(name))
    err, query, ret, code = [], [], None, None
    with _stderr_lines(err):
        try:
            query, ret = fn(hip, lambda *s: torch.randn(*s, generator=g))
        except hip.NopeError as e:
            code = int(re.search(r"\((-?\d+)\)$", str(e)).group(1))
    lines = [f"case {name}"] + ["trace " + e for e in err if e.startswith("conv ")]
    if code is not None:
        return lines + [f"refused {code}"]
    return lines + [" ".join(["query"] + [repr(q) for q in query])] + _result_lines(ret)


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


@pytest.mark.parametrize("name", list(CASES))
def test_entry_matches_the_table(emu, name, monkeypatch):
    want = _table()[name]
    got = run_case(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"{name}: differs from tests/op_entries_table.txt ({len(got)} / {len(want)} lines), first at line {first} of the case:\n"
                    f"  table: {want[first] if first < len(want) else '(end)'}\n  now:   {got[first] if first < len(got) else '(end)'}")


def test_table_is_whole():
    """Every case is in the table, a refused one with its code and no launch, every other with at least one hashed tensor; the cases that are
    here for one form of a launch did take it when the table was recorded."""
    t = _table()
    assert list(t) == list(CASES)
    for name, lines in t.items():
        if name.startswith("refused_"):
            assert lines[-1].startswith("refused -") and not any(l.startswith("trace ") for l in lines), (name, lines)
        else:
            assert any(" sha1 " in l for l in lines) and not any(l.startswith("refused") for l in lines), (name, lines)
    trace = lambda name: [l for l in t[name] if l.startswith("trace ")]
    grid_z = lambda l: int(l.split()[l.split().index("grid") + 1].split(",")[2])
    assert any(grid_z(l) > 1 for l in trace("conv_f32_3x3_long_k_split_k")), "no split-K launch"
    for name in t:
        if name.startswith("gn_tail_"):
            assert len(trace(name)) == 1 and trace(name)[0].endswith(" lean gn-tail"), (name, trace(name))
        if name.startswith("conv_ex_"):
            assert len(trace(name)) == 1 and " pp256 " in trace(name)[0], (name, trace(name))


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_op_entries.py --record   (in a checkout of the commit the change starts from)")
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import build_emu
    from nope_amd import hip
    hip._set_library_for_testing(hip.NopeLib(build_emu.build()))
    out = ["# The operator-level conv / GroupNorm entries under the interpreter (tests/test_op_entries.py --record).",
           "# Per case: the NOPE_CONV_TRACE lines, the query answers, every returned value (tensors by SHA-1); or the error code of a refusal."]
    for name in CASES:
        out += run_case(name, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        print(name, len(out), flush=True)
    with open(TABLE, "w") as f:
        f.write("\n".join(out) + "\n")
