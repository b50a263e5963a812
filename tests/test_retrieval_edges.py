"""Scoring and top-k (csrc/kernels_retrieval.hip) at the shapes, settings and inputs where a wrong kernel still passes a tolerance on randn data.

Exact-arithmetic scoring inputs (`exact_case`): q is integer-valued, every template equals q except in ONE channel per pixel, where it
differs by a small integer d.  Then sum_c (q - t)^4 = d^4, its square root is d^2, and a score is a sum of at most 2048 small integers:
exact in f32 in any summation order, exact in bf16 / f16 storage.  Scores are compared with the float64 oracle as BIT PATTERNS, so there
is no tolerance for a dropped half-word, a skipped tail pixel or the last lane of P to hide under.  (Several differing channels in one
pixel would make the root irrational; quartic sums are 0 or >= 1 because the hardware square root of the 16-bit path flushes denormals.)
16-bit banks use d in {0, +-1, +-2, +-4} (quartic sums 1, 16, 256: even powers of two) on both backends, f32 banks d in [-3, 3].

What each group would catch:
  * scoring forms -- every instantiation launch_similarity can pick (register kernel: LV, CMAX, CEXACT, non-temporal, QLDS, P from 1 to
    256; LDS kernel: P not dividing 256, P > 256, exactly 16384 words), with a ragged last group and a planted exact match.  Each case
    asserts the NOPE_SIM_TRACE line of its launch: a variant bit or NOPE_SIM_MINGROUPS that silently took another path fails;
  * several groups per workgroup -- the software pipeline of sim_reg_kernel: the prefetch of group g + gs, the peeled last group, the
    double-buffered partials (`buf ^= 1`), workgroups of one launch that run different iteration counts;
  * one-element probes -- template n differs from q in element n only: a kernel that drops, swaps or double-counts one (channel, lane,
    word, half-word) position fails on exactly that column;
  * non-finite inputs -- NaN / inf / overflowing quartics come out as the f32 oracle's NaN, -inf and -0.0, and rank as torch.topk ranks them;
  * top-k ties -- equal values with different indices across lanes, waves and the n += 256 stride (the `better()` rule in the xor tree, the
    per-wave fold, the exclusion list), rows of different kinds in one launch;
  * nope_gather_topk -- every case of the base / extra / cut split, NaN in the pad columns (a pad that is read ranks first);
  * nope_topk_merge -- per-shard lists with pads next to real -inf scores: the merged list is nope_topk of the full row.

Every test runs on the interpreter (tests/hipemu) and, marked `gpu`, on the device."""
import re

import pytest
import torch

from oracle import nope_ref as R

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
D_F32 = (-3, -2, -1, 0, 1, 2, 3)
D_16 = (-4, -2, -1, 0, 1, 2, 4)
NT = 256
INF, NAN = float("inf"), float("nan")
PAD_IDX = torch.iinfo(torch.int64).max


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


_CACHE = {}


def cached(key, make):
    """Inputs and float64 references are built once per key and shared by both backends (never modified by a test)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(got, want):
    """f32 tensors equal as bit patterns (-0.0 is not 0.0); a NaN matches any NaN."""
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    if got.shape != want.shape:
        return False
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


def first_diff(got, want):
    got, want = got.detach().cpu().float(), want.detach().cpu().float()
    bad = (bits(got) != bits(want)).nonzero()
    return None if not len(bad) else (bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]), len(bad))


def _hw(HW):
    return (HW // 4, 4) if HW % 4 == 0 else (1, HW)


def _ref_scores(q, bank):
    """oracle.nope_ref.similarity_scores on float64 inputs (a shared bank broadcasts), 256 samples at a time."""
    q, bank = q.double(), bank.double()
    return torch.cat([R.similarity_scores(q[i:i + 256], bank if bank.shape[0] == 1 else bank[i:i + 256]) for i in range(0, q.shape[0], 256)]).float()


def exact_case(seed, dt, B, N, C, HW):
    """q (B, C, h, w) f32, bank (B, N, C, h, w) of type dt, float64-oracle scores (B, N) f32.  Template n of sample b equals q[b] except
    in one random channel per pixel, by a random d; template N // 2 of the last sample is an exact match (score -0.0)."""
    def make():
        g = torch.Generator().manual_seed(seed)
        dv = torch.tensor(D_F32 if dt == "f32" else D_16, dtype=torch.float32)
        q = torch.randint(-3, 4, (B, C, HW), generator=g).float()
        ch = torch.randint(0, C, (B, N, 1, HW), generator=g)
        d = dv[torch.randint(0, len(dv), (B, N, 1, HW), generator=g)]
        d[B - 1, N // 2] = 0
        bank = q[:, None].repeat(1, N, 1, 1)
        bank.scatter_add_(2, ch, d)
        h, w = _hw(HW)
        q, bank = q.reshape(B, C, h, w), bank.reshape(B, N, C, h, w).to(DT[dt])
        assert torch.equal(bank.float().to(DT[dt]), bank)
        return q, bank, _ref_scores(q, bank)
    return cached(("exact", seed, dt, B, N, C, HW), make)


def shared_case(seed, dt, B, N, C, HW):
    """One bank (1, N, C, h, w) for B queries: the channel that differs is chosen per PIXEL, the query adds s in {0, 2} to it and template
    n adds d in {-2, 0, 2, 4}, so q - t = s - d in {0, +-2, +-4} in one channel and the scores stay exact."""
    def make():
        g = torch.Generator().manual_seed(seed)
        base = torch.randint(-3, 4, (1, C, HW), generator=g).float()
        ch = torch.randint(0, C, (1, 1, HW), generator=g)
        s = 2.0 * torch.randint(0, 2, (B, 1, HW), generator=g)
        d = 2.0 * torch.randint(-1, 3, (N, 1, HW), generator=g)
        q = base.repeat(B, 1, 1).scatter_add_(1, ch.expand(B, 1, HW), s)
        bank = base.repeat(N, 1, 1).scatter_add_(1, ch.expand(N, 1, HW), d)
        h, w = _hw(HW)
        q, bank = q.reshape(B, C, h, w), bank.reshape(1, N, C, h, w).to(DT[dt])
        return q, bank, _ref_scores(q, bank)
    return cached(("shared", seed, dt, B, N, C, HW), make)


# ---- which kernel ran ------------------------------------------------------------------------------------------------------------------
_LINE = re.compile(r"^sim (reg|lds) (f32|bf16|f16) LV (\d+) CMAX (\d+) CEXACT (\d+) nt (\d+) qlds (\d+) P (\d+) hpi (\d+) groups (\d+) nsplit (\d+)$")
_FIELDS = ("form", "dt", "LV", "CMAX", "CEXACT", "nt", "qlds", "P", "hpi", "groups", "nsplit")


def set_tuning(monkeypatch, variant=None, mingroups=None):
    monkeypatch.setenv("NOPE_SIM_TRACE", "1")
    for name, v in (("NOPE_SIM_VARIANT", variant), ("NOPE_SIM_MINGROUPS", mingroups)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def traced(capfd, fn):
    """fn() and the fields of the ONE NOPE_SIM_TRACE line it printed."""
    capfd.readouterr()
    out = fn()
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("sim ")]
    assert len(lines) == 1, lines
    m = _LINE.match(lines[0])
    assert m, lines[0]
    return out, {k: (v if k in ("form", "dt") else int(v)) for k, v in zip(_FIELDS, m.groups())}


def reg_grid(B, N, hpi, mingroups=1):
    """groups and workgroups per sample of the register kernel (default grid: ~4096 workgroups, at least `mingroups` groups each)."""
    groups = -(-N // hpi)
    return groups, max(1, min(4096 // B, groups // mingroups, groups))


def lds_grid(B, N):
    return N, min(-(-4096 // B), N)


def reg(dt, LV, CMAX, CEXACT, nt, qlds, P):
    return dict(form="reg", dt=dt, LV=LV, CMAX=CMAX, CEXACT=CEXACT, nt=nt, qlds=qlds, P=P, hpi=NT // P)


def lds(dt, P):
    return dict(form="lds", dt=dt, LV=4 if dt == "f32" else 8, CMAX=0, CEXACT=0, nt=0, qlds=0, P=P, hpi=1)


def check_exact(got, want, what, line):
    """Scores against the float64 oracle, bit for bit."""
    print(f"retrieval_edges {what}: {line}")
    assert same_bits(got, want), (what, line, first_diff(got, want))


def run_scoring(be, monkeypatch, capfd, dt, B, N, C, HW, want_line, seed, variant=None, mingroups=None, free_nsplit=False):
    hip, dev, _ = be
    q, bank, want = exact_case(seed, dt, B, N, C, HW)
    set_tuning(monkeypatch, variant, mingroups)
    got, line = traced(capfd, lambda: hip.similarity(q.to(dev), bank.to(dev)))
    groups, nsplit = lds_grid(B, N) if want_line["form"] == "lds" else reg_grid(B, N, want_line["hpi"], mingroups or 1)
    if free_nsplit:      # (NOPE_SIM_VARIANT & 2 sizes the grid by the device: CUs x resident workgroups)
        assert 1 <= line["nsplit"] <= groups, line
        nsplit = line["nsplit"]
    assert line == dict(want_line, groups=groups, nsplit=nsplit), (line, want_line)
    what = f"{dt} C {C} HW {HW} N {N} variant {variant} mingroups {mingroups}"
    check_exact(got, want, what, line)
    assert bits(got)[B - 1, N // 2] == bits(torch.tensor([-0.0]))[0], what      # the planted match: -0.0
    assert int(hip.topk(got, 1)[1][B - 1, 0]) == N // 2, what
    return line


# (dt, C, HW, expected form): the dispatch table of launch_similarity under the default NOPE_SIM_VARIANT (1: non-temporal loads)
FORMS = [
    # register kernel, f32, LV 4: the four-wave fold, one wave, the shuffle fold, no reduction at all
    ("f32", 8, 1024, reg("f32", 4, 8, 1, 1, 0, 256)), ("f32", 8, 256, reg("f32", 4, 8, 1, 1, 0, 64)),
    ("f32", 8, 64, reg("f32", 4, 8, 1, 1, 0, 16)), ("f32", 8, 4, reg("f32", 4, 8, 1, 1, 0, 1)),
    # register kernel, 16-bit, LV 8
    ("bf16", 8, 2048, reg("bf16", 8, 8, 1, 1, 0, 256)), ("bf16", 8, 512, reg("bf16", 8, 8, 1, 1, 0, 64)),
    ("bf16", 8, 64, reg("bf16", 8, 8, 1, 1, 0, 8)), ("bf16", 8, 8, reg("bf16", 8, 8, 1, 1, 0, 1)),
    ("f16", 8, 2048, reg("f16", 8, 8, 1, 1, 0, 256)), ("f16", 8, 512, reg("f16", 8, 8, 1, 1, 0, 64)),
    ("f16", 8, 64, reg("f16", 8, 8, 1, 1, 0, 8)), ("f16", 8, 8, reg("f16", 8, 8, 1, 1, 0, 1)),
    # channel forms: CMAX 8 with guards, CMAX 16
    ("f32", 1, 64, reg("f32", 4, 8, 0, 1, 0, 16)), ("f32", 5, 64, reg("f32", 4, 8, 0, 1, 0, 16)),
    ("f32", 9, 64, reg("f32", 4, 16, 0, 1, 0, 16)), ("f32", 16, 64, reg("f32", 4, 16, 0, 1, 0, 16)),
    ("bf16", 1, 64, reg("bf16", 8, 8, 0, 1, 0, 8)), ("bf16", 5, 64, reg("bf16", 8, 8, 0, 1, 0, 8)),
    ("bf16", 9, 64, reg("bf16", 8, 16, 0, 1, 0, 8)), ("bf16", 16, 64, reg("bf16", 8, 16, 0, 1, 0, 8)),
    ("f16", 5, 64, reg("f16", 8, 8, 0, 1, 0, 8)), ("f16", 16, 64, reg("f16", 8, 16, 0, 1, 0, 8)),
    # LDS kernel: C > 16; P not dividing 256; P > 256 (pv strides by 256, ragged); C HW = 16384 exactly
    ("f32", 17, 64, lds("f32", 16)), ("bf16", 17, 64, lds("bf16", 8)), ("f32", 24, 64, lds("f32", 16)), ("f16", 24, 64, lds("f16", 8)),
    ("f32", 4, 48, lds("f32", 12)), ("bf16", 4, 48, lds("bf16", 6)), ("f16", 4, 48, lds("f16", 6)),
    ("f32", 4, 2052, lds("f32", 513)), ("f32", 4, 4096, lds("f32", 1024)),
]


@pytest.mark.parametrize("dt,C,HW,want", FORMS, ids=[f"{f[3]['form']}-{f[0]}-C{f[1]}-HW{f[2]}" for f in FORMS])
def test_scoring_forms_exact(be, monkeypatch, capfd, dt, C, HW, want):
    """Every form of the dispatch table on exact-arithmetic inputs, B = 2, N = 2 hpi + 1 (three groups, the last one ragged; 5 for the
    LDS kernel), bit for bit against the float64 oracle, with the launch's NOPE_SIM_TRACE line asserted.
    On an MI355X every case holds with equality, the 16-bit ones included: v_sqrt_f32 returns 1, 4 and 16 for 1, 16 and 256 (worst
    per-score relative error 0.0), so the 64 * 2^-24 fallback bound is not used anywhere in this file."""
    N = 5 if want["form"] == "lds" else 2 * want["hpi"] + 1
    run_scoring(be, monkeypatch, capfd, dt, 2, N, C, HW, want, seed=100 + C + HW)


def _variant_form(dt, C, HW, v):
    """The form NOPE_SIM_VARIANT = v selects for C <= 8 or C = 16, written out by hand: bit 0 non-temporal loads (and with it the CEXACT
    and QLDS forms), bit 8 LV 4 for 16-bit banks with C <= 8 and HW / 4 <= 256, bit 16 the LDS query tile for 16-bit C = 8 banks."""
    if dt == "f32":
        return reg(dt, 4, 8 if C <= 8 else 16, int(C == 8 and bool(v & 1)), v & 1, 0, HW // 4)
    if (v & 8) and C <= 8 and HW // 4 <= 256:
        return reg(dt, 4, 8, 0, v & 1, 0, HW // 4)
    return reg(dt, 8, 8 if C <= 8 else 16, int(C == 8 and bool(v & 1)), v & 1, int(C == 8 and (v & 17) == 17), HW // 8)


VARIANTS = [(dt, 8, HW, v) for v in (0, 2, 3, 8, 9, 16, 17, 24, 25) for HW in (256, 1024) for dt in ("f32", "bf16")]
VARIANTS += [("f16", 8, 256, v) for v in (0, 8, 17)] + [("f16", 8, 1024, 17)]
VARIANTS += [("bf16", 16, 256, 8), ("bf16", 16, 256, 9), ("bf16", 8, 2048, 8), ("bf16", 8, 2048, 9), ("f16", 8, 2048, 9)]      # bit 8 refused: stays LV 8


@pytest.mark.parametrize("dt,C,HW,v", VARIANTS, ids=[f"v{v[3]}-{v[0]}-C{v[1]}-HW{v[2]}" for v in VARIANTS])
def test_scoring_variants_exact(be, monkeypatch, capfd, dt, C, HW, v):
    """The tuning forms tools/sim_bench.py and tools/small_bank_sweep.py select: plain loads (bit 0 clear), the one-round grid (2), LV 4 for
    16-bit banks (8), the swizzled LDS query tile (16, which takes effect with bit 0 only: 17).  f32 banks under the 16-bit-only bits,
    C = 16 and HW = 2048 under bit 8 show the fallback that is taken.  Same inputs and equality as test_scoring_forms_exact."""
    want = _variant_form(dt, C, HW, v)
    line = run_scoring(be, monkeypatch, capfd, dt, 2, 2 * want["hpi"] + 1, C, HW, want, seed=200 + HW, variant=v, free_nsplit=bool(v & 2))
    if v == 17 and dt != "f32":
        assert line["qlds"] == 1
    if v in (8, 9) and dt != "f32":
        assert line["LV"] == (4 if C == 8 and HW <= 1024 else 8)


PIPELINE = [("f32", 8, 1024, 11, reg("f32", 4, 8, 1, 1, 0, 256)), ("f32", 8, 256, 43, reg("f32", 4, 8, 1, 1, 0, 64)),
            ("f16", 8, 512, 43, reg("f16", 8, 8, 1, 1, 0, 64)), ("bf16", 8, 64, 325, reg("bf16", 8, 8, 1, 1, 0, 8)),
            ("f32", 5, 64, 165, reg("f32", 4, 8, 0, 1, 0, 16))]


@pytest.mark.parametrize("mingroups", [2, 3, 100])
@pytest.mark.parametrize("dt,C,HW,N,want", PIPELINE, ids=[f"{p[0]}-C{p[1]}-HW{p[2]}-N{p[3]}" for p in PIPELINE])
def test_scoring_several_groups_per_workgroup(be, monkeypatch, capfd, dt, C, HW, N, want, mingroups):
    """The software-pipelined loop: 11 groups, the last one ragged, over 5 / 3 / 1 workgroups per sample (NOPE_SIM_MINGROUPS 2 / 3 / 100), so
    workgroups of one launch run 3 and 2, 4 and 3, or all 11 iterations: the prefetch at stride gs, the peeled last group and both
    buffers of the partials (P >= 64) are used, and P < 64 takes the shuffle fold.  Bit for bit against the float64 oracle."""
    line = run_scoring(be, monkeypatch, capfd, dt, 2, N, C, HW, want, seed=300 + HW, mingroups=mingroups)
    assert line["groups"] == 11 and line["nsplit"] == {2: 5, 3: 3, 100: 1}[mingroups]
    assert mingroups == 100 or line["groups"] % line["nsplit"] != 0


def test_scoring_partials_under_adversarial_wave_order():
    """The double-buffered partials of the P >= 64 fold are a hand-off between waves with ONE barrier per iteration: wave 0 reads the four
    partials of iteration i while the other waves may already write those of iteration i + 1.  The interpreter's default schedule moves
    the waves in step and cannot see a missing `buf ^= 1`; its adversarial schedule (HIPEMU_SHUFFLE: each wave runs as far ahead as the
    barriers allow, in a pseudo-random order) is fixed when the library is first used, so the cases of
    test_scoring_several_groups_per_workgroup run again in two fresh interpreter processes, one per seed.  (The device half of that test
    is the run with real barrier timing.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "not gpu", "-k", "several_groups_per_workgroup", os.path.abspath(__file__)]
    procs = [subprocess.Popen(cmd, cwd=root, env=dict(os.environ, HIPEMU_SHUFFLE=seed), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for seed in ("1", "2")]
    for seed, pr in zip(("1", "2"), procs):
        out, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0 and " passed" in out and "failed" not in out, (seed, out[-3000:])


@pytest.mark.parametrize("dt,B,N,C,HW,want,grid", [
    ("bf16", 4100, 2 * 256 + 40, 2, 8, reg("bf16", 8, 8, 0, 1, 0, 1), (3, 1)),
    ("f32", 700, 7 * 256 + 40, 2, 4, reg("f32", 4, 8, 0, 1, 0, 1), (8, 5)),
    ("f32", 2100, 5, 17, 8, lds("f32", 2), (5, 2))], ids=["bf16-B4100", "f32-B700", "lds-B2100"])
def test_scoring_many_samples_shared_bank(be, monkeypatch, capfd, dt, B, N, C, HW, want, grid):
    """More samples than the ~4096 workgroups of a launch, one stride-0 bank: B = 4100 clamps nsplit to 1 and every workgroup walks all
    three groups; B = 700 gives 5 workgroups per sample over 8 groups (two or one each); B = 2100 on the LDS kernel gives two workgroups
    per sample with 3 and 2 templates (its n-loop iterates, both barriers of an iteration matter).  Bit for bit against the oracle."""
    hip, dev, _ = be
    q, bank, want_s = shared_case(400 + B, dt, B, N, C, HW)
    set_tuning(monkeypatch)
    got, line = traced(capfd, lambda: hip.similarity(q.to(dev), bank.to(dev)))
    assert line == dict(want, groups=grid[0], nsplit=grid[1]), line
    check_exact(got, want_s, f"shared bank {dt} B {B} N {N}", line)


@pytest.mark.parametrize("dt,C,HW,want", [("f32", 8, 64, reg("f32", 4, 8, 1, 1, 0, 16)), ("bf16", 17, 64, lds("bf16", 8))], ids=["reg", "lds"])
def test_scoring_output_placement(be, monkeypatch, capfd, dt, C, HW, want):
    """`out` (B, N + 6) prefilled with a sentinel, col_offset = 3: the scores land in columns [3, 3 + N) and the columns on either side
    keep the sentinel bit for bit (a ragged last group must not write past N)."""
    hip, dev, _ = be
    B, N = 2, 5 if want["form"] == "lds" else 2 * want["hpi"] + 1
    q, bank, want_s = exact_case(500 + C, dt, B, N, C, HW)
    set_tuning(monkeypatch)
    sentinel = -12345.5
    out = torch.full((B, N + 6), sentinel, device=dev)
    _, line = traced(capfd, lambda: hip.similarity(q.to(dev), bank.to(dev), out=out, col_offset=3))
    assert line["form"] == want["form"] and line["P"] == want["P"], line
    want_out = torch.full((B, N + 6), sentinel)
    want_out[:, 3:3 + N] = want_s
    check_exact(out, want_out, f"col_offset {dt} C {C}", line)


def test_scoring_rejected_shapes(be):
    """Shapes no kernel takes come back as error codes: more than 16384 query words for the LDS kernel, HW that is no multiple of 16 bytes
    (-> NOPE_ERR_UNSUPPORTED, -6), score_ld < N (-> NOPE_ERR_ARG, -1).  Nothing is launched."""
    hip, dev, _ = be
    d = hip.lib().dll
    q = torch.zeros(5 * 4096).to(dev)
    bank = torch.zeros(2 * 5 * 4096).to(dev)
    out = torch.zeros(8).to(dev)

    def call(dt, N, C, H, W, ld):
        return d.nope_similarity(q.data_ptr(), bank.data_ptr(), dt, out.data_ptr(), 1, N, C, H, W, N * C * H * W, ld, None)
    assert call(hip.F32, 2, 4, 64, 64, 2) == 0
    assert call(hip.F32, 2, 5, 64, 64, 2) == -6
    assert call(hip.F32, 2, 8, 1, 6, 2) == -6
    assert call(hip.BF16, 2, 8, 1, 12, 2) == -6 and call(hip.F16, 2, 8, 1, 12, 2) == -6
    assert call(hip.F32, 3, 8, 1, 4, 2) == -1
    with pytest.raises(hip.NopeError):
        hip.similarity(torch.zeros(1, 5, 64, 64).to(dev), torch.zeros(1, 2, 5, 64, 64).to(dev))


# ---- one-element probes ----------------------------------------------------------------------------------------------------------------
def probe_case(dt, C, HW, positions):
    """q (1, C, h, w), bank (1, len(positions), C, h, w): template n equals q except element positions[n] of its (C, HW) block: q + 2."""
    def make():
        g = torch.Generator().manual_seed(C * HW)
        q = torch.randint(-3, 4, (1, C * HW), generator=g).float()
        bank = q.repeat(len(positions), 1)
        bank[torch.arange(len(positions)), torch.tensor(positions)] += 2
        h, w = _hw(HW)
        q, bank = q.reshape(1, C, h, w), bank.reshape(1, len(positions), C, h, w).to(DT[dt])
        want = _ref_scores(q, bank)
        assert bool((want == -4.0).all())
        return q, bank, want
    return cached(("probe", dt, C, HW, tuple(positions)), make)


def _spread(C, HW, LV, lanes, channels):
    return [c * HW + lane * LV + e for c in channels for lane in lanes for e in range(LV)]


PROBES = [("f32", 8, 256, None, 64), ("bf16", 8, 256, None, 32), ("f16", 8, 256, None, 32),
          ("f32", 8, 1024, _spread(8, 1024, 4, (0, 63, 64, 255), (0, 3, 4, 7)), 256),
          ("bf16", 8, 2048, _spread(8, 2048, 8, (0, 63, 64, 255), (0, 7)), 256)]


@pytest.mark.parametrize("dt,C,HW,positions,P", PROBES, ids=[f"{p[0]}-HW{p[2]}" for p in PROBES])
def test_scoring_one_element_probes(be, monkeypatch, capfd, dt, C, HW, positions, P):
    """Template n differs from q in ONE element, by 2: every score is exactly -4.0.  At (8, 256) there are C HW = 2048 templates, one per
    (channel, lane, word, half-word) position; at (8, 1024) f32 and (8, 2048) bf16, 64 positions: lanes 0, 63, 64 and 255 (both ends of
    the first wave, the start of the second, the end of the last), the first / last (and for f32 the two middle) channels, every
    element of the lane's vector."""
    hip, dev, _ = be
    positions = list(range(C * HW)) if positions is None else positions
    q, bank, want = probe_case(dt, C, HW, positions)
    set_tuning(monkeypatch)
    got, line = traced(capfd, lambda: hip.similarity(q.to(dev), bank.to(dev)))
    assert line["form"] == "reg" and line["P"] == P and line["CEXACT"] == 1, line
    bad = (bits(got) != bits(want)).nonzero()
    assert not len(bad), (dt, HW, "columns", bad[:8, 1].tolist(), "elements", [positions[i] for i in bad[:8, 1].tolist()], got[0, bad[:8, 1]].tolist())


# ---- non-finite inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,HW,form", [(8, 64, "reg"), (8, 2048, "reg"), (17, 64, "lds")])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_scoring_nonfinite(be, monkeypatch, capfd, dt, C, HW, form):
    """A zero query against templates with one NaN element, one inf element, one 1e10 element (its quartic overflows f32), all elements
    3e9 (the channel sum overflows; inf in f16), and three all-zero templates: the scores are the f32 oracle's NaN, -inf, -inf, -inf and
    -0.0 as bit patterns (any NaN for a NaN), and nope_topk over them is topk_desc_lowest_index: the NaN first, then the zeros by index."""
    hip, dev, _ = be
    if HW == 2048 and dt == "f32":
        HW = 1024

    def make():
        bank = torch.zeros(1, 7, C * HW)
        bank[0, 1, 3 * HW + 17] = NAN
        bank[0, 2, HW - 1] = INF
        bank[0, 4, (C - 1) * HW + 5] = 1e10
        bank[0, 5] = 3e9
        h, w = _hw(HW)
        q, bank = torch.zeros(1, C, h, w), bank.reshape(1, 7, C, h, w).to(DT[dt])
        want = R.similarity_scores(q, bank.float())          # in f32: the overflow is part of the contract
        assert torch.isnan(want[0, 1]) and want[0, [2, 4, 5]].tolist() == [-INF] * 3 and bool((bits(want)[0, [0, 3, 6]] == bits(torch.tensor(-0.0))).all())
        return q, bank, want
    q, bank, want = cached(("nonfinite", dt, C, HW), make)
    set_tuning(monkeypatch)
    got, line = traced(capfd, lambda: hip.similarity(q.to(dev), bank.to(dev)))
    assert line["form"] == form, line
    assert same_bits(got, want), (got.tolist(), want.tolist())
    vals, idx = hip.topk(got, 5)
    assert torch.equal(idx.cpu(), R.topk_desc_lowest_index(want, 5)) and idx.cpu().tolist() == [[1, 0, 3, 6, 2]]
    assert same_bits(vals, torch.gather(got.cpu(), 1, idx.cpu()))


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------
TOPK_N = [8, 64, 65, 256, 257, 513, 1000, 4096]


def tie_rows(N):
    """(9, N) f32: rows whose equal values sit on different lanes, waves and strides of the 256-thread scan."""
    def make():
        g = torch.Generator().manual_seed(N)
        three = lambda: torch.tensor([-2.0, 1.0, 5.0])[torch.randint(0, 3, (N,), generator=g)]
        low = lambda: -1.0 - torch.randperm(N, generator=g).float()          # distinct, all below the planted maxima
        rows = [torch.full((N,), 2.0), three()]
        r = low()                                                            # equal maxima on one thread, two strides (n, n + 256)
        a = 5 if N > 261 else 0
        r[a] = r[a + 256 if N > 261 else N - 1] = 7.0
        if N > 3 * 256:
            r[a + 512] = 7.0
        rows.append(r)
        r = low()                                                            # equal maxima across a wave and across the stride
        for n, v in ((63, 9.0), (64, 9.0), (255, 8.0), (256, 8.0), (N - 2, 6.0), (N - 1, 6.0), (0, 6.0)):
            if n < N:
                r[n] = v
        rows.append(r)
        r = three()
        r[0::2] = -INF
        rows.append(r)
        r = three()
        r[0], r[N - 1] = INF, NAN
        rows.append(r)
        r = three()                                                          # NaNs in different waves and strides
        for n in (1, 70, 130, 200, 300, 257 + 64, N - 1):
            if n < N:
                r[n] = NAN
        rows.append(r)
        rows += [torch.arange(N).float(), -torch.arange(N).float()]
        s = torch.stack(rows)
        return s, {k: R.topk_desc_lowest_index(s, k) for k in (1, 5, 16, N) if k <= min(N, 16)}
    return cached(("ties", N), make)


def check_topk(scores_cpu, vals, idx, want_idx, what):
    assert torch.equal(idx.cpu(), want_idx), (what, idx.cpu().tolist(), want_idx.tolist())
    assert bool(torch.equal(bits(vals), bits(torch.gather(scores_cpu, 1, want_idx)))), what


@pytest.mark.parametrize("N", TOPK_N)
def test_topk_ties_across_lanes_waves_strides(be, N):
    """k = 1, 5, 16 (= KMAX; and k = N for N = 8) over rows of nine kinds -- all equal; three distinct values (hundreds of ties); equal
    maxima at n and n + 256 (one thread, two strides); equal maxima at 63 / 64 and 255 / 256; -inf on every even column; +inf at column 0
    with NaN at the last; NaNs in several waves; ascending; descending -- three rows of different kinds per launch.  Indices are
    topk_desc_lowest_index, values the gathered scores as bit patterns, NaN included."""
    hip, dev, _ = be
    s, want = tie_rows(N)
    sd = s.to(dev)
    for k, want_idx in want.items():
        for r0 in (0, 3, 6):
            vals, idx = hip.topk(sd[r0:r0 + 3].contiguous(), k)
            check_topk(s[r0:r0 + 3], vals, idx, want_idx[r0:r0 + 3], (N, k, r0))


def test_topk_c_abi_ld_vals_and_kmax(be):
    """nope_topk through the C ABI: score_ld > N with sentinel columns past N that beat every score (never chosen, in any of 3 rows);
    vals = NULL; k = 17 > KMAX and k > N -> NOPE_ERR_ARG."""
    hip, dev, _ = be
    d = hip.lib().dll
    N, ld, k = 300, 307, 16
    s, _ = tie_rows(513)
    full = torch.full((3, ld), 1e30)
    full[:, :N] = s[[1, 3, 6], :N]
    want_idx = R.topk_desc_lowest_index(full[:, :N], k)
    fd = full.to(dev)
    idx = torch.full((3, k), -1, dtype=torch.int64).to(dev)
    vals = torch.zeros(3, k).to(dev)
    assert d.nope_topk(fd.data_ptr(), idx.data_ptr(), vals.data_ptr(), 3, N, k, ld, None) == 0
    check_topk(full, vals, idx, want_idx, "ld > N")
    idx2 = torch.full((3, k), -1, dtype=torch.int64).to(dev)
    assert d.nope_topk(fd.data_ptr(), idx2.data_ptr(), None, 3, N, k, ld, None) == 0
    assert torch.equal(idx2.cpu(), want_idx)
    assert d.nope_topk(fd.data_ptr(), idx2.data_ptr(), None, 3, N, 17, ld, None) == -1
    assert d.nope_topk(fd.data_ptr(), idx2.data_ptr(), None, 3, 8, 9, ld, None) == -1
    assert d.nope_topk(fd.data_ptr(), idx2.data_ptr(), None, 3, N, k, N - 1, None) == -1
    assert torch.equal(idx2.cpu(), want_idx)          # (the refused calls wrote nothing)


# ---- nope_gather_topk ------------------------------------------------------------------------------------------------------------------
GATHER = [(1, 7), (2, 7), (3, 7), (8, 7), (8, 8), (4, 10), (5, 3), (7, 100), (8, 341)]


def shard_bounds(N, G):
    base, extra = divmod(N, G)
    lo = [r * base + min(r, extra) for r in range(G + 1)]
    return list(zip(lo[:-1], lo[1:]))


def gather_case(G, N):
    """full (3, N) scores with ties across the shard boundaries (and a NaN, a -inf), the (G, 3, nmax) gathered tensor with NaN pads."""
    def make():
        g = torch.Generator().manual_seed(G * 1000 + N)
        full = torch.tensor([-3.0, 0.5, 4.0])[torch.randint(0, 3, (3, N), generator=g)]
        full[1] = 4.0                                                        # one value everywhere: every boundary is a tie
        if N > 6:
            full[2, N - 1], full[2, N // 2] = NAN, -INF
        nmax = -(-N // G)
        gathered = torch.full((G, 3, nmax), NAN)
        for r, (lo, hi) in enumerate(shard_bounds(N, G)):
            gathered[r, :, :hi - lo] = full[:, lo:hi]
        return full, gathered
    return cached(("gather", G, N), make)


@pytest.mark.parametrize("G,N", GATHER)
def test_gather_topk_every_split(be, G, N):
    """The (G, B, nmax) all-gathered slices built by hand from a full (B, N) matrix, for N < G (base = 0), N % G = 0 (no cut), G = 1 and
    uneven splits, with NaN in every pad column: the owned similarity is the full matrix bit for bit, the indices are nope_topk's on the
    full matrix (a pad that is read would rank first), k = 0 fills the similarity only, and `vals` through the C ABI are nope_topk's."""
    hip, dev, _ = be
    full, gathered = gather_case(G, N)
    k = min(5, N)
    gd = gathered.to(dev)
    want_vals, want_idx = hip.topk(full.to(dev), k)
    assert torch.equal(want_idx.cpu(), R.topk_desc_lowest_index(full, k))
    sim, idx = hip.gather_topk(gd, N, k)
    assert same_bits(sim, full) and sim.shape == (3, N), (G, N)
    assert torch.equal(idx.cpu(), want_idx.cpu()), (G, N, idx.cpu().tolist(), want_idx.cpu().tolist())
    sim0, idx0 = hip.gather_topk(gd, N, 0)
    assert idx0 is None and same_bits(sim0, full)
    d = hip.lib().dll
    sim2 = torch.full((3, N), -7.0).to(dev)
    idx2 = torch.full((3, k), -1, dtype=torch.int64).to(dev)
    vals2 = torch.zeros(3, k).to(dev)
    assert d.nope_gather_topk(gd.data_ptr(), G, 3, N, sim2.data_ptr(), idx2.data_ptr(), vals2.data_ptr(), k, None) == 0
    assert same_bits(sim2, full) and torch.equal(idx2.cpu(), want_idx.cpu())
    assert torch.equal(torch.isnan(vals2.cpu()), torch.isnan(want_vals.cpu())) and same_bits(vals2, want_vals)


# ---- nope_topk_merge -------------------------------------------------------------------------------------------------------------------
def merge_rows(N):
    def make():
        g = torch.Generator().manual_seed(7000 + N)
        three = lambda: torch.tensor([-2.0, 1.0, 5.0])[torch.randint(0, 3, (N,), generator=g)]
        rows = [torch.full((N,), 3.0), three(), torch.randn(N, generator=g)]
        r = torch.full((N,), -INF)                                           # real -inf scores next to pads
        r[N - 2] = 1.0
        rows.append(r)
        r = three()
        r[1::2] = -INF
        r[N - 1], r[N // 2] = NAN, NAN
        rows.append(r)
        rows.append(torch.full((N,), -INF))
        return torch.stack(rows)
    return cached(("merge", N), make)


def shard_lists(hip, dev, full, G, k):
    """The (B, G k) candidate lists all_gather_topk_pairs hands to nope_topk_merge: per shard, nope_topk with min(k, n_local) on its
    contiguous slice, local -> global indices, padded to k with (-inf, INT64_MAX), shards in rank order."""
    B, N = full.shape
    cv = torch.full((B, G, k), -INF)
    ci = torch.full((B, G, k), PAD_IDX, dtype=torch.int64)
    for r, (lo, hi) in enumerate(shard_bounds(N, G)):
        kl = min(k, hi - lo)
        if kl:
            v, i = hip.topk(full[:, lo:hi].contiguous().to(dev), kl)
            cv[:, r, :kl], ci[:, r, :kl] = v.cpu(), i.cpu() + lo
    return cv.reshape(B, G * k), ci.reshape(B, G * k)


def test_topk_merge_pad_before_real_minus_inf(be):
    """The list the tie rule used to get wrong: [-1, pad, pad, -inf (idx 5), -2 (idx 3), -inf (idx 4)], k = 3.  Ordered by list position
    the first pad beat both real -inf scores (-> [0, 3, INT64_MAX]); ordered by the carried index the answer is nope_topk's on the full
    row: [0, 3, 4].  With k = 6 the two pads come last, in list order."""
    hip, dev, _ = be
    cv = torch.tensor([[-1.0, -INF, -INF, -INF, -2.0, -INF]])
    ci = torch.tensor([[0, PAD_IDX, PAD_IDX, 5, 3, 4]])
    vals, idx = hip.topk_merge(cv.to(dev), ci.to(dev), 3)
    assert idx.cpu().tolist() == [[0, 3, 4]] and vals.cpu().tolist() == [[-1.0, -2.0, -INF]]
    vals, idx = hip.topk_merge(cv.to(dev), ci.to(dev), 6)
    assert idx.cpu().tolist() == [[0, 3, 4, 5, PAD_IDX, PAD_IDX]]


@pytest.mark.parametrize("G", [1, 2, 3, 8])
@pytest.mark.parametrize("N", [5, 7, 20, 100])
def test_topk_merge_equals_full_topk(be, G, N):
    """Per-shard top-k lists of a full matrix split over G shards (shards with fewer than k columns, or none: N = 5 and 7 over 8), padded as
    all_gather_topk_pairs pads them: ties inside and across shards, NaN scores, and rows of real -inf scores next to the pads.  The merge is
    nope_topk of the full matrix, indices and value bits, for k = 1 and 5 (the shards always hold k real candidates together: N >= k)."""
    hip, dev, _ = be
    full = merge_rows(N)
    for k in (1, 5):
        want_vals, want_idx = hip.topk(full.to(dev), k)
        assert torch.equal(want_idx.cpu(), R.topk_desc_lowest_index(full, k))
        cv, ci = cached(("lists", be[2], N, G, k), lambda: shard_lists(hip, dev, full, G, k))
        vals, idx = hip.topk_merge(cv.to(dev), ci.to(dev), k)
        assert torch.equal(idx.cpu(), want_idx.cpu()), (G, N, k, idx.cpu().tolist(), want_idx.cpu().tolist())
        assert same_bits(vals, want_vals), (G, N, k)
