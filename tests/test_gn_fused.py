"""Operator-level parity of the fused GroupNorm statistics plumbing (include/nope_hip.h: nope_conv_op, nope_gn_op,
nope_op_gn_finalize, nope_op_absmax_f32), each piece against float64 torch on operands rounded to the mode's storage type:

  (a) the four emitters of ConvArgs::colstats -- the wide epilogue's 64-row and 16-row forms, the small-tile kernel's 16 / 32 / 64-row form,
      splitk_reduce_stats_kernel -- and conv_stat_rows, which says which of them a shape may use;
  (b) the consumer, gn_apply_kernel<FOLD = true> and gn_fold_kernel + the partial path, on statistics built in torch;
  (c) FiLM (gn_apply_kernel<FILM = true>);
  (d) out_stats (gn_apply_kernel<OS = true>) -> gn_finalize_kernel -> the PreNorm epilogue of a 1x1 conv;
  (e) the range maxima (absmax_f32_kernel, gn_apply's AMAX, ConvArgs::out_amax), which are exact.

Every test runs on the device and, in f32 at its smallest shapes, on the interpreter (tests/hipemu).  Inputs carry a DC offset of 0.3 .. 0.5
standard deviations like the other GroupNorm tests: the one-pass f32 variance (Q / cnt - mean^2) is a known property of these kernels and not
what is measured here."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_sweeps import _ref as _conv_ref

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
OP_TOL = {0: 2e-5, 1: 4e-2, 2: 5e-3, 3: 3e-5}                   # tests/test_kernels_parity.py
SWEEP_TOL = {0: 1e-5, 1: 8e-3, 2: 1e-3, 3: 3e-5, 4: 3e-5}       # tests/test_gpu_sweeps.py: test_conv_random_sweep / _f16x2
# (a): a conv element error e (relative to max |v|) moves |S - sum v| / sum |v| by <= ~5 e and |Q - sum v^2| / sum v^2 by <= ~6.4 e for Gaussian
# outputs: 8 x the sweep bound of modes 0, 3, 4; the 16-bit modes sum their f32 accumulators BEFORE the output rounding: the f32 bound
# -> {0: 8e-5, 1: 8e-5, 2: 8e-5, 3: 2.4e-4, 4: 2.4e-4}.  An MI355X shows 1.4e-6 / 4.5e-7 / 5.6e-7 / 1.1e-5 / 1.8e-5, each more than 10 x under
# its bound, so (tests/util.py: guards sit ~3 x above what is observed) the bounds are tightened to:
STAT_TOL = {0: 5e-6, 1: 2e-6, 2: 2e-6, 3: 3e-5, 4: 6e-5}
POLICY_KEYS = ("NOPE_CONV_SMALL", "NOPE_CONV_PP", "NOPE_STATS16", "NOPE_HALO_SPLIT_MIN_CHUNKS", "NOPE_GN_MIN_GRID")
SPLIT = {"NOPE_HALO_SPLIT_MIN_CHUNKS": "2", "NOPE_CONV_PP": "3"}      # (f32 plans no ping-pong kernel by itself: the tap-resident split needs bit 0)


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def _q(x, dt, hip):
    return x.to(hip.torch_dtype(dt)).float()


def _policy(monkeypatch, pol):
    for k in POLICY_KEYS:
        if k in pol:
            monkeypatch.setenv(k, pol[k])
        else:
            monkeypatch.delenv(k, raising=False)


def _trace(err):
    """(kernel, K splits) of the one conv launch in a NOPE_CONV_TRACE capture."""
    lines = [ln for ln in err.splitlines() if ln.startswith("conv ")]
    assert len(lines) == 1, err
    f = lines[0].split()
    return ("small" if f[1].startswith("small") else f[1]), int(f[f.index("grid") + 1].split(",")[2]), lines[0]


def _expected_kernel(hip, pol, mode, k, dma, rep1, split):
    if not dma:
        return "generic"
    if split:
        return "halo256"
    if mode == hip.CONV_UP2:
        return "dma128"
    if pol.get("NOPE_CONV_PP") == "11":           # the ping-pong kernels at any tile count: tap-resident for 3x3 in (sample, pixel) order
        if mode == hip.CONV_STRIDE2:
            return "dma128"
        return "halo256" if (mode == hip.CONV_PLAIN and k == 3 and rep1 == 1) else "pp256"
    return "dma128" if pol.get("NOPE_CONV_SMALL") == "0" else "small"


class _ConvCase:
    """One conv problem: operands, float64 result of the rounded operands (computed once, shared by every launch policy)."""

    def __init__(self, hip, dev, dt, g, mode, k, n, c1, c2, rep1, hs, ws, cout, bias):
        self.mode, self.k, self.n, self.c1, self.c2, self.rep1, self.hs, self.ws, self.cout = mode, k, n, c1, c2, rep1, hs, ws, cout
        rn = lambda *s: torch.randn(*s, generator=g)
        x1 = rn(n // rep1, c1, hs, ws) * 2 + 0.4
        x2 = rn(n, c2, hs, ws) * 2 + 0.4 if c2 else None
        cin = c1 + c2
        wshape = (cout, cin * 4, 1, 1) if mode == hip.CONV_DOWN2 else (cout, cin, k, k)
        self.w = (rn(*wshape) / (wshape[1] * k * k) ** 0.5).to(dev)
        self.b = rn(cout).to(dev) if bias else None
        self.ntaps = 4 if mode == hip.CONV_DOWN2 else k * k
        self.x1, self.x2 = hip.to_nhwc(x1.to(dev), dt), (hip.to_nhwc(x2.to(dev), dt) if c2 else None)
        xin = _q(x1, dt, hip).repeat_interleave(rep1, 0)
        if c2:
            xin = torch.cat((xin, _q(x2, dt, hip)), 1)
        v = _conv_ref(mode, hip, xin.double(), _q(self.w.cpu(), dt, hip).double(), self.b.cpu().double() if bias else None)
        self.v64 = v.permute(0, 2, 3, 1).reshape(-1, cout)          # [M][Cout], NHWC row order
        self.M = self.v64.shape[0]
        self.hw = v.shape[2] * v.shape[3]

    def rows(self, hip, dt, **kw):
        return hip.op_conv_stat_rows(dt, self.c1, self.c2, self.rep1, self.hs, self.ws, self.mode, self.ntaps, self.cout, self.n, **kw)

    def launch(self, hip, dt, **kw):
        return hip.op_conv_ex(dt, self.x1, self.w, self.b, src2=self.x2, mode=self.mode, rep1=self.rep1, n_hyp=self.n, **kw)

    def stat_errors(self, cs, rows):
        v = self.v64.reshape(self.M // rows, rows, self.cout)
        cs = cs.double().cpu().reshape(self.M // rows, self.cout, 2)
        e1 = ((cs[..., 0] - v.sum(1)).abs() / v.abs().sum(1)).max()
        e2 = ((cs[..., 1] - (v * v).sum(1)).abs() / (v * v).sum(1)).max()
        return float(e1), float(e2)


GUARD = 256


def _emit_and_check(hip, dev, dt, case, rows, split_k, capfd, tag):
    """The four requirements of an emitting launch; returns (kernel, splits, e1, e2)."""
    used = (case.M // rows) * case.cout * 2
    buf = torch.full((used + GUARD,), float("nan"), device=dev)
    capfd.readouterr()
    out = case.launch(hip, dt, colstats=buf, stat_rows=rows, split_k=split_k)
    kind, splits, line = _trace(capfd.readouterr().err)
    assert not torch.isnan(buf[:used]).any(), (tag, "unwritten statistics", line)
    assert torch.isnan(buf[used:]).all(), (tag, "wrote past the statistics", line)
    plain = case.launch(hip, dt, split_k=split_k)
    assert torch.equal(out, plain), (tag, "the output changed with colstats", line)
    again = torch.full((used + GUARD,), float("nan"), device=dev)
    case.launch(hip, dt, colstats=again, stat_rows=rows, split_k=split_k)
    assert torch.equal(buf[:used], again[:used]), (tag, "statistics not reproducible", line)
    e1, e2 = case.stat_errors(buf[:used], rows)
    return kind, splits, e1, e2


def _refused(hip, dev, case, dt, rows, **kw):
    buf = torch.full((2 * case.M * case.cout + GUARD,), float("nan"), device=dev)
    with pytest.raises(hip.NopeError):
        case.launch(hip, dt, colstats=buf, stat_rows=rows, **kw)
    assert torch.isnan(buf).all()


@pytest.mark.parametrize("dt", [0, 1, 2, 3, 4])
def test_conv_colstats_emitters(be, dt, monkeypatch, capfd):
    """(a) Every emitter of the fused column statistics against float64 column sums of the conv + bias of the rounded operands, per entry
    |S - sum v| / sum |v| and |Q - sum v^2| / sum v^2 (bounds: STAT_TOL).  Per launch: the buffer is pre-filled with NaN and must be fully
    written, a NaN guard behind it untouched, the output bit-identical to the launch without colstats, a second launch bit-identical
    statistics; NOPE_CONV_TRACE says which kernel ran and every case states what conv_stat_rows must answer.
    Emitters: wide epilogue 64-row (dma128 / pp256 / halo256 / generic) and 16-row (dma128, halo256), small-tile kernel 64 / 32 / 16-row,
    splitk_reduce_stats_kernel 64 / 32 / 16-row.  Mode 4 (f16x2) exists on the ping-pong kernels only: NOPE_CONV_PP=11, device.
    The interpreter runs f32 on two shapes per group.
    Worst on an MI355X, (e1, e2) per mode: f32 (4.6e-7, 1.4e-6), bf16 (1.9e-7, 4.5e-7), f16 (2.0e-7, 5.6e-7), bf16x3 (5.8e-6, 1.1e-5),
    f16x2 (1.6e-5, 1.8e-5); bounds STAT_TOL 5e-6 / 2e-6 / 2e-6 / 3e-5 / 6e-5."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs every mode)")
    P, UP2, DOWN2, UP2P, S2 = hip.CONV_PLAIN, hip.CONV_UP2, hip.CONV_DOWN2, hip.CONV_UP2P, hip.CONV_STRIDE2
    g = torch.Generator().manual_seed(700 + dt)
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    tol = STAT_TOL[dt]
    worst, seen = [0.0, 0.0], set()
    mk = lambda *a: _ConvCase(hip, dev, dt, g, *a)

    def run(case, pol, want_rows, dma=True, split_k=False, tag=""):
        _policy(monkeypatch, pol)
        rows = case.rows(hip, dt)
        tag = (tag, dt, sorted(pol.items()), case.mode, case.k, case.n, case.c1, case.c2, case.cout, case.hs, case.ws)
        assert rows == want_rows, (tag, rows)
        if rows == 0:
            for r in (16, 32, 64):
                if case.M % r == 0:
                    _refused(hip, dev, case, dt, r, split_k=split_k)
            return
        kind, splits, e1, e2 = _emit_and_check(hip, dev, dt, case, rows, split_k, capfd, tag)
        want = _expected_kernel(hip, pol, case.mode, case.k, dma, case.rep1, split_k)
        assert kind == want and (splits > 1) == split_k, (tag, kind, want, splits)
        seen.add((kind, rows, splits > 1))
        worst[0], worst[1] = max(worst[0], e1), max(worst[1], e2)
        assert e1 < tol and e2 < tol, (tag, kind, e1, e2)

    # ---- 8 x 8 maps: 64-row blocks.  (mode, k, c1, c2, rep1, source side, LDS-DMA eligible)
    geoms = [(P, 3, 64, 0, 1, 8, True), (P, 1, 64, 0, 1, 8, True), (P, 3, 64, 64, 1, 8, True), (DOWN2, 1, 64, 0, 1, 16, True),
             (S2, 3, 64, 0, 1, 16, True), (UP2, 3, 64, 0, 1, 4, True), (P, 3, 40, 0, 1, 8, False), (P, 1, 40, 0, 1, 8, False)]
    couts = [8, 24, 64, 200, 384]
    policies = [{}, {"NOPE_CONV_SMALL": "0"}, {"NOPE_CONV_SMALL": "2"}]
    if name == "gpu":
        policies.append({"NOPE_CONV_PP": "11"})
    if dt == 4:
        policies = [{"NOPE_CONV_PP": "11"}] if name == "gpu" else []
        geoms = [gm for gm in geoms if gm[0] in (P, DOWN2) and gm[6]]
    if name == "emu":
        geoms, couts = [geoms[2], geoms[6]], [24]
    cases64 = []
    for gi, (mode, k, c1, c2, rep1, side, dma) in enumerate(geoms):
        for ci, cout in enumerate(couts):
            n = 3 if (gi + ci) % 2 == 0 else 1          # M = 192 (M % 128 == 64: the last tile's second wave row owns no block) / 64
            if c2:                                      # two sources, the first shared by all hypotheses of a sample pair
                n, rep1 = (4 if n == 3 else 2), 2
            cases64.append((mk(mode, k, n, c1, c2, rep1, side, side, cout, (gi + ci) % 3 != 1), dma))
    assert {c.cout for c, _ in cases64} == set(couts) and {c.b is None for c, _ in cases64} == {True, False}
    for pol in policies:
        for case, dma in cases64:
            run(case, pol, 64, dma, tag="8x8")
    # ---- a 16 x 16 map, two samples: four blocks per sample
    c16 = mk(P, 3, 2, 64, 0, 1, 16, 16, 24, True)
    for pol in (policies[:1] if name == "emu" else policies):
        run(c16, pol, 64, tag="16x16")
    # ---- 4 x 4 maps: 16-row blocks; 4 x 8 maps: 32-row blocks
    for n in ((4,) if name == "emu" else (4, 5)):
        m44, m48 = mk(P, 3, n, 64, 0, 1, 4, 4, 24, True), mk(P, 3, n, 64, 0, 1, 4, 8, 200, n == 4)
        long44, long48 = mk(P, 3, n, 128, 0, 1, 4, 4, 72, True), mk(P, 3, n, 128, 0, 1, 4, 8, 24, False)
        g44 = mk(P, 3, n, 40, 0, 1, 4, 4, 24, True)
        if dt != 4:
            run(m44, {}, 16, tag="4x4 small-tile")
            run(m44, {"NOPE_CONV_SMALL": "0"}, 16, tag="4x4 wide 16-row")
            run(m44, {"NOPE_CONV_SMALL": "0", "NOPE_STATS16": "0"}, 0, tag="4x4 wide, 16-row form off")
            run(g44, {}, 0, dma=False, tag="4x4 generic")
            run(long44, SPLIT, 16, split_k=True, tag="4x4 split-K reduce")
            run(m48, {}, 32, tag="4x8 small-tile")
            run(m48, {"NOPE_CONV_SMALL": "0"}, 0, tag="4x8 wide")
            if name == "gpu":
                run(long48, SPLIT, 32, split_k=True, tag="4x8 split-K reduce")
        if name == "gpu":
            run(m44, {"NOPE_CONV_PP": "11"}, 16, tag="4x4 tap-resident 16-row")
            run(m48, {"NOPE_CONV_PP": "11"}, 0, tag="4x8 tap-resident")
    if dt != 4 and name == "gpu":
        # 128 samples of a 4 x 4 map: WITHOUT colstats this 3x3 launch runs position-major on the 128 x 192 kernel, whose row order has no
        # per-sample 16-row blocks (launch_conv refuses that pair); with colstats it is planned in (sample, pixel) order -- same output bits
        pm = mk(P, 3, 128, 64, 0, 1, 4, 4, 24, True)
        _policy(monkeypatch, {"NOPE_CONV_SMALL": "0"})
        assert pm.rows(hip, dt) == 16
        capfd.readouterr()
        pm.launch(hip, dt)
        assert " posmajor 1 " in _trace(capfd.readouterr().err)[2]
        kind, splits, e1, e2 = _emit_and_check(hip, dev, dt, pm, 16, False, capfd, "posmajor")
        buf = torch.empty(pm.M // 16 * pm.cout * 2, device=dev)
        capfd.readouterr()
        pm.launch(hip, dt, colstats=buf, stat_rows=16)
        assert " posmajor 0 " in _trace(capfd.readouterr().err)[2] and kind == "dma128"
        assert e1 < tol and e2 < tol, ("posmajor", e1, e2)
        worst[0], worst[1] = max(worst[0], e1), max(worst[1], e2)
    # ---- refusals: NopeError and an untouched buffer
    if dt != 4:
        _policy(monkeypatch, {})
        rc = mk(P, 3, 2, 64, 0, 1, 8, 8, 24, True)
        rs = torch.zeros_like(rc.launch(hip, dt))
        assert rc.rows(hip, dt) == 64 and rc.rows(hip, dt, resid=True) == 0 and rc.rows(hip, dt, out_nchw=True) == 0 and rc.rows(hip, dt, act_relu=True) == 0
        _refused(hip, dev, rc, dt, 64, resid=rs)
        _refused(hip, dev, rc, dt, 64, act_relu=True)
        _refused(hip, dev, rc, dt, 64, out_nchw=True)
        for bad in (0, 16, 32, 128):
            _refused(hip, dev, rc, dt, bad)
        up = mk(UP2P, 3, 2, 64, 0, 1, 4, 4, 24, True)
        up.ntaps = 4
        assert up.rows(hip, dt) == 0
        _refused(hip, dev, up, dt, 64)
    print(f"colstats emitters dt {dt} [{name}]: worst e1 {worst[0]:.2e} e2 {worst[1]:.2e} (bound {tol:.1e}); emitters {sorted(seen)}")
    if name == "gpu" and dt != 4:
        assert {("dma128", 64, False), ("dma128", 16, False), ("small", 64, False), ("small", 32, False), ("small", 16, False), ("generic", 64, False),
                ("halo256", 16, True), ("halo256", 32, True), ("halo256", 64, False), ("halo256", 16, False), ("pp256", 64, False)} <= seen, seen
    if name == "gpu" and dt == 4:
        assert {("halo256", 64, False), ("halo256", 16, False), ("pp256", 64, False)} <= seen, seen


def _torch_colstats(xq, blocks):
    """[n][blocks][C][2] (sum, sum of squares) of x (n, C, h, w) over `blocks` runs of pixels, float64 -> f32 (any block count: runs may be empty)."""
    n, C = xq.shape[:2]
    px = xq.double().reshape(n, C, -1)
    HW = px.shape[2]
    cs = torch.zeros(n, blocks, C, 2, dtype=torch.float64)
    for b in range(blocks):
        run = px[:, :, b * HW // blocks:(b + 1) * HW // blocks]
        cs[:, b, :, 0], cs[:, b, :, 1] = run.sum(2), (run * run).sum(2)
    return cs.float()


def _gn_ref(xq, G, ga, be_, eps, act, emb=None, resid=None, x_rep=1, resid_rep=1, film=None):
    y = F.group_norm(xq.double().repeat_interleave(x_rep, 0), G, ga.double(), be_.double(), eps)
    if film is not None:
        C = xq.shape[1]
        f = film.double().reshape(-1, 2 * C)
        y = y * (1 + f[:, :C, None, None]) + f[:, C:, None, None]
    if act:
        y = F.silu(y)
    if emb is not None:
        y = y + emb.double()[:, :, None, None]
    if resid is not None:
        y = y + resid.double().repeat_interleave(resid_rep, 0)
    return y


SHAPES = {16: (4, 4), 60: (6, 10), 64: (8, 8), 256: (16, 16)}


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_gn_consumer_of_colstats(be, dt):
    """(b) gn_apply_kernel<FOLD = true> (every workgroup folds its sample's column statistics: the 8-wide unrolled loop and its tail) and
    gn_fold_kernel + the partial path, on statistics computed in torch (float64 sums of the rounded x, cast to f32: any block count),
    against float64 group_norm + SiLU + emb + resid at OP_TOL; the two forms give bit-identical y.  Block counts 1 .. 17, groups
    narrower than a 16-byte vector ((16, 8), (24, 8): the coefficient path without `one_group`) up to C = 2048 (the ch_s[2048] arrays),
    16 .. 256 pixels, x / resid shared by 2 or 3 hypotheses, eps 1e-5 and 1e-6, every (act, resid, emb) combination, the libm and (f32) the
    hardware SiLU.  Refused: C > 2048, FiLM with colstats, FiLM with out_stats.  The interpreter runs f32 on two shapes.
    Worst on an MI355X: f32 2.1e-7 (bound 2e-5), bf16 3.7e-3 (4e-2), f16 4.5e-4 (5e-3)."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs every storage type)")
    g = torch.Generator().manual_seed(800 + dt)
    rn = lambda *s: torch.randn(*s, generator=g)
    tol = OP_TOL[dt]
    worst = 0.0

    def one(C, G, HW, blocks, n, x_rep, resid_rep, eps, act=True, use_emb=True, use_rs=True, fast=False):
        nonlocal worst
        h, w = SHAPES[HW]
        x = rn(n // x_rep, C, h, w) * 2 + 0.5
        ga, be_, emb, rs = rn(C), rn(C), rn(n, C), rn(n // resid_rep, C, h, w)
        xq = _q(x, dt, hip)
        cs = _torch_colstats(xq, blocks).to(dev)
        kw = dict(act_silu=act, emb=emb.to(dev) if use_emb else None, resid=hip.to_nhwc(rs.to(dev), dt) if use_rs else None,
                  x_rep=x_rep, resid_rep=resid_rep, eps=eps, fast_silu=fast)
        xs = hip.to_nhwc(x.to(dev), dt)
        y_inline = hip.op_group_norm_ex(dt, xs, ga.to(dev), be_.to(dev), G, colstats=cs, **kw)
        y_fold = hip.op_group_norm_ex(dt, xs, ga.to(dev), be_.to(dev), G, colstats=cs, fold_launch=True, **kw)
        tag = (dt, C, G, HW, blocks, n, x_rep, resid_rep, eps, act, use_emb, use_rs, fast)
        assert torch.equal(y_inline, y_fold), (tag, "inline fold and gn_fold differ")
        ref = _gn_ref(xq, G, ga, be_, eps, act, emb if use_emb else None, _q(rs, dt, hip) if use_rs else None, x_rep, resid_rep)
        e = float((hip.to_nchw(y_inline, dt).cpu().double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, e)
        assert e < tol, (tag, e)

    CG = [(16, 8), (24, 8), (48, 8), (192, 8), (192, 1), (384, 32), (1536, 8), (2048, 1), (2048, 32)]
    BLOCKS, HWS = [1, 3, 8, 9, 16, 17], [16, 60, 64, 256]
    NREP = [(1, 1, 1), (3, 1, 1), (3, 3, 1), (6, 2, 1), (6, 3, 2), (6, 1, 2), (6, 2, 2)]       # (n, x_rep, resid_rep)
    if name == "emu":
        one(24, 8, 16, 9, 3, 3, 1, 1e-5)
        one(48, 8, 60, 3, 2, 1, 2, 1e-6)
    else:
        seen = set()
        for i, (C, G) in enumerate(CG):
            for j in range(len(BLOCKS)):
                blocks, HW, (n, xr, rr) = BLOCKS[(i + j) % 6], HWS[(i + 2 * j + j // 2) % 4], NREP[(3 * i + j) % 7]
                seen |= {("b", blocks, i), ("hw", HW), ("rep", n, xr, rr)}
                one(C, G, HW, blocks, n, xr, rr, 1e-5 if (i + j) % 2 else 1e-6, fast=(dt == 0 and j == 2))
        assert {s[1] for s in seen if s[0] == "hw"} == set(HWS) and len([s for s in seen if s[0] == "rep"]) == len(NREP)
        assert len([s for s in seen if s[0] == "b"]) == len(CG) * len(BLOCKS)
        for act in (False, True):
            for use_rs in (False, True):
                for use_emb in (False, True):
                    one(48, 8, 60, 3, 2, 1, 1, 1e-5, act, use_emb, use_rs)
    print(f"gn consumer dt {dt} [{name}]: worst {worst:.2e} (bound {tol:.1e})")
    # refusals, as the launcher defines them
    x = hip.to_nhwc((rn(1, 2112, 2, 2) * 2 + 0.5).to(dev), dt)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_ex(dt, x, torch.ones(2112, device=dev), torch.zeros(2112, device=dev), 1, colstats=torch.zeros(1, 1, 2112, 2, device=dev))
    x = hip.to_nhwc((rn(1, 32, 2, 2) * 2 + 0.5).to(dev), dt)
    one_, zero, film = torch.ones(32, device=dev), torch.zeros(32, device=dev), torch.zeros(1, 64, device=dev)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_ex(dt, x, one_, zero, 8, colstats=torch.zeros(1, 1, 32, 2, device=dev), film=film)
    with pytest.raises(hip.NopeError):
        hip.op_group_norm_ex(dt, x, one_, zero, 8, film=film, out_stats=True)


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_gn_film(be, dt):
    """(c) gn_apply_kernel<FILM = true>, statistics from gn_stats: y = act(norm(x) (1 + scale) + shift) [+ emb] [+ resid] against float64 at
    OP_TOL, one [scale | shift] row per hypothesis (film_stride = 2 C) and one row for all (film_stride = 0), n in {1, 5}, G = 32,
    C in {32, 64, 320, 96} (1, 2, 10, 3 channels per group: no 16-byte vector lies in one group, the coefficient path without `one_group`) and
    C = 256 (8 per group: with it).
    The scale rows have std 1: a shift that missed its (1 + scale) factor, or a scale applied without the 1, is an O(1) error.
    The interpreter runs f32 on two shapes.  Worst on an MI355X: f32 1.7e-7 (bound 2e-5), bf16 3.3e-3 (4e-2), f16 4.1e-4 (5e-3)."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs every storage type)")
    g = torch.Generator().manual_seed(900 + dt)
    rn = lambda *s: torch.randn(*s, generator=g)
    tol, worst, k = OP_TOL[dt], 0.0, 0
    for C in ((32, 96) if name == "emu" else (32, 64, 320, 96, 256)):
        for n in ((5,) if name == "emu" else (1, 5)):
            for shared in (False, True):
                act, use_rs, use_emb = k % 2 == 0, k % 3 != 0, k % 4 == 1
                k += 1
                x = rn(n, C, 5, 4) * 2 + 0.3
                ga, be_, emb, rs = rn(C), rn(C), rn(n, C), rn(n, C, 5, 4)
                film = rn(2 * C) if shared else rn(n, 2 * C)
                y = hip.op_group_norm_ex(dt, hip.to_nhwc(x.to(dev), dt), ga.to(dev), be_.to(dev), 32, act_silu=act, film=film.to(dev),
                                         emb=emb.to(dev) if use_emb else None, resid=hip.to_nhwc(rs.to(dev), dt) if use_rs else None)
                ref = _gn_ref(_q(x, dt, hip), 32, ga, be_, 1e-5, act, emb if use_emb else None, _q(rs, dt, hip) if use_rs else None, film=film)
                e = float((hip.to_nchw(y, dt).cpu().double() - ref).abs().max() / ref.abs().max())
                worst = max(worst, e)
                assert e < tol, (dt, C, n, shared, act, use_rs, use_emb, e)
    print(f"gn FiLM dt {dt} [{name}]: worst {worst:.2e} (bound {tol:.1e})")


def _chunk_sums(y64, blocks):
    """[n][blocks][2] float64 (sum, sum of squares) and (sum |y|) of y (n, C, h, w) over gn_apply's pixel chunks (ceil(HW / blocks) pixels each)."""
    n, C = y64.shape[:2]
    px = y64.reshape(n, C, -1)
    HW = px.shape[2]
    pper = (HW + blocks - 1) // blocks
    out, mag = torch.zeros(n, blocks, 2, dtype=torch.float64), torch.zeros(n, blocks, dtype=torch.float64)
    for b in range(blocks):
        run = px[:, :, b * pper:min((b + 1) * pper, HW)]
        out[:, b, 0], out[:, b, 1], mag[:, b] = run.sum((1, 2)), (run * run).sum((1, 2)), run.abs().sum((1, 2))
    return out, mag


@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_out_stats_and_prenorm_chain(be, dt, monkeypatch, capfd):
    """(d) gn_apply_kernel<OS = true>: out_stats[n][gn_apply_blocks][2] against the float64 sum and sum of squares, per chunk and per sample,
    of the y the launch wrote (f32 storage, bound 1e-5; modes 0 and 3, the latter with the hardware SiLU as its runtimes launch it) or of
    the unrounded float64 y (16-bit storage: the sums are taken before the rounding; OP_TOL), measures as in (a).  Then gn_finalize_kernel
    and a 1x1 conv with the PreNorm epilogue (pn_ms / pn_c0 / pn_c1; hip.prenorm_fold) against float64 conv1x1(group_norm(y, 1, gamma,
    beta)) of the stored y and the stored weights W gamma, at the conv sweep's tolerance, on the small-tile kernel, the 128 x 192 kernel and
    (device) the per-tap ping-pong kernel; C in {64, 192}, Cout in {96, 384}, 16 / 64 / 100 pixels (whole 64-row blocks inside a sample and
    not), n in {1, 3} and (device) 1040 = more workgroups than NOPE_GN_MIN_GRID spreads, and NOPE_GN_MIN_GRID=0.  The unfused pair
    op_group_norm(G = 1) + op_conv agrees within the same tolerance.  The interpreter runs f32 on two shapes.
    Worst on an MI355X (out_stats | PreNorm conv against float64 | against the unfused pair): f32 1.3e-7 | 6.4e-7 | 8.3e-7 (bounds 1e-5 | 1e-5);
    bf16 2.0e-7 | 3.4e-3 | 7.2e-3 (4e-2 | 8e-3); f16 1.6e-7 | 4.2e-4 | 8.2e-4 (5e-3 | 1e-3); bf16x3 1.4e-7 | 8.8e-6 | 1.0e-5 (1e-5 | 3e-5)."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs every mode)")
    sdt = hip.storage_code(dt)
    g = torch.Generator().manual_seed(1000 + dt)
    rn = lambda *s: torch.randn(*s, generator=g)
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    os_tol = 1e-5 if sdt == 0 else OP_TOL[dt]
    tol = SWEEP_TOL[dt]
    worst_os, worst_pn, worst_un, kinds, chunkings = 0.0, 0.0, 0.0, set(), set()
    policies = [{}, {"NOPE_CONV_SMALL": "2"}, {"NOPE_CONV_SMALL": "0"}] + ([{"NOPE_CONV_PP": "11"}] if name == "gpu" else [])
    shapes = [(C, cout, hw, n) for C in (64, 192) for cout in (96, 384) for hw in ((4, 4), (8, 8), (10, 10)) for n in (1, 3)]
    shapes = [s for i, s in enumerate(shapes) if i % 2 == (i // 6) % 2]      # 12 of the 24: every value of every axis, both n at every (C, hw)
    if name == "gpu":
        shapes += [(64, 96, (4, 4), 1040)]
    else:
        shapes = [(64, 96, (10, 10), 3), (192, 96, (8, 8), 1)]
    for si, (C, cout, (h, w), n) in enumerate(shapes):
        HW = h * w
        x = rn(n, C, h, w) * 2 + 0.4
        ga1, be1, ga2, be2 = rn(C), rn(C), rn(C) * 0.5 + 1, rn(C) * 0.5
        W, b = rn(cout, C, 1, 1) / C ** 0.5, rn(cout)
        xq = _q(x, dt, hip)
        for grid_pol in (({}, {"NOPE_GN_MIN_GRID": "0"}) if si % 4 == 0 else ({},)):
            _policy(monkeypatch, grid_pol)
            y, ex = hip.op_group_norm_ex(dt, hip.to_nhwc(x.to(dev), dt), ga1.to(dev), be1.to(dev), 8, act_silu=True, out_stats=True, fast_silu=(dt == 3))
            blocks = hip.op_gn_apply_blocks(dt, HW, C, n)
            chunkings.add((blocks > 1, n * blocks > 1024))
            got = ex["out_stats"].double().cpu()
            assert got.shape == (n, blocks, 2)
            yw = hip.to_nchw(y, dt).cpu().double()                          # what the launch wrote
            y64 = yw if sdt == 0 else _gn_ref(xq, 8, ga1, be1, 1e-5, True)   # 16-bit storage: the values before the rounding
            want, mag = _chunk_sums(y64, blocks)
            e1 = float(((got[..., 0] - want[..., 0]).abs() / mag).max())
            e2 = float(((got[..., 1] - want[..., 1]).abs() / want[..., 1]).max())
            s1 = float(((got[..., 0].sum(1) - want[..., 0].sum(1)).abs() / mag.sum(1)).max())
            s2 = float(((got[..., 1].sum(1) - want[..., 1].sum(1)).abs() / want[..., 1].sum(1)).max())
            worst_os = max(worst_os, e1, e2, s1, s2)
            assert max(e1, e2, s1, s2) < os_tol, (dt, C, HW, n, blocks, e1, e2, s1, s2)
        ms = hip.op_gn_finalize(ex["out_stats"], HW * C)
        mean64, var64 = yw.mean((1, 2, 3)), yw.var((1, 2, 3), unbiased=False)
        ms_want = torch.stack((mean64, (var64 + 1e-5).rsqrt()), 1)
        assert float(((ms.double().cpu() - ms_want).abs() / ms_want.abs().max(0).values).max()) < os_tol * 4, (dt, C, HW, n)
        wg = (W.double().reshape(cout, C) * ga2.double()).float()
        wq = _q(wg, dt, hip).double()
        yn = (yw - mean64[:, None, None, None]) * (var64 + 1e-5).rsqrt()[:, None, None, None]
        ref = torch.einsum("nc,bchw->bnhw", wq, yn) + (W.double().reshape(cout, C) @ be2.double() + b.double())[None, :, None, None]
        unfused = hip.to_nchw(hip.op_conv(dt, hip.op_group_norm(dt, y, ga2.to(dev), be2.to(dev), 1), W.to(dev), b.to(dev)), dt).cpu().double()
        for pol in (policies if n < 1000 else policies[:1]):
            _policy(monkeypatch, pol)
            capfd.readouterr()
            out = hip.op_conv_ex(dt, y, W.to(dev), b.to(dev), prenorm=(ms, ga2, be2))
            kind = _trace(capfd.readouterr().err)[0]
            want_kind = "pp256" if pol.get("NOPE_CONV_PP") == "11" else "dma128" if pol.get("NOPE_CONV_SMALL") == "0" else "small"
            assert kind == want_kind, (dt, pol, kind)
            kinds.add((kind, HW % 64 == 0))
            e = float((hip.to_nchw(out, dt).cpu().double() - ref).abs().max() / ref.abs().max())
            eu = float((hip.to_nchw(out, dt).cpu().double() - unfused).abs().max() / unfused.abs().max())
            worst_pn, worst_un = max(worst_pn, e), max(worst_un, eu)
            assert e < tol and eu < tol, (dt, sorted(pol.items()), kind, C, cout, HW, n, e, eu)
    print(f"out_stats dt {dt} [{name}]: worst {worst_os:.2e} (bound {os_tol:.1e}); PreNorm conv worst {worst_pn:.2e}, against the unfused pair {worst_un:.2e} (bound {tol:.1e}); {sorted(kinds)}")
    if name == "gpu":
        assert {(k, u) for k in ("small", "dma128", "pp256") for u in (False, True)} <= kinds, kinds
        assert {(True, False), (False, True), (False, False)} <= chunkings, chunkings
    # the launcher's refusals around the PreNorm epilogue: 3x3, with colstats
    _policy(monkeypatch, {})
    with pytest.raises(hip.NopeError):
        hip.op_conv_ex(dt, y, rn(8, C, 3, 3).to(dev), None, prenorm=(ms, ga2, be2))
    with pytest.raises(hip.NopeError):
        hip.op_conv_ex(dt, y, W.to(dev), None, prenorm=(ms, ga2, be2), colstats=torch.zeros(2 * n * HW * cout, device=dev), stat_rows=64)


def test_absmax_is_exact(be):
    """(e) nope_op_absmax_f32 == max |x| exactly: lengths around the 4-wide vectors and one grid (1 .. 2^20 + 3), the extreme element first,
    in the middle and last (inside the tail that is no whole vector), negative, all zeros -> 0, NaNs ignored.  The interpreter runs the
    lengths up to 4097."""
    hip, dev, name = be
    g = torch.Generator().manual_seed(1100)
    for n in (1, 3, 4, 5, 1023, 4097) + ((2 ** 20 + 3,) if name == "gpu" else ()):
        base = torch.randn(n, generator=g)
        assert hip.op_absmax(base.to(dev)) == float(base.abs().max()), n
        for pos in sorted({0, n // 2, n - 1}):
            for sign in (1.0, -1.0):
                x = base.clone()
                x[pos] = sign * 77.25
                assert hip.op_absmax(x.to(dev)) == 77.25, (n, pos, sign)
        assert hip.op_absmax(torch.zeros(n, device=dev)) == 0.0
        x = base.clone()
        x[::3] = float("nan")
        rest = x[~torch.isnan(x)]
        assert hip.op_absmax(x.to(dev)) == (float(rest.abs().max()) if rest.numel() else 0.0), ("nan", n)


def test_gn_amax_is_exact(be):
    """(e) GnApplyArgs::amax_out on f32 storage with the hardware SiLU (gn_apply_kernel's AMAX) == max |y| of what the launch wrote, exactly:
    statistics from colstats and from gn_stats, threads without a row (C = 192: 240 of 256 threads work), more publishing waves than the slot
    has lines (n x blocks x 4 > 32), with out_stats.  With the libm SiLU or FiLM AMAX is compiled out and the slot stays 0: asserted, so that
    nobody relies on a maximum there.  The interpreter runs the two smallest shapes."""
    hip, dev, name = be
    g = torch.Generator().manual_seed(1200)
    rn = lambda *s: torch.randn(*s, generator=g)
    shapes = [(24, 8, 16, 3, 1), (192, 8, 60, 2, 2)] + ([(192, 8, 256, 6, 1), (1536, 8, 64, 6, 3), (2048, 32, 16, 3, 1), (384, 32, 256, 6, 2)] if name == "gpu" else [])
    for i, (C, G, HW, n, x_rep) in enumerate(shapes):
        h, w = SHAPES[HW]
        x = rn(n // x_rep, C, h, w) * 2 + 0.5
        ga, be_, emb, rs = rn(C).to(dev), rn(C).to(dev), rn(n, C).to(dev), hip.to_nhwc(rn(n, C, h, w).to(dev), 0)
        xs = hip.to_nhwc(x.to(dev), 0)
        cs = _torch_colstats(x, 3).to(dev) if i % 2 == 0 else None
        kw = dict(act_silu=i != 1, emb=emb, resid=rs if i % 3 else None, x_rep=x_rep, colstats=cs, want_amax=True)
        y, ex = hip.op_group_norm_ex(0, xs, ga, be_, G, fast_silu=True, out_stats=(i % 2 == 1), **kw)
        assert ex["amax"] == float(y.abs().max()) and ex["amax"] > 0, (C, G, HW, n, ex["amax"], float(y.abs().max()))
        y, ex = hip.op_group_norm_ex(0, xs, ga, be_, G, fast_silu=False, **kw)
        assert ex["amax"] == 0.0, "the libm SiLU instantiation records no maximum"
        if cs is None:
            y, ex = hip.op_group_norm_ex(0, xs, ga, be_, G, fast_silu=True, film=rn(2 * C).to(dev), **kw)
            assert ex["amax"] == 0.0, "the FiLM instantiation records no maximum"


@pytest.mark.parametrize("dt", [0, 3, 4])
def test_conv_out_amax_is_exact(be, dt, monkeypatch, capfd):
    """(e) ConvArgs::out_amax (f32 storage): where conv_records_out_amax says the launch records, the maximum == max |out| exactly -- the wide
    epilogue of the 128 x 192 kernel (dma128), the tap-resident kernel (halo256) and the per-tap ping-pong kernel (pp256), with bias and
    residual, ragged Cout; where it says not -- the small-tile kernel, a split-K launch, an NCHW output -- the slot stays 0.
    The interpreter runs f32 on the 128 x 192 and small-tile kernels."""
    hip, dev, name = be
    if name == "emu" and dt != 0:
        pytest.skip("interpreter: f32 (the device runs the three f32-storage modes)")
    P = hip.CONV_PLAIN
    g = torch.Generator().manual_seed(1300 + dt)
    monkeypatch.setenv("NOPE_CONV_TRACE", "1")
    # (policy, k, n, cin, cout, side, split_k, out_nchw, kernel, records)
    table = [({"NOPE_CONV_SMALL": "0"}, 3, 3, 64, 200, 8, False, False, "dma128", True), ({"NOPE_CONV_SMALL": "0"}, 1, 2, 64, 24, 6, False, False, "dma128", True),
             ({}, 3, 3, 64, 24, 8, False, False, "small", False), ({"NOPE_CONV_SMALL": "0"}, 1, 2, 64, 24, 8, False, True, "dma128", False)]
    if name == "gpu":
        table += [({"NOPE_CONV_PP": "11"}, 3, 3, 64, 200, 8, False, False, "halo256", True), ({"NOPE_CONV_PP": "11"}, 1, 5, 128, 72, 8, False, False, "pp256", True),
                  (SPLIT, 3, 4, 128, 72, 4, True, False, "halo256", False)]
    if dt == 4:
        table = [t for t in table if t[0].get("NOPE_CONV_PP") == "11"]
    seen = set()
    for pol, k, n, cin, cout, side, split_k, nchw, want_kind, want_rec in table:
        _policy(monkeypatch, pol)
        case = _ConvCase(hip, dev, dt, g, P, k, n, cin, 0, 1, side, side, cout, True)
        rs = None if nchw else hip.to_nhwc(torch.randn(n, cout, side, side, generator=g).to(dev), dt)
        capfd.readouterr()
        out, amax, rec = case.launch(hip, dt, resid=rs, split_k=split_k, out_nchw=nchw, want_amax=True)
        kind, splits, line = _trace(capfd.readouterr().err)
        assert kind == want_kind and (splits > 1) == split_k and rec == want_rec, (dt, line, rec)
        assert amax == (float(out.abs().max()) if rec else 0.0), (dt, line, amax, float(out.abs().max()))
        assert torch.equal(out, case.launch(hip, dt, resid=rs, split_k=split_k, out_nchw=nchw)), (dt, line)
        seen.add((kind, rec))
    print(f"conv out_amax dt {dt} [{name}]: {sorted(seen)}")
