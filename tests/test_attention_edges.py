"""The hand-written softmaxes at the inputs where a missing maximum or a missing rescale shows: linattn_kernel / attn_kernel
(csrc/kernels_attn.hip) and the token / wide attention kernels (csrc/kernels_ldm.hip).

Unit-variance inputs cannot overflow exp() whether or not a maximum was subtracted, so the rest of the suite does not notice a wrong
`kmax`, a wrong row maximum or a wrong online-softmax correction.  Here every case plants large values where the code under test has
to find them (every unroll slot, tail and LDS row of linattn_kernel's first sweep; a running maximum that rises or falls key block by
key block), against plain torch in float64 on the storage-rounded inputs -- the formulas of test_attention_cores and _attention_f64.

Error metric (`row_err`): per (sample, pixel / token) row, max |got - want| over the row's channels / max |want| over the same row,
then the maximum over all rows -- one bad row cannot hide under a large value elsewhere in the tensor, as it can under tests/util.rel.
Bounds: OP_TOL of test_kernels_parity.py per storage type; 2e-4 for the split-precision kernels at large scores (the bound of
test_ldm_token_attention_split_precision).  Worst values observed on an MI355X are in each test's docstring.

Every test runs on the interpreter (tests/hipemu) and, marked `gpu`, on the device."""
import os

import pytest
import torch

from tests.test_kernels_parity import OP_TOL as _OP_TOL

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
OP_TOL = dict(_OP_TOL)
OP_TOL[3] = OP_TOL[4] = 2e-4          # bf16x3 / f16x2 at scores of +-50 and beyond: a score's absolute error is its exponential's relative error
D = 32                                # head width of the U-Net's attention cores
BIG = 96.0                            # exact in bf16 and f16; exp(96 - 4) overflows f32
LIN_N = [1, 15, 17, 31, 33, 64, 65, 97, 129, 193, 257, 517]


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


def row_err(got, want):
    """max over rows of (max |got - want| over the last axis / max |want| over the last axis)."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(((got - want).abs().amax(-1) / (want.abs().amax(-1) + 1e-30)).max())


def check(got, want, tol, what):
    assert bool(torch.isfinite(got).all()), ("not finite", what)
    e = row_err(got, want)
    print(f"attention_edges {what}: per-row error {e:.3e} (bound {tol:.1e})")
    assert e < tol, (what, e, tol)


_CACHE = {}


def cached(key, make):
    """Inputs and float64 references are built once and shared by both backends (never modified by a test)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- linattn_kernel / attn_kernel -----------------------------------------------------------------------------------------------------
def _split(qkv, tdt, heads):
    """(b, 3 * heads * 32, 1, n) -> q, k, v (b, heads, 32, n) in float64, rounded to the storage type first."""
    b, _, _, n = qkv.shape
    return (t.reshape(b, heads, D, n) for t in qkv.to(tdt).double().chunk(3, 1))


def linattn_f64(qkv, tdt, heads=4):
    """LinearAttention: softmax_d(q) * d^-0.5, softmax_n(k), ctx = k v^T, out = ctx^T q.  Returns (b, n, heads * 32) rows."""
    qq, kk, vv = _split(qkv, tdt, heads)
    ctx = torch.einsum("bhdn,bhen->bhde", kk.softmax(-1), vv)
    o = torch.einsum("bhde,bhdn->bhen", ctx, qq.softmax(-2) * D ** -0.5)
    return o.reshape(o.shape[0], heads * D, -1).permute(0, 2, 1).contiguous()


def attn_f64(qkv, tdt, heads=4):
    """Attention: softmax_j(q_i . k_j * d^-0.5) v_j.  Returns (b, n, heads * 32) rows."""
    qq, kk, vv = _split(qkv, tdt, heads)
    sim = torch.einsum("bhdi,bhdj->bhij", qq * D ** -0.5, kk).softmax(-1)
    o = torch.einsum("bhij,bhdj->bhid", sim, vv)                       # (b, h, i, d)
    return o.permute(0, 2, 1, 3).reshape(o.shape[0], o.shape[2], heads * D).contiguous()


def run_cores(hip, dev, dt, qkv, heads=4, full=False):
    """The operator on an NCHW (b, 3 * heads * 32, 1, n) tensor -> (b, n, heads * 32) rows in f32 on the host."""
    y = hip.op_linear_attention(dt, hip.to_nhwc(qkv.to(dev), dt), heads=heads, full=full)
    b, _, n, c = y.shape
    return y.float().cpu().reshape(b, n, c)


def planted(seed, b, heads, n, peak=None):
    """randn qkv (b, 3 * heads * 32, 1, n) with one pixel of every k column at BIG: column c of sample s peaks at pixel
    (columns * s + c) % n -- with b = ceil(n / columns) samples every pixel is some column's arg-max -- or at pixel `peak`."""
    g = torch.Generator().manual_seed(seed)
    hd = heads * D
    qkv = torch.randn(b, 3 * hd, 1, n, generator=g)
    for s in range(b):
        for c in range(hd):
            qkv[s, hd + c, 0, (hd * s + c) % n if peak is None else peak] = BIG
    return qkv


def q_times(qkv, gain):
    out = qkv.clone()
    out[:, :qkv.shape[1] // 3] *= gain
    return out


def _tdt(hip, dt):
    return hip.torch_dtype(hip.storage_code(dt))


@pytest.mark.parametrize("n", LIN_N)
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_linattn_planted_k_maxima(be, dt, n):
    """k-softmax over pixels with the arg-max of every k column planted at 96.0 (exp(96 - 4) overflows f32: a column whose maximum the
    first sweep misses turns into inf / NaN), every pixel the arg-max of some column.  Token counts around the 16-pixel groups of the
    third sweep, the staging pass PT (32 pixels f32, 64 pixels 16-bit), 3 PT (first pixel of the fourth load slot), 4 PT and 8 PT.  The
    same inputs with q * 40: the per-pixel softmax over d is close to one-hot and needs ITS maximum.
    Worst per-row error on an MI355X: f32 4.6e-7, bf16 3.9e-3, f16 4.9e-4 (bounds 2e-5 / 4e-2 / 5e-3)."""
    hip, dev, name = be
    tdt = _tdt(hip, dt)
    b = -(-n // 128)
    for gain in (1.0, 40.0):
        qkv, want = cached(("lin", n, gain, tdt), lambda: (lambda x: (x, linattn_f64(x, tdt)))(q_times(planted(100 + n, b, 4, n), gain)))
        check(run_cores(hip, dev, dt, qkv), want, OP_TOL[dt], f"linattn planted dt {dt} n {n} q x{gain:g} [{name}]")


@pytest.mark.parametrize("peak", [256, 96, 192])
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_linattn_all_maxima_on_one_pixel(be, dt, peak):
    """n = 257, all 128 k columns peak at the same pixel: the last one (a tail pixel that a single thread row of the first sweep
    loads, past every whole 4 PT stride) and pixel 3 PT of either storage width (96 / 192: first pixel of the fourth unroll slot).
    Worst per-row error on an MI355X: f32 3.4e-7, bf16 2.5e-3, f16 2.8e-4 (bounds 2e-5 / 4e-2 / 5e-3)."""
    hip, dev, name = be
    tdt = _tdt(hip, dt)
    n = 257
    for gain in (1.0, 40.0):
        qkv, want = cached(("lin1", peak, gain, tdt), lambda: (lambda x: (x, linattn_f64(x, tdt)))(q_times(planted(200 + peak, 1, 4, n, peak), gain)))
        check(run_cores(hip, dev, dt, qkv), want, OP_TOL[dt], f"linattn one-pixel dt {dt} peak {peak} q x{gain:g} [{name}]")


@pytest.mark.parametrize("n", [1, 17, 65, 193, 257, 517])
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_linattn_constant_k(be, dt, n):
    """k constant along the pixels (0, and 80: a maximum that every pixel attains, and exp(80) = 5.5e34 per pixel where
    it is not subtracted): every weight is 1 / n and ctx is the mean of v.
    Worst per-row error on an MI355X: f32 5.6e-7, bf16 3.7e-3, f16 4.1e-4 (bounds 2e-5 / 4e-2 / 5e-3)."""
    hip, dev, name = be
    tdt = _tdt(hip, dt)

    def make(const):
        qkv = torch.randn(2, 384, 1, n, generator=torch.Generator().manual_seed(300 + n))
        qkv[:, 128:256] = const
        want = linattn_f64(qkv, tdt)
        qq, _, vv = _split(qkv, tdt, 4)       # the closed form: out = mean_n(v)^T softmax_d(q) d^-0.5
        closed = torch.einsum("bhe,bhdn->bhen", vv.mean(-1), qq.softmax(-2) * D ** -0.5).reshape(2, 128, n).permute(0, 2, 1)
        assert row_err(closed, want) < 1e-12
        return qkv, want

    for const in (0.0, 80.0):
        qkv, want = cached(("link", n, const, tdt), lambda: make(const))
        check(run_cores(hip, dev, dt, qkv), want, OP_TOL[dt], f"linattn constant k = {const:g} dt {dt} n {n} [{name}]")


@pytest.mark.parametrize("heads,nhyp", [(4, 3), (4, 4), (4, 8), (4, 12), (1, 2), (2, 2), (8, 2)])
@pytest.mark.parametrize("dt", [0, 1])
def test_linattn_block_index_maps(be, dt, heads, nhyp):
    """(hypothesis, head) of a workgroup: 4 heads on grids of 16, 32 and 48 take the XCD head-pair remap, a grid of 12 does not; 1, 2 and
    8 heads never do (8 heads x 2 = a grid of 16 without it).  Every block's data differs, so a swapped pair cannot pass the whole-tensor
    comparison; plain randn and one planted-maximum input; 8 hypotheses == its two halves of 4, bit for bit (both remapped).
    Worst per-row error on an MI355X: f32 4.6e-7, bf16 3.8e-3 (bounds 2e-5 / 4e-2)."""
    hip, dev, name = be
    tdt = _tdt(hip, dt)
    for n in (17, 65):
        def make(kind):
            if kind == "planted":
                return (lambda x: (x, linattn_f64(x, tdt, heads)))(planted(400 + n + heads, nhyp, heads, n))
            qkv = torch.randn(nhyp, 3 * heads * D, 1, n, generator=torch.Generator().manual_seed(410 + n + heads + nhyp))
            return qkv, linattn_f64(qkv, tdt, heads)
        for kind in ("randn", "planted") if n == 65 else ("randn",):
            qkv, want = cached(("map", kind, heads, nhyp, n, tdt), lambda: make(kind))
            got = run_cores(hip, dev, dt, qkv, heads=heads)
            check(got, want, OP_TOL[dt], f"linattn map dt {dt} heads {heads} nhyp {nhyp} n {n} {kind} [{name}]")
            if nhyp == 8:
                halves = torch.cat([run_cores(hip, dev, dt, qkv[i:i + 4], heads=heads) for i in (0, 4)])
                assert torch.equal(got, halves), (dt, n, kind)


@pytest.mark.parametrize("n", [1, 2, 16, 63, 64])
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_attn_large_scores(be, dt, n):
    """attn_kernel (full attention, n <= 64) with q, k = 6 randn -- scores reach about +-100: exp() of them overflows f32 without the
    row maximum -- and with each query's best key planted (key (5 i + 1) % n is 2 q_i, q = 3 randn: a score of ~100 there).
    Worst per-row error on an MI355X: f32 8.9e-6 (6 randn inputs: the f32 rounding of a score of ~100 is ~1e-5 of its exponential), bf16 3.6e-3,
    f16 4.4e-4 (bounds 2e-5 / 4e-2 / 5e-3)."""
    hip, dev, name = be
    tdt = _tdt(hip, dt)

    def make(kind):
        g = torch.Generator().manual_seed(500 + n)
        qkv = torch.randn(3, 384, 1, n, generator=g)
        if kind == "x6":
            qkv[:, :256] *= 6.0
        else:
            qkv[:, :128] *= 3.0
            for i in range(n):
                qkv[:, 128:256, 0, (i * 5 + 1) % n] = qkv[:, :128, 0, i] * 2.0
        return qkv, attn_f64(qkv, tdt)

    for kind in ("x6", "planted"):
        qkv, want = cached(("attn", kind, n, tdt), lambda: make(kind))
        check(run_cores(hip, dev, dt, qkv, full=True), want, OP_TOL[dt], f"attn {kind} dt {dt} n {n} [{name}]")


def test_attn_rejects_more_than_64_tokens(be):
    """nope_op_attention holds the whole score matrix of a head in LDS: 65 tokens is NOPE_ERR_UNSUPPORTED, not a launch."""
    hip, dev, _ = be
    qkv = hip.to_nhwc(torch.randn(1, 384, 1, 65).to(dev), 0)
    with pytest.raises(hip.NopeError, match="nope_op_attention"):
        hip.op_linear_attention(0, qkv, full=True)
    assert hip.op_linear_attention(0, qkv[:, :, :64].contiguous(), full=True).shape == (1, 1, 64, 128)


# ---- token attention / wide attention (csrc/kernels_ldm.hip) ----------------------------------------------------------------------------
def token_f64(qkv, d):
    n, N, c3 = qkv.shape
    C = c3 // 3
    qq, kk, vv = (t.reshape(n, N, C // d, d).permute(0, 2, 1, 3) for t in qkv.double().chunk(3, dim=-1))
    return ((qq @ kk.transpose(-1, -2) * d ** -0.5).softmax(-1) @ vv).permute(0, 2, 1, 3).reshape(n, N, C)


def token_input(kind, seed, n, N, C, d):
    """qkv (n, N, 3 C) in f32.  "randn4": 4 randn.  "ascending": every query is 3 u for one sign vector u (per head), key j is
    3 u ramp_j + 0.05 randn with ramp rising linearly from -1 to 1: the scores rise by 18 sqrt(d) over the keys, so the running maximum
    of an online softmax rises in every key block and its correction factor is far from 1.  "descending": the ramp reversed -- the
    maximum sits in the first block and the correction is exactly 1 afterwards."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, N, 3 * C, generator=g)
    if kind == "randn4":
        return qkv * 4.0
    u = (torch.randint(0, 2, (d,), generator=g).float() * 2 - 1).repeat(C // d)
    ramp = torch.linspace(-1.0, 1.0, N)
    if kind == "descending":
        ramp = ramp.flip(0)
    qkv[:, :, :C] = 3.0 * u
    qkv[:, :, C:2 * C] = 3.0 * u * ramp[None, :, None] + 0.05 * qkv[:, :, C:2 * C]
    return qkv


TOKEN_N = [1, 63, 65, 129, 200]          # ragged against the 64 keys per iteration and the 128 queries per workgroup of the MFMA kernels


@pytest.mark.parametrize("kind", ["randn4", "ascending", "descending"])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dt", [1, 2])
def test_token_attention_16bit_large_scores(be, dt, d, kind):
    """token_attn_mfma_kernel (bf16 / f16 storage) at scores of +-50 and beyond, and with a running maximum that rises (falls) block by
    block; on the device also the VALU kernel of the same storage types (NOPE_LDM_ATTN=0).  Two heads, token counts ragged against
    64 keys / 128 queries.  Interpreter: bf16, d = 32 / 64 (the f16 kernel differs in one MFMA builtin, d = 128 in two trip counts).
    Worst per-row error on an MI355X: bf16 MFMA 3.8e-3, VALU 3.8e-3; f16 MFMA 5.0e-4, VALU 4.9e-4 (bounds 4e-2 / 5e-3)."""
    hip, dev, name = be
    if name == "emu" and (dt != 1 or d == 128):
        pytest.skip("interpreter: the bf16 kernel at d = 32 / 64 (all of them run on the device)")
    tdt = _tdt(hip, dt)
    for N in TOKEN_N:
        qkv, want = cached(("tok", kind, d, N, tdt), lambda: (lambda x: (x, token_f64(x, d)))(token_input(kind, 600 + d + N, 1, N, 2 * d, d).to(tdt)))
        got = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).float().cpu()
        check(got, want, OP_TOL[dt], f"token mfma dt {dt} d {d} N {N} {kind} [{name}]")
        if name == "gpu":
            os.environ["NOPE_LDM_ATTN"] = "0"
            try:
                valu = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).float().cpu()
            finally:
                os.environ.pop("NOPE_LDM_ATTN", None)
            check(valu, want, OP_TOL[dt], f"token valu dt {dt} d {d} N {N} {kind} [{name}]")


@pytest.mark.parametrize("kind", ["ascending", "descending"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_token_attention_f32_running_maximum(be, d, kind):
    """The rising / falling running maximum in the f32-storage kernels: the all-f32 VALU kernel (dt 0, bound OP_TOL[0]) and the
    split-precision MFMA kernel (bf16x3 / f16x2, bound 2e-4 as in the existing large-score tests).
    Worst per-row error on an MI355X: f32 6.0e-6, bf16x3 6.6e-5, f16x2 6.6e-5 (bounds 2e-5 / 2e-4 / 2e-4)."""
    hip, dev, name = be
    for N in TOKEN_N:
        qkv, want = cached(("tok", kind, d, N, torch.float32), lambda: (lambda x: (x, token_f64(x, d)))(token_input(kind, 600 + d + N, 1, N, 2 * d, d)))
        for dt in (0, 3, 4):
            got = hip.op_token_attention(dt, qkv.to(dev), dim_head=d).cpu()
            check(got, want, OP_TOL[dt], f"token f32-storage dt {dt} d {d} N {N} {kind} [{name}]")


@pytest.mark.parametrize("C", [256, 512])
@pytest.mark.parametrize("dt", [1, 2])
def test_wide_attention_16bit_large_scores(be, dt, C):
    """nope_op_wide_attention on bf16 / f16 storage: the construction of test_wide_attention_large_scores (normalised q = k, scores of
    +-50) at 65 and 130 tokens, and the rising-maximum input at 200 tokens.  Interpreter: bf16, C = 256.
    Worst per-row error on an MI355X: bf16 3.0e-3, f16 3.5e-4 (bounds 4e-2 / 5e-3)."""
    hip, dev, name = be
    if name == "emu" and (dt != 1 or C != 256):
        pytest.skip("interpreter: the bf16 kernel at C = 256 (all of them run on the device)")
    tdt = _tdt(hip, dt)

    def make(N):
        g = torch.Generator().manual_seed(700 + C + N)
        q = torch.randn(2, N, C, generator=g)
        q = q / q.norm(dim=-1, keepdim=True) * (50.0 * C ** 0.5) ** 0.5
        qkv = torch.cat([q, q, torch.randn(2, N, C, generator=g)], dim=-1).to(tdt)
        return qkv, token_f64(qkv, C)

    for N in (65, 130):
        qkv, want = cached(("wide", C, N, tdt), lambda: make(N))
        check(hip.op_wide_attention(dt, qkv.to(dev)).float().cpu(), want, OP_TOL[dt], f"wide dt {dt} C {C} N {N} q=k [{name}]")
    qkv, want = cached(("wide-asc", C, tdt), lambda: (lambda x: (x, token_f64(x, C)))(token_input("ascending", 710 + C, 1, 200, C, C).to(tdt)))
    check(hip.op_wide_attention(dt, qkv.to(dev)).float().cpu(), want, OP_TOL[dt], f"wide dt {dt} C {C} N 200 ascending [{name}]")
