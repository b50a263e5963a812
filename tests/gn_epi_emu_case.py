"""The tap-resident 3x3 kernel that normalises its own output (epilogue_wide, LEANM = 3: conv_gemm_common.h; ConvArgs::gn_self) against the two launches
it replaces -- the conv with fused column statistics, then the GroupNorm apply pass that folds them -- bit for bit, output and recorded range maximum.
Shared by tests/test_gn_epilogue.py (interpreter and device); `python tests/gn_epi_emu_case.py` runs the interpreter cases alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
import torch

from tests.util import switches

PP = dict(NOPE_CONV_PP=11, NOPE_CONV_SMALL=0, NOPE_CONV_STREAM=0)      # bit 3: small shapes reach the tap-resident kernel
CIN = 32
# (samples, H = W): M = 256 each -- one tile that holds 1, 4 and 16 whole samples (row blocks of 64, 64 and 16 rows)
MAPS = [(1, 16), (4, 8), (16, 4)]
# (Cout, G, emb, resid): group widths 24 (a lane's pass holds parts of two groups), 96 (one wave column), 192 (a group spans both wave columns),
# with and without the embedding row and the identity residual; and two 192-column tiles
FORMS = [(192, 8, True, True), (192, 8, False, False), (192, 2, False, True), (192, 1, True, False), (384, 8, True, True)]


def inputs(n, hw, cout, G, emb, resid, dev, seed):
    """Inputs with a DC offset and per-sample / per-group scales: a wrong mean, sample or group index cannot pass."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    scale = (1.0 + 0.75 * torch.arange(n).float())[:, None, None, None]
    x = (rn(n, hw, hw, CIN) * scale + 0.4).contiguous().to(dev)
    grp = (0.5 + torch.arange(G).float()).repeat_interleave(cout // G)
    w = (rn(cout, CIN, 3, 3) / (9 * CIN) ** 0.5 * grp[:, None, None, None]).to(dev)
    b = (0.6 * grp + 0.2 * rn(cout)).to(dev)
    ga, bt = (1.0 + 0.3 * rn(cout)).to(dev), (0.5 * rn(cout)).to(dev)
    e = (rn(n, cout + 64)).to(dev) if emb else None            # (a row stride wider than Cout, as the runtime's embedding table)
    r = (rn(n, hw, hw, cout) * scale).contiguous().to(dev) if resid else None
    return x, w, b, ga, bt, e, r


def two_launches(hip, dt, x, w, b, ga, bt, G, e, r):
    """conv with fused column statistics, then GroupNorm + SiLU (+ emb, + resid) folding them: (y, recorded max |y|, raw conv output)"""
    n, hw, _, _ = x.shape
    cout = w.shape[0]
    sr = hip.op_conv_stat_rows(dt, CIN, 0, 1, hw, hw, hip.CONV_PLAIN, 9, cout, n)
    assert sr == (16 if hw == 4 else 64), sr
    cs = torch.zeros((n, hw * hw // sr, cout, 2), dtype=torch.float32, device=x.device)
    raw = hip.op_conv_ex(dt, x, w, b, colstats=cs, stat_rows=sr)
    y, ex = hip.op_group_norm_ex(dt, raw, ga, bt, G, act_silu=True, emb=None if e is None else e[:, :cout].contiguous(), resid=r, colstats=cs, fast_silu=True,
                                 want_amax=True)
    return y, ex["amax"], raw


def one_case(hip, dev, dt, nmap, form, seed=9100):
    n, hw = nmap
    cout, G, emb, resid = form
    x, w, b, ga, bt, e, r = inputs(n, hw, cout, G, emb, resid, dev, seed + 10 * MAPS.index(nmap) + FORMS.index(form))
    with switches(**PP):
        two, amax2, raw = two_launches(hip, dt, x, w, b, ga, bt, G, e, r)
        one, amax1 = hip.op_conv_gn_self(dt, x, w, b, ga, bt, G, emb=e, resid=r, want_amax=True)
    two, one, raw = two.cpu(), one.cpu(), raw.cpu()
    assert torch.isfinite(two).all() and not torch.equal(two, raw)
    assert float(raw.mean().abs()) > 0.1, "the conv output must carry a DC offset"
    assert torch.equal(one, two), (nmap, form, dt, float((one - two).abs().max()))
    assert amax1 == amax2 == float(two.abs().max()), (nmap, form, dt, amax1, amax2)


def run(hip, dev, dts=None, light=False):
    dts = dts or (hip.BF16X3, hip.F16X2)
    k = 0
    for dt in dts:
        for nmap in MAPS:
            for form in (FORMS[:1] + FORMS[3:4] if light else FORMS):
                one_case(hip, dev, dt, nmap, form)
                k += 1
    return k


if __name__ == "__main__":
    import build_emu
    from nope_amd import hip
    hip._set_library_for_testing(hip.NopeLib(build_emu.build()))
    print(f"gn_epi_emu_case OK, {run(hip, 'cpu', light='--light' in sys.argv)} cases")
