"""The visualisation outputs (nope_amd.vis, csrc/kernels_vis.hip): nope_op_vis_grid / nope_op_vis_sheet against a torch restatement of the
reference's op chain and against results recorded from the reference's own put_image_to_grid / unnormalize_to_zero_to_one
(tests/golden/make_golden_vis.py: vis.npz), the launchers' argument checks, and the Python flow -- generate_templates / eval_geodesic with
visualize=True -- with stub networks on the interpreter and with the real VAE + U-Net on the device.

The restatement (`expected_grid`, `expected_sheet`) is the chain the reference runs per picture, on the CPU: the column flags in f32, .half(),
index-assignment into a zero f16 grid (visualization_utils.py:51-56), F.interpolate(grid, (tile, tile), bilinear, align_corners=False) ON
THE F16 TENSOR, torchvision's make_grid(nrow, padding, pad_value=0) written out (torchvision is not installed), and save_image's
mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8) on the f16 grid.

Conditions everywhere: the f16 grid is bit-identical; no sheet byte differs by more than one level; at most 1e-3 of the bytes differ at all."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN_CASES = (32, 72)          # tests/golden/make_golden_vis.py: CASES

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]
MAX_LEVELS, MAX_FRACTION = 1, 1e-3


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    dev = "cuda" if request.param == "gpu" else "cpu"
    return hip, dev, request.param


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def expected_grid(cols):
    """cols: [(images (B, 3, H, W) f32 on the CPU, unnormalize, clamp)] -> put_image_to_grid's (B * (n + 1), 3, H, W) f16."""
    n, (B, _, H, W) = len(cols), cols[0][0].shape
    grid = torch.zeros((B * (n + 1), 3, H, W)).to(torch.float16)
    idx = torch.arange(0, grid.shape[0], n + 1).to(torch.int64)
    for i, (x, unnormalize, clamp) in enumerate(cols):
        x = x.clone().float()
        if unnormalize:
            x = (x + 1) * 0.5
        if clamp:
            x = x.clamp(0, 1)
        grid[idx + i] = x.to(torch.float16)
    return grid


def expected_sheet(grid, tile=64, nrow=16, padding=2):
    """(n_img, 3, H, W) f16 -> the PNG's (Hs, Ws, 3) u8."""
    small = F.interpolate(grid.clone(), (tile, tile), mode="bilinear", align_corners=False)
    assert small.dtype == torch.float16
    n_img = small.shape[0]
    xmaps = min(nrow, n_img)
    ymaps = -(-n_img // xmaps)
    cell = tile + padding
    sheet = torch.zeros((3, cell * ymaps + padding, cell * xmaps + padding), dtype=torch.float16)
    for k in range(n_img):
        y, x = (k // xmaps) * cell + padding, (k % xmaps) * cell + padding
        sheet[:, y:y + tile, x:x + tile] = small[k]
    return sheet.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def check_sheet(got, want, what=""):
    got, want = torch.as_tensor(np.asarray(got)), torch.as_tensor(np.asarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.uint8, (what, got.shape, want.shape)
    d = (got.int() - want.int()).abs()
    worst, frac = int(d.max()), float((d > 0).float().mean())
    print(f"{what}: {tuple(got.shape)} worst level difference {worst}, fraction of bytes that differ {frac:.2e}")
    assert worst <= MAX_LEVELS and frac <= MAX_FRACTION, (what, worst, frac)


def check_grid(got, want, what=""):
    got, want = torch.as_tensor(np.asarray(got)), torch.as_tensor(np.asarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float16, (what, got.shape, want.shape)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (what, int((got.view(torch.int16) != want.view(torch.int16)).sum()))


def _uniform(g, lo, hi, *shape):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ---- 1. sheet and grid against the restatement -------------------------------------------------------------------------------------------
N_BANK, N_FRAMES = 4, 3
_PICTURES = {}


def _pictures(B, S):
    """Seeded inputs and the expectation of the two pictures of one (B, S), built once and shared by the backends:
    "framed":   a column that is the same in every frame, one with its own image per frame (clamp only), one gathered through a
                (B, 5)-strided index;
    "gathered": the shared column, the gathered one, and one gathered through an index that lies outside the bank for every sample."""
    key = (B, S)
    if key not in _PICTURES:
        g = torch.Generator().manual_seed(1000 * B + S)
        shared = _uniform(g, -1.4, 1.4, B, 3, S, S)
        framed = _uniform(g, -0.2, 1.2, B, N_FRAMES, 3, S, S)
        bank = _uniform(g, -1.4, 1.4, B, N_BANK, 3, S, S)
        idx5 = torch.randint(0, N_BANK, (B, 5), generator=g)
        bad = torch.tensor([N_BANK + 3, -2, 1 << 40, -(1 << 40), N_BANK][:B], dtype=torch.int64)
        rows = torch.arange(B)
        picked, clamped = bank[rows, idx5[:, 0]], bank[rows, bad.clamp(0, N_BANK - 1)]
        want = {"framed": [], "gathered": []}
        for f in range(N_FRAMES):
            want["framed"].append(expected_grid([(shared, True, True), (framed[:, f], False, True), (picked, True, True)]))
            want["gathered"].append(expected_grid([(shared, True, True), (picked, True, True), (clamped, True, False)]))
        grids = {k: torch.stack(v) for k, v in want.items()}
        sheets = {k: torch.stack([expected_sheet(gr) for gr in v]) for k, v in grids.items()}
        _PICTURES[key] = (shared, framed, bank, idx5, bad, grids, sheets)
    return _PICTURES[key]


@pytest.mark.parametrize("S", [32, 64, 72, 128])
@pytest.mark.parametrize("B", [2, 5])
def test_sheet_and_grid_match_the_restatement(be, B, S):
    """B = 2: 8 images, one row, xmaps < nrow; B = 5: 20 images, a ragged second row of 4.  S = 32 / 64 / 72 / 128: up-sampling, identity,
    a non-integer scale, 2 : 1.  Three frames.  Inputs in [-1.4, 1.4] (unnormalised columns) and [-0.2, 1.2] (clamp only): both clamps act."""
    hip, dev, _ = be
    from nope_amd.vis import Column, contact_sheet
    shared, framed, bank, idx5, bad, grids, sheets = _pictures(B, S)
    idx5d, bank_d, shared_d = idx5.to(dev), bank.to(dev), shared.to(dev)
    assert idx5d[:, 0].stride(0) == 5
    pictures = {
        "framed": [Column(shared_d, True, True), Column(framed.to(dev), False, True), Column(bank_d, True, True, index=idx5d[:, 0])],
        "gathered": [Column(shared_d, True, True), Column(bank_d, True, True, index=idx5d[:, 0]), Column(bank_d, True, False, index=bad.to(dev))],
    }
    for name, cols in pictures.items():
        nf = None if name == "framed" else N_FRAMES          # (no column of "gathered" has a frame axis: the caller says how many frames)
        check_grid(hip.op_vis_grid(cols, n_frames=nf).cpu(), grids[name], f"{name} B={B} S={S}")
        got = contact_sheet(cols, nrow=16).cpu() if name == "framed" else hip.op_vis_sheet(cols, 64, 16, 2, n_frames=nf).cpu()
        assert got.shape[0] == N_FRAMES
        check_sheet(got, sheets[name], f"{name} B={B} S={S}")


def test_contact_sheet_chunks(be, monkeypatch):
    """Seven frames under a max_bytes of two frames: four launches, the same bytes as one launch; and frames whose size is not a multiple of
    four bytes, one launch each: every chunk then starts inside a dword (1 890-byte frames; tile 16, padding 1, nrow 2)."""
    hip, dev, _ = be
    from nope_amd import vis
    g = torch.Generator().manual_seed(5)
    ref, tpl = _uniform(g, -1.4, 1.4, 2, 3, 32, 32), _uniform(g, -0.2, 1.2, 2, 7, 3, 32, 32)
    cols = [vis.Column(ref.to(dev), True, True), vis.Column(tpl.to(dev), False, True)]
    calls = []
    real = hip.op_vis_sheet
    monkeypatch.setattr(hip, "op_vis_sheet", lambda *a, **k: calls.append((k.get("frame0"), k.get("n_frames"))) or real(*a, **k))
    one = 2 * 3 * ((64 + 2) * 1 + 2) * ((64 + 2) * 6 + 2)
    got = vis.contact_sheet(cols, max_bytes=one + 17).cpu()
    assert calls == [(0, 2), (2, 2), (4, 2), (6, 1)]
    want = torch.stack([expected_sheet(expected_grid([(ref, True, True), (tpl[:, f], False, True)]), nrow=12) for f in range(7)])
    check_sheet(got, want, "four chunks")
    assert torch.equal(got, real(cols, 64, 12, 2).cpu())
    # a chunk at a time, each in memory of its own and within max_bytes: what bounds the device memory of a long stack
    calls.clear()
    chunks = list(vis.contact_sheet_chunks(cols, max_bytes=one + 17))
    assert [f0 for f0, _ in chunks] == [0, 2, 4, 6] and calls == [(0, 2), (2, 2), (4, 2), (6, 1)]
    assert all(c.numel() <= one + 17 and c.is_contiguous() for _, c in chunks)
    assert len({c.untyped_storage().data_ptr() for _, c in chunks}) == 4
    assert torch.equal(torch.cat([c for _, c in chunks]).cpu(), got)
    # one column, one sample: two images of 16 x 16 -> (18, 35, 3) = 1 890 bytes per frame
    calls.clear()
    small = _uniform(g, -1.4, 1.4, 1, 5, 3, 32, 32)
    got = vis.contact_sheet([vis.Column(small.to(dev), True, True)], tile=16, nrow=2, padding=1, max_bytes=1).cpu()
    assert got.shape == (5, 18, 35, 3) and [c[1] for c in calls] == [1] * 5
    want = torch.stack([expected_sheet(expected_grid([(small[:, f], True, True)]), tile=16, nrow=2, padding=1) for f in range(5)])
    check_sheet(got, want, "unaligned frames")


def test_put_image_to_grid(be):
    hip, dev, _ = be
    from nope_amd.vis import put_image_to_grid
    g = torch.Generator().manual_seed(6)
    imgs = [_uniform(g, 0, 1, 3, 3, 9, 7) for _ in range(2)]          # (3 * 9 * 7 elements per image: the one-element path)
    grid, ncol = put_image_to_grid([t.to(dev) for t in imgs])
    assert ncol == 3
    check_grid(grid.cpu(), expected_grid([(t, False, False) for t in imgs]))
    flat, ncol = put_image_to_grid([t.to(dev) for t in imgs], adding_margin=False)
    assert ncol == 3 and torch.equal(flat.cpu(), torch.stack([t.half() for t in imgs], 1).reshape(6, 3, 9, 7))


# ---- 2. recorded from the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", GOLDEN_CASES)
def test_matches_the_reference_record(be, golden, S):
    """vis.npz: the reference's put_image_to_grid over its unnormalize_to_zero_to_one of a reference image, a query image and a decoded
    prediction (its `sample` hands out unnormalize_to_zero_to_one(decode); ours (decode + 1) / 2, clamped by the column), then
    F.interpolate and the make_grid / quantisation restatement.  Inputs and results are read from the file."""
    hip, dev, _ = be
    from nope_amd.vis import Column, contact_sheet
    z = golden("vis.npz")
    ref, query, decoded = (z[f"s{S}/{k}"] for k in ("reference", "query", "decoded"))
    assert ref.shape == query.shape == decoded.shape == (2, 3, S, S) and ref.dtype == torch.float32
    cols = [Column(ref.to(dev), True, True), Column(query.to(dev), True, True), Column(((decoded + 1) / 2).to(dev), False, True)]
    check_grid(hip.op_vis_grid(cols)[0].cpu(), z[f"s{S}/grid"], f"golden S={S}")
    check_sheet(contact_sheet(cols)[0].cpu(), z[f"s{S}/sheet"], f"golden S={S}")


# ---- 3. argument checks ------------------------------------------------------------------------------------------------------------------
def test_argument_checks(emu):
    """Every bad argument returns a non-zero code without a launch and raises NopeError through the wrapper; F = 0 succeeds and writes nothing."""
    hip = emu
    dll = hip.lib().dll
    B, H, W = 2, 8, 8
    img = torch.rand(B, 4, 3, H, W)
    idx = torch.zeros(B, dtype=torch.int64)
    sheet = torch.full((4, 12, 42, 3), 7, dtype=torch.uint8)       # tile 8, padding 2, nrow 4: (8 + 2) * 1 + 2, (8 + 2) * 4 + 2
    grid = torch.full((4, 2 * B, 3, H, W), 7.0, dtype=torch.float16)

    def col(**kw):
        c = hip.VisColumn(data=img.data_ptr(), stride_b=img.stride(0), stride_f=img.stride(1), index=None, index_stride=0, index_limit=0, flags=3)
        for k, v in kw.items():
            setattr(c, k, v)
        return (hip.VisColumn * 9)(*([c] * 9))

    def run_sheet(cols=None, n_cols=1, B=B, F=4, H=H, W=W, tile=8, nrow=4, padding=2, out=sheet.data_ptr()):
        return dll.nope_op_vis_sheet(col() if cols is None else cols, n_cols, B, F, H, W, tile, nrow, padding, out, None)

    def run_grid(cols=None, n_cols=1, B=B, F=4, H=H, W=W, out=grid.data_ptr()):
        return dll.nope_op_vis_grid(col() if cols is None else cols, n_cols, B, F, H, W, out, None)

    assert run_sheet() == 0 and run_grid() == 0 and int(sheet.max()) > 7 and float(grid.max()) < 7
    sheet.fill_(7)
    grid.fill_(7.0)
    bad = [dict(n_cols=0), dict(n_cols=9), dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(F=-1), dict(out=None), dict(cols=col(data=None)),
           dict(cols=col(index=idx.data_ptr(), index_stride=1, index_limit=0))]
    for kw in bad:
        assert run_grid(**kw) != 0, kw
    for kw in bad + [dict(tile=0), dict(tile=-3), dict(nrow=0), dict(padding=-1)]:
        assert run_sheet(**kw) != 0, kw
    assert dll.nope_op_vis_sheet(None, 1, B, 4, H, W, 8, 4, 2, sheet.data_ptr(), None) != 0
    assert dll.nope_op_vis_grid(None, 1, B, 4, H, W, grid.data_ptr(), None) != 0
    # F = 0: success, nothing written -- with null pointers too
    assert run_sheet(F=0) == 0 and run_grid(F=0) == 0 and run_sheet(F=0, out=None) == 0 and run_grid(F=0, out=None) == 0
    assert dll.nope_op_vis_sheet(None, 1, B, 0, H, W, 8, 4, 2, None, None) == 0
    assert int(sheet.min()) == int(sheet.max()) == 7 and float(grid.min()) == float(grid.max()) == 7.0      # nothing above wrote anything
    assert run_sheet(F=0, tile=0) != 0            # (a bad argument is a bad argument with no frames too)
    # through the wrappers
    one = hip.VisCol(img[:, 0])
    for kw in (dict(tile=0), dict(nrow=0), dict(padding=-1)):
        with pytest.raises(hip.NopeError, match="nope_op_vis_sheet"):
            hip.op_vis_sheet([one], **{**dict(tile=8, nrow=4, padding=2), **kw})
    with pytest.raises(hip.NopeError, match="nope_op_vis_sheet"):
        hip.op_vis_sheet([one] * 9, 8, 4, 2)
    with pytest.raises(hip.NopeError, match="nope_op_vis_grid"):
        hip.op_vis_grid([one] * 9)
    with pytest.raises(hip.NopeError):
        hip.op_vis_sheet([], 8, 4, 2)
    empty = hip.op_vis_sheet([hip.VisCol(img[:, :0])], 8, 4, 2)
    assert empty.shape == (0, 12, 42, 3) and hip.op_vis_grid([hip.VisCol(img[:, :0])]).shape == (0, 2 * B, 3, H, W)


# ---- 4. / 5. the Python flow -------------------------------------------------------------------------------------------------------------
class _StubVae(torch.nn.Module):
    """A foreign decoder (decode_latent without `unnormalize`, as test_sample_with_a_foreign_decoder's): 8 x 8 average pooling as the
    encoder, nearest-neighbour up-sampling times 20 -- well beyond [-1, 1], so the pictures' clamps act -- as the decoder."""
    latent_dim, name = 3, "vae"

    def encode_image(self, image, mode=None):
        return F.avg_pool2d(image, 8)

    def decode_latent(self, latent):
        return F.interpolate(latent, scale_factor=8, mode="nearest") * 20


class _StubUNet(torch.nn.Module):
    """What PoseConditional reads from a U-Net: `encoder`, `channels`, forward, forward_hypotheses, finish_range_check."""

    def __init__(self, encoder):
        super().__init__()
        self.encoder, self.channels = encoder, 3

    def forward(self, x, pose):
        return x * (1 + 0.3 * pose[:, 0])[:, None, None, None]

    def forward_hypotheses(self, feat, poses, out=None, out_dtype=None, defer_range_check=False):
        out.copy_(feat[:, None] * (1 + 0.3 * poses[..., 0])[:, :, None, None, None])
        return out

    def finish_range_check(self):
        return False


def _batch(B, N, S, seed, dev):
    from nope_amd.harness import synthetic_batch
    batch = synthetic_batch(B, N, S, seed, dev, gt_templates=True)
    assert batch["gt_templates"].shape == (B, N, 3, S, S)
    return batch


def _media(save_dir):
    return sorted(os.listdir(os.path.join(save_dir, "media")))


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _check_flow(make_pc, batch, tmp_path, N):
    """eval_geodesic(visualize=True, save_prediction=True) against the restatement for the tensors sample / generate_templates return,
    and against the visualize=False run."""
    from PIL import Image
    B, S = batch["query"].shape[0], batch["query"].shape[-1]
    plain_dir, vis_dir = str(tmp_path / "plain"), str(tmp_path / "vis")
    pc = make_pc(plain_dir)
    res0 = pc.eval_geodesic(batch, "synthetic", visualize=False, save_prediction=True)
    assert _media(plain_dir) == []
    z0 = np.load(os.path.join(plain_dir, "predictions", "pred_step0_rank0.npz"))
    assert sorted(z0.files) == ["query_pose", "similarity"]
    pc = make_pc(vis_dir)
    res1 = pc.eval_geodesic(batch, "synthetic", visualize=True, save_prediction=True)
    names = _media(vis_dir)
    video = [n for n in names if n.startswith("video_")]
    assert video in (["video_step0_rank0.apng"], ["video_step0_rank0.mp4"])
    assert sorted(set(names) - set(video)) == sorted(["reconst_step0_rank0.png", "retrieved_step0_rank0.png"] + [f"template{i}_rank0.png" for i in range(N)])
    # scores, indices, metrics: the bits of the visualize=False run
    z1 = np.load(os.path.join(vis_dir, "predictions", "pred_step0_rank0.npz"))
    assert sorted(z1.files) == ["query_pose", "similarity", "vis_imgs"]
    assert np.array_equal(z0["similarity"], z1["similarity"]) and np.array_equal(z0["query_pose"], z1["query_pose"]) and res0 == res1
    sim, idx = pc.retrieval(batch["query"], pc.generate_templates(batch["reference"], batch["all_relativeR"])[0])
    assert np.array_equal(sim.cpu().numpy(), z1["similarity"])
    # the pictures
    ref, query, gt = batch["reference"].cpu(), batch["query"].cpu(), batch["gt_templates"].cpu()
    media = os.path.join(vis_dir, "media")
    _, pred_rgb = pc.sample(batch["reference"], batch["gt_relativeR"])
    want = expected_sheet(expected_grid([(ref, True, True), (query, True, True), (pred_rgb.cpu(), False, True)]))
    check_sheet(_png(os.path.join(media, "reconst_step0_rank0.png")), want, "reconst")
    _, tpl, _ = pc.generate_templates(batch["reference"], batch["all_relativeR"])      # (the decoder's output in [-1, 1]: the column unnormalises it)
    frames = []
    for i in range(N):
        want = expected_sheet(expected_grid([(ref, True, True), (gt[:, i], True, True), (tpl[:, i].cpu(), True, True)]))
        frames.append(_png(os.path.join(media, f"template{i}_rank0.png")))
        check_sheet(frames[-1], want, f"template {i}")
    retrieved = expected_grid([(ref, True, True), (query, True, True), (gt[torch.arange(B), idx[:, 0].cpu()], True, True)])
    check_sheet(_png(os.path.join(media, "retrieved_step0_rank0.png")), expected_sheet(retrieved), "retrieved")
    assert z1["vis_imgs"].shape == (4 * B, 3, S, S) and z1["vis_imgs"].dtype == np.float16
    check_grid(z1["vis_imgs"], retrieved, "vis_imgs")
    if video[0].endswith(".apng"):          # lossless: the video's frames are the PNGs
        with Image.open(os.path.join(media, video[0])) as im:
            assert im.n_frames == N
            for i in range(N):
                im.seek(i)
                assert np.array_equal(np.array(im.convert("RGB")), frames[i])
    return pc


def test_flow_with_stub_networks(emu, tmp_path, monkeypatch):
    """B = 2, S = 32 and SIX templates: retrieval ranks a top-5 (nope_topk: k <= N, as torch.topk), so the bank needs at least five."""
    from nope_amd.model import PoseConditional
    from tests.util import StubEncoder
    B, N, S = 2, 6, 32
    batch = _batch(B, N, S, 11, "cpu")

    def make_pc(save_dir):
        return PoseConditional(_StubUNet(_StubVae()), None, {"similarity_metric": "l2"}, save_dir)

    pc = _check_flow(make_pc, batch, tmp_path, N)
    tpl = pc.generate_templates(batch["reference"], batch["all_relativeR"])[1]
    assert float(tpl.min()) < -1 and float(tpl.max()) > 1                # (the clamp has something to do)
    with pytest.raises(ValueError, match="gt_templates"):
        pc.generate_templates(batch["reference"], batch["all_relativeR"], visualize=True)
    # a batch without ground-truth templates: the caller is told which key is missing, before anything is written
    nogt = str(tmp_path / "nogt")
    with pytest.raises(ValueError, match="gt_templates"):
        make_pc(nogt).eval_geodesic({k: v for k, v in batch.items() if k != "gt_templates"}, "synthetic", visualize=True, save_prediction=True)
    assert _media(nogt) == [] and os.listdir(os.path.join(nogt, "predictions")) == []
    # nothing to decode with: visualize is forced off (model.py:269-274) and everything is as it was
    nodec = str(tmp_path / "nodec")
    u = _StubUNet(StubEncoder(3))
    lat = {**batch, "query": F.avg_pool2d(batch["query"], 8), "reference": F.avg_pool2d(batch["reference"], 8)}
    pcn = PoseConditional(u, None, {"similarity_metric": "l2"}, nodec)
    resn = pcn.eval_geodesic(lat, "synthetic", visualize=True, save_prediction=True)
    assert _media(nodec) == [] and sorted(np.load(os.path.join(nodec, "predictions", "pred_step0_rank0.npz")).files) == ["query_pose", "similarity"]
    assert resn == PoseConditional(u, None, {"similarity_metric": "l2"}, None).eval_geodesic(lat, "synthetic")
    assert pcn.generate_templates(lat["reference"], lat["all_relativeR"], gt_templates=batch["gt_templates"], visualize=True)[1:] == (None, None)
    # no save_dir: nothing is written, the third value stays None, the tensors are the same
    free = make_pc(None)
    bank, tpl, vid = free.generate_templates(batch["reference"], batch["all_relativeR"], gt_templates=batch["gt_templates"], visualize=True)
    bank0, tpl0, vid0 = pc.generate_templates(batch["reference"], batch["all_relativeR"])
    assert vid is None and vid0 is None and torch.equal(bank, bank0) and torch.equal(tpl, tpl0)
    # rank 1 of 2 under template_parallel: only its slice's pictures, and no collective
    from nope_amd import dist as ndist
    monkeypatch.setattr(ndist, "world", lambda: (1, 2))
    for name in ("all_gather_scores", "all_gather_scores_topk", "all_gather_topk_pairs", "gather_buffers"):
        monkeypatch.setattr(ndist, name, lambda *a, **k: pytest.fail("generate_templates entered a collective"))
    shard_dir = str(tmp_path / "shard")
    sharded = PoseConditional(_StubUNet(_StubVae()), None, {"similarity_metric": "l2"}, shard_dir, template_parallel=True)
    lo, hi = ndist.shard_range(N, 1, 2)
    sbank, stpl, svid = sharded.generate_templates(batch["reference"], batch["all_relativeR"], gt_templates=batch["gt_templates"], visualize=True)
    assert (lo, hi) == (3, 6) and stpl.shape[1] == hi - lo and os.path.basename(svid).startswith("video_step0_rank1.")
    assert _media(shard_dir) == sorted([f"template{i}_rank1.png" for i in range(lo, hi)] + [os.path.basename(svid)])
    for i in range(lo, hi):
        assert np.array_equal(_png(os.path.join(shard_dir, "media", f"template{i}_rank1.png")), _png(str(tmp_path / "vis" / "media" / f"template{i}_rank0.png")))


@pytest.mark.gpu
@pytest.mark.parametrize("cdt", ["f32", "f16x2"])
def test_flow_with_the_real_networks(gpu, tmp_path, cdt):
    """The setup of test_pose_conditional_with_vae: the tiny VAE, a U-Net of width 32, B = 2, six templates, 32 x 32 images."""
    from nope_amd.model import PoseConditional
    from tests.golden.make_golden_vae import SEED, make_vae
    from tests.test_vae import _unet
    B, N, S = 2, 6, 32
    batch = _batch(B, N, S, 12, "cuda")

    def make_pc(save_dir):
        vae = make_vae("tiny", compute_dtype=cdt)
        u = _unet(cdt, vae)
        vae.synth_init_(SEED)
        return PoseConditional(u, None, {"similarity_metric": "l2"}, save_dir).cuda()

    _check_flow(make_pc, batch, tmp_path, N)
