"""nope_op_crop_frames (ABI 13) and the batched sample assembly on top of it (nope_amd/dataset.py: crop_frames, process_test_batch): the loader's
chain -- paste on black through alpha, crop_frame's warp, ToTensor, * 2 - 1 (dataloader/shapeNet.py:184-210,167-182,64-69) -- for a stack of frames
in one launch.  The references are PIL's own `Image.paste` (computed here) and the per-frame `nope_op_warp_perspective` / `process_test_sample`
path on PIL-composited frames, which the batched path must reproduce bit for bit.  Every case runs on the CPU interpreter build of the kernels and,
marked `gpu`, on the device."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

BACKENDS = [pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def be(request):
    hip = request.getfixturevalue(request.param)
    return hip, ("cuda" if request.param == "gpu" else "cpu")


def paste_on_black(rgba: np.ndarray) -> np.ndarray:
    """shapeNet.py:206-210: (H, W, 4) uint8 -> (H, W, 3) uint8, by PIL."""
    img = Image.fromarray(rgba, "RGBA")
    black = Image.new("RGB", img.size, (0, 0, 0))
    black.paste(img, mask=img.getchannel("A"))
    return np.asarray(black).copy()


def test_every_composite_value(be):
    """One 256 x 256 frame with every (value, alpha) pair once, the value in R, G and B; identity map, no scaling: the three planes are PIL's paste."""
    hip, dev = be
    v, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))      # [alpha, value]
    rgba = np.ascontiguousarray(np.stack([v, v, v, a], -1))
    want = paste_on_black(rgba)
    assert np.array_equal(want[:, :, 0].astype(np.int64), (2 * v.astype(np.int64) * a + 255) // 510)      # (the closed form the header states)
    out = hip.op_crop_frames(torch.from_numpy(rgba)[None].to(dev), torch.eye(3).reshape(1, 9).to(dev), 256, 1.0, 0.0, round_u8=True)
    assert out.shape == (1, 3, 256, 256) and out.dtype == torch.float32
    got = out[0].cpu().numpy()
    for c in range(3):
        assert np.array_equal(got[c], want[:, :, c].astype(np.float32)), c


def _five_maps():
    """Inverse maps (output pixel -> source pixel) for 20 x 20 crops of 20-row, 24-column frames."""
    from nope_amd.dataset import SHAPENET_INTRINSIC, crop_transform
    from nope_amd.poses import get_obj_poses_from_template_level
    ident = np.eye(3)
    half = np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1.0]])
    c, s = np.cos(0.6), np.sin(0.6)
    rot = np.array([[1.4 * c, -1.4 * s, 12.0], [1.4 * s, 1.4 * c, 10.0], [0, 0, 1.0]]) @ np.array([[1.0, 0, -10], [0, 1.0, -10], [0, 0, 1]])
    persp = np.array([[1.1, 0.1, -1.0], [0.05, 0.9, 0.5], [0.004, -0.003, 1.0]])
    pose = get_obj_poses_from_template_level(0, "upper")[5].copy()
    pose[:3, 3] += [0.01, -0.02, 0.0]
    # the crop of a 512 x 512 render, then the 24 x 20 frame stretched over that render: source pixel = (24 / 512, 20 / 512) x render pixel
    crop = np.diag([24 / 512, 20 / 512, 1.0]) @ np.linalg.inv(crop_transform(SHAPENET_INTRINSIC, pose, 20, virtual_bbox_size=1))
    return np.stack([ident, half, rot, persp, crop])


@pytest.mark.parametrize("round_u8,scale,shift", [(True, 2.0 / 255.0, -1.0), (False, 2.0 / 255.0, -1.0)])
def test_batch_equals_loop_bit_for_bit(be, round_u8, scale, shift):
    """Five 20 x 24 RGBA frames (alpha 0 and 255 included), size 20 = 400 pixels (two blocks, the second partial), five different maps: frame f
    is op_warp_perspective of the PIL-composited frame f, bit for bit; the same frames as RGB equal op_warp_perspective on the raw frames."""
    hip, dev = be
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(5, 20, 24, 4), dtype=np.uint8)
    frames[:, :5, :, 3] = 0
    frames[:, 5:10, :, 3] = 255
    minv = _five_maps()
    # the rotation really samples beyond every border, the perspective map really has a varying w
    xs, ys = np.meshgrid(np.arange(20.0), np.arange(20.0))
    p = minv[2] @ np.stack([xs.ravel(), ys.ravel(), np.ones(400)])
    assert p[0].min() < -1 and p[0].max() > 24 and p[1].min() < -1 and p[1].max() > 20
    got = hip.op_crop_frames(torch.from_numpy(frames).to(dev), torch.from_numpy(minv).to(dev), 20, scale, shift, round_u8=round_u8)
    got3 = hip.op_crop_frames(torch.from_numpy(np.ascontiguousarray(frames[..., :3])).to(dev), torch.from_numpy(minv).to(dev), 20, scale, shift,
                              round_u8=round_u8)
    assert got.shape == got3.shape == (5, 3, 20, 20)
    for f in range(5):
        want = hip.op_warp_perspective(torch.from_numpy(paste_on_black(frames[f])).to(dev), minv[f], 20, scale, shift, round_u8=round_u8)
        assert torch.equal(got[f], want), f
        want3 = hip.op_warp_perspective(torch.from_numpy(np.ascontiguousarray(frames[f, :, :, :3])).to(dev), minv[f], 20, scale, shift, round_u8=round_u8)
        assert torch.equal(got3[f], want3), f
        assert float(want.abs().max()) > 0
    assert not torch.equal(got, got3)           # (the alpha channel mattered)


def test_crop_frames_mixed_sizes_and_per_frame_arguments(be):
    """crop_frames: one launch per source size, results back in frame order; intrinsics and box sizes given once or per frame."""
    hip, dev = be
    from nope_amd.dataset import SHAPENET_INTRINSIC, crop_frame, crop_frames
    from nope_amd.poses import get_obj_poses_from_template_level
    rng = np.random.default_rng(9)
    grid = get_obj_poses_from_template_level(0, "upper")
    frames = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((32, 32, 4), (16, 24, 4), (32, 32, 4))]
    Ks = np.stack([np.diag([32 / 512, 32 / 512, 1.0]) @ SHAPENET_INTRINSIC, np.diag([24 / 512, 16 / 512, 1.0]) @ SHAPENET_INTRINSIC,
                   np.diag([32 / 512, 32 / 512, 1.0]) @ SHAPENET_INTRINSIC])
    vbs = [1.0, 0.8, 1.2]
    out = crop_frames(frames, grid[:3], Ks, 12, vbs)
    assert out.shape == (3, 3, 12, 12) and out.device.type == dev
    for f in range(3):
        want = crop_frame(torch.from_numpy(paste_on_black(frames[f])).to(dev), None, Ks[f], grid[f], 12, virtual_bbox_size=vbs[f], normalize=True,
                          round_u8=True)
        assert torch.equal(out[f], want), f
    one = crop_frames(np.stack([frames[0], frames[2]]), grid[:2], Ks[0], 12, 1.0, normalize=False, round_u8=False)
    want = crop_frame(torch.from_numpy(paste_on_black(frames[2])).to(dev), None, Ks[0], grid[1], 12, virtual_bbox_size=1.0)
    assert torch.equal(one[1], want)
    # one RGB frame of 5 x 5: 75 bytes, no multiple of anything
    rgb = rng.integers(0, 256, size=(5, 5, 3), dtype=np.uint8)
    K5 = np.diag([5 / 512, 5 / 512, 1.0]) @ SHAPENET_INTRINSIC
    got = crop_frames([rgb], grid[3:4], K5, 6, 1.0)
    assert torch.equal(got[0], crop_frame(torch.from_numpy(rgb).to(dev), None, K5, grid[3], 6, virtual_bbox_size=1.0, normalize=True, round_u8=True))


def test_process_test_batch_equals_stacked_samples(be):
    """B = 2, N = 3, 32 x 32 RGBA sources, img_size 16: exactly the stacked process_test_sample results on PIL-composited frames."""
    hip, dev = be
    from nope_amd.dataset import process_test_batch, process_test_sample
    from nope_amd.poses import get_obj_poses_from_template_level
    rng = np.random.default_rng(3)
    B, N = 2, 3
    grid = get_obj_poses_from_template_level(0, "upper")
    # SHAPENET_INTRINSIC looks at a 512-pixel render: an object 16 units away, up and left of the optical axis, has its unit crop box (33 pixels)
    # over the 32 x 32 frame
    def shift(p, k):
        p = p.copy()
        p[:3, 3] = [-7.3 + 0.1 * k, -7.3 - 0.07 * k, 16.0]
        return p
    testing = grid[:N]
    q_poses = [shift(grid[4 + b], b) for b in range(B)]
    r_poses = [shift(grid[9 + b], b + 2) for b in range(B)]
    t_poses = [[shift(grid[i], i + b) for i in range(N)] for b in range(B)]
    q = rng.integers(0, 256, size=(B, 32, 32, 4), dtype=np.uint8)
    r = rng.integers(0, 256, size=(B, 32, 32, 4), dtype=np.uint8)
    t = rng.integers(0, 256, size=(B, N, 32, 32, 4), dtype=np.uint8)
    batch = process_test_batch(list(q), list(r), [list(t[b]) for b in range(B)], q_poses, r_poses, t_poses, testing, img_size=16, symmetries=[2, 0])
    dv = lambda a: torch.from_numpy(paste_on_black(a)).to(dev)
    samples = [process_test_sample(dv(q[b]), dv(r[b]), [dv(t[b, i]) for i in range(N)], q_poses[b], r_poses[b], t_poses[b], testing, img_size=16,
                                   symmetry=[2, 0][b]) for b in range(B)]
    assert sorted(batch) == sorted(samples[0])
    for k in samples[0]:
        want = torch.stack([s[k].cpu() for s in samples])
        assert batch[k].dtype == want.dtype and batch[k].shape == want.shape, k
        assert torch.equal(batch[k].cpu(), want), k
        assert batch[k].device.type == dev, k
    assert float((batch["query"] + 1).abs().max()) > 0 and float((batch["gt_templates"] + 1).abs().max()) > 0      # (not all border)
    nt = process_test_batch(list(q), list(r), None, q_poses, r_poses, None, testing, img_size=16, symmetries=[2, 0])
    nt2 = process_test_batch(list(q), list(r), [list(t[b]) for b in range(B)], q_poses, r_poses, t_poses, testing, img_size=16, symmetries=[2, 0],
                             with_templates=False)
    for other in (nt, nt2):
        assert sorted(other) == sorted(k for k in batch if k != "gt_templates")
        for k in other:
            assert torch.equal(other[k], batch[k]), k


def test_error_codes(be):
    """NOPE_ERR_UNSUPPORTED for a channel count other than 3 / 4, NOPE_ERR_ARG for no frames and for a null map pointer; nothing is launched."""
    hip, dev = be
    dll = hip.lib().dll
    fr = torch.zeros(2, 4, 4, 4, dtype=torch.uint8, device=dev)
    m = torch.eye(3, device=dev).reshape(1, 9).repeat(2, 1).contiguous()
    out = torch.full((2, 3, 4, 4), 7.0, device=dev)
    call = lambda frames, F, Cs, minv: dll.nope_op_crop_frames(frames, F, 4, 4, Cs, minv, out.data_ptr(), 4, 4, C.c_float(1.0), C.c_float(0.0), 1, None)
    assert call(fr.data_ptr(), 2, 2, m.data_ptr()) == -6
    assert call(fr.data_ptr(), 2, 1, m.data_ptr()) == -6
    assert call(fr.data_ptr(), 0, 4, m.data_ptr()) == -1
    assert call(fr.data_ptr(), 2, 4, None) == -1
    assert call(None, 2, 4, m.data_ptr()) == -1
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(fr.data_ptr(), 2, 4, m.data_ptr()) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    with pytest.raises(hip.NopeError, match="unsupported|UNSUPPORTED|not supported"):
        hip.op_crop_frames(torch.zeros(1, 4, 4, 2, dtype=torch.uint8, device=dev), m[:1], 4)


def _warp_restated(img, minv, size, scale, shift, round_u8):
    """kernels_misc.hip's warp_taps / warp_interp in numpy, operation for operation in f32: which products are fused (w and sy: one fma each; sx:
    none; every tap and the final scale / shift: fma) is part of the definition.  fma(a, b, c) is formed in f64, where a * b is exact."""
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, c: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)
    m = np.asarray(minv, f64).reshape(9).astype(f32)
    H, W, C = img.shape
    ys, xs = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    xf, yf = xs.astype(f32), ys.astype(f32)
    with np.errstate(all="ignore"):
        w = fma(m[7], yf, m[6] * xf) + m[8]
        sx = ((m[0] * xf + m[1] * yf) + m[2]) / w
        sy = (fma(m[3], xf, m[4] * yf) + m[5]) / w
    fx, fy = np.floor(sx), np.floor(sy)
    ax, ay = sx - fx, sy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    out = np.zeros((C, size, size), f32)
    for c in range(C):
        v = np.zeros((size, size), f32)
        for t in range(4):
            xx, yy = x0 + (t & 1), y0 + (t >> 1)
            wt = ((ax if t & 1 else f32(1) - ax) * (ay if t >> 1 else f32(1) - ay)).astype(f32)
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (w != 0)
            val = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), c].astype(f32)
            v = np.where(ok, fma(wt, val, v), v)
        if round_u8:
            v = np.clip(np.rint(v), 0, 255).astype(f32)
        out[c] = fma(f32(scale), v, f32(shift))
    return out


@pytest.mark.parametrize("round_u8", [True, False])
def test_warp_arithmetic_is_pinned(be, round_u8):
    """nope_op_warp_perspective's bits on a perspective map, a rotation and a crop map are those of the restated f32 operation sequence -- on
    the interpreter build and on the device alike: a compiler (or a refactor) that fuses another product changes a source position by an ulp
    and, after round_u8, a grey level."""
    hip, dev = be
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, size=(20, 24, 3), dtype=np.uint8)
    maps = _five_maps()
    for k in (1, 2, 3, 4):
        got = hip.op_warp_perspective(torch.from_numpy(img).to(dev), maps[k], 20, 2.0 / 255.0, -1.0, round_u8=round_u8).cpu().numpy()
        want = _warp_restated(img, maps[k], 20, 2.0 / 255.0, -1.0, round_u8)
        assert np.array_equal(got, want), (k, int((got != want).sum()), float(np.abs(got - want).max()))
