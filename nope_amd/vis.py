"""Visualisation outputs of the evaluation flow, on the device: the contact sheets the reference saves as PNGs, their video and the
`vis_imgs` grid of its predictions file (src/model/model.py:214-249, :284-351, :367-375).

The reference builds every picture from a chain of small torch / torchvision ops -- unnormalize_to_zero_to_one, put_image_to_grid (f16
cast + scatter), clone, F.interpolate to 64 x 64, torchvision.utils.save_image (make_grid + an f16 quantisation to u8), re-opening the
PNG, imageio.mimwrite.  Here the arithmetic is one gather-resample-quantise kernel per stack of pictures (nope_op_vis_sheet: the PNG's
bytes, defined on the reference's f16 intermediate values) and one for the full-size f16 grid (nope_op_vis_grid); torch provides memory
only, PIL encodes the files (as nope_amd/vsd.py reads depth PNGs with it).  torchvision and imageio are not needed; an installed imageio
is used for the mp4, as the reference does.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .hip import VisCol as Column      # Column(tensor, unnormalize=False, clamp=False, index=None)

TILE, PADDING = 64, 2                  # model.py:233-235 (F.interpolate to 64 x 64); torchvision make_grid's default padding


def put_image_to_grid(list_imgs: Sequence[torch.Tensor], adding_margin: bool = True) -> Tuple[torch.Tensor, int]:
    """visualization_utils.py:43-57: (B, 3, H, W) images -> ((B * (ncol + 1), 3, H, W) f16 with a zero margin image behind every sample's
    columns, ncol + 1).  adding_margin=False: (B * ncol, 3, H, W) without the margin images (and still ncol + 1, as the reference returns)."""
    cols = [Column(t) for t in list_imgs]
    grid = hip.op_vis_grid(cols)[0]
    if not adding_margin:
        B, n = cols[0].tensor.shape[0], len(cols)
        grid = grid.reshape(B, n + 1, *grid.shape[1:])[:, :n].reshape(B * n, *grid.shape[1:])
    return grid, len(cols) + 1


def _chunk_plan(columns, tile, nrow, padding, max_bytes):
    """-> (columns as Columns, nrow, F, (Hs, Ws) or None, frames per launch): the frame axis cut into launches of at most max_bytes of sheet
    (at least one frame, at most 65 535 -- the launch grid's z limit)."""
    columns = [c if isinstance(c, Column) else Column(*c) if isinstance(c, (tuple, list)) else Column(c) for c in columns]
    if nrow is None:
        nrow = 4 * (len(columns) + 1)
    counts = {c.frames for c in columns if c.frames is not None}
    F = max(counts) if counts else 1
    if not columns or F == 0:
        return columns, nrow, F, None, 0
    Hs, Ws = hip.vis_sheet_shape(len(columns), columns[0].tensor.shape[0], max(int(tile), 0), int(nrow), max(int(padding), 0))
    return columns, nrow, F, (Hs, Ws), max(1, min(65535, int(max_bytes) // max(1, Hs * Ws * 3)))


def contact_sheet_chunks(columns, tile: int = TILE, nrow: Optional[int] = None, padding: int = PADDING, max_bytes: int = 64 << 20):
    """contact_sheet a chunk at a time: yields (first frame, uint8 (n, Hs, Ws, 3)) with n * Hs * Ws * 3 <= max_bytes (n >= 1), each chunk in
    memory of its own.  A caller that copies a chunk out and drops it before taking the next one holds at most max_bytes of sheet on the
    device, however many frames the stack has (PoseConditional's template pictures do)."""
    columns, nrow, F, _, per = _chunk_plan(columns, tile, nrow, padding, max_bytes)
    if per == 0:
        yield 0, hip.op_vis_sheet(columns, tile, nrow, padding)          # (the library's own argument checks; F = 0: an empty stack)
        return
    for f0 in range(0, F, per):
        yield f0, hip.op_vis_sheet(columns, tile, nrow, padding, frame0=f0, n_frames=min(per, F - f0))


def contact_sheet(columns, tile: int = TILE, nrow: Optional[int] = None, padding: int = PADDING, max_bytes: int = 64 << 20) -> torch.Tensor:
    """columns: `Column`s of one picture stack -> the PNG bytes of every frame, uint8 (F, Hs, Ws, 3).  nrow defaults to
    4 * (len(columns) + 1) (model.py:239: nrow = ncol * 4).  The whole stack is returned, so its memory is F * Hs * Ws * 3 bytes whatever
    max_bytes says: max_bytes only cuts the work into launches of at most that much sheet each (at least one frame, at most 65 535
    frames).  To bound memory, take the frames from contact_sheet_chunks."""
    columns, nrow, F, shape, per = _chunk_plan(columns, tile, nrow, padding, max_bytes)
    if per == 0:
        return hip.op_vis_sheet(columns, tile, nrow, padding)          # (the library's own argument checks; F = 0: an empty stack)
    out = torch.empty((F, *shape, 3), dtype=torch.uint8, device=columns[0].tensor.device)
    for f0 in range(0, F, per):
        n = min(per, F - f0)
        hip.op_vis_sheet(columns, tile, nrow, padding, frame0=f0, n_frames=n, out=out[f0:f0 + n])
    return out


def _hw3(sheet) -> np.ndarray:
    a = sheet.cpu().numpy() if isinstance(sheet, torch.Tensor) else np.asarray(sheet)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"sheet {a.shape} {a.dtype}: expected (H, W, 3) uint8")
    return np.ascontiguousarray(a)


def save_png(sheet_hw3_u8, path: str) -> str:
    """Image.fromarray(ndarr).save(path): what torchvision's save_image does with the quantised grid."""
    from PIL import Image
    Image.fromarray(_hw3(sheet_hw3_u8)).save(path)
    return path


def write_video(frames, path_stem: str, fps: int = 5) -> str:
    """frames: (F, H, W, 3) uint8 (tensor / array / list of (H, W, 3)).  With imageio: imageio.mimwrite(path_stem + ".mp4", frames, fps=5,
    macro_block_size=8), as model.py:249; otherwise a lossless animated PNG written with PIL to path_stem + ".apng".  Returns the path."""
    frames = [_hw3(f) for f in frames]
    if not frames:
        raise ValueError("write_video: no frames")
    try:
        import imageio
    except ImportError:
        imageio = None
    if imageio is not None:
        path = path_stem + ".mp4"
        imageio.mimwrite(path, frames, fps=fps, macro_block_size=8)
        return path
    from PIL import Image
    path = path_stem + ".apng"
    imgs = [Image.fromarray(f) for f in frames]
    imgs[0].save(path, format="PNG", save_all=True, append_images=imgs[1:], duration=int(round(1000 / fps)), loop=0)
    return path


def triptych(reference: torch.Tensor, second: torch.Tensor, third: torch.Tensor, third_unnormalize: bool, index: Optional[torch.Tensor] = None) -> List[Column]:
    """The three columns of every picture of the evaluation flow: unnormalize(reference), unnormalize(second), and the third either
    unnormalised (ground-truth images) or only clamped (decoded predictions, already in [0, 1] up to overshoot)."""
    return [Column(reference, unnormalize=True, clamp=True), Column(second, unnormalize=True, clamp=True),
            Column(third, unnormalize=third_unnormalize, clamp=True, index=index)]
