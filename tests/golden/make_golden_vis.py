"""Fixture of the visualisation pictures (nope_amd.vis, nope_op_vis_grid / nope_op_vis_sheet), recorded from THE REFERENCE'S
`unnormalize_to_zero_to_one` (src/model/utils.py:12-15) and `put_image_to_grid` (src/utils/visualization_utils.py:43-57):

    python tests/golden/make_golden_vis.py        # build container only (needs the reference sources)

A picture as PoseConditional.eval_geodesic builds it (src/model/model.py:290-306): reference image, query image and the decoded
prediction `sample` returns -- unnormalize_to_zero_to_one(decode_latent(.)) -- through put_image_to_grid, a clone, F.interpolate to
64 x 64 (bilinear, align_corners=False, on the f16 grid) and torchvision.utils.save_image(grid, path, nrow=16).  torchvision is not
installed here: make_grid(nrow, padding=2, pad_value=0) and save_image's mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)
are restated below, line for line of what they do to the tensor.  visualization_utils imports matplotlib (imported here first, so that
the MPLCONFIGDIR the module sets on import has no effect), torchvision, cv2 and moviepy (stubbed by _ref_import: import-time only).

The file stores the inputs (drawn here from a seeded generator, f32), the f16 grid and the u8 sheet of each case: the test reads nothing
else.  Values lie in [-1.4, 1.4]: both ends of the clamp act.  Random f32 does not compress, so the inputs are 0.45 MB of the file's
0.8 MB.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SEED = 2025
B = 2
CASES = (32, 72)            # image sizes: up-sampling to 64 x 64, and the non-integer scale 72 / 64
TILE, NROW, PADDING = 64, 16, 2


def inputs(S):
    """reference, query, decoded (B, 3, S, S) uniform in [-1.4, 1.4]: torch's CPU generator, seeded per case."""
    g = torch.Generator().manual_seed(SEED + S)
    return tuple(torch.rand(B, 3, S, S, generator=g) * 2.8 - 1.4 for _ in range(3))


def make_grid_and_quantise(tensor, nrow, padding):
    """torchvision.utils.make_grid(tensor, nrow, padding, pad_value=0.0) of a (n, 3, h, w) batch, then save_image's quantisation."""
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(np.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), 0.0)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)


def main():
    import matplotlib.pyplot  # noqa: F401  (before the reference module sets MPLCONFIGDIR)
    import _ref_import
    _ref_import.install()
    from src.model.utils import unnormalize_to_zero_to_one
    from src.utils.visualization_utils import put_image_to_grid
    out = {}
    for S in CASES:
        ref, query, decoded = inputs(S)
        pred_rgb = unnormalize_to_zero_to_one(decoded)                        # model.py:117-123: what `sample` returns
        vis_imgs = [unnormalize_to_zero_to_one(ref), unnormalize_to_zero_to_one(query), pred_rgb]
        vis_imgs, ncol = put_image_to_grid(vis_imgs)
        assert ncol == 4 and vis_imgs.dtype == torch.float16
        resized = F.interpolate(vis_imgs.clone(), (TILE, TILE), mode="bilinear", align_corners=False)
        sheet = make_grid_and_quantise(resized, nrow=ncol * 4, padding=PADDING)
        out[f"s{S}/reference"], out[f"s{S}/query"], out[f"s{S}/decoded"] = ref.numpy(), query.numpy(), decoded.numpy()
        out[f"s{S}/grid"] = vis_imgs.numpy()
        out[f"s{S}/sheet"] = sheet.numpy()
        print(S, vis_imgs.shape, sheet.shape)
    path = os.path.join(HERE, "vis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
