"""Coarse-to-fine pose retrieval over nested viewpoint grids (no reference counterpart: the reference scores every
pose of the grid, src/model/model.py:313,323).

Icosphere levels are nested (nope_amd.poses.icosphere_vertices: coarser grids are prefixes of finer ones), and the U-Net takes any relative
rotation, so a query can be scored in stages: the poses of the coarsest level, then the next level's neighbours of the best few, and so on.
What costs time in a retrieval step is the U-Net pass per pose; the search decides which poses get one.  The stage loop below runs two device
ops (hip.op_c2f_expand / hip.op_c2f_commit, csrc/kernels_search.hip) around the caller's `evaluate` and hip.topk; nothing in it is read by the host.

The result's similarity row is sparse: -inf where nothing was evaluated.  That is an ordinary input to hip.topk, hip.op_pose_modes and
PoseConditional.refine_from_feat.  With synthetic weights the U-Net's score landscape is not smooth: the feature claims nothing about
accuracy on real data; on a planted unimodal landscape three seeds reach the exhaustive top-1 (tests/test_coarse_to_fine.py).
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import hip


class C2FResult(NamedTuple):
    """coarse_to_fine_search: similarity (B, N) f32 (-inf where not evaluated), nearest_idx (B, k) int64 (hip.topk of it), evaluated (B, N)
    uint8, n_evaluated (B,) int32, cand (one (B, M_s) int32 per stage: the candidates in emission order, then -1), n_dropped (n_stages, B)
    int32 (candidates beyond a stage's capacity: not evaluated), status (n_stages,) int32 (hip.C2F_OVERFLOW | hip.C2F_BAD_SEED per stage).
    Everything stays on the device."""
    similarity: torch.Tensor
    nearest_idx: torch.Tensor
    evaluated: torch.Tensor
    n_evaluated: torch.Tensor
    cand: List[torch.Tensor]
    n_dropped: torch.Tensor
    status: torch.Tensor


def stage_capacities(stage_of: np.ndarray, n_stages: int, seeds: int, capacity: Union[None, int, Sequence[int]]) -> List[int]:
    """The candidate slots of each stage: stage 0 holds every pose of its level (a host-known count); a later stage `capacity`
    (default 6 per seed: a vertex of an icosphere grid has 4 to 6 neighbours one level down).  A sequence gives
    every stage its own."""
    if capacity is not None and not isinstance(capacity, (int, np.integer)):
        caps = [int(c) for c in capacity]
        if len(caps) != n_stages:
            raise ValueError(f"capacity has {len(caps)} entries for {n_stages} stages")
        return caps
    later = 6 * seeds if capacity is None else int(capacity)
    return [int((stage_of == 0).sum())] + [later] * (n_stages - 1)


def coarse_to_fine_search(evaluate: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], all_relativeR: torch.Tensor, template_poses: torch.Tensor,
                          stage_of, n_stages: Optional[int] = None, seeds: int = 3, radii_rad=..., capacity=None, k: int = 5,
                          dist_kind: int = hip.C2F_VIEWPOINT) -> C2FResult:
    """The stage loop.  evaluate(rows (B, M, 6) f32, cand (B, M) int32) -> scores (B, M) f32 scores the poses `rows` (a padded slot, cand
    -1, carries a finite pose whose score is discarded).  all_relativeR (B, N, 6), template_poses (B|1, N, 3, 3), stage_of (N,) on the HOST
    (nope_amd.poses.grid_stages: the level at which a pose first appears), n_stages (default: max(stage_of) + 1).
      stage 0: every pose with stage_of == 0 is evaluated;
      stage s >= 1: the `seeds` best poses so far (hip.topk of the sparse row) each admit the not yet evaluated poses with stage_of <= s
      within radii_rad[s] of them under `dist_kind` (hip.C2F_VIEWPOINT / hip.C2F_ROTATION), at most `capacity` per query;
    then the top-k of the sparse row.  radii_rad: a sequence indexed by stage (entry 0 unused), a scalar for every stage, or -- the default --
    nope_amd.poses.stage_radii of the first sample's grid (host NumPy, before the loop).  capacity: see stage_capacities.
    Needs count(stage_of == 0) >= max(k, seeds): the seeds and the answer are evaluated poses."""
    stage_np = np.asarray(stage_of.cpu() if isinstance(stage_of, torch.Tensor) else stage_of).astype(np.int32)
    B, N = all_relativeR.shape[:2]
    if stage_np.shape != (N,):
        raise ValueError(f"stage_of {stage_np.shape}: expected ({N},)")
    n_stages = int(stage_np.max()) + 1 if n_stages is None else int(n_stages)
    seeds, k = int(seeds), int(k)
    if n_stages < 1 or not 1 <= seeds <= hip.C2F_MAX_SEEDS or not 1 <= k <= 16:
        raise ValueError(f"n_stages {n_stages} >= 1, seeds {seeds} in [1, {hip.C2F_MAX_SEEDS}] and k {k} in [1, 16]")
    if int((stage_np == 0).sum()) < max(k, seeds):
        raise ValueError(f"coarse_to_fine_search: stage 0 holds {int((stage_np == 0).sum())} poses, fewer than max(k, seeds) = {max(k, seeds)}")
    if radii_rad is ...:
        from .poses import stage_radii
        radii = stage_radii(np.asarray(template_poses[0].detach().cpu(), dtype=np.float64), stage_np, dist_kind)
        radii = np.concatenate([radii, np.full(max(0, n_stages - len(radii)), radii[-1])])
    elif np.ndim(radii_rad) == 0:
        radii = np.full(n_stages, float(radii_rad))
    else:
        radii = np.asarray(radii_rad, dtype=np.float64)
    if len(radii) < n_stages:
        raise ValueError(f"radii_rad has {len(radii)} entries for {n_stages} stages (entry s is stage s's; entry 0 is unused)")
    caps = stage_capacities(stage_np, n_stages, seeds, capacity)

    hip.require_device(all_relativeR)
    dev = all_relativeR.device
    rel = all_relativeR.float().contiguous()
    poses = template_poses.to(device=dev, dtype=torch.float64).contiguous()
    stage_dev = torch.from_numpy(stage_np).to(dev)
    similarity = torch.full((B, N), float("-inf"), dtype=torch.float32, device=dev)
    state = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    cands, n_cand, n_dropped, status = [], [], [], []
    for s in range(n_stages):
        seed_idx = hip.topk(similarity, seeds)[1] if s > 0 else None
        ex = hip.op_c2f_expand(poses, stage_dev, s, state, seed_idx, rel, radius_rad=float(radii[s]) if s > 0 else 0.0, dist_kind=dist_kind,
                               capacity=caps[s])
        hip.op_c2f_commit(evaluate(ex.rows, ex.cand), ex.cand, similarity)
        cands.append(ex.cand)
        n_cand.append(ex.n_cand)
        n_dropped.append(ex.n_dropped)
        status.append(ex.status)
    _, nearest_idx = hip.topk(similarity, k)
    return C2FResult(similarity, nearest_idx, state, torch.stack(n_cand).sum(0, dtype=torch.int32), cands, torch.stack(n_dropped), torch.cat(status))
